// Joined rows in HBM: for every row of a resident source the table row with the same key tuple, and chosen columns of
// that row written into a copy of the source's row (join.hpp, include/tapstark.h "joined rows").  The hash table is the
// one of logup_mult.hip (MultTuple, mult_hash, mult_equal and the TS_LOGUP_HASH_BITS knob of logup_dev.hpp, as they
// are); what is new is that the row a probe finds is kept and read.
//
// Two plain launches behind the fills of the slot table and the report, then one small copy back; no grid barrier, no
// cooperative launch, no workgroup waits for another; every probe loop is bounded by the capacity (the power of two at
// or above 2 table_rows):
//   k_join_insert  one table row per lane, the protocol k_mult_insert documents: atomicCAS(slot, EMPTY, row) inserts
//                  the row or returns the row that holds the slot; an equal tuple -> atomicMin(slot, row), else the next
//                  slot.  A slot's content is only ever taken from what an atomic returned.  Each class ends in one
//                  slot that holds its lowest row, whatever the order.  It is a second kernel and not k_mult_insert
//                  moved: that one reads a table trace AND its preprocessed matrix through a MultDev, and sharing it
//                  would have changed the argument list of the three multiplicity calls for no saved instruction.
//   k_join_fetch   a workgroup owns JOIN_BLOCK_ROWS consecutive source rows.  Phase one, one lane per row: evaluate
//                  `when`, build the tuple, probe with plain loads (the slots are final: an earlier launch wrote them),
//                  leave the matched row or JOIN_NO_MATCH in LDS.  The misses of a wave are one ballot, one 64-bit add
//                  and one atomicMin on the lowest missing lane's row.  Phase two, all lanes: the block's rows are ONE
//                  contiguous word range of the result, walked with consecutive lanes on consecutive words: word ->
//                  (local row, column) -> is the column a dst column? -> the source word as stored, a table word
//                  through the LDS match, the row index, 1, or a default.  Coalesced stores, source reads coalesced in
//                  runs of src_width words, table reads gathered.  Every result word is written exactly once and nothing
//                  reads the result, so a dst column that overwrites a key column is safe.
// The dst list (at most 34 columns, sorted) is tested per word without a table over the result's 2^16 columns: the
// columns below 64 are one 64-bit mask in scalar registers (bit test; the rank below the bit is the list index), the
// columns from 64 on a binary search of at most six steps in the LDS copy of the list.
// Addressing: row * width and every offset into the result are 64-bit; what is 32-bit is an index inside one block's
// words (<= 256 * 2^16).
#include <string.h>

#include <string>

#include "join.hpp"
#include "logup_dev.hpp"
#include "prover_internal.hpp"

namespace ts {

static_assert(JOIN_MAX_KEYS == LOGUP_MAX_VALUES, "the key tuple is the LogUp tuple");

constexpr int JOIN_THREADS = 256;
constexpr uint32_t JOIN_BLOCK_ROWS = JOIN_THREADS;  // one lane per row in phase one
// the image the device reads: the dst columns (sorted), where each comes from, its default
constexpr uint32_t JOIN_IMG_FROM = JOIN_MAX_DST, JOIN_IMG_DEFAULT = 2 * JOIN_MAX_DST, JOIN_IMG_WORDS = 3 * JOIN_MAX_DST;

struct JoinDev {
    uint32_t n_keys, src_width, table_width, out_width, n_dst, keep, hash_mask, cap_mask;
    uint32_t when_kind, when_val, first_wide, pad;  // first_wide: the first list index whose column is >= 64
    unsigned long long low_mask;                    // bit c: column c < 64 is a dst column
    uint32_t s_kind[JOIN_MAX_KEYS], s_val[JOIN_MAX_KEYS], t_kind[JOIN_MAX_KEYS], t_val[JOIN_MAX_KEYS];
};

// what the one copy back holds (32 bytes)
struct JoinBack {
    unsigned long long n_missing, first_missing;
    uint32_t error, pad[3];
};

__device__ __forceinline__ MultTuple join_tuple(uint32_t n_keys, const uint32_t (&kind)[JOIN_MAX_KEYS],
                                                const uint32_t (&val)[JOIN_MAX_KEYS], const uint32_t* __restrict__ row) {
    MultTuple out;
#pragma unroll
    for (int q = 0; q < (int)JOIN_MAX_KEYS; q++) out.v[q] = q < (int)n_keys ? mult_term(kind[q], val[q], row, row) : 0;
    return out;
}

__global__ void __launch_bounds__(JOIN_THREADS)
k_join_insert(const JoinDev d, const uint32_t* __restrict__ table, uint64_t n, uint32_t* __restrict__ slots,
              JoinBack* __restrict__ back) {
    const uint64_t t = (uint64_t)blockIdx.x * JOIN_THREADS + threadIdx.x;
    if (t >= n) return;
    const MultTuple mine = join_tuple(d.n_keys, d.t_kind, d.t_val, table + t * d.table_width);
    const uint32_t h = mult_hash(mine, d.n_keys) & d.hash_mask;
    for (uint64_t step = 0; step <= d.cap_mask; step++) {
        uint32_t* slot = slots + ((h + (uint32_t)step) & d.cap_mask);
        const uint32_t old = atomicCAS(slot, JOIN_NO_MATCH, (uint32_t)t);
        if (old == JOIN_NO_MATCH) return;
        if (mult_equal(join_tuple(d.n_keys, d.t_kind, d.t_val, table + (uint64_t)old * d.table_width), mine)) {
            atomicMin(slot, (uint32_t)t);
            return;
        }
    }
    atomicOr(&back->error, 1u);  // every slot holds another class: impossible at load <= 1/2
}

__global__ void __launch_bounds__(JOIN_THREADS)
k_join_fetch(const JoinDev d, const uint32_t* __restrict__ image, const uint32_t* __restrict__ src, uint64_t n_src,
             const uint32_t* __restrict__ table, const uint32_t* __restrict__ slots, JoinBack* __restrict__ back,
             uint32_t* __restrict__ out) {
    __shared__ uint32_t match[JOIN_BLOCK_ROWS];
    __shared__ uint32_t list[JOIN_IMG_WORDS];
    const uint32_t SW = d.src_width, W = d.out_width;
    const uint64_t base = (uint64_t)blockIdx.x * JOIN_BLOCK_ROWS;
    const uint64_t left = n_src - base;  // >= 1: the grid holds ceil(n_src / JOIN_BLOCK_ROWS) workgroups
    const uint32_t rows = left < JOIN_BLOCK_ROWS ? (uint32_t)left : JOIN_BLOCK_ROWS;
    if (threadIdx.x < JOIN_IMG_WORDS) list[threadIdx.x] = image[threadIdx.x];

    // ---- phase one: lane = row
    uint32_t m = JOIN_NO_MATCH;
    bool miss = false;
    if (threadIdx.x < rows) {
        const uint32_t* row = src + (base + threadIdx.x) * SW;
        if (join_takes_part(mult_term(d.when_kind, d.when_val, row, row))) {
            const MultTuple mine = join_tuple(d.n_keys, d.s_kind, d.s_val, row);
            const uint32_t h = mult_hash(mine, d.n_keys) & d.hash_mask;
            for (uint64_t step = 0; step <= d.cap_mask; step++) {
                const uint32_t at = slots[(h + (uint32_t)step) & d.cap_mask];
                if (at == JOIN_NO_MATCH) break;
                if (mult_equal(join_tuple(d.n_keys, d.t_kind, d.t_val, table + (uint64_t)at * d.table_width), mine)) {
                    m = at;
                    break;
                }
            }
            miss = m == JOIN_NO_MATCH;  // (a full table of other classes is a miss too)
        }
    }
    match[threadIdx.x] = m;
    const unsigned long long missed = __ballot(miss);
    if (missed && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)missed) - 1)) {  // the wave's lowest missing row
        atomicAdd(&back->n_missing, (unsigned long long)__popcll(missed));
        atomicMin(&back->first_missing, (unsigned long long)(base + threadIdx.x));
    }
    __syncthreads();

    // ---- phase two: lane = word of the block's range of the result
    const uint32_t* dcol = list;
    const uint32_t* dfrom = list + JOIN_IMG_FROM;
    const uint32_t* ddef = list + JOIN_IMG_DEFAULT;
    const uint32_t words = rows * W;  // <= 2^8 * 2^16
    const uint32_t* s = src + base * SW;
    uint32_t* o = out + base * W;
    for (uint32_t i = threadIdx.x; i < words; i += JOIN_THREADS) {
        const uint32_t local = i / W, c = i - local * W;
        int f = -1;
        if (c < 64) {
            if ((d.low_mask >> c) & 1) f = __popcll(d.low_mask & ((1ull << c) - 1));
        } else {
            uint32_t lo = d.first_wide, hi = d.n_dst;  // the answer, if any, is in [lo, hi)
            while (lo < hi) {
                const uint32_t mid = (lo + hi) / 2;
                if (dcol[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo < d.n_dst && dcol[lo] == c) f = (int)lo;
        }
        uint32_t v;
        if (f < 0) {
            v = s[(uint64_t)local * SW + c];  // (c < SW: every column behind the source is a dst column)
        } else {
            const uint32_t at = match[local], from = dfrom[f];
            if (at != JOIN_NO_MATCH)
                v = from == JOIN_FROM_ROW ? at : from == JOIN_FROM_HIT ? 1u : table[(uint64_t)at * d.table_width + from];
            else if (d.keep && c < SW)
                v = s[(uint64_t)local * SW + c];
            else
                v = ddef[f];
        }
        o[i] = v;
    }
}

DeviceMatrix join_matrix(Context& ctx, const JoinPlan& plan, const DeviceMatrix& src, const DeviceMatrix& table,
                         bool fail_on_miss, uint64_t* n_missing, uint64_t* first_missing) {
    StageTimer timer(&ctx, "join");
    require_resident(ctx, src, "join", "the source");
    require_resident(ctx, table, "join", "the table");
    TS_REQUIRE(src.width == plan.src_width && table.width == plan.table_width, TS_ERR_INVALID,
               "join: the plan is written for other widths");
    const uint64_t n_table = join_table_rows(plan, src.height, table.height);

    JoinDev d;
    memset(&d, 0, sizeof d);
    d.n_keys = plan.n_keys;
    d.src_width = plan.src_width;
    d.table_width = plan.table_width;
    d.out_width = plan.out_width;
    d.n_dst = plan.n_dst;
    d.keep = (plan.flags & JOIN_KEEP) ? 1 : 0;
    d.hash_mask = mult_hash_mask();
    d.when_kind = plan.when.kind;
    d.when_val = plan.when.value;
    for (uint32_t q = 0; q < plan.n_keys; q++) {
        d.s_kind[q] = plan.src_keys[q].kind;
        d.s_val[q] = plan.src_keys[q].value;
        d.t_kind[q] = plan.table_keys[q].kind;
        d.t_val[q] = plan.table_keys[q].value;
    }
    uint32_t image[JOIN_IMG_WORDS] = {};
    d.first_wide = plan.n_dst;
    for (uint32_t f = 0; f < plan.n_dst; f++) {
        image[f] = plan.dst_col[f];
        image[JOIN_IMG_FROM + f] = plan.dst_from[f];
        image[JOIN_IMG_DEFAULT + f] = plan.dst_default[f];
        if (plan.dst_col[f] < 64) d.low_mask |= 1ull << plan.dst_col[f];
        else if (d.first_wide == plan.n_dst) d.first_wide = f;
    }
    uint64_t capacity = 2;
    while (capacity < 2 * n_table) capacity <<= 1;  // <= 2^28
    d.cap_mask = (uint32_t)(capacity - 1);

    // the dst list in one upload through the context's page-locked arena: no wait of its own
    DevBuf<uint32_t> d_image(&ctx, JOIN_IMG_WORDS);
    h2d(ctx, d_image.p, image, sizeof image);
    DevBuf<uint32_t> slots(&ctx, capacity);
    DevBuf<JoinBack> back(&ctx, 1);
    DeviceMatrix out;
    out.buf = DevBuf<uint32_t>(&ctx, (size_t)src.height * plan.out_width);
    out.height = src.height;
    out.width = plan.out_width;
    out.layout = DeviceMatrix::ROW_MAJOR;
    TS_HIP(hipMemsetAsync(slots.p, 0xff, capacity * sizeof(uint32_t), ctx.stream));
    TS_HIP(hipMemsetAsync(back.p, 0, sizeof(JoinBack), ctx.stream));
    TS_HIP(hipMemsetAsync(&back.p->first_missing, 0xff, sizeof(unsigned long long), ctx.stream));
    const dim3 block(JOIN_THREADS);
    TS_LAUNCH(ctx, k_join_insert, dim3((unsigned)((n_table + JOIN_THREADS - 1) / JOIN_THREADS)), block, 0, d,
              (const uint32_t*)table.buf.p, n_table, slots.p, back.p);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_join_fetch, dim3((unsigned)((src.height + JOIN_BLOCK_ROWS - 1) / JOIN_BLOCK_ROWS)), block, 0, d,
              (const uint32_t*)d_image.p, (const uint32_t*)src.buf.p, src.height, (const uint32_t*)table.buf.p,
              (const uint32_t*)slots.p, back.p, out.buf.p);
    TS_HIP(hipGetLastError());
    JoinBack host;
    d2h_sync(ctx, &host, back.p, sizeof host);  // the call's one wait
    if (host.error) throw Error(TS_ERR_INVARIANT, "join: internal error: the slot table was full");
    if (fail_on_miss && host.n_missing)
        throw Error(TS_ERR_INVARIANT, join_miss_text(host.n_missing, host.first_missing));  // (out goes back to the pool)
    if (n_missing) *n_missing = host.n_missing;
    if (first_missing) *first_missing = host.n_missing ? host.first_missing : ~0ull;
    return out;
}

}  // namespace ts
