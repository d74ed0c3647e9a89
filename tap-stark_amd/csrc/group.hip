// Grouped rows in HBM: one output row per distinct key tuple among the rows of a resident source that take part, in
// order of first appearance (group.hpp, include/tapstark.h "grouped rows").  The pieces are the project's own: the slot
// table and the atomicCAS / atomicMin "lowest row of a class" protocol of join.hip and logup_mult.hip (MultTuple,
// mult_hash, mult_equal and the TS_LOGUP_HASH_BITS knob of logup_dev.hpp, as they are), the count, offsets and pad rows
// of collect.hip (its block scan and its offsets kernel, as they are), and the wave-combined add of the multiplicity
// fill, here over every accumulator of a group at once.
//
// Plain launches behind the fill of the slot table; no grid barrier, no cooperative launch, no workgroup waits for
// another; every probe loop is bounded by the capacity (the power of two at or above 2 height):
//   k_group_insert      one source row per lane: the selector, the tuple, then the insert protocol.  A wave whose rows
//                       all carry ONE tuple (a sorted source) sends its lowest lane alone.  cls[row] <- the slot of the
//                       row's class, GROUP_NONE for a row that takes no part: no later pass probes again.  After this
//                       launch each class owns one slot, which holds its least row.
//   k_group_count       per block of at most TS_COLLECT_BLOCK_ROWS rows: its leaders (rows r with slots[cls[r]] == r).
//   k_collect_offsets   collect.hip's: where each block's groups start, and the total.  The host reads the total in
//                       one copy, the call's only wait: it sizes the result and the records.
//   k_group_fill        every word of the groups' records <- its identity.
//   k_group_index       the blocks again: a leader takes index = block offset + rank, writes its row as the record's
//                       FIRST and leaves GROUP_LEADER | index in its own cls word, where the rows of its class find it.
//   k_group_accumulate  one row per lane: index = through cls, the slot and the leader's cls word; then LAST by
//                       atomicMax, COUNT and the sums by 64-bit atomicAdd, minima and maxima by 32-bit atomicMin /
//                       atomicMax on the low half.  A wave whose rows all go to ONE group combines with shuffles first
//                       and issues one atomic per accumulator.  Every aggregate is order-independent, so the words
//                       are the same on every run.
//   k_group_finish      the result as one word range, consecutive lanes on consecutive words: word -> (group, column) ->
//                       term (group_term of group.hpp); FIRST and LAST words are gathered from the source.  The
//                       workgroups behind the grid fill the pad rows, as in the collect.
// Every result word is written exactly once and nothing reads the result; everything a kernel reads was written by a
// fill or a kernel of this call.  Addressing: row * width, group * record and every offset into the result are 64-bit.
#include <string>

#include "collect_dev.hpp"
#include "group.hpp"
#include "logup_dev.hpp"
#include "prover_internal.hpp"

namespace ts {

static_assert(GROUP_MAX_KEYS == LOGUP_MAX_VALUES, "the key tuple is the LogUp tuple");

constexpr uint32_t GROUP_NONE = 0xFFFFFFFFu;    // slots: empty; cls: the row takes no part
constexpr uint32_t GROUP_LEADER = 0x80000000u;  // cls of a leader after k_group_index: this bit and its group's index
constexpr uint32_t GROUP_FINISH_BLOCKS = 1u << 16;
// the image the device reads: the pad row, the terms, the aggregates' kinds and columns
constexpr uint32_t GROUP_IMG_TERMS = GROUP_MAX_WIDTH, GROUP_IMG_AGG = GROUP_IMG_TERMS + 3 * GROUP_MAX_WIDTH;
constexpr uint32_t GROUP_IMG_WORDS = GROUP_IMG_AGG + 2 * GROUP_MAX_AGGREGATES;

struct GroupDev {
    uint32_t n_keys, src_width, out_width, sel, hash_mask, cap_mask, n_aggregates, stride;
    uint32_t block_rows, rpt, n_blocks, min_mask;  // min_mask: bit a, aggregate a is a minimum
    uint32_t k_kind[GROUP_MAX_KEYS], k_val[GROUP_MAX_KEYS];
};

__device__ __forceinline__ MultTuple group_tuple(const GroupDev& d, const uint32_t* __restrict__ row) {
    MultTuple out;
#pragma unroll
    for (int q = 0; q < (int)GROUP_MAX_KEYS; q++) out.v[q] = q < (int)d.n_keys ? mult_term(d.k_kind[q], d.k_val[q], row, row) : 0;
    return out;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = wave_shfl_xor(v, s);
        v = o > v ? o : v;
    }
    return v;
}

// `error` <- 1 where every slot holds another class: impossible at load <= 1/2
__global__ void __launch_bounds__(COLLECT_THREADS)
k_group_insert(const GroupDev d, const uint32_t* __restrict__ src, uint64_t n, uint32_t* __restrict__ slots,
               uint32_t* __restrict__ cls, uint32_t* __restrict__ error) {
    const uint64_t t = (uint64_t)blockIdx.x * COLLECT_THREADS + threadIdx.x;
    const unsigned lane = threadIdx.x & 63;
    bool part = false;
    MultTuple mine = {};
    if (t < n) {
        const uint32_t* row = src + t * d.src_width;
        part = d.sel == COLLECT_ALWAYS || collect_fires(row[d.sel]);
        if (part) mine = group_tuple(d, row);
    }
    // the wave's rows ascend with the lane, so where all of them carry one tuple the lowest lane's row is the least
    const unsigned long long parts = __ballot(part);
    if (parts == 0) {  // (wave-uniform)
        if (t < n) cls[t] = GROUP_NONE;
        return;
    }
    const int first = __ffsll((long long)parts) - 1;
    bool eq = true;
#pragma unroll
    for (int q = 0; q < (int)GROUP_MAX_KEYS; q++) eq = eq && mine.v[q] == (uint32_t)__shfl((int)mine.v[q], first, 64);
    const bool one = __ballot(part && eq) == parts;

    uint32_t at = GROUP_NONE;
    if (part && (!one || lane == (unsigned)first)) {
        const uint32_t h = mult_hash(mine, d.n_keys) & d.hash_mask;
        for (uint64_t step = 0; step <= d.cap_mask; step++) {
            const uint32_t s = (h + (uint32_t)step) & d.cap_mask;
            const uint32_t old = atomicCAS(slots + s, GROUP_NONE, (uint32_t)t);
            if (old == GROUP_NONE) {
                at = s;
                break;
            }
            if (mult_equal(group_tuple(d, src + (uint64_t)old * d.src_width), mine)) {
                if ((uint32_t)t < old) atomicMin(slots + s, (uint32_t)t);  // (a slot's row only ever descends)
                at = s;
                break;
            }
        }
        if (at == GROUP_NONE) atomicOr(error, 1u);
    }
    const uint32_t shared = (uint32_t)__shfl((int)at, first, 64);
    if (t < n) cls[t] = !part ? GROUP_NONE : one ? shared : at;
}

// The leaders among this lane's rows: bit k for its k-th row.  A lane owns d.rpt consecutive rows of the block.
__device__ __forceinline__ uint32_t group_lane_leaders(const GroupDev& d, uint64_t base, uint32_t tile_rows,
                                                       const uint32_t* __restrict__ slots, const uint32_t* cls) {
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < COLLECT_RPT; k++) {
        const uint32_t local = threadIdx.x * d.rpt + k;
        if (k < (int)d.rpt && local < tile_rows) {
            const uint32_t c = cls[base + local];
            if (c != GROUP_NONE && slots[c] == (uint32_t)(base + local)) mask |= 1u << k;
        }
    }
    return mask;
}

__device__ __forceinline__ uint32_t group_tile_rows(const GroupDev& d, uint64_t base, uint64_t n) {
    const uint64_t left = n - base;  // >= 1: the grid holds ceil(n / block_rows) blocks
    return left < d.block_rows ? (uint32_t)left : d.block_rows;
}

__global__ void __launch_bounds__(COLLECT_THREADS)
k_group_count(const GroupDev d, uint64_t n, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ cls,
              uint32_t* __restrict__ counts) {
    __shared__ uint32_t wave_sums[COLLECT_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * d.block_rows;
    uint32_t total;
    collect_block_scan((uint32_t)__popc(group_lane_leaders(d, base, group_tile_rows(d, base, n), slots, cls)), wave_sums, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;  // <= 1024
}

__global__ void __launch_bounds__(COLLECT_THREADS)
k_group_fill(const GroupDev d, uint64_t n_words, unsigned long long* __restrict__ records) {
    for (uint64_t i = (uint64_t)blockIdx.x * COLLECT_THREADS + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * COLLECT_THREADS) {
        const uint32_t k = (uint32_t)(i % d.stride);
        records[i] = k >= GROUP_RECORD_HEAD && ((d.min_mask >> (k - GROUP_RECORD_HEAD)) & 1) ? group_identity(G_MIN) : 0ull;
    }
}

// (cls is read and written: a leader's own word, by the lane that owns the row)
__global__ void __launch_bounds__(COLLECT_THREADS)
k_group_index(const GroupDev d, uint64_t n, const uint32_t* __restrict__ slots, uint32_t* cls,
              const uint64_t* __restrict__ offsets, unsigned long long* __restrict__ records) {
    __shared__ uint32_t wave_sums[COLLECT_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * d.block_rows;
    const uint32_t mask = group_lane_leaders(d, base, group_tile_rows(d, base, n), slots, cls);
    uint32_t total;
    uint64_t index = offsets[blockIdx.x] + collect_block_scan((uint32_t)__popc(mask), wave_sums, total);
#pragma unroll
    for (int k = 0; k < COLLECT_RPT; k++)
        if (mask & (1u << k)) {
            const uint64_t row = base + threadIdx.x * d.rpt + k;
            records[index * d.stride + GROUP_FIRST] = row;
            cls[row] = GROUP_LEADER | (uint32_t)index;  // index < 2^27
            index++;
        }
}

__global__ void __launch_bounds__(COLLECT_THREADS)
k_group_accumulate(const GroupDev d, const uint32_t* __restrict__ image, const uint32_t* __restrict__ src, uint64_t n,
                   const uint32_t* __restrict__ slots, const uint32_t* __restrict__ cls,
                   unsigned long long* __restrict__ records) {
    const uint64_t t = (uint64_t)blockIdx.x * COLLECT_THREADS + threadIdx.x;
    const unsigned lane = threadIdx.x & 63;
    uint32_t index = GROUP_NONE;
    if (t < n) {
        const uint32_t c = cls[t];
        if (c != GROUP_NONE) index = (c & GROUP_LEADER ? c : cls[slots[c]]) & ~GROUP_LEADER;
    }
    const bool part = index != GROUP_NONE;
    const unsigned long long parts = __ballot(part);
    if (parts == 0) return;  // (wave-uniform)
    const int first = __ffsll((long long)parts) - 1;
    const uint32_t dest = (uint32_t)__shfl((int)index, first, 64);
    const bool one = (parts & (parts - 1)) && __ballot(part && index == dest) == parts;  // (wave-uniform)
    const uint32_t* row = src + (part ? t : 0) * d.src_width;
    const uint32_t* agg = image + GROUP_IMG_AGG;
    if (one) {  // every lane walks this branch: the shuffles need them all
        unsigned long long* rec = records + (uint64_t)dest * d.stride;
        const unsigned long long last = wave_max(part ? t : 0ull);
        if (lane == (unsigned)first) {
            atomicMax(rec + GROUP_LAST, last);
            atomicAdd(rec + GROUP_COUNT, (unsigned long long)__popcll(parts));
        }
        for (uint32_t a = 0; a < d.n_aggregates; a++) {  // (uniform bounds, kinds and columns: scalar loads)
            const uint32_t kind = agg[2 * a];
            const uint32_t v = part ? group_canonical(row[agg[2 * a + 1]]) : (uint32_t)group_identity(kind);
            const unsigned long long all = kind == G_SUM ? wave_sum(v) : kind == G_MIN ? wave_min(v) : wave_max(v);
            if (lane != (unsigned)first) continue;
            unsigned long long* w = rec + GROUP_RECORD_HEAD + a;
            if (kind == G_SUM) atomicAdd(w, all);
            else if (kind == G_MIN) atomicMin(reinterpret_cast<uint32_t*>(w), (uint32_t)all);
            else atomicMax(reinterpret_cast<uint32_t*>(w), (uint32_t)all);
        }
    } else if (part) {
        unsigned long long* rec = records + (uint64_t)index * d.stride;
        atomicMax(rec + GROUP_LAST, (unsigned long long)t);
        atomicAdd(rec + GROUP_COUNT, 1ull);
        for (uint32_t a = 0; a < d.n_aggregates; a++) {
            const uint32_t kind = agg[2 * a];
            const uint32_t v = group_canonical(row[agg[2 * a + 1]]);
            unsigned long long* w = rec + GROUP_RECORD_HEAD + a;
            if (kind == G_SUM) atomicAdd(w, (unsigned long long)v);
            else if (kind == G_MIN) atomicMin(reinterpret_cast<uint32_t*>(w), v);
            else atomicMax(reinterpret_cast<uint32_t*>(w), v);
        }
    }
}

__global__ void __launch_bounds__(COLLECT_THREADS)
k_group_finish(const GroupDev d, const uint32_t* __restrict__ image, const uint32_t* __restrict__ src,
               const unsigned long long* __restrict__ records, uint32_t n_blocks, uint64_t n_live, uint64_t height,
               uint32_t* __restrict__ out) {
    __shared__ GroupTermWord terms[GROUP_MAX_WIDTH];
    const uint32_t W = d.out_width;

    if (blockIdx.x >= n_blocks) {  // the pad rows: tiles of 256 rows, dealt round to the workgroups behind the grid
        const uint32_t* pad = image;
        const uint64_t n_pad = height - n_live;
        const uint64_t n_tiles = (n_pad + COLLECT_PAD_TILE_ROWS - 1) / COLLECT_PAD_TILE_ROWS;
        for (uint64_t t = blockIdx.x - n_blocks; t < n_tiles; t += gridDim.x - n_blocks) {
            const uint64_t r0 = t * COLLECT_PAD_TILE_ROWS, left = n_pad - r0;
            const uint32_t words = (left < COLLECT_PAD_TILE_ROWS ? (uint32_t)left : COLLECT_PAD_TILE_ROWS) * W;
            uint32_t* o = out + (n_live + r0) * W;
            for (uint32_t i = threadIdx.x; i < words; i += COLLECT_THREADS) o[i] = pad[i % W];
        }
        return;
    }

    if (threadIdx.x < W) {
        const uint32_t* t = image + GROUP_IMG_TERMS + 3 * threadIdx.x;
        terms[threadIdx.x] = {t[0], t[1], t[2]};
    }
    __syncthreads();
    const uint64_t words = n_live * W;  // <= 2^27 * 2^6
    for (uint64_t i = (uint64_t)blockIdx.x * COLLECT_THREADS + threadIdx.x; i < words; i += (uint64_t)n_blocks * COLLECT_THREADS) {
        const uint64_t g = i / W;
        const uint32_t c = (uint32_t)(i - g * W);
        out[i] = group_term(terms[c], records + g * d.stride, g, src, d.src_width);
    }
}

DeviceMatrix group_matrix(Context& ctx, const GroupPlan& plan, const DeviceMatrix& src, uint64_t out_height,
                          uint64_t* n_live_out) {
    StageTimer timer(&ctx, "group");
    require_resident(ctx, src, "group", "source 0");
    TS_REQUIRE(src.width == plan.src_width, TS_ERR_INVALID,
               "group: the spec is written for a source 0 of " + std::to_string(plan.src_width) +
                   " columns, this one has " + std::to_string(src.width));
    collect_check_out_height(out_height);
    // both knobs are read on every call and no output word depends on either
    const uint32_t knob =
        (uint32_t)mult_knob("TS_COLLECT_BLOCK_ROWS", 1, COLLECT_THREADS * COLLECT_RPT, COLLECT_THREADS * COLLECT_RPT);
    const uint64_t n = src.height;
    const uint64_t n_blocks = (n + knob - 1) / knob;
    // (a launch takes fewer than 2^32 threads; only the knob can ask for more)
    TS_REQUIRE(n_blocks < (1ull << 24), TS_ERR_INVALID,
               "group: TS_COLLECT_BLOCK_ROWS is too small for a source of this height");

    GroupDev d = {};
    d.n_keys = plan.n_keys;
    d.src_width = plan.src_width;
    d.out_width = plan.out_width;
    d.sel = plan.sel;
    d.hash_mask = mult_hash_mask();
    d.n_aggregates = plan.n_aggregates;
    d.stride = GROUP_RECORD_HEAD + plan.n_aggregates;
    d.block_rows = knob;
    d.rpt = (knob + COLLECT_THREADS - 1) / COLLECT_THREADS;
    d.n_blocks = (uint32_t)n_blocks;
    for (uint32_t q = 0; q < plan.n_keys; q++) {
        d.k_kind[q] = plan.keys[q].kind;
        d.k_val[q] = plan.keys[q].value;
    }
    uint64_t capacity = 2;
    while (capacity < 2 * n) capacity <<= 1;  // <= 2^28
    d.cap_mask = (uint32_t)(capacity - 1);

    // pad row, terms and aggregates in one upload through the context's page-locked arena: no wait of its own
    uint32_t image[GROUP_IMG_WORDS] = {};
    for (uint32_t c = 0; c < plan.out_width; c++) {
        const GroupTermWord& t = plan.terms[c];
        image[c] = plan.pad[c];
        image[GROUP_IMG_TERMS + 3 * c] = t.kind;
        image[GROUP_IMG_TERMS + 3 * c + 1] = t.value;
        image[GROUP_IMG_TERMS + 3 * c + 2] = t.slot;
        if (t.kind >= G_SUM && t.kind <= G_MAX) {
            image[GROUP_IMG_AGG + 2 * t.slot] = t.kind;
            image[GROUP_IMG_AGG + 2 * t.slot + 1] = t.value;
            if (t.kind == G_MIN) d.min_mask |= 1u << t.slot;
        }
    }
    DevBuf<uint32_t> d_image(&ctx, GROUP_IMG_WORDS);
    h2d(ctx, d_image.p, image, sizeof image);
    DevBuf<uint32_t> slots(&ctx, capacity);
    DevBuf<uint32_t> cls(&ctx, n);
    DevBuf<uint32_t> counts(&ctx, d.n_blocks);
    DevBuf<uint64_t> offsets(&ctx, (size_t)d.n_blocks + 2);  // behind them the total, then the error word
    uint32_t* error = reinterpret_cast<uint32_t*>(offsets.p + d.n_blocks + 1);

    const dim3 block(COLLECT_THREADS);
    const dim3 per_row((unsigned)((n + COLLECT_THREADS - 1) / COLLECT_THREADS));
    TS_HIP(hipMemsetAsync(slots.p, 0xff, capacity * sizeof(uint32_t), ctx.stream));
    TS_HIP(hipMemsetAsync(error, 0, sizeof(uint64_t), ctx.stream));
    TS_LAUNCH(ctx, k_group_insert, per_row, block, 0, d, (const uint32_t*)src.buf.p, n, slots.p, cls.p, error);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_group_count, dim3(d.n_blocks), block, 0, d, n, (const uint32_t*)slots.p, (const uint32_t*)cls.p,
              counts.p);
    TS_HIP(hipGetLastError());
    collect_launch_offsets(ctx, counts.p, d.n_blocks, offsets.p);
    uint64_t back[2] = {0, 0};
    d2h_sync(ctx, back, offsets.p + d.n_blocks, sizeof back);  // the call's one wait
    if (back[1]) throw Error(TS_ERR_INVARIANT, "group: internal error: the slot table was full");
    const uint64_t n_live = back[0];
    const uint64_t height = group_height(n_live, out_height);  // throws: the buffers above go back to the pool

    DeviceMatrix out;
    out.buf = DevBuf<uint32_t>(&ctx, (size_t)height * plan.out_width);
    out.height = height;
    out.width = plan.out_width;
    out.layout = DeviceMatrix::ROW_MAJOR;
    const uint64_t record_words = (n_live ? n_live : 1) * d.stride;
    DevBuf<unsigned long long> records(&ctx, record_words);
    const auto blocks_for = [](uint64_t items) {
        const uint64_t b = (items + COLLECT_THREADS - 1) / COLLECT_THREADS;
        return (uint32_t)(b < GROUP_FINISH_BLOCKS ? b : GROUP_FINISH_BLOCKS);
    };
    if (n_live) {
        TS_LAUNCH(ctx, k_group_fill, dim3(blocks_for(record_words)), block, 0, d, record_words, records.p);
        TS_HIP(hipGetLastError());
        TS_LAUNCH(ctx, k_group_index, dim3(d.n_blocks), block, 0, d, n, (const uint32_t*)slots.p, cls.p,
                  (const uint64_t*)offsets.p, records.p);
        TS_HIP(hipGetLastError());
        TS_LAUNCH(ctx, k_group_accumulate, per_row, block, 0, d, (const uint32_t*)d_image.p, (const uint32_t*)src.buf.p, n,
                  (const uint32_t*)slots.p, (const uint32_t*)cls.p, records.p);
        TS_HIP(hipGetLastError());
    }
    const uint32_t live_blocks = blocks_for(n_live * plan.out_width);
    const uint64_t pad_tiles = (height - n_live + COLLECT_PAD_TILE_ROWS - 1) / COLLECT_PAD_TILE_ROWS;
    const uint32_t pad_blocks = (uint32_t)(pad_tiles < COLLECT_PAD_BLOCKS ? pad_tiles : COLLECT_PAD_BLOCKS);
    TS_LAUNCH(ctx, k_group_finish, dim3(live_blocks + pad_blocks), block, 0, d, (const uint32_t*)d_image.p,
              (const uint32_t*)src.buf.p, (const unsigned long long*)records.p, live_blocks, n_live, height, out.buf.p);
    TS_HIP(hipGetLastError());
    if (n_live_out) *n_live_out = n_live;
    return out;
}

}  // namespace ts
