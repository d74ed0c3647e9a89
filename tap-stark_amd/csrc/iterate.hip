// Iterated trace columns in HBM: a lowered TITR list (derive.hpp, iterate.hpp) walked down every group of rows of a
// resident row-major matrix, one lane per group (include/tapstark.h "iterated columns").
//
// The recurrence is sequential inside a group and a trace has thousands of groups, so the parallelism lies across the
// groups.  Four plain launches, the reduce-then-scan shape of collect.hip and expand.hip: no grid barrier, no flag
// another workgroup waits for, nothing spins on another workgroup.
//   k_iterate_count    one workgroup per block of at most TS_ITERATE_BLOCK_ROWS rows, a lane owns rpt =
//                      ceil(block_rows / 256) <= 4 consecutive rows.  Reads the reset column only.  The number of group
//                      starts in the block -> counts[block]; its last start, plus one (0: none) -> lasts[block].
//   k_iterate_offsets  one workgroup: the exclusive scan of the counts, 256 per trip, with the carry -> offsets[block];
//                      the running maximum of the last starts -> prevs[block], the last start BEFORE the block, so that
//                      a group that straddles blocks is measured.  Behind the loop tail[0] <- n_groups and tail[1] <- the
//                      final group (it ends at row h, which no start marks), packed as below, when it is over-long.
//   k_iterate_starts   the first grid again: starts[g] <- the row group g starts at, starts[n_groups] <- h.  A start
//                      also knows the start before it -- inside its lane, from the lanes below (a running maximum, by
//                      shuffles and LDS) or from prevs[block] -- and so the length of the group that ENDS at it: an
//                      over-long one goes into tail[1] with atomicMin, packed start << 32 | rows, so the least start
//                      row wins and brings its length (both are at most 2^27).  The minimum of a set does not depend
//                      on the order of the atomics: the same 16 bytes every run.
//   the host reads tail, 16 bytes: the call's ONE wait.  It sizes the last grid and decides the refusal.
//   k_iterate_walk     workgroups of ONE wave; lane l of workgroup w owns group 64 w + l.  The workgroup first copies
//                      the untouched columns of its contiguous row range [starts[64 w], starts[min(64 w + 64,
//                      n_groups)]), consecutive lanes on consecutive words, a bit per column, as k_derive does.  Then it
//                      walks t = 0 .. (its longest group) - 1, a wave-uniform loop around k_derive's interpreter: one
//                      scalar 16-byte fetch per instruction, one ahead; the slot file in LDS [slot][lane]; the last
//                      value forwarded in a VGPR.  Carry k lives in slot k from the group's first row to its last.  A
//                      lane past its group's end computes and stores nothing.  At 48 slots a workgroup holds 12 KiB of
//                      LDS, so several share a CU (a lone wave on a CU gets a fraction of the LDS read rate).
// Every out word is written exactly once -- by the copy if no output names its column, by one store otherwise -- and
// nothing reads out.  Widths: a row, a start and a group count are below 2^27 + 1 and 32-bit (a group holds a row, so
// there are no more groups than rows); row * width and every offset into src or out is 64-bit.
// The lanes of a wave read rows a group apart, each streaming down its own cache lines: accepted here, unmeasured.
#include <string>

#include "iterate.hpp"
#include "logup_dev.hpp"  // mult_knob
#include "prover_internal.hpp"

namespace ts {

constexpr int ITER_THREADS = 256;  // count, offsets, starts
constexpr int ITER_RPT = 4;        // rows per lane at most: a workgroup owns up to 1024 rows
constexpr int ITER_WAVES = ITER_THREADS / 64;
constexpr uint32_t ITER_MAX_BLOCK_ROWS = ITER_THREADS * ITER_RPT;
constexpr int ITER_WALK_THREADS = 64;
constexpr uint32_t ITER_COPY_ROWS = 256;  // of one copy tile: tile words <= 2^8 * 2^16

struct IterateDev {
    const uint32_t* src;
    uint64_t height;
    uint32_t src_width, out_width, reset_column, max_group_rows;
    uint32_t block_rows, rpt, n_blocks, n_instr, n_carries, any_copy;
};

__device__ __forceinline__ uint64_t iterate_pack(uint32_t start, uint32_t rows) { return (uint64_t)start << 32 | rows; }

// Over the workgroup's lanes in lane order: sum <- the sum of `sum` over the lanes BEFORE this one, high <- the maximum
// of `high` over them (0 when there are none); all_sum, all_high <- over every lane.  Every thread calls it.
__device__ __forceinline__ void iterate_block_scan(uint32_t& sum, uint32_t& high, uint32_t (&wave_sum)[ITER_WAVES],
                                                   uint32_t (&wave_high)[ITER_WAVES], uint32_t& all_sum, uint32_t& all_high) {
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t s = sum, m = high;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const uint32_t us = (uint32_t)__shfl_up((int)s, d, 64), um = (uint32_t)__shfl_up((int)m, d, 64);
        if (lane >= d) {
            s += us;
            m = um > m ? um : m;
        }
    }
    __syncthreads();  // (a second call reuses the arrays)
    if (lane == 63) {
        wave_sum[wv] = s;
        wave_high[wv] = m;
    }
    __syncthreads();
    uint32_t before_s = 0, before_m = 0, as = 0, am = 0;
#pragma unroll
    for (int k = 0; k < ITER_WAVES; k++) {
        const uint32_t ws = wave_sum[k], wm = wave_high[k];
        if (k < (int)wv) {
            before_s += ws;
            before_m = wm > before_m ? wm : before_m;
        }
        as += ws;
        am = wm > am ? wm : am;
    }
    // exclusive: the inclusive value of the lane below, behind the waves below
    const uint32_t below_s = (uint32_t)__shfl_up((int)s, 1, 64), below_m = (uint32_t)__shfl_up((int)m, 1, 64);
    sum = before_s + (lane == 0 ? 0u : below_s);
    high = lane == 0 ? before_m : (below_m > before_m ? below_m : before_m);
    all_sum = as;
    all_high = am;
}

// The lane's rows of the block: bit k of the result is set where local row threadIdx.x * rpt + k starts a group.
__device__ __forceinline__ uint32_t iterate_lane_starts(const IterateDev& d, uint64_t base, uint32_t rows) {
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < ITER_RPT; k++) {
        const uint32_t local = threadIdx.x * d.rpt + k;
        if (k < (int)d.rpt && local < rows && iterate_starts(d.src, base + local, d.src_width, d.reset_column)) bits |= 1u << k;
    }
    return bits;
}

__global__ void __launch_bounds__(ITER_THREADS)
k_iterate_count(const IterateDev d, uint32_t* __restrict__ counts, uint32_t* __restrict__ lasts) {
    __shared__ uint32_t wave_sum[ITER_WAVES], wave_high[ITER_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * d.block_rows;
    const uint64_t left = d.height - base;  // >= 1: the grid holds ceil(height / block_rows) blocks
    const uint32_t rows = left < d.block_rows ? (uint32_t)left : d.block_rows;
    const uint32_t bits = iterate_lane_starts(d, base, rows);
    uint32_t sum = (uint32_t)__popc(bits);
    // the lane's last start, plus one: rows ascend with the lanes, so the maximum is the last
    uint32_t high = bits ? (uint32_t)(base + threadIdx.x * d.rpt + (31 - __clz((int)bits))) + 1 : 0u;
    uint32_t all_sum, all_high;
    iterate_block_scan(sum, high, wave_sum, wave_high, all_sum, all_high);
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = all_sum;
        lasts[blockIdx.x] = all_high;
    }
}

// In place: offsets[b] <- counts[0] + ... + counts[b-1]; prevs[b] <- the last start before block b, plus one (0 for
// block 0).  tail[0] <- n_groups; tail[1] <- the final group when it is over-long, else ~0.
__global__ void __launch_bounds__(ITER_THREADS)
k_iterate_offsets(const IterateDev d, uint32_t* __restrict__ offsets, uint32_t* __restrict__ prevs, uint64_t* __restrict__ tail) {
    __shared__ uint32_t wave_sum[ITER_WAVES], wave_high[ITER_WAVES];
    uint32_t carry_sum = 0, carry_high = 0;
    for (uint32_t b0 = 0; b0 < d.n_blocks; b0 += ITER_THREADS) {  // (uniform bounds: every thread loops alike)
        const uint32_t b = b0 + threadIdx.x;
        uint32_t sum = b < d.n_blocks ? offsets[b] : 0u, high = b < d.n_blocks ? prevs[b] : 0u;
        uint32_t pass_sum, pass_high;
        iterate_block_scan(sum, high, wave_sum, wave_high, pass_sum, pass_high);
        if (b < d.n_blocks) {  // (this lane alone read and writes words b)
            offsets[b] = carry_sum + sum;
            prevs[b] = high > carry_high ? high : carry_high;
        }
        carry_sum += pass_sum;
        carry_high = pass_high > carry_high ? pass_high : carry_high;
    }
    if (threadIdx.x == 0) {
        const uint32_t last_start = carry_high - 1;  // row 0 starts a group, so there is one
        const uint64_t rows = d.height - last_start;
        tail[0] = carry_sum;
        tail[1] = rows > d.max_group_rows ? iterate_pack(last_start, (uint32_t)rows) : ~0ull;
    }
}

__global__ void __launch_bounds__(ITER_THREADS)
k_iterate_starts(const IterateDev d, const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ prevs,
                 uint32_t* __restrict__ starts, uint64_t* __restrict__ tail) {
    __shared__ uint32_t wave_sum[ITER_WAVES], wave_high[ITER_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * d.block_rows;
    const uint64_t left = d.height - base;
    const uint32_t rows = left < d.block_rows ? (uint32_t)left : d.block_rows;
    const uint32_t bits = iterate_lane_starts(d, base, rows);
    uint32_t g = (uint32_t)__popc(bits);
    uint32_t prev = bits ? (uint32_t)(base + threadIdx.x * d.rpt + (31 - __clz((int)bits))) + 1 : 0u;
    uint32_t all_sum, all_high;
    iterate_block_scan(g, prev, wave_sum, wave_high, all_sum, all_high);
    g += offsets[blockIdx.x];
    const uint32_t before = prevs[blockIdx.x];
    prev = prev > before ? prev : before;  // the last start before this lane's rows, plus one
#pragma unroll
    for (int k = 0; k < ITER_RPT; k++) {
        if (!((bits >> k) & 1)) continue;
        const uint32_t row = (uint32_t)(base + threadIdx.x * d.rpt + k);
        starts[g++] = row;  // g < n_groups <= height: starts[] holds height + 1 words
        if (prev != 0) {    // (row 0 ends no group)
            const uint32_t len = row - (prev - 1);
            if (len > d.max_group_rows) atomicMin((unsigned long long*)&tail[1], (unsigned long long)iterate_pack(prev - 1, len));
        }
        prev = row + 1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) starts[tail[0]] = (uint32_t)d.height;  // (tail[0] is k_iterate_offsets')
}

__global__ void __launch_bounds__(ITER_WALK_THREADS)
k_iterate_walk(const uint4* __restrict__ code, const uint32_t* __restrict__ named, const uint32_t* __restrict__ inits,
               const IterateDev d, const uint32_t* __restrict__ starts, uint32_t n_groups, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t iterate_slots[];  // [n_live][ITER_WALK_THREADS]
    const uint32_t* __restrict__ src = d.src;
    const uint32_t g0 = blockIdx.x * ITER_WALK_THREADS;  // < n_groups: the grid holds ceil(n_groups / 64) workgroups
    const uint32_t g1 = n_groups - g0 < ITER_WALK_THREADS ? n_groups : g0 + ITER_WALK_THREADS;

    // the untouched columns of the workgroup's rows, coalesced on both sides
    if (d.any_copy) {
        const uint64_t r_end = starts[g1];
        for (uint64_t r0 = starts[g0]; r0 < r_end; r0 += ITER_COPY_ROWS) {
            const uint64_t left = r_end - r0;
            const uint32_t tile_words = (left < ITER_COPY_ROWS ? (uint32_t)left : ITER_COPY_ROWS) * d.out_width;
            for (uint32_t j = threadIdx.x; j < tile_words; j += ITER_WALK_THREADS) {
                const uint32_t lr = j / d.out_width, c = j - lr * d.out_width;
                if ((named[c >> 5] >> (c & 31)) & 1) continue;  // (a column at or beyond src_width always is)
                out[(r0 + lr) * d.out_width + c] = src[(r0 + lr) * d.src_width + c];
            }
        }
    }

    const uint32_t g = g0 + threadIdx.x;
    const bool owner = g < g1;
    const uint32_t first = owner ? starts[g] : 0u;
    const uint32_t len = owner ? starts[g + 1] - first : 0u;
    uint32_t longest = len;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)longest, o, 64);
        longest = other > longest ? other : longest;
    }
    longest = (uint32_t)__builtin_amdgcn_readfirstlane((int)longest);  // the same in every lane: a scalar loop bound

    uint32_t* my = iterate_slots + threadIdx.x;
    for (uint32_t k = 0; k < d.n_carries; k++) my[k * ITER_WALK_THREADS] = inits[k];
    uint32_t fwd_slot = ~0u, fwd_val = 0;
    auto rd = [&](uint32_t slot) { return slot == fwd_slot ? fwd_val : my[slot * ITER_WALK_THREADS]; };
    auto wr = [&](uint32_t slot, uint32_t v) {
        my[slot * ITER_WALK_THREADS] = v;
        fwd_slot = slot;
        fwd_val = v;
    };

    for (uint32_t t = 0; t < longest; t++) {
        const bool active = t < len;
        const uint64_t row = active ? (uint64_t)first + t : 0;  // an idle lane points at row 0 and touches nothing
        const uint32_t* rows0 = src + row * d.src_width;
        const uint32_t* rows1 = src + (row + 1 == d.height ? 0 : row + 1) * d.src_width;
        const uint32_t* rows2 = src + (row == 0 ? d.height - 1 : row - 1) * d.src_width;
        uint32_t* o = out + row * d.out_width;
        // all three row pointers read first and chosen with selects: an index into an array of them would go to scratch
        auto ld = [&](uint32_t offset, uint32_t column) {
            const uint32_t *p0 = rows0, *p1 = rows1, *p2 = rows2;
            return (offset == 0 ? p0 : offset == 1 ? p1 : p2)[column];
        };
        auto st = [&](uint32_t column, uint32_t word) { o[column] = word; };
        const bool group_last = t + 1 == len;
        uint4 ins = code[0];
        for (uint32_t pc = 0; pc < d.n_instr; pc++) {
            const uint4 nxt = code[pc + 1 < d.n_instr ? pc + 1 : pc];
            if (active) iterate_instruction(ins.x, ins.y, ins.z, ins.w, row, d.height, t, group_last, rd, wr, ld, st);
            ins = nxt;
        }
    }
}

DeviceMatrix iterate_matrix(Context& ctx, const DeriveProgram& prog, const DeviceMatrix& src) {
    // TS_ITERATE_BLOCK_ROWS (1 .. 1024, read on every call): the rows of a count block, a test knob that makes small
    // matrices cross the lane, the wave, the workgroup and several trips of the offsets loop.  No output word depends
    // on it.
    const uint32_t knob = (uint32_t)mult_knob("TS_ITERATE_BLOCK_ROWS", 1, ITER_MAX_BLOCK_ROWS, ITER_MAX_BLOCK_ROWS);
    const uint64_t n_blocks = (src.height + knob - 1) / knob;
    // (a launch takes fewer than 2^32 threads; only the knob can ask for more)
    TS_REQUIRE(n_blocks < (1ull << 24), TS_ERR_INVALID,
               "iterate: TS_ITERATE_BLOCK_ROWS is too small for a source of this height");

    IterateDev d = {};
    d.src = src.buf.p;
    d.height = src.height;
    d.src_width = src.width;
    d.out_width = prog.out_width;
    d.reset_column = prog.reset_column;
    d.max_group_rows = prog.max_group_rows;
    d.block_rows = knob;
    d.rpt = (knob + ITER_THREADS - 1) / ITER_THREADS;
    d.n_blocks = (uint32_t)n_blocks;
    d.n_instr = prog.n_instr();
    d.n_carries = (uint32_t)prog.inits.size();
    for (uint32_t c = 0; c < prog.out_width; c++) d.any_copy |= !((prog.named[c >> 5] >> (c & 31)) & 1);

    // the list, the column bits and the inits in one upload through the context's page-locked arena: no wait of its own
    std::vector<uint32_t> image(prog.code);
    image.insert(image.end(), prog.named.begin(), prog.named.end());
    image.insert(image.end(), prog.inits.begin(), prog.inits.end());
    DevBuf<uint32_t> d_image(&ctx, image.size());
    h2d(ctx, d_image.p, image.data(), image.size() * 4);
    // scratch: 4 bytes per row and one more word for the starts, 8 per block, 16 for what the host reads
    DevBuf<uint32_t> starts(&ctx, (size_t)src.height + 1);
    DevBuf<uint32_t> per_block(&ctx, 2 * (size_t)d.n_blocks);  // counts -> offsets, then lasts -> prevs
    DevBuf<uint64_t> tail(&ctx, 2);
    uint32_t* offsets = per_block.p;
    uint32_t* prevs = per_block.p + d.n_blocks;

    const dim3 block(ITER_THREADS);
    TS_LAUNCH(ctx, k_iterate_count, dim3(d.n_blocks), block, 0, d, offsets, prevs);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_iterate_offsets, dim3(1), block, 0, d, offsets, prevs, tail.p);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_iterate_starts, dim3(d.n_blocks), block, 0, d, (const uint32_t*)offsets, (const uint32_t*)prevs,
              starts.p, tail.p);
    TS_HIP(hipGetLastError());
    uint64_t seen[2] = {0, 0};
    d2h_sync(ctx, seen, tail.p, sizeof(seen));  // the call's one wait
    IterateLong bad;
    if (seen[1] != ~0ull) {
        bad.start = seen[1] >> 32;
        bad.rows = seen[1] & 0xFFFFFFFFu;
    }
    iterate_refuse_long(prog, bad);  // throws: the buffers above go back to the pool, the walk is never launched
    const uint32_t n_groups = (uint32_t)seen[0];

    DeviceMatrix out;
    out.buf = DevBuf<uint32_t>(&ctx, (size_t)src.height * prog.out_width);
    out.height = src.height;
    out.width = prog.out_width;
    out.layout = DeviceMatrix::ROW_MAJOR;
    const size_t lds = (size_t)prog.n_live * ITER_WALK_THREADS * 4;  // <= 12 KiB
    const uint32_t* img = d_image.p;
    TS_LAUNCH(ctx, k_iterate_walk, dim3((n_groups + ITER_WALK_THREADS - 1) / ITER_WALK_THREADS), dim3(ITER_WALK_THREADS), lds,
              (const uint4*)img, img + prog.code.size(), img + prog.code.size() + prog.named.size(), d,
              (const uint32_t*)starts.p, n_groups, out.buf.p);
    TS_HIP(hipGetLastError());
    return out;
}

}  // namespace ts
