// Expanded rows in HBM: every row of one resident row-major matrix repeated by a count read from the row itself, each
// copy reshaped to one tuple form, in (row, inner index) order, padded to its height (expand.hpp, include/tapstark.h
// "expanded rows").  The inverse of collect.hip: a load-balanced expansion.
//
// Three plain launches, the reduce-then-scan shape of collect.hip: no grid barrier, no flag another workgroup waits
// for, no look-back; nothing spins on another workgroup.
//   k_expand_count    one workgroup per block of at most TS_EXPAND_BLOCK_ROWS source rows, a lane owns rpt =
//                     ceil(block_rows / 256) <= 4 consecutive rows.  Reads the selector and count columns only.  The
//                     exclusive scan of the counts over the block, shuffles inside a wave, LDS across the four waves ->
//                     pos[row], the row's position inside its block; the block's sum -> sums[block]; the least row of
//                     the block over max_count and its count -> bad_row[block], bad_cnt[block].
//   k_expand_offsets  one workgroup: the exclusive scan of the block sums, 256 per trip, in place -> offsets[block];
//                     behind them the total, the least offending row of all and its count.  The host reads those three
//                     words in one copy, the call's only wait: they size the result and decide both refusals.
//   k_expand_write    the grid is partitioned by OUTPUT rows: a workgroup owns a tile of at most
//                     min(TS_EXPAND_BLOCK_ROWS, 1024) consecutive output rows, so one source row asking for 2^22 rows
//                     costs what 2^22 rows asking for one do.  The source row of output row o is the LARGEST r whose
//                     exclusive offset is <= o (a row asking for nothing shares its offset with a later row and loses):
//                     the workgroup finds the blocks of its first and last output row by binary search over offsets;
//                     when they are one block its pos[] are staged in LDS and every lane searches there, else every
//                     lane searches offsets between the two blocks and then pos[] of its block in HBM.  Runs of rows
//                     asking for nothing cost that search, not a walk.  Each lane leaves (r, j, cnt) of its output rows
//                     in LDS; the tile is then ONE contiguous word range of the result, walked with consecutive lanes on
//                     consecutive words: word -> (row, column) -> term (expand_term).  Coalesced writes, gathered reads
//                     in the source rows, the term table in LDS.  The workgroups behind the tiles fill rows
//                     [n_live, height) with the pad row, tile by tile.
// Every result word is written exactly once and nothing reads the result.
// Widths of the sums.  64-bit: a lane's sum, the in-block scan and so sums[block]; the carry and offsets[]; the total
// (exact for 2^27 rows of any count below p: less than 2^58); row * width and every offset into the result.  32-bit:
// pos[row], the low word of the 64-bit in-block scan.  It wraps only where a block asks for 2^32 rows or more; the total
// is then above 2^27 and the call is refused after the wait, before anything reads pos[].  In an accepted call the total
// is at most 2^27, so every pos[] and every (o - offsets[block]) is exact in 32 bits; also 32-bit are a word index
// inside one tile (< 1024 * 64) or one pad tile, and a row index (< 2^27).
#include <string>

#include "expand.hpp"
#include "logup_dev.hpp"  // mult_knob
#include "prover_internal.hpp"

namespace ts {

constexpr int EXPAND_THREADS = 256;
constexpr int EXPAND_RPT = 4;  // rows per lane at most: a workgroup owns up to 1024 source rows or output rows
constexpr int EXPAND_WAVES = EXPAND_THREADS / 64;
constexpr uint32_t EXPAND_MAX_BLOCK_ROWS = EXPAND_THREADS * EXPAND_RPT;
constexpr uint32_t EXPAND_PAD_TILE_ROWS = 256;
constexpr uint32_t EXPAND_PAD_BLOCKS = 1024;
constexpr uint32_t EXPAND_NONE = 0xFFFFFFFFu;  // bad_row[]: no row of the block is over max_count
// the image the device reads: the pad row, then out_width terms of three words
constexpr uint32_t EXPAND_IMG_TERMS = EXPAND_MAX_WIDTH;

struct ExpandDev {
    const uint32_t* src;
    uint64_t height;
    uint32_t width, out_width, sel, count_col, count_const, max_count;
    uint32_t block_rows, rpt, n_blocks, tile_rows;
};

__device__ __forceinline__ uint64_t expand_shfl_up(uint64_t v, unsigned d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return (uint64_t)hi << 32 | lo;
}

// Over the workgroup's lanes in lane order: the sum of v over the lanes BEFORE this one; total <- over all lanes.
// Wave-64 shuffles inside a wave, LDS across the waves; 64-bit throughout.  Every thread calls it.
__device__ __forceinline__ uint64_t expand_block_scan(uint64_t v, uint64_t (&wave_sums)[EXPAND_WAVES], uint64_t& total) {
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const uint64_t up = expand_shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    __syncthreads();  // (a second call reuses wave_sums)
    if (lane == 63) wave_sums[wv] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < EXPAND_WAVES; k++) {
        const uint64_t w = wave_sums[k];
        if (k < (int)wv) before += w;
        all += w;
    }
    total = all;
    return before + inc - v;
}

// The largest b in [lo, hi) with offsets[b] <= o, given offsets[lo] <= o: blocks asking for nothing share their offset
// with a later block and lose.
__device__ __forceinline__ uint32_t expand_find_block(const uint64_t* __restrict__ offsets, uint32_t lo, uint32_t hi,
                                                      uint64_t o) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= o) lo = mid; else hi = mid;
    }
    return lo;
}

// The largest l in [0, n) with pos[l] <= rel, given pos[0] == 0.
__device__ __forceinline__ uint32_t expand_find_row(const uint32_t* pos, uint32_t n, uint32_t rel) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pos[mid] <= rel) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(EXPAND_THREADS)
k_expand_count(const ExpandDev d, uint32_t* __restrict__ pos, uint64_t* __restrict__ sums, uint32_t* __restrict__ bad_row,
               uint32_t* __restrict__ bad_cnt) {
    __shared__ uint64_t wave_sums[EXPAND_WAVES];
    __shared__ uint32_t least_bad;
    const uint64_t base = (uint64_t)blockIdx.x * d.block_rows;
    const uint64_t left = d.height - base;  // >= 1: the grid holds ceil(height / block_rows) blocks
    const uint32_t rows = left < d.block_rows ? (uint32_t)left : d.block_rows;
    if (threadIdx.x == 0) least_bad = EXPAND_NONE;  // (the scan's barriers stand before its first use)

    uint32_t cnt[EXPAND_RPT];
    uint64_t mine = 0;
    uint32_t my_bad = EXPAND_NONE, my_bad_cnt = 0;
#pragma unroll
    for (int k = 0; k < EXPAND_RPT; k++) {
        const uint32_t local = threadIdx.x * d.rpt + k;
        cnt[k] = 0;
        if (k < (int)d.rpt && local < rows) {
            cnt[k] = expand_row_count(d.src + (base + local) * d.width, d.sel, d.count_col, d.count_const);
            if (cnt[k] > d.max_count && my_bad == EXPAND_NONE) {
                my_bad = local;
                my_bad_cnt = cnt[k];
            }
            mine += cnt[k];
        }
    }
    uint64_t total;
    uint64_t at = expand_block_scan(mine, wave_sums, total);
#pragma unroll
    for (int k = 0; k < EXPAND_RPT; k++) {
        const uint32_t local = threadIdx.x * d.rpt + k;
        if (k < (int)d.rpt && local < rows) pos[base + local] = (uint32_t)at;  // (the low word: see the header)
        at += cnt[k];
    }
    if (my_bad != EXPAND_NONE) atomicMin(&least_bad, my_bad);
    __syncthreads();
    if (my_bad != EXPAND_NONE && least_bad == my_bad) {  // one lane: a local row has one owner
        bad_row[blockIdx.x] = (uint32_t)(base + my_bad);  // < 2^27
        bad_cnt[blockIdx.x] = my_bad_cnt;
    }
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = total;
        if (least_bad == EXPAND_NONE) {
            bad_row[blockIdx.x] = EXPAND_NONE;
            bad_cnt[blockIdx.x] = 0;
        }
    }
}

// In place: offsets[b] <- sums[0] + ... + sums[b-1], b < n_blocks; offsets[n_blocks] <- the sum of all;
// offsets[n_blocks + 1] <- the least row over max_count (~0: none), offsets[n_blocks + 2] <- its count.
__global__ void __launch_bounds__(EXPAND_THREADS)
k_expand_offsets(uint64_t* __restrict__ offsets, uint32_t n_blocks, const uint32_t* __restrict__ bad_row,
                 const uint32_t* __restrict__ bad_cnt) {
    __shared__ uint64_t wave_sums[EXPAND_WAVES];
    __shared__ uint32_t least_bad;
    if (threadIdx.x == 0) least_bad = EXPAND_NONE;
    uint64_t carry = 0;
    uint32_t my_bad = EXPAND_NONE, my_bad_cnt = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += EXPAND_THREADS) {  // (uniform bounds: every thread loops alike)
        const uint32_t b = b0 + threadIdx.x;
        uint64_t pass;
        const uint64_t before = expand_block_scan(b < n_blocks ? offsets[b] : 0ull, wave_sums, pass);
        if (b < n_blocks) {
            offsets[b] = carry + before;  // (this lane alone read and writes word b)
            if (bad_row[b] < my_bad) {    // blocks ascend, so the first hit is the lane's least
                my_bad = bad_row[b];
                my_bad_cnt = bad_cnt[b];
            }
        }
        carry += pass;
    }
    __syncthreads();  // (n_blocks >= 1, but least_bad's store must not depend on the loop)
    if (my_bad != EXPAND_NONE) atomicMin(&least_bad, my_bad);
    __syncthreads();
    if (my_bad != EXPAND_NONE && least_bad == my_bad) offsets[n_blocks + 2] = my_bad_cnt;  // a row lies in one block
    if (threadIdx.x == 0) {
        offsets[n_blocks] = carry;
        offsets[n_blocks + 1] = least_bad == EXPAND_NONE ? ~0ull : (uint64_t)least_bad;
        if (least_bad == EXPAND_NONE) offsets[n_blocks + 2] = 0;
    }
}

__global__ void __launch_bounds__(EXPAND_THREADS)
k_expand_write(const ExpandDev d, const uint32_t* __restrict__ image, const uint32_t* __restrict__ pos,
               const uint64_t* __restrict__ offsets, uint64_t n_live, uint64_t height, uint32_t n_tiles,
               uint32_t* __restrict__ out) {
    __shared__ uint32_t s_pos[EXPAND_MAX_BLOCK_ROWS];  // pos[] of the one block a tile lies in
    __shared__ uint32_t s_row[EXPAND_MAX_BLOCK_ROWS], s_inner[EXPAND_MAX_BLOCK_ROWS], s_cnt[EXPAND_MAX_BLOCK_ROWS];
    __shared__ ExpandTermWord terms[EXPAND_MAX_WIDTH];
    const uint32_t W = d.out_width;

    if (blockIdx.x >= n_tiles) {  // the pad rows: tiles of 256 rows, dealt round to the workgroups behind the tiles
        const uint64_t n_pad = height - n_live;
        const uint64_t n_pad_tiles = (n_pad + EXPAND_PAD_TILE_ROWS - 1) / EXPAND_PAD_TILE_ROWS;
        for (uint64_t t = blockIdx.x - n_tiles; t < n_pad_tiles; t += gridDim.x - n_tiles) {
            const uint64_t r0 = t * EXPAND_PAD_TILE_ROWS, left = n_pad - r0;
            const uint32_t words = (left < EXPAND_PAD_TILE_ROWS ? (uint32_t)left : EXPAND_PAD_TILE_ROWS) * W;
            uint32_t* o = out + (n_live + r0) * W;
            for (uint32_t i = threadIdx.x; i < words; i += EXPAND_THREADS) o[i] = image[i % W];
        }
        return;
    }

    const uint64_t o0 = (uint64_t)blockIdx.x * d.tile_rows;
    const uint64_t left = n_live - o0;  // >= 1: the grid holds ceil(n_live / tile_rows) tiles
    const uint32_t rows = left < d.tile_rows ? (uint32_t)left : d.tile_rows;
    const ExpandTermWord* table = reinterpret_cast<const ExpandTermWord*>(image + EXPAND_IMG_TERMS);
    for (uint32_t i = threadIdx.x; i < W; i += EXPAND_THREADS) terms[i] = table[i];

    // (uniform: every lane makes the same two searches)
    const uint32_t b_first = expand_find_block(offsets, 0, d.n_blocks, o0);
    const uint32_t b_last = expand_find_block(offsets, b_first, d.n_blocks, o0 + rows - 1);
    const bool one_block = b_first == b_last;
    if (one_block) {
        const uint64_t base = (uint64_t)b_first * d.block_rows, in_block = d.height - base;
        const uint32_t n = in_block < d.block_rows ? (uint32_t)in_block : d.block_rows;
        for (uint32_t l = threadIdx.x; l < n; l += EXPAND_THREADS) s_pos[l] = pos[base + l];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < rows; i += EXPAND_THREADS) {
        const uint64_t o = o0 + i;
        const uint32_t b = one_block ? b_first : expand_find_block(offsets, b_first, b_last + 1, o);
        const uint64_t base = (uint64_t)b * d.block_rows, in_block = d.height - base;
        const uint32_t n = in_block < d.block_rows ? (uint32_t)in_block : d.block_rows;
        const uint32_t rel = (uint32_t)(o - offsets[b]);  // < the block's sum <= 2^27
        const uint32_t* p = one_block ? s_pos : pos + base;
        const uint32_t l = expand_find_row(p, n, rel);
        const uint64_t r = base + l;
        s_row[i] = (uint32_t)r;
        s_inner[i] = rel - p[l];
        s_cnt[i] = expand_row_count(d.src + r * d.width, d.sel, d.count_col, d.count_const);
    }
    __syncthreads();

    const uint32_t words = rows * W;  // <= 2^10 * 2^6
    uint32_t* o = out + o0 * W;
    for (uint32_t i = threadIdx.x; i < words; i += EXPAND_THREADS) {
        const uint32_t entry = i / W, c = i - entry * W;
        const uint64_t r = s_row[entry];
        o[i] = expand_term(terms[c], d.src + r * d.width, r, s_inner[entry], s_cnt[entry]);
    }
}

DeviceMatrix expand_matrix(Context& ctx, const ExpandPlan& plan, const DeviceMatrix& src, uint64_t out_height,
                           uint64_t* n_live_out) {
    StageTimer timer(&ctx, "expand");
    require_resident(ctx, src, "expand", "the source");
    TS_REQUIRE(src.width == plan.src_width, TS_ERR_INVALID,
               "expand: the spec is written for a source of " + std::to_string(plan.src_width) +
                   " columns, this one has " + std::to_string(src.width));
    expand_check_out_height(out_height);
    // TS_EXPAND_BLOCK_ROWS (1 .. 1024, read on every call): the source rows of a count block and the output rows of a
    // write tile at most, a test knob that makes small matrices cross the lane, the wave, the workgroup, several trips of
    // the offsets loop and tiles that straddle blocks.  No output word depends on it.
    const uint32_t knob = (uint32_t)mult_knob("TS_EXPAND_BLOCK_ROWS", 1, EXPAND_MAX_BLOCK_ROWS, EXPAND_MAX_BLOCK_ROWS);

    ExpandDev d = {};
    d.src = src.buf.p;
    d.height = src.height;
    d.width = src.width;
    d.out_width = plan.out_width;
    d.sel = plan.sel;
    d.count_col = plan.count_col;
    d.count_const = plan.count_const;
    d.max_count = plan.max_count;
    d.block_rows = d.tile_rows = knob;
    d.rpt = (knob + EXPAND_THREADS - 1) / EXPAND_THREADS;
    const uint64_t n_blocks = (src.height + knob - 1) / knob;
    // (a launch takes fewer than 2^32 threads; only the knob can ask for more)
    const char* too_small = "expand: TS_EXPAND_BLOCK_ROWS is too small for a source or a result of this height";
    TS_REQUIRE(n_blocks + EXPAND_PAD_BLOCKS < (1ull << 24), TS_ERR_INVALID, too_small);
    d.n_blocks = (uint32_t)n_blocks;

    // pad row and term table in one upload through the context's page-locked arena: no wait of its own
    std::vector<uint32_t> image(EXPAND_IMG_TERMS + 3 * plan.terms.size(), 0);
    for (uint32_t c = 0; c < plan.out_width; c++) {
        image[c] = plan.pad[c];
        image[EXPAND_IMG_TERMS + 3 * c] = plan.terms[c].kind;
        image[EXPAND_IMG_TERMS + 3 * c + 1] = plan.terms[c].value;
        image[EXPAND_IMG_TERMS + 3 * c + 2] = plan.terms[c].step;
    }
    DevBuf<uint32_t> d_image(&ctx, image.size());
    h2d(ctx, d_image.p, image.data(), image.size() * 4);
    // scratch: 4 bytes per source row, 16 per block, 24 for what the host reads
    DevBuf<uint32_t> pos(&ctx, (size_t)src.height);
    DevBuf<uint64_t> offsets(&ctx, (size_t)d.n_blocks + 3);
    DevBuf<uint32_t> bad(&ctx, 2 * (size_t)d.n_blocks);  // bad_row[], then bad_cnt[]

    const dim3 block(EXPAND_THREADS);
    TS_LAUNCH(ctx, k_expand_count, dim3(d.n_blocks), block, 0, d, pos.p, offsets.p, bad.p, bad.p + d.n_blocks);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_expand_offsets, dim3(1), block, 0, offsets.p, d.n_blocks, (const uint32_t*)bad.p,
              (const uint32_t*)(bad.p + d.n_blocks));
    TS_HIP(hipGetLastError());
    uint64_t tail[3] = {0, 0, 0};
    d2h_sync(ctx, tail, offsets.p + d.n_blocks, sizeof(tail));  // the call's one wait
    ExpandTotals totals;
    totals.total = tail[0];
    totals.bad_row = tail[1];
    totals.bad_count = tail[2];
    const uint64_t height = expand_height(plan, totals, out_height);  // throws: the buffers above go back to the pool
    const uint64_t n_live = totals.total;
    const uint64_t n_tiles = (n_live + d.tile_rows - 1) / d.tile_rows;
    TS_REQUIRE(n_tiles + EXPAND_PAD_BLOCKS < (1ull << 24), TS_ERR_INVALID, too_small);

    DeviceMatrix out;
    out.buf = DevBuf<uint32_t>(&ctx, (size_t)height * plan.out_width);
    out.height = height;
    out.width = plan.out_width;
    out.layout = DeviceMatrix::ROW_MAJOR;
    const uint64_t pad_tiles = (height - n_live + EXPAND_PAD_TILE_ROWS - 1) / EXPAND_PAD_TILE_ROWS;
    const uint32_t pad_blocks = (uint32_t)(pad_tiles < EXPAND_PAD_BLOCKS ? pad_tiles : EXPAND_PAD_BLOCKS);
    TS_LAUNCH(ctx, k_expand_write, dim3((uint32_t)n_tiles + pad_blocks), block, 0, d, (const uint32_t*)d_image.p,
              (const uint32_t*)pos.p, (const uint64_t*)offsets.p, n_live, height, (uint32_t)n_tiles, out.buf.p);
    TS_HIP(hipGetLastError());
    if (n_live_out) *n_live_out = n_live;
    return out;
}

}  // namespace ts
