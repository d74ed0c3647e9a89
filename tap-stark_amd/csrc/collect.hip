// Collected rows in HBM: the rows the emitters of a spec select from up to four resident row-major matrices, written
// as one new matrix in (source, row, emitter) order and padded to its height (collect.hpp, include/tapstark.h
// "collected rows").  A stream compaction, so the only call here whose output has another height than its source.
//
// Three plain launches, the reduce-then-scan shape of scan.hip and logup.hip: no grid barrier, no flag another
// workgroup waits for, no look-back.  The blocks of all sources form ONE job grid: source s owns the block numbers
// [first_block[s], first_block[s+1]), a block is block_rows[s] = min(TS_COLLECT_BLOCK_ROWS, 4096 / E_s) consecutive rows
// of that one source (E_s: its emitters), so it never straddles two sources and never fires more than 4096 times.  A
// lane owns rpt = ceil(block_rows / 256) <= 4 consecutive rows of the block; what fired there is one 64-bit mask, bit
// 16 k + e for emitter e (in the source's spec order) on the lane's k-th row: ascending bits are the order rule.
//   k_collect_count    per block: the lanes' popcounts summed, shuffles inside a wave, LDS across the four waves ->
//                      counts[block].  Reads the selector columns only.
//   k_collect_offsets  one workgroup: the exclusive scan of counts, 256 per trip, the carry in 64 bits ->
//                      offsets[block] and, behind them, the total.  The host reads the total in one copy, the call's
//                      only wait: it sizes the result and decides the overflow refusal.
//   k_collect_write    the job grid again: masks and in-block scan redone; each lane lists its fired (local row,
//                      emitter) pairs in LDS at their in-block position.  The block's rows are then ONE contiguous
//                      word range of the result, walked with consecutive lanes on consecutive words: word -> (entry,
//                      column) -> term -> a constant, the source word as stored, or the row index.  Coalesced writes,
//                      gathered reads inside the block's own rows.  The source's term table sits in LDS.
//                      The workgroups behind the job grid fill rows [n_live, height) with the pad row, tile by tile.
// Every result word is written exactly once and nothing reads the result.  Addressing: row * width and every offset
// into the result are 64-bit; what is 32-bit is an index inside one block (< 4096 * 64 words) or one pad tile.
#include <string>

#include "collect.hpp"
#include "collect_dev.hpp"  // the block scan, shared with group.hip
#include "logup_dev.hpp"  // mult_knob
#include "prover_internal.hpp"

namespace ts {

// the image the device reads: selectors, pad row, then out_width terms per emitter (grouped by source)
constexpr uint32_t COLLECT_IMG_PAD = COLLECT_MAX_EMITTERS;
constexpr uint32_t COLLECT_IMG_TERMS = COLLECT_IMG_PAD + COLLECT_MAX_WIDTH;

struct CollectDev {
    uint32_t n_sources, out_width, n_blocks, pad0;
    struct Src {
        const uint32_t* p;
        uint64_t height;
        uint32_t width, block_rows, rpt, first_block, first_emitter, n_emitters;
    } src[COLLECT_MAX_SOURCES];
};

// The block a workgroup owns.
struct CollectJob {
    const uint32_t* p;
    uint64_t base;  // its first row
    uint32_t width, rpt, tile_rows, first_emitter, n_emitters;
};

// The sources' block ranges ascend, so the last source whose range starts at or below b owns it.  Unrolled with
// selects: the launch arguments are never indexed by a variable.
__device__ __forceinline__ CollectJob collect_job(const CollectDev& d, uint32_t b) {
    CollectJob j = {};
    uint64_t height = 0;
    uint32_t block_rows = 0, first_block = 0;
#pragma unroll
    for (int s = 0; s < (int)COLLECT_MAX_SOURCES; s++)
        if (s < (int)d.n_sources && b >= d.src[s].first_block) {
            const CollectDev::Src& q = d.src[s];
            j.p = q.p;
            j.width = q.width;
            j.rpt = q.rpt;
            j.first_emitter = q.first_emitter;
            j.n_emitters = q.n_emitters;
            height = q.height;
            block_rows = q.block_rows;
            first_block = q.first_block;
        }
    j.base = (uint64_t)(b - first_block) * block_rows;
    const uint64_t left = height - j.base;  // >= 1: the grid holds ceil(height / block_rows) blocks of the source
    j.tile_rows = left < block_rows ? (uint32_t)left : block_rows;
    return j;
}

// What fired on this lane's rows: bit 16 k + e for emitter e on its k-th row.
__device__ __forceinline__ uint64_t collect_lane_mask(const CollectJob& j, const uint32_t* __restrict__ sel) {
    uint64_t mask = 0;
#pragma unroll
    for (int k = 0; k < COLLECT_RPT; k++) {
        const uint32_t local = threadIdx.x * j.rpt + k;
        if (k < (int)j.rpt && local < j.tile_rows) {
            const uint32_t* row = j.p + (j.base + local) * j.width;
            for (uint32_t e = 0; e < j.n_emitters; e++) {  // (uniform bounds and a uniform selector: a scalar load)
                const uint32_t c = sel[j.first_emitter + e];
                const bool fired = c == COLLECT_ALWAYS || collect_fires(row[c]);
                mask |= (uint64_t)fired << (16 * k + e);
            }
        }
    }
    return mask;
}

__global__ void __launch_bounds__(COLLECT_THREADS)
k_collect_count(const CollectDev d, const uint32_t* __restrict__ image, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wave_sums[COLLECT_WAVES];
    const CollectJob j = collect_job(d, blockIdx.x);
    uint32_t total;
    collect_block_scan((uint32_t)__popcll(collect_lane_mask(j, image)), wave_sums, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;  // <= 4096
}

// offsets[b] <- counts[0] + ... + counts[b-1], b < n_blocks; offsets[n_blocks] <- the sum of all
__global__ void __launch_bounds__(COLLECT_THREADS)
k_collect_offsets(const uint32_t* __restrict__ counts, uint32_t n_blocks, uint64_t* __restrict__ offsets) {
    __shared__ uint32_t wave_sums[COLLECT_WAVES];
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += COLLECT_THREADS) {  // (uniform bounds: every thread loops alike)
        const uint32_t b = b0 + threadIdx.x;
        uint32_t pass;  // <= 256 * 4096
        const uint32_t before = collect_block_scan(b < n_blocks ? counts[b] : 0u, wave_sums, pass);
        if (b < n_blocks) offsets[b] = carry + before;
        carry += pass;
    }
    if (threadIdx.x == 0) offsets[n_blocks] = carry;
}

__global__ void __launch_bounds__(COLLECT_THREADS)
k_collect_write(const CollectDev d, const uint32_t* __restrict__ image, const uint64_t* __restrict__ offsets,
                uint64_t n_live, uint64_t height, uint32_t* __restrict__ out) {
    __shared__ uint16_t list[COLLECT_MAX_ENTRIES];  // local row << 4 | emitter, in output order
    __shared__ CollectTermWord terms[COLLECT_MAX_EMITTERS * COLLECT_MAX_WIDTH];
    __shared__ uint32_t wave_sums[COLLECT_WAVES];
    const uint32_t W = d.out_width;

    if (blockIdx.x >= d.n_blocks) {  // the pad rows: tiles of 256 rows, dealt round to the workgroups behind the job grid
        const uint32_t* pad = image + COLLECT_IMG_PAD;
        const uint64_t n_pad = height - n_live;
        const uint64_t n_tiles = (n_pad + COLLECT_PAD_TILE_ROWS - 1) / COLLECT_PAD_TILE_ROWS;
        for (uint64_t t = blockIdx.x - d.n_blocks; t < n_tiles; t += gridDim.x - d.n_blocks) {
            const uint64_t r0 = t * COLLECT_PAD_TILE_ROWS, left = n_pad - r0;
            const uint32_t words = (left < COLLECT_PAD_TILE_ROWS ? (uint32_t)left : COLLECT_PAD_TILE_ROWS) * W;
            uint32_t* o = out + (n_live + r0) * W;
            for (uint32_t i = threadIdx.x; i < words; i += COLLECT_THREADS) o[i] = pad[i % W];
        }
        return;
    }

    const CollectJob j = collect_job(d, blockIdx.x);
    const uint64_t mask = collect_lane_mask(j, image);
    uint32_t total;
    uint32_t at = collect_block_scan((uint32_t)__popcll(mask), wave_sums, total);
    if (total == 0) return;  // (uniform)

    const CollectTermWord* mine = reinterpret_cast<const CollectTermWord*>(image + COLLECT_IMG_TERMS) + j.first_emitter * W;
    for (uint32_t i = threadIdx.x; i < j.n_emitters * W; i += COLLECT_THREADS) terms[i] = mine[i];
    for (uint64_t m = mask; m; m &= m - 1) {  // ascending bits: row after row, emitter after emitter
        const uint32_t bit = (uint32_t)__ffsll((long long)m) - 1;
        list[at++] = (uint16_t)((threadIdx.x * j.rpt + (bit >> 4)) << 4 | (bit & 15));  // at < total <= 4096
    }
    __syncthreads();

    const uint32_t words = total * W;  // <= 2^12 * 2^6
    uint32_t* o = out + offsets[blockIdx.x] * W;
    for (uint32_t i = threadIdx.x; i < words; i += COLLECT_THREADS) {
        const uint32_t entry = i / W, c = i - entry * W;
        const uint32_t en = list[entry], local = en >> 4;
        const CollectTermWord t = terms[(en & 15) * W + c];
        const uint64_t row = j.base + local;
        o[i] = t.kind == C_CONST ? t.value : t.kind == C_COL ? j.p[row * j.width + t.value] : (uint32_t)row;
    }
}

void collect_launch_offsets(Context& ctx, const uint32_t* counts, uint32_t n_blocks, uint64_t* offsets) {
    TS_LAUNCH(ctx, k_collect_offsets, dim3(1), dim3(COLLECT_THREADS), 0, counts, n_blocks, offsets);
    TS_HIP(hipGetLastError());
}

DeviceMatrix collect_matrix(Context& ctx, const CollectPlan& plan, const DeviceMatrix* const* sources,
                            uint64_t out_height, uint64_t* n_live_out) {
    StageTimer timer(&ctx, "collect");
    for (uint32_t s = 0; s < plan.n_sources; s++) {
        const std::string what = "source " + std::to_string(s);
        require_resident(ctx, *sources[s], "collect", what.c_str());
        TS_REQUIRE(sources[s]->width == plan.src_width[s], TS_ERR_INVALID,
                   "collect: the spec is written for a " + what + " of " + std::to_string(plan.src_width[s]) +
                       " columns, this one has " + std::to_string(sources[s]->width));
    }
    collect_check_out_height(out_height);
    // TS_COLLECT_BLOCK_ROWS (1 .. 1024, read on every call): the rows one workgroup owns at most, a test knob that makes
    // small matrices cross the wave, the workgroup and several trips of the offsets loop.  No output word depends on it.
    const uint32_t knob =
        (uint32_t)mult_knob("TS_COLLECT_BLOCK_ROWS", 1, COLLECT_THREADS * COLLECT_RPT, COLLECT_THREADS * COLLECT_RPT);

    CollectDev d = {};
    d.n_sources = plan.n_sources;
    d.out_width = plan.out_width;
    uint64_t n_blocks = 0;
    for (uint32_t s = 0; s < plan.n_sources; s++) {
        CollectDev::Src& q = d.src[s];
        q.p = sources[s]->buf.p;
        q.height = sources[s]->height;
        q.width = sources[s]->width;
        q.first_emitter = plan.first_emitter[s];
        q.n_emitters = plan.first_emitter[s + 1] - plan.first_emitter[s];
        const uint32_t cap = q.n_emitters ? COLLECT_MAX_ENTRIES / q.n_emitters : COLLECT_MAX_ENTRIES;  // >= 256
        q.block_rows = knob < cap ? knob : cap;
        q.rpt = (q.block_rows + COLLECT_THREADS - 1) / COLLECT_THREADS;
        q.first_block = (uint32_t)n_blocks;
        if (q.n_emitters) n_blocks += (q.height + q.block_rows - 1) / q.block_rows;  // a source nothing reads has no blocks
    }
    // (a launch takes fewer than 2^32 threads; only the knob can ask for more)
    TS_REQUIRE(n_blocks + COLLECT_PAD_BLOCKS < (1ull << 24), TS_ERR_INVALID,
               "collect: TS_COLLECT_BLOCK_ROWS is too small for sources of these heights");
    d.n_blocks = (uint32_t)n_blocks;

    // selectors, pad row and term table in one upload through the context's page-locked arena: no wait of its own
    std::vector<uint32_t> image(COLLECT_IMG_TERMS + 2 * plan.terms.size(), 0);
    for (size_t e = 0; e < plan.sel.size(); e++) image[e] = plan.sel[e];
    for (uint32_t c = 0; c < plan.out_width; c++) image[COLLECT_IMG_PAD + c] = plan.pad[c];
    for (size_t i = 0; i < plan.terms.size(); i++) {
        image[COLLECT_IMG_TERMS + 2 * i] = plan.terms[i].kind;
        image[COLLECT_IMG_TERMS + 2 * i + 1] = plan.terms[i].value;
    }
    DevBuf<uint32_t> d_image(&ctx, image.size());
    h2d(ctx, d_image.p, image.data(), image.size() * 4);
    DevBuf<uint32_t> counts(&ctx, d.n_blocks);
    DevBuf<uint64_t> offsets(&ctx, (size_t)d.n_blocks + 1);  // and the total behind them

    const dim3 block(COLLECT_THREADS);
    TS_LAUNCH(ctx, k_collect_count, dim3(d.n_blocks), block, 0, d, (const uint32_t*)d_image.p, counts.p);
    TS_HIP(hipGetLastError());
    collect_launch_offsets(ctx, counts.p, d.n_blocks, offsets.p);
    uint64_t n_live = 0;
    d2h_sync(ctx, &n_live, offsets.p + d.n_blocks, sizeof(n_live));  // the call's one wait
    const uint64_t height = collect_height(n_live, out_height);  // throws: the buffers above go back to the pool

    DeviceMatrix out;
    out.buf = DevBuf<uint32_t>(&ctx, (size_t)height * plan.out_width);
    out.height = height;
    out.width = plan.out_width;
    out.layout = DeviceMatrix::ROW_MAJOR;
    const uint64_t pad_tiles = (height - n_live + COLLECT_PAD_TILE_ROWS - 1) / COLLECT_PAD_TILE_ROWS;
    const uint32_t pad_blocks = (uint32_t)(pad_tiles < COLLECT_PAD_BLOCKS ? pad_tiles : COLLECT_PAD_BLOCKS);
    TS_LAUNCH(ctx, k_collect_write, dim3(d.n_blocks + pad_blocks), block, 0, d, (const uint32_t*)d_image.p,
              (const uint64_t*)offsets.p, n_live, height, out.buf.p);
    TS_HIP(hipGetLastError());
    if (n_live_out) *n_live_out = n_live;
    return out;
}

}  // namespace ts
