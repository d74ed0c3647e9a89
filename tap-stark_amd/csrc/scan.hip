// Scanned trace columns in HBM: up to SCAN_MAX_COLUMNS recurrences y[i] = a[i] y[i-1] + b[i] down the rows of a resident
// row-major matrix, all in one pass over the rows (scan.hpp has the operator on the maps x -> a x + b).
//
// Three plain launches, the reduce-then-scan shape of logup.hip: no grid barrier and no flag another workgroup waits
// for.  A workgroup owns block_rows consecutive rows (TS_SCAN_BLOCK_ROWS, 1024 unless a test says otherwise), a lane
// rpt = ceil(block_rows / 256) consecutive rows of them.
//   k_scan_reduce  a lane composes the maps of its rows, for every scan at once: (A, B) per scan in VGPRs, Montgomery
//                  form from the load on (to_mont of a stored word also reduces it).  A wave scan over 64 lanes with
//                  shuffles and an LDS step across the four waves give the workgroup's map -> totals[block][scan].
//                  Reads only the a, b and reset columns the scans name.
//   k_scan_totals  one workgroup: the exclusive scan of the block maps, 256 per trip of its loop with the map of the
//                  trips before carried along; applied to init -> state_in[block][scan], the value of y before the
//                  block's first row, a field element.  The map of all blocks applied to init is y[h-1] -> last[scan].
//   k_scan_apply   the same in-block scan again, exclusive, applied to state_in: y before the lane's first row.  Then one
//                  product and one add per row and scan give y; the dst word is y, or for an exclusive scan the state
//                  before the row (init on a reset row).  The untouched kept columns of the workgroup's rows are one
//                  contiguous range of the result, copied with consecutive lanes on consecutive words, a bit per column
//                  saying whether a scan owns it, as k_derive does.
// A reset row is the constant map (0, a init + b), so the operator has no branch for it.  Field arithmetic is exact and
// the composition associative, so the words are those of the sequential loop for every block_rows.  Every result word
// is written exactly once -- by the copy, or by the one scan whose dst it is -- and nothing reads the result.
// Addressing: row * width is 64-bit everywhere.
#include <string>

#include "logup_dev.hpp"  // mult_knob
#include "prover_internal.hpp"
#include "scan.hpp"

namespace ts {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_RPT = 4;  // rows per lane at most: a workgroup owns up to 1024 rows
constexpr int SCAN_WAVES = SCAN_THREADS / 64;
constexpr int SCAN_N = (int)SCAN_MAX_COLUMNS;

struct ScanDev {
    uint64_t height;
    uint32_t src_width, out_width, n, block_rows, rpt, pad;
    struct Col {
        uint32_t a_kind, a, b_kind, b;  // a constant is in Montgomery form, a column is its number
        uint32_t init_m, reset, dst, exclusive;
    } col[SCAN_N];
};

__device__ __forceinline__ ScanMap scan_shfl_up(ScanMap v, unsigned delta) {
    return ScanMap{(uint32_t)__shfl_up((int)v.a, delta, 64), (uint32_t)__shfl_up((int)v.b, delta, 64)};
}

__device__ __forceinline__ uint32_t scan_term(uint32_t kind, uint32_t val, const uint32_t* __restrict__ row) {
    return kind ? to_mont(row[val]) : val;
}
__device__ __forceinline__ bool scan_resets(const ScanDev::Col& c, const uint32_t* __restrict__ row) {
    return c.reset != SCAN_NO_RESET && to_mont(row[c.reset]) != 0;  // (the Montgomery form of 0 is 0)
}

// m[s] <- the composition of the maps of this lane's rows, the identity for a lane with none.  The loops over the
// scans are unrolled with a uniform guard, so m[] is indexed by constants and stays in registers.
__device__ __forceinline__ void scan_lane_maps(const ScanDev& d, const uint32_t* __restrict__ src, uint64_t base,
                                               ScanMap (&m)[SCAN_N]) {
#pragma unroll
    for (int s = 0; s < SCAN_N; s++) m[s] = scan_identity();
#pragma unroll
    for (int k = 0; k < SCAN_RPT; k++) {
        const uint32_t local = threadIdx.x * d.rpt + k;
        const uint64_t r = base + local;
        if (k < (int)d.rpt && local < d.block_rows && r < d.height) {
            const uint32_t* row = src + r * d.src_width;
#pragma unroll
            for (int s = 0; s < SCAN_N; s++)
                if (s < (int)d.n) {
                    const ScanDev::Col& c = d.col[s];
                    const ScanMap here = scan_row_map(scan_term(c.a_kind, c.a, row), scan_term(c.b_kind, c.b, row),
                                                      scan_resets(c, row), c.init_m);
                    m[s] = scan_compose(here, m[s]);
                }
        }
    }
}

// Over the workgroup's lanes in lane order, for n scans at once: v[s] <- the composition of the maps of the lanes
// BEFORE this one (exclusive; a map has no inverse, so it is the inclusive one of the lane below), total[s] <- that of
// all lanes.  Wave-64 shuffles inside a wave, LDS across the waves.  Every thread calls it.
__device__ __forceinline__ void scan_block_maps(uint32_t n, ScanMap (&v)[SCAN_N], ScanMap (&wave_maps)[SCAN_WAVES][SCAN_N],
                                                ScanMap (&total)[SCAN_N]) {
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < SCAN_N; s++)
        if (s < (int)n) {
#pragma unroll
            for (unsigned d = 1; d < 64; d <<= 1) {
                const ScanMap up = scan_shfl_up(v[s], d);
                if (lane >= d) v[s] = scan_compose(v[s], up);
            }
        }
    __syncthreads();  // (a second call reuses wave_maps)
    if (lane == 63) {
#pragma unroll
        for (int s = 0; s < SCAN_N; s++)
            if (s < (int)n) wave_maps[wv][s] = v[s];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SCAN_N; s++)
        if (s < (int)n) {
            ScanMap before = scan_identity(), all = scan_identity();
#pragma unroll
            for (int k = 0; k < SCAN_WAVES; k++) {
                const ScanMap w = wave_maps[k][s];
                if (k < (int)wv) before = scan_compose(w, before);
                all = scan_compose(w, all);
            }
            const ScanMap below = scan_shfl_up(v[s], 1);
            v[s] = lane == 0 ? before : scan_compose(below, before);
            total[s] = all;
        }
}

__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_reduce(const ScanDev d, const uint32_t* __restrict__ src, ScanMap* __restrict__ totals) {
    __shared__ ScanMap wave_maps[SCAN_WAVES][SCAN_N];
    ScanMap m[SCAN_N], total[SCAN_N];
    scan_lane_maps(d, src, (uint64_t)blockIdx.x * d.block_rows, m);
    scan_block_maps(d.n, m, wave_maps, total);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < SCAN_N; s++)
            if (s < (int)d.n) totals[(uint64_t)blockIdx.x * d.n + s] = total[s];
    }
}

// state_in[b][s] <- (totals[b-1] o ... o totals[0])(init_s), b < n_blocks; last[s] <- y[h-1], canonical
__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_totals(const ScanDev d, const ScanMap* __restrict__ totals, uint32_t n_blocks, uint32_t* __restrict__ state_in,
              uint32_t* __restrict__ last) {
    __shared__ ScanMap wave_maps[SCAN_WAVES][SCAN_N];
    ScanMap carry[SCAN_N], v[SCAN_N], pass[SCAN_N];
#pragma unroll
    for (int s = 0; s < SCAN_N; s++) carry[s] = scan_identity();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += SCAN_THREADS) {  // (uniform bounds: every thread loops alike)
        const uint32_t b = b0 + threadIdx.x;
#pragma unroll
        for (int s = 0; s < SCAN_N; s++)
            v[s] = s < (int)d.n && b < n_blocks ? totals[(uint64_t)b * d.n + s] : scan_identity();
        scan_block_maps(d.n, v, wave_maps, pass);
#pragma unroll
        for (int s = 0; s < SCAN_N; s++)
            if (s < (int)d.n) {
                if (b < n_blocks) state_in[(uint64_t)b * d.n + s] = scan_apply(scan_compose(v[s], carry[s]), d.col[s].init_m);
                carry[s] = scan_compose(pass[s], carry[s]);
            }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < SCAN_N; s++)
            if (s < (int)d.n) last[s] = from_mont(scan_apply(carry[s], d.col[s].init_m));
    }
}

__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_apply(const ScanDev d, const uint32_t* __restrict__ named, const uint32_t* __restrict__ src,
             const uint32_t* __restrict__ state_in, uint32_t* __restrict__ out) {
    __shared__ ScanMap wave_maps[SCAN_WAVES][SCAN_N];
    const uint64_t base = (uint64_t)blockIdx.x * d.block_rows;
    const uint64_t left = d.height - base;
    const uint32_t tile_rows = left < d.block_rows ? (uint32_t)left : d.block_rows;

    // the untouched kept columns, coalesced on both sides
    const uint32_t tile_words = tile_rows * d.out_width;  // <= 2^10 * 2^16
    for (uint32_t j = threadIdx.x; j < tile_words; j += SCAN_THREADS) {
        const uint32_t lr = j / d.out_width, c = j - lr * d.out_width;
        if ((named[c >> 5] >> (c & 31)) & 1) continue;  // (a column at or beyond src_width always is)
        out[(base + lr) * d.out_width + c] = src[(base + lr) * d.src_width + c];
    }

    ScanMap m[SCAN_N], total[SCAN_N];
    scan_lane_maps(d, src, base, m);
    scan_block_maps(d.n, m, wave_maps, total);
    uint32_t y[SCAN_N];  // the state before this lane's next row
#pragma unroll
    for (int s = 0; s < SCAN_N; s++)
        y[s] = s < (int)d.n ? scan_apply(m[s], state_in[(uint64_t)blockIdx.x * d.n + s]) : 0u;
#pragma unroll
    for (int k = 0; k < SCAN_RPT; k++) {
        const uint32_t local = threadIdx.x * d.rpt + k;
        const uint64_t r = base + local;
        if (k < (int)d.rpt && local < d.block_rows && r < d.height) {
            const uint32_t* row = src + r * d.src_width;
            uint32_t* o = out + r * d.out_width;
#pragma unroll
            for (int s = 0; s < SCAN_N; s++)
                if (s < (int)d.n) {
                    const ScanDev::Col& c = d.col[s];
                    const uint32_t before = scan_resets(c, row) ? c.init_m : y[s];
                    y[s] = scan_apply(ScanMap{scan_term(c.a_kind, c.a, row), scan_term(c.b_kind, c.b, row)}, before);
                    o[c.dst] = from_mont(c.exclusive ? before : y[s]);
                }
        }
    }
}

DeviceMatrix scan_matrix(Context& ctx, const ScanSpec& spec, const DeviceMatrix& src, uint32_t* finals) {
    StageTimer timer(&ctx, "scan");
    require_resident(ctx, src, "scan", "the source");
    const ScanPlan plan = scan_check(spec, src.width);
    // TS_SCAN_BLOCK_ROWS (1 .. 1024, read on every call): the rows one workgroup owns, a test knob that makes small
    // matrices cross the wave, the workgroup and several trips of the totals loop.  The result does not depend on it.
    const uint32_t block_rows =
        (uint32_t)mult_knob("TS_SCAN_BLOCK_ROWS", 1, SCAN_THREADS * SCAN_RPT, SCAN_THREADS * SCAN_RPT);

    ScanDev d = {};
    d.height = src.height;
    d.src_width = src.width;
    d.out_width = plan.out_width;
    d.n = (uint32_t)spec.columns.size();
    d.block_rows = block_rows;
    d.rpt = (block_rows + SCAN_THREADS - 1) / SCAN_THREADS;
    for (uint32_t s = 0; s < d.n; s++) {
        const ScanColumn& c = spec.columns[s];
        d.col[s] = {c.a_kind, c.a_kind ? c.a_value : to_mont(c.a_value), c.b_kind, c.b_kind ? c.b_value : to_mont(c.b_value),
                    to_mont(c.init), c.reset_column, c.dst_column, c.flags & SCAN_EXCLUSIVE};
    }
    const uint32_t n_blocks = (uint32_t)((src.height + block_rows - 1) / block_rows);  // <= 2^27

    DeviceMatrix out;
    out.buf = DevBuf<uint32_t>(&ctx, (size_t)src.height * plan.out_width);
    out.height = src.height;
    out.width = plan.out_width;
    out.layout = DeviceMatrix::ROW_MAJOR;

    // the column bits through the context's page-locked arena: no wait of its own
    DevBuf<uint32_t> d_named(&ctx, plan.named.size());
    h2d(ctx, d_named.p, plan.named.data(), plan.named.size() * 4);
    DevBuf<ScanMap> totals(&ctx, (size_t)n_blocks * d.n);
    DevBuf<uint32_t> state_in(&ctx, (size_t)n_blocks * d.n + SCAN_MAX_COLUMNS);  // and the last values behind it
    uint32_t* last = state_in.p + (size_t)n_blocks * d.n;

    const dim3 grid(n_blocks), block(SCAN_THREADS);
    TS_LAUNCH(ctx, k_scan_reduce, grid, block, 0, d, (const uint32_t*)src.buf.p, totals.p);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_scan_totals, dim3(1), block, 0, d, (const ScanMap*)totals.p, n_blocks, state_in.p, last);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_scan_apply, grid, block, 0, d, (const uint32_t*)d_named.p, (const uint32_t*)src.buf.p,
              (const uint32_t*)state_in.p, out.buf.p);
    TS_HIP(hipGetLastError());
    if (finals) d2h_sync(ctx, finals, last, d.n * sizeof(uint32_t));
    return out;
}

}  // namespace ts
