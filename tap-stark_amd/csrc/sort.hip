// Rows of a resident row-major matrix in sorted order: a stable least-significant-digit radix sort (8-bit digits) of a
// uint32 source-row permutation over 1 .. 4 key columns, and the gather that writes the rows through it.  The keys
// are compared as stored, unsigned; the order is unique, so every run and every TS_SORT_BLOCK_ROWS gives the same
// matrix.
//
// The conventions of logup_mult.hip: plain launches only, no grid barrier, no cooperative launch, no workgroup waits
// for another (so no decoupled look-back: the count scan is a bounded tree of launches); every loop is bounded by a
// launch argument or the wave size; every temporary comes from the context's pool and is written before it is read.
//   k_sort_hist     once, over the live rows, for all 4 * n_keys byte digits: LDS-private bins per workgroup, integer
//                   atomics into a global [digit][256] table, ONE copy back (the call's only host wait).  A digit
//                   whose rows all fall into one bin is a pass that would move nothing: it is skipped.
//   per remaining pass, from byte 0 of the last key to byte 3 of the first:
//   k_sort_count    a workgroup owns block_rows consecutive positions of the current permutation and writes its 256
//                   digit counts digit-major: counts[digit][workgroup].
//   k_sort_scan     an exclusive scan over that array in tiles of 1024: tile totals upward until one tile is left,
//                   that tile scanned, then downward each tile scanned on top of its parent's offset (1, 3 or 5
//                   launches: 256 * workgroups <= 2^10, 2^20, 2^30 words).
//   k_sort_scatter  the stable scatter: position -> offsets[digit][workgroup] + rank, where rank is the number of
//                   positions of the workgroup with the same digit and a smaller position.  Chunks of 256 positions in
//                   ascending order; in a chunk a wave's lanes with one digit are found with one ballot per digit bit
//                   (the match mask), a lane's rank in its wave is the population count of the mask below it, the
//                   wave's count goes to LDS and the waves before it are added in wave order.  No atomic hands out a
//                   rank: arrival order never decides anything.
//   k_sort_load_keys  once per key column: its words through the permutation into a dense array that count and scatter
//                   read and scatter moves along with the rows (the key word is CARRIED beside the row; re-reading it
//                   from the matrix through the permutation in every pass was measured and lost on wide rows and on
//                   single keys: DESIGN.md has both figures).
//   k_sort_gather   out from src through the final permutation, lanes along the words of rows so that both sides
//                   coalesce; the source-row and group-start columns; rows [n_live, height) copied in place.  With a
//                   caller's index column and a range check it is gather_rows.
// Addressing: row * width is 64-bit everywhere (2^27 rows of a wide row pass 2^32 words).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "logup_dev.hpp"
#include "sort.hpp"

namespace ts {

constexpr int SORT_THREADS = 256;
constexpr int SORT_WAVES = SORT_THREADS / 64;
constexpr uint32_t SORT_SCAN_TILE = 4 * SORT_THREADS;
constexpr uint32_t SORT_HIST_GROUPS = 1024;

struct SortKeyCols {
    uint32_t n, col[SORT_MAX_KEYS];
};

// the lanes of this wave that hold `digit`, among the valid ones (0 on an invalid lane): one ballot per digit bit
__device__ __forceinline__ unsigned long long sort_match(uint32_t digit, bool valid) {
    unsigned long long mask = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (digit >> b) & 1;
        const unsigned long long has = __ballot(valid && bit);
        mask &= bit ? has : ~has;
    }
    return valid ? mask : 0ull;
}

__device__ __forceinline__ unsigned long long sort_lanes_below() {
    return (1ull << (threadIdx.x & 63)) - 1;
}

__global__ void __launch_bounds__(SORT_THREADS)
k_sort_hist(const uint32_t* __restrict__ src, uint32_t width, const SortKeyCols k, uint64_t n, uint32_t iters,
            uint32_t* __restrict__ table) {
    __shared__ uint32_t bins[4 * SORT_MAX_KEYS * 256];
    for (uint32_t t = threadIdx.x; t < 4 * SORT_MAX_KEYS * 256; t += SORT_THREADS) bins[t] = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63;
    for (uint32_t it = 0; it < iters; it++) {
        const uint64_t r = ((uint64_t)it * gridDim.x + blockIdx.x) * SORT_THREADS + threadIdx.x;
        const bool valid = r < n;
        const unsigned long long vm = __ballot(valid);
        if (vm == 0) continue;  // (wave-uniform)
        const int leader = __ffsll((long long)vm) - 1;
#pragma unroll
        for (int q = 0; q < (int)SORT_MAX_KEYS; q++) {
            if (q >= (int)k.n) continue;
            const uint32_t w = valid ? src[r * width + k.col[q]] : 0;
#pragma unroll
            for (int byte = 0; byte < 4; byte++) {
                const uint32_t d = (w >> (8 * byte)) & 255;
                const uint32_t first = (uint32_t)__shfl((int)d, leader, 64);
                uint32_t* bin = bins + (q * 4 + byte) * 256;
                if (__ballot(valid && d == first) == vm) {  // one digit in the whole wave: one add
                    if ((int)lane == leader) atomicAdd(bin + first, (uint32_t)__popcll(vm));
                } else if (valid) {
                    atomicAdd(bin + d, 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < 4 * k.n * 256; t += SORT_THREADS)
        if (bins[t]) atomicAdd(table + t, bins[t]);
}

// keys[i] = the word of column `col` on the row at position i of the permutation (perm null: the identity)
__global__ void __launch_bounds__(SORT_THREADS)
k_sort_load_keys(const uint32_t* __restrict__ src, uint32_t width, uint32_t col, const uint32_t* __restrict__ perm,
                 uint64_t n, uint32_t* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * SORT_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t row = perm ? perm[i] : i;
    keys[i] = src[row * width + col];
}

__global__ void __launch_bounds__(SORT_THREADS)
k_sort_count(const uint32_t* __restrict__ keys, uint32_t shift, uint64_t n, uint32_t block_rows, uint32_t chunks,
             uint32_t n_blocks, uint32_t* __restrict__ counts) {
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * block_rows;
    const uint64_t end = begin + block_rows < n ? begin + block_rows : n;
    for (uint32_t c = 0; c < chunks; c++) {
        const uint64_t i = begin + (uint64_t)c * SORT_THREADS + threadIdx.x;
        const bool valid = i < end;
        const uint32_t digit = valid ? (keys[i] >> shift) & 255 : 0;
        const unsigned long long mask = sort_match(digit, valid);
        if (valid && (mask & sort_lanes_below()) == 0) atomicAdd(hist + digit, (uint32_t)__popcll(mask));
    }
    __syncthreads();
    counts[(uint64_t)threadIdx.x * n_blocks + blockIdx.x] = hist[threadIdx.x];
}

// exclusive scan of the 256 per-thread values of a workgroup; *total (if given) receives their sum on every thread
__device__ __forceinline__ uint32_t sort_block_scan(uint32_t v, uint32_t* total) {
    __shared__ uint32_t wave_total[SORT_WAVES];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if ((int)lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; w++) {
        const uint32_t t = wave_total[w];
        before += w < (int)wave ? t : 0;
        all += t;
    }
    if (total) *total = all;
    return before + incl - v;
}

// REDUCE: sums[tile] = the tile's total.  Otherwise the tile is scanned in place, exclusively, on top of sums[tile]
// (sums null: on top of 0 -- the one tile of the top level).
template <bool REDUCE>
__global__ void __launch_bounds__(SORT_THREADS)
k_sort_scan(uint32_t* __restrict__ data, uint64_t len, uint32_t* __restrict__ sums) {
    const uint64_t e0 = (uint64_t)blockIdx.x * SORT_SCAN_TILE + 4 * threadIdx.x;
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = e0 + j < len ? data[e0 + j] : 0;
    uint32_t total;
    uint32_t at = sort_block_scan(v[0] + v[1] + v[2] + v[3], &total);
    if (REDUCE) {
        if (threadIdx.x == 0) sums[blockIdx.x] = total;
        return;
    }
    at += sums ? sums[blockIdx.x] : 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (e0 + j < len) data[e0 + j] = at;
        at += v[j];
    }
}

__global__ void __launch_bounds__(SORT_THREADS)
k_sort_scatter(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm /* null: the identity */,
               uint32_t shift, uint64_t n, uint32_t block_rows, uint32_t chunks, uint32_t n_blocks,
               const uint32_t* __restrict__ offsets, uint32_t* __restrict__ keys_out, uint32_t* __restrict__ perm_out) {
    __shared__ uint32_t base[256];
    __shared__ uint32_t wave_count[SORT_WAVES][256];
    const unsigned wave = threadIdx.x >> 6;
    base[threadIdx.x] = offsets[(uint64_t)threadIdx.x * n_blocks + blockIdx.x];
#pragma unroll
    for (int w = 0; w < SORT_WAVES; w++) wave_count[w][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * block_rows;
    const uint64_t end = begin + block_rows < n ? begin + block_rows : n;
    for (uint32_t c = 0; c < chunks; c++) {  // ascending positions: chunk, then wave, then lane
        const uint64_t i = begin + (uint64_t)c * SORT_THREADS + threadIdx.x;
        const bool valid = i < end;
        const uint32_t key = valid ? keys[i] : 0;
        const uint32_t row = valid && perm ? perm[i] : (uint32_t)i;
        const uint32_t digit = (key >> shift) & 255;
        const unsigned long long mask = sort_match(digit, valid);
        const uint32_t rank = (uint32_t)__popcll(mask & sort_lanes_below());
        if (valid && rank == 0) wave_count[wave][digit] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (valid) {
            uint32_t dst = base[digit] + rank;
#pragma unroll
            for (int w = 0; w < SORT_WAVES - 1; w++) dst += w < (int)wave ? wave_count[w][digit] : 0;
            if (dst < n) {  // (always: the offsets are the scan of this permutation's own counts)
                keys_out[dst] = key;
                perm_out[dst] = row;
            }
        }
        __syncthreads();
        uint32_t sum = 0;  // thread t owns digit t: the chunk's rows leave the running base
#pragma unroll
        for (int w = 0; w < SORT_WAVES; w++) {
            sum += wave_count[w][threadIdx.x];
            wave_count[w][threadIdx.x] = 0;
        }
        base[threadIdx.x] += sum;
        __syncthreads();
    }
}

struct GatherDev {
    uint64_t height, n_indexed, src_height;  // out's rows; rows below n_indexed go through the index; src's rows
    uint32_t src_width, out_width, flags, group_keys;
    uint32_t key_col[SORT_MAX_KEYS];
    uint32_t index_stride, index_column;     // the index word of row i is index[i * index_stride + index_column]
    uint32_t rows_per_block, iters;
};

// out[i] = src[s_i] with s_i = index word of row i below n_indexed (index null: i), i itself from there on.  An index
// word outside src: the row is not written and (i, word) goes into *back by a 64-bit minimum.
__global__ void __launch_bounds__(SORT_THREADS)
k_sort_gather(const GatherDev g, const uint32_t* __restrict__ src, const uint32_t* __restrict__ index,
              uint32_t* __restrict__ out, unsigned long long* __restrict__ back) {
    const uint64_t r0 = (uint64_t)blockIdx.x * g.rows_per_block;
    const uint64_t left = g.height - r0;
    const uint32_t words = (uint32_t)(left < g.rows_per_block ? left : g.rows_per_block) * g.out_width;
    for (uint32_t it = 0; it < g.iters; it++) {
        const uint32_t j = it * SORT_THREADS + threadIdx.x;
        if (j >= words) break;
        const uint32_t lr = j / g.out_width, c = j - lr * g.out_width;
        const uint64_t i = r0 + lr;
        const bool indexed = i < g.n_indexed && index;
        const uint64_t s = indexed ? index[i * g.index_stride + g.index_column] : i;
        if (s >= g.src_height) {
            if (c == 0 && back) atomicMin(back, ((unsigned long long)i << 32) | s);
            continue;
        }
        uint32_t v;
        if (c < g.src_width) {
            v = src[s * g.src_width + c];
        } else if (c == g.src_width && (g.flags & 1)) {
            v = (uint32_t)s;
        } else {  // group start: a live row whose leading keys differ from the row before it
            v = 0;
            if (i < g.n_indexed) {
                v = i == 0;
                const uint64_t prev = i == 0 ? s : index ? index[(i - 1) * g.index_stride + g.index_column] : i - 1;
#pragma unroll
                for (int q = 0; q < (int)SORT_MAX_KEYS; q++)
                    if (q < (int)g.group_keys && prev < g.src_height &&
                        src[s * g.src_width + g.key_col[q]] != src[prev * g.src_width + g.key_col[q]])
                        v = 1;
            }
        }
        out[i * g.out_width + c] = v;
    }
}

namespace {

void launch_gather(Context& ctx, GatherDev g, const uint32_t* src, const uint32_t* index, uint32_t* out,
                   unsigned long long* back) {
    g.rows_per_block = std::min(256u, std::max(1u, 4096u / g.out_width));
    g.iters = (g.rows_per_block * g.out_width + SORT_THREADS - 1) / SORT_THREADS;
    const dim3 grid((unsigned)((g.height + g.rows_per_block - 1) / g.rows_per_block)), block(SORT_THREADS);
    TS_LAUNCH(ctx, k_sort_gather, grid, block, 0, g, src, index, out, back);
    TS_HIP(hipGetLastError());
}

// exclusive scan of level 0 of `levels` (tile totals in the levels above it), in place
void launch_scan(Context& ctx, uint32_t* data, const std::vector<uint64_t>& offs, const std::vector<uint64_t>& lens) {
    const dim3 block(SORT_THREADS);
    const size_t top = lens.size() - 1;
    auto tiles = [](uint64_t len) { return dim3((unsigned)((len + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE)); };
    for (size_t l = 0; l < top; l++) {
        TS_LAUNCH(ctx, k_sort_scan<true>, tiles(lens[l]), block, 0, data + offs[l], lens[l], data + offs[l + 1]);
        TS_HIP(hipGetLastError());
    }
    TS_LAUNCH(ctx, k_sort_scan<false>, dim3(1), block, 0, data + offs[top], lens[top], (uint32_t*)nullptr);
    TS_HIP(hipGetLastError());
    for (size_t l = top; l-- > 0;) {
        TS_LAUNCH(ctx, k_sort_scan<false>, tiles(lens[l]), block, 0, data + offs[l], lens[l], data + offs[l + 1]);
        TS_HIP(hipGetLastError());
    }
}

}  // namespace

DeviceMatrix sort_rows(Context& ctx, const SortSpec& spec, const DeviceMatrix& src) {
    StageTimer timer(&ctx, "sort rows");
    const size_t nk = spec.key_columns.size();
    TS_REQUIRE(nk >= 1 && nk <= SORT_MAX_KEYS, TS_ERR_INVALID, "sort rows: between 1 and 4 keys");
    require_resident(ctx, src, "sort rows", "the source");
    for (size_t q = 0; q < nk; q++) {
        TS_REQUIRE(spec.key_columns[q] < src.width, TS_ERR_INVALID, "sort rows: a key column outside the source");
        for (size_t e = 0; e < q; e++)
            TS_REQUIRE(spec.key_columns[e] != spec.key_columns[q], TS_ERR_INVALID, "sort rows: a key column named twice");
    }
    TS_REQUIRE(spec.group_keys <= nk, TS_ERR_INVALID, "sort rows: group_keys above n_keys");
    TS_REQUIRE(spec.flags <= 3, TS_ERR_INVALID, "sort rows: a flag bit above 1");
    TS_REQUIRE(spec.n_live <= src.height, TS_ERR_INVALID, "sort rows: n_live above the height");
    const uint64_t out_width = (uint64_t)src.width + (spec.flags & 1) + ((spec.flags >> 1) & 1);
    TS_REQUIRE(out_width <= SORT_MAX_WIDTH, TS_ERR_INVALID, "sort rows: the output is wider than 2^16 columns");
    const uint32_t block_rows = (uint32_t)mult_knob("TS_SORT_BLOCK_ROWS", 1, SORT_DEFAULT_BLOCK_ROWS, SORT_DEFAULT_BLOCK_ROWS);

    const uint64_t n = spec.n_live;
    SortKeyCols kc;
    memset(&kc, 0, sizeof kc);
    kc.n = (uint32_t)nk;
    for (size_t q = 0; q < nk; q++) kc.col[q] = spec.key_columns[q];

    DeviceMatrix out;
    out.buf = DevBuf<uint32_t>(&ctx, (size_t)src.height * out_width);
    out.height = src.height;
    out.width = (uint32_t)out_width;
    out.layout = DeviceMatrix::ROW_MAJOR;

    const dim3 block(SORT_THREADS);
    DevBuf<uint32_t> perm[2], keys[2], counts;
    const uint32_t* cur = nullptr;  // the permutation so far; null: the identity
    if (n >= 2) {
        // which digits move anything
        std::vector<uint32_t> table(4 * nk * 256);
        DevBuf<uint32_t> d_table(&ctx, table.size());
        TS_HIP(hipMemsetAsync(d_table.p, 0, table.size() * 4, ctx.stream));
        const uint32_t groups = (uint32_t)std::min<uint64_t>((n + SORT_THREADS - 1) / SORT_THREADS, SORT_HIST_GROUPS);
        const uint32_t iters = (uint32_t)((n + (uint64_t)groups * SORT_THREADS - 1) / ((uint64_t)groups * SORT_THREADS));
        TS_LAUNCH(ctx, k_sort_hist, dim3(groups), block, 0, (const uint32_t*)src.buf.p, src.width, kc, n, iters, d_table.p);
        TS_HIP(hipGetLastError());
        d2h_sync(ctx, table.data(), d_table.p, table.size() * 4);
        auto moves = [&](size_t q, int byte) {
            const uint32_t* bins = table.data() + (q * 4 + byte) * 256;
            for (int d = 0; d < 256; d++)
                if (bins[d] == n) return false;
            return true;
        };

        const uint64_t n_blocks = (n + block_rows - 1) / block_rows;
        const uint32_t chunks = (block_rows + SORT_THREADS - 1) / SORT_THREADS;
        std::vector<uint64_t> lens{256 * n_blocks}, offs{0};
        while (lens.back() > SORT_SCAN_TILE) {
            offs.push_back(offs.back() + lens.back());
            lens.push_back((lens.back() + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE);
        }
        int side = 0;
        for (size_t q = nk; q-- > 0;) {
            bool loaded = false;
            for (int byte = 0; byte < 4; byte++) {
                if (!moves(q, byte)) continue;
                if (!counts.p) {
                    counts = DevBuf<uint32_t>(&ctx, offs.back() + lens.back());
                    perm[0] = DevBuf<uint32_t>(&ctx, n);
                    perm[1] = DevBuf<uint32_t>(&ctx, n);
                    keys[0] = DevBuf<uint32_t>(&ctx, n);
                    keys[1] = DevBuf<uint32_t>(&ctx, n);
                }
                if (!loaded) {  // the first pass over this key column: its words in the order reached so far
                    TS_LAUNCH(ctx, k_sort_load_keys, dim3((unsigned)((n + SORT_THREADS - 1) / SORT_THREADS)), block, 0,
                              (const uint32_t*)src.buf.p, src.width, kc.col[q], cur, n, keys[side].p);
                    TS_HIP(hipGetLastError());
                    loaded = true;
                }
                const uint32_t shift = 8 * byte;
                TS_LAUNCH(ctx, k_sort_count, dim3((unsigned)n_blocks), block, 0, (const uint32_t*)keys[side].p, shift, n,
                          block_rows, chunks, (uint32_t)n_blocks, counts.p);
                TS_HIP(hipGetLastError());
                launch_scan(ctx, counts.p, offs, lens);
                TS_LAUNCH(ctx, k_sort_scatter, dim3((unsigned)n_blocks), block, 0, (const uint32_t*)keys[side].p, cur, shift,
                          n, block_rows, chunks, (uint32_t)n_blocks, (const uint32_t*)counts.p, keys[side ^ 1].p,
                          perm[side ^ 1].p);
                TS_HIP(hipGetLastError());
                side ^= 1;
                cur = perm[side].p;
            }
        }
    }

    GatherDev g;
    memset(&g, 0, sizeof g);
    g.height = src.height;
    g.n_indexed = n;
    g.src_height = src.height;
    g.src_width = src.width;
    g.out_width = out.width;
    g.flags = spec.flags;
    g.group_keys = spec.group_keys;
    for (size_t q = 0; q < nk; q++) g.key_col[q] = kc.col[q];
    g.index_stride = 1;
    launch_gather(ctx, g, src.buf.p, cur, out.buf.p, nullptr);
    return out;
}

DeviceMatrix gather_rows(Context& ctx, const DeviceMatrix& src, const DeviceMatrix& index, uint32_t index_column) {
    StageTimer timer(&ctx, "gather rows");
    require_resident(ctx, src, "gather", "the source");
    require_resident(ctx, index, "gather", "the index");
    TS_REQUIRE(index_column < index.width, TS_ERR_INVALID, "gather: index_column outside the index matrix");
    TS_REQUIRE(src.width <= SORT_MAX_WIDTH, TS_ERR_INVALID, "gather: the source is wider than 2^16 columns");
    DeviceMatrix out;
    out.buf = DevBuf<uint32_t>(&ctx, (size_t)index.height * src.width);
    out.height = index.height;
    out.width = src.width;
    out.layout = DeviceMatrix::ROW_MAJOR;
    DevBuf<unsigned long long> back(&ctx, 1);
    TS_HIP(hipMemsetAsync(back.p, 0xff, sizeof(unsigned long long), ctx.stream));
    GatherDev g;
    memset(&g, 0, sizeof g);
    g.height = g.n_indexed = index.height;
    g.src_height = src.height;
    g.src_width = g.out_width = src.width;
    g.index_stride = index.width;
    g.index_column = index_column;
    launch_gather(ctx, g, src.buf.p, index.buf.p, out.buf.p, back.p);
    unsigned long long bad;
    d2h_sync(ctx, &bad, back.p, sizeof bad);
    TS_REQUIRE(bad == ~0ull, TS_ERR_INVALID,
               "gather: row index " + std::to_string(bad & 0xFFFFFFFFull) + " at row " + std::to_string(bad >> 32) +
                   " outside the source");
    return out;
}

}  // namespace ts
