// Coset LDE on column-major BabyBear columns: inverse NTT -> coset scaling -> forward NTT, with
// the result in bit-reversed row order (reference fri/src/two_adic_pcs.rs:233-241:
// `dft.coset_lde_batch(evals, log_blowup, shift).bit_reverse_rows()`).
//
// Formulation (DESIGN.md "NTT"): block-twiddle radix-2 transform.  Forward stage s (m = 2^s
// blocks, distance t = n/2^(s+1)) applies (a, b) -> (a + w b, a - w b) with ONE twiddle per block,
// w = W[m + blk] = omega_{2m}^bitrev(blk); natural-order input, bit-reversed output, no separate
// twist between passes.  The inverse runs the stages backwards with (A, B) -> (A + B, (A - B)/w).
//
// Execution: up to 4 stages at a time are done in registers (a thread owns the 16 elements of a
// radix-16 group), with one LDS exchange between such rounds; the LDS image is padded so that every
// round's access pattern is bank-conflict free (ntt_lde.hip).  Three kernels there:
//   k_intt_contig    stages log_n-1 .. sA of the inverse on 4096-element chunks   (only n > 4096)
//   k_lde_mid        the strided stages of the inverse (sA-1 .. 0), coefficient k scaled by shift^k / n,
//                    then for every coset the strided stages of the forward transform with the N-point
//                    twiddles of block beta (ntt_lde.hip), writing coset block beta -- the coefficients
//                    never touch HBM
//   k_lde_fwd_contig stages sA .. log_n-1 of the forward transform, in place on 4096-element chunks
// For n <= 4096 k_lde_mid alone does everything.  Data in HBM is canonical; twiddles are
// Montgomery, so mont_mul(data, twiddle) is canonical -- or, for the NTT passes that take them, Plantard
// words (bb.hpp plant_const): plant_mul(any word, twiddle) is canonical in three instructions, a butterfly
// 8 instead of 10 (ntt_rounds.hpp states the two forms; ntt_lde.hip says which kernel takes which).
#include "kernels.hpp"

namespace ts {

constexpr int SHIFT_LO_BITS = 10;  // coset scale s^k = hi[k >> 10] * lo[k & 1023]

// ------------------------------------------------------------------ tables
// entry idx of the table, Montgomery form: w_{2m}^bitrev(i) for idx = m + i (1 at the unused index 0)
__device__ __forceinline__ uint32_t twiddle_mont(uint32_t idx) {
    if (idx == 0) return R_MOD_P;
    unsigned logm = 31 - __clz(idx);
    uint32_t i = idx - (1u << logm);
    // omega_{2m}: generator of the subgroup of order 2^(logm+1)
    uint32_t g27 = to_mont(TWO_ADIC_GEN_27);
    uint32_t g = mont_pow(g27, 1ull << (27 - (logm + 1)));
    uint32_t e = bitrev32(i, logm);
    return mont_pow(g, e);
}

__global__ void k_build_twiddles(uint32_t* __restrict__ W, uint32_t* __restrict__ Winv,
                                 unsigned log_size) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (1u << log_size)) return;
    const uint32_t w = twiddle_mont(idx);
    W[idx] = w;
    Winv[idx] = mont_inv(w);
}

// the Plantard words of the same entries, one direction (the NTT passes' own tables: ntt_rounds.hpp)
__global__ void k_build_plant_twiddles(uint2* __restrict__ WP, unsigned log_size, bool inverse) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (1u << log_size)) return;
    const uint32_t w = twiddle_mont(idx);
    const uint64_t f = plant_const(from_mont(inverse ? mont_inv(w) : w));
    WP[idx] = make_uint2((uint32_t)f, (uint32_t)(f >> 32));
}

void launch_build_twiddles(Context& ctx, uint32_t* W, uint32_t* Winv, unsigned log_size) {
    uint32_t n = 1u << log_size;
    TS_LAUNCH(ctx, k_build_twiddles, dim3((n + 255) / 256), dim3(256), 0, W, Winv, log_size);
    TS_HIP(hipGetLastError());
}

void launch_build_plant_twiddles(Context& ctx, uint2* WP, unsigned log_size, bool inverse) {
    uint32_t n = 1u << log_size;
    TS_LAUNCH(ctx, k_build_plant_twiddles, dim3((n + 255) / 256), dim3(256), 0, WP, log_size, inverse);
    TS_HIP(hipGetLastError());
}

// lo[beta][j] = s_beta^j * scale,  hi[beta][j] = s_beta^(j << 10)   (Montgomery)
__global__ void k_build_shift_tables(uint32_t* __restrict__ lo, uint32_t* __restrict__ hi,
                                     uint32_t n_hi, uint32_t shift_mont, unsigned log_N,
                                     unsigned log_blowup, uint32_t scale_mont) {
    uint32_t beta = blockIdx.y;
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t n_lo = 1u << SHIFT_LO_BITS;
    if (j >= n_lo + n_hi) return;
    // s_beta = shift * omega_N^bitrev_b(beta)
    uint32_t g27 = to_mont(TWO_ADIC_GEN_27);
    uint32_t gN = mont_pow(g27, 1ull << (27 - log_N));
    uint32_t s = mont_mul(shift_mont, mont_pow(gN, bitrev32(beta, log_blowup)));
    if (j < n_lo) {
        lo[beta * n_lo + j] = mont_mul(mont_pow(s, j), scale_mont);
    } else {
        uint32_t jj = j - n_lo;
        hi[beta * n_hi + jj] = mont_pow(s, (uint64_t)jj << SHIFT_LO_BITS);
    }
}

void launch_build_shift_tables(Context& ctx, uint32_t* lo, uint32_t* hi, uint32_t n_hi,
                               uint32_t n_cosets, uint32_t shift_mont, unsigned log_N,
                               unsigned log_blowup, uint32_t scale_mont) {
    const uint32_t n_lo = 1u << SHIFT_LO_BITS;
    TS_LAUNCH(ctx, k_build_shift_tables, dim3((n_lo + n_hi + 255) / 256, n_cosets), dim3(256), 0, lo,
              hi, n_hi, shift_mont, log_N, log_blowup, scale_mont);
    TS_HIP(hipGetLastError());
}

// T[k] = lo[k & 1023] * hi[k >> 10] = shift^k * scale   (Montgomery), k < n
__global__ void __launch_bounds__(256)
k_build_scale_table(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, unsigned log_n,
                    uint32_t* __restrict__ T) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (1ull << log_n)) return;
    T[k] = mont_mul(lo[k & ((1u << SHIFT_LO_BITS) - 1)], hi[k >> SHIFT_LO_BITS]);
}

const uint32_t* coset_scale_table(Context& ctx, unsigned log_n, uint32_t shift) {
    if (shift == 1) return nullptr;  // the constant 1/n: coset_lde passes it as a value
    for (auto& t : ctx.scale_tables)
        if (t.log_n == log_n && t.shift == shift) {
            t.last_use = ++ctx.scale_clock;
            return t.d;
        }
    const size_t words = (size_t)1 << log_n;
    // keep at most 8 tables / 2 GiB; evicting needs the stream idle (a launch may still read one)
    size_t total = words * 4;
    for (auto& t : ctx.scale_tables) total += t.words * 4;
    while (!ctx.scale_tables.empty() && (ctx.scale_tables.size() >= 8 || total > (2ull << 30))) {
        size_t victim = 0;
        for (size_t i = 1; i < ctx.scale_tables.size(); i++)
            if (ctx.scale_tables[i].last_use < ctx.scale_tables[victim].last_use) victim = i;
        ctx.sync();
        total -= ctx.scale_tables[victim].words * 4;
        (void)hipFree(ctx.scale_tables[victim].d);
        ctx.scale_tables.erase(ctx.scale_tables.begin() + victim);
    }
    uint32_t* d = nullptr;
    TS_HIP(hipMalloc((void**)&d, words * 4));
    if (ctx.poison_on) ctx.poison(d, words * 4);
    const uint64_t n = 1ull << log_n;
    const uint32_t n_lo = 1u << SHIFT_LO_BITS;
    const uint32_t n_hi = log_n > (unsigned)SHIFT_LO_BITS ? 1u << (log_n - SHIFT_LO_BITS) : 1u;
    DevBuf<uint32_t> lo(&ctx, n_lo), hi(&ctx, n_hi);
    // one coset, no blowup: s_0 = shift (as the standalone transforms build their factor, ntt_dft.hip)
    launch_build_shift_tables(ctx, lo.p, hi.p, n_hi, 1, to_mont(shift), log_n, 0, lde_inv_n_mont(log_n));
    TS_LAUNCH(ctx, k_build_scale_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const uint32_t*)lo.p,
              (const uint32_t*)hi.p, log_n, d);
    TS_HIP(hipGetLastError());
    ctx.scale_tables.push_back(Context::ScaleTable{log_n, shift, d, words, ++ctx.scale_clock});
    return d;
}

// ------------------------------------------------------------------ transposes
// One 64 x 64 LDS tile transpose between a row-major matrix rm[r][c] (rows of rm_width words) and a
// column-major one cm[c][p] (columns col_stride apart), w columns of h rows.  TO_COLUMNS: rm -> cm, else
// cm -> rm.  BITREV: p = bitrev(r) over log_h bits (h = 2^log_h), else p = r and h is any height.
// tile[i][j] is element (p0 + i, c0 + j).  On the row-major side a thread takes column c0 + tx of the rows
// i = ty + 4 k (a wave moves 256 consecutive bytes of a row), on the column-major side slot p0 + tx of the
// columns c0 + ty + 4 k.
template <bool TO_COLUMNS, bool BITREV>
__global__ void __launch_bounds__(256)
k_transpose_tile(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint64_t h, unsigned log_h,
                 uint32_t w, uint64_t col_stride, uint32_t rm_width) {
    __shared__ uint32_t tile[64][65];
    const uint64_t p0 = (uint64_t)blockIdx.x * 64;
    const uint32_t c0 = blockIdx.y * 64;
    const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    auto row_of = [&](uint64_t p) -> uint64_t { return BITREV ? bitrev32((uint32_t)p, log_h) : p; };
    if (p0 + 64 <= h && c0 + 64 <= w) {
        // full tile: 16 loads in flight, then 16 LDS writes; as run-time loops every iteration waited
        // for its own load.  bitrev(p0 + i) for i < 64 = bitrev(p0) + (bitrev6(i) << (log_h - 6))
        // (p0 is a multiple of 64: its six low bits are free), so the rows of a thread on the row-major
        // side are a base plus constants.
        const uint64_t rm = row_of(p0) * rm_width + c0 + tx;
        const uint64_t rm_step = BITREV ? (uint64_t)rm_width << (log_h - 6) : rm_width;
        const uint64_t cm = (uint64_t)(c0 + ty) * col_stride + p0 + tx;
        auto rm_at = [&](int k) {
            const uint32_t i = ty + 4 * (uint32_t)k;  // tile row
            return rm + (uint64_t)(BITREV ? __brev(i) >> 26 : i) * rm_step;
        };
        auto cm_at = [&](int k) { return cm + (uint64_t)(4 * k) * col_stride; };
        uint32_t t[16];
#pragma unroll
        for (int k = 0; k < 16; k++) t[k] = src[TO_COLUMNS ? rm_at(k) : cm_at(k)];
#pragma unroll
        for (int k = 0; k < 16; k++) (TO_COLUMNS ? tile[ty + 4 * k][tx] : tile[tx][ty + 4 * k]) = t[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; k++) t[k] = TO_COLUMNS ? tile[tx][ty + 4 * k] : tile[ty + 4 * k][tx];
#pragma unroll
        for (int k = 0; k < 16; k++) dst[TO_COLUMNS ? cm_at(k) : rm_at(k)] = t[k];
        return;
    }
    // partial tile (also h < 64 and heights that are no power of two): every element guarded
    auto rm_ok = [&](uint32_t j) { return p0 + j < h && c0 + tx < w; };  // (row p0 + j, column c0 + tx)
    auto cm_ok = [&](uint32_t j) { return c0 + j < w && p0 + tx < h; };  // (column c0 + j, slot p0 + tx)
    auto rm_at = [&](uint32_t j) { return row_of(p0 + j) * rm_width + c0 + tx; };
    auto cm_at = [&](uint32_t j) { return (uint64_t)(c0 + j) * col_stride + p0 + tx; };
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t j = ty + 4 * (uint32_t)k;
        if (TO_COLUMNS ? rm_ok(j) : cm_ok(j)) (TO_COLUMNS ? tile[j][tx] : tile[tx][j]) = src[TO_COLUMNS ? rm_at(j) : cm_at(j)];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t j = ty + 4 * (uint32_t)k;
        if (TO_COLUMNS ? cm_ok(j) : rm_ok(j)) dst[TO_COLUMNS ? cm_at(j) : rm_at(j)] = TO_COLUMNS ? tile[tx][j] : tile[j][tx];
    }
}

// `name`: the kernel-timer name of the use (bench.py looks k_transpose_bitrev up)
template <bool TO_COLUMNS, bool BITREV>
static void launch_transpose_tile(Context& ctx, const char* name, const uint32_t* src, uint32_t* dst, uint64_t h,
                                  unsigned log_h, uint32_t w, uint64_t col_stride, uint32_t rm_width) {
    if (w == 0 || h == 0) return;
    TS_LAUNCH_NAMED(ctx, name, (k_transpose_tile<TO_COLUMNS, BITREV>), dim3((unsigned)((h + 63) / 64), (w + 63) / 64),
                    dim3(256), 0, src, dst, h, log_h, w, col_stride, rm_width);
    TS_HIP(hipGetLastError());
}

// src row-major [n][w] natural  ->  dst[c][p] = src[bitrev(p)][c]
void launch_transpose_bitrev(Context& ctx, const uint32_t* src, uint32_t* dst, unsigned log_n,
                             uint32_t w, uint64_t dst_col_stride, uint32_t src_width) {
    launch_transpose_tile<true, true>(ctx, "k_transpose_bitrev", src, dst, 1ull << log_n, log_n, w, dst_col_stride,
                                      src_width ? src_width : w);
}

// src row-major [n][w]  ->  dst[c][r] = src[r][c], any n
void launch_transpose_plain(Context& ctx, const uint32_t* src, uint32_t* dst, uint64_t n, uint32_t w,
                            uint64_t dst_col_stride) {
    launch_transpose_tile<true, false>(ctx, "k_transpose_plain", src, dst, n, 0, w, dst_col_stride, w);
}

// dst row-major [h][w]  <-  src column-major, any h
void launch_transpose_to_row_major(Context& ctx, const uint32_t* src, uint64_t col_stride,
                                   uint32_t* dst, uint64_t h, uint32_t w) {
    launch_transpose_tile<false, false>(ctx, "k_transpose_to_row_major", src, dst, h, 0, w, col_stride, w);
}

// dst[bitrev(p)][c] row-major, natural rows  <-  src column-major, rows p < 2^log_h in bit-reversed order
void launch_transpose_unbitrev(Context& ctx, const uint32_t* src, uint64_t col_stride, uint32_t* dst,
                               unsigned log_h, uint32_t w) {
    launch_transpose_tile<false, true>(ctx, "k_transpose_unbitrev", src, dst, 1ull << log_h, log_h, w, col_stride, w);
}

}  // namespace ts
