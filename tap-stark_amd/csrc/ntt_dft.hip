// Standalone transforms of TwoAdicSubgroupDft on device matrices: dft_batch /
// coset_dft_batch, idft_batch / coset_idft_batch, coset_lde_batch, bit_reverse_rows -- what a caller that
// drives its own flow through the Dft and Pcs traits needs between ts_pcs_commit, ts_quotient_chunks and
// ts_pcs_open, without a trip to the host.
//
// The arithmetic is that of the coset LDE (ntt_lde.hip: block-twiddle radix-2 stages in register rounds of
// up to 16 / 32 elements, the padded LDS image, the same plan split -- ntt_rounds.hpp); what is new is
// every pass on its own, in one direction:
//   k_dft_mid     the strided stages 0 .. sA-1 of ONE direction on tiles of 2^sA rows x 2^log_T slots,
//                 with the per-coefficient factor of a coset applied where the coefficients are:
//                 forward  x_k *= shift^k on the way in, then stages 0 .. sA-1   (natural in)
//                 inverse  stages sA-1 .. 0, then x_k *= shift^-k / n on the way out (natural, canonical out)
//                 For n <= 4096 it is the whole transform (one tile = one column).
//   k_dft_contig  stages sA .. log_n-1 on 2^LM-element chunks, in place, either direction with its
//                 twiddle table (forward: after k_dft_mid, canonical out; inverse: before it, lazy out)
//   k_transpose_unbitrev   column-major with bit-reversed rows -> row-major with natural rows: the
//                 output transpose of the forward transforms and of the LDE, and -- on the first
//                 2^log_size rows of a committed LDE -- get_evaluations_on_domain
//   k_bit_reverse_rows     row-major -> row-major, rows permuted
// Forward: natural coefficients in, bit-reversed evaluations out; inverse: the reverse (ntt.hip header).
// The factor is lo[k & 1023] * hi[k >> 10] from the two small tables of launch_build_shift_tables (one
// coset): 2 loads and 2 products per element in one pass, instead of an n-word table per (n, shift) in
// the context's cache.  Everything that reaches HBM at the end of a transform is canonical.
#include <algorithm>

#include "ntt_rounds.hpp"

namespace ts {

constexpr int DFT_LO_BITS = 10;  // launch_build_shift_tables: s^k = hi[k >> 10] * lo[k & 1023]

__device__ __forceinline__ uint32_t dft_factor(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                               uint32_t k) {
    return mont_mul(lo[k & ((1u << DFT_LO_BITS) - 1)], hi[k >> DFT_LO_BITS]);
}

// ------------------------------------------------------------------ strided pass, one direction
// Tile = slots {(row << row_shift) + j2_0 + jj : row < 2^log_len, jj < 2^log_T} of column blockIdx.y, in
// place (row_shift = LM for n > 2^LM; 0 with log_T = 0 where the tile is the whole column).
// PLAN 0: run-time round plan.  PLAN 1: log_len = 8, log_T = 5 (n = 2^(LM + 8)): two radix-16 rounds with
// compile-time distances 2^9 and 2^5, the first of them from stage 0 (no product for the twiddle 1).
template <bool INV, bool SCALE, int PLAN, int TILE = TILE_ELEMS, int NTM = NT_MID>
__global__ void __launch_bounds__(NTM)
k_dft_mid(uint32_t* data, uint64_t col_stride, unsigned log_len, unsigned log_T, unsigned row_shift,
          const uint32_t* __restrict__ W, const uint32_t* __restrict__ f_lo, const uint32_t* __restrict__ f_hi) {
    __shared__ uint32_t s[padded(TILE)];
    constexpr int PER_THREAD = TILE / NTM;
    if (PLAN == 1) {
        log_len = 8;
        log_T = 5;
    }
    const uint32_t j2_0 = blockIdx.x << log_T;
    uint32_t* g = data + (uint64_t)blockIdx.y * col_stride + j2_0;
    const uint32_t total = 1u << (log_len + log_T);
    const uint32_t tmask = (1u << log_T) - 1;
    // slot i of the tile is coefficient / element off(i) + j2_0 of the column
    auto off = [&](uint32_t i) { return ((i >> log_T) << row_shift) + (i & tmask); };
    if constexpr (PLAN == 1) {
        uint32_t t[PER_THREAD];
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) t[k] = g[off(threadIdx.x + (uint32_t)k * NTM)];
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) {
            const uint32_t i = threadIdx.x + (uint32_t)k * NTM;
            if (!INV && SCALE) t[k] = mont_mul_lazy(t[k], dft_factor(f_lo, f_hi, off(i) + j2_0));
            s[pad(i)] = t[k];
        }
    } else {
        for (uint32_t i = threadIdx.x; i < total; i += NTM) {
            uint32_t v = g[off(i)];
            if (!INV && SCALE) v = mont_mul_lazy(v, dft_factor(f_lo, f_hi, off(i) + j2_0));
            s[pad(i)] = v;
        }
    }
    __syncthreads();
    if constexpr (PLAN == 1) {
        if (!INV) {
            radix_round<4, false, 9, NTM, true>(s, 13, 0, 0, 0, W);
            radix_round<4, false, 5, NTM>(s, 13, 4, 0, 0, W);
        } else {
            radix_round<4, true, 5, NTM>(s, 13, 4, 0, 0, W);
            radix_round<4, true, 9, NTM, true>(s, 13, 0, 0, 0, W);
        }
    } else {
        if (!INV) tile_forward_rt<NTM>(s, log_len, log_T, 0, 0, W);
        else tile_inverse_rt<NTM>(s, log_len, log_T, 0, 0, W);
    }
    // forward with a contiguous pass to follow (row_shift != 0): that pass takes lazy values; everything
    // else is the end of a transform and leaves canonical ones (mont_mul of a value < 2p is canonical)
    auto finish = [&](uint32_t v, uint32_t i) {
        if (INV) return SCALE ? mont_mul(v, dft_factor(f_lo, f_hi, off(i) + j2_0)) : red2p(v);
        return row_shift != 0 ? v : red2p(v);
    };
    if constexpr (PLAN == 1) {
        uint32_t t[PER_THREAD];
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) t[k] = s[pad(threadIdx.x + (uint32_t)k * NTM)];
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) {
            const uint32_t i = threadIdx.x + (uint32_t)k * NTM;
            g[off(i)] = finish(t[k], i);
        }
    } else {
        for (uint32_t i = threadIdx.x; i < total; i += NTM) g[off(i)] = finish(s[pad(i)], i);
    }
}

// ------------------------------------------------------------------ contiguous pass, one direction
// chunk blockIdx.x of column blockIdx.y, in place: global stages log_n-LM .. log_n-1 (forward, after the
// strided pass: canonical out) or the same backwards (inverse, before it: lazy out)
template <int LM, bool INV>
__global__ void __launch_bounds__(chunk_threads(LM))
k_dft_contig(uint32_t* __restrict__ data, uint64_t col_stride, unsigned log_n, const uint32_t* __restrict__ W) {
    __shared__ uint32_t s[padded(1 << LM)];
    const uint32_t c = blockIdx.x;
    uint32_t* g = data + (uint64_t)blockIdx.y * col_stride + ((uint64_t)c << LM);
    chunk_load<LM>(s, g);
    chunk_rounds<LM, INV>(s, log_n - LM, c, W);
    chunk_store<LM, !INV>(s, g);
}

// ------------------------------------------------------------------ transposes
// src column-major, rows p < 2^log_h in bit-reversed order  ->  dst[bitrev(p)][c] row-major, natural rows
__global__ void __launch_bounds__(256)
k_transpose_unbitrev(const uint32_t* __restrict__ src, uint64_t col_stride, uint32_t* __restrict__ dst,
                     unsigned log_h, uint32_t w) {
    __shared__ uint32_t tile[64][65];
    const unsigned tr = log_h < 6 ? log_h : 6;  // log2 of tile rows
    const uint32_t rows = 1u << tr;
    const uint32_t p0 = blockIdx.x << tr;
    const uint32_t c0 = blockIdx.y * 64;
    const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    // 16 loads in flight (64 consecutive p of one column each), then 16 row pieces of 64 columns
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t c = c0 + ty + 4 * (uint32_t)k;
        if (c < w && tx < rows) tile[tx][ty + 4 * k] = src[(uint64_t)c * col_stride + p0 + tx];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t i = ty + 4 * (uint32_t)k;
        if (i < rows && c0 + tx < w) dst[(uint64_t)bitrev32(p0 + i, log_h) * w + c0 + tx] = tile[i][tx];
    }
}

void launch_transpose_unbitrev(Context& ctx, const uint32_t* src, uint64_t col_stride, uint32_t* dst,
                               unsigned log_h, uint32_t w) {
    if (w == 0) return;
    const unsigned tr = log_h < 6 ? log_h : 6;
    TS_LAUNCH(ctx, k_transpose_unbitrev, dim3(1u << (log_h - tr), (w + 63) / 64), dim3(256), 0, src, col_stride,
              dst, log_h, w);
    TS_HIP(hipGetLastError());
}

// dst[r] = src[bitrev(r)], both row-major h x w
__global__ void __launch_bounds__(256)
k_bit_reverse_rows(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, unsigned log_h, uint32_t w) {
    const uint64_t idx = ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    const uint64_t r = idx / w;
    if (r >> log_h) return;
    const uint32_t c = (uint32_t)(idx - r * w);
    dst[idx] = src[(uint64_t)bitrev32((uint32_t)r, log_h) * w + c];
}

void launch_bit_reverse_rows(Context& ctx, const uint32_t* src, uint32_t* dst, unsigned log_h, uint32_t w) {
    const uint64_t blocks = ((((uint64_t)w) << log_h) + 255) / 256;
    const uint32_t gx = (uint32_t)std::min<uint64_t>(blocks, 1u << 20);
    TS_LAUNCH(ctx, k_bit_reverse_rows, dim3(gx, (uint32_t)((blocks + gx - 1) / gx)), dim3(256), 0, src, dst, log_h, w);
    TS_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ host drivers
void dft_columns(Context& ctx, uint32_t* cols, uint64_t col_stride, uint32_t ncols, unsigned log_n, bool inverse,
                 uint32_t shift) {
    if (ncols == 0) return;
    TS_REQUIRE(shift != 0 && shift < P, TS_ERR_INVALID, "dft: the coset shift must be in [1, p)");
    TS_REQUIRE(ncols <= 65535, TS_ERR_INVALID, "dft: more than 65535 columns");
    const unsigned LM = lde_chunk_log(log_n);
    const bool two_pass = log_n > LM;
    const unsigned sA = two_pass ? log_n - LM : 0;  // stages of the strided pass
    // sA <= 13 fits the 8192-element tile, sA = 14 (n = 2^26) the 16384-element one, as in coset_lde
    TS_REQUIRE(sA <= 14, TS_ERR_INVALID, "dft: height above 2^26");
    TS_REQUIRE(!two_pass || col_stride % 4 == 0, TS_ERR_INVALID, "dft: column stride must be a multiple of 4 elements");
    ctx.ensure_twiddles(log_n == 0 ? 1 : log_n);
    const uint32_t* W = inverse ? ctx.d_twiddle_inv : ctx.d_twiddle_fwd;
    unsigned log_T = 0;
    if (two_pass && sA <= 13)
        while ((1u << (sA + log_T + 1)) <= (unsigned)TILE_ELEMS && log_T < 6) log_T++;

    // factor of coefficient k: shift^k (forward; none for shift 1) or shift^-k / n (inverse)
    const bool scale = inverse || shift != 1;
    DevBuf<uint32_t> lo, hi;
    if (scale) {
        const uint32_t n_hi = log_n > (unsigned)DFT_LO_BITS ? 1u << (log_n - DFT_LO_BITS) : 1u;
        lo = DevBuf<uint32_t>(&ctx, 1u << DFT_LO_BITS);
        hi = DevBuf<uint32_t>(&ctx, n_hi);
        const uint32_t n_inv = inv_canon((uint32_t)((1ull << log_n) % P));
        launch_build_shift_tables(ctx, lo.p, hi.p, n_hi, 1, to_mont(inverse ? inv_canon(shift) : shift), log_n, 0,
                                  inverse ? to_mont(n_inv) : R_MOD_P);
    }
    const uint32_t* flo = lo.p;
    const uint32_t* fhi = hi.p;

    auto contig = [&] {
        const dim3 g(1u << sA, ncols);
#define TS_DFT_CONTIG(LMV)                                                                                     \
    do {                                                                                                       \
        if (inverse)                                                                                           \
            TS_LAUNCH(ctx, (k_dft_contig<LMV, true>), g, dim3(chunk_threads(LMV)), 0, cols, col_stride, log_n, W); \
        else                                                                                                   \
            TS_LAUNCH(ctx, (k_dft_contig<LMV, false>), g, dim3(chunk_threads(LMV)), 0, cols, col_stride, log_n, W); \
    } while (0)
        if (LM == 12) TS_DFT_CONTIG(12);
        else if (LM == 13) TS_DFT_CONTIG(13);
        else TS_DFT_CONTIG(14);
#undef TS_DFT_CONTIG
    };
    auto mid = [&] {
        const dim3 grid(two_pass ? 1u << (LM - log_T) : 1u, ncols);
        const unsigned log_len = two_pass ? sA : log_n, row_shift = two_pass ? LM : 0;
#define TS_DFT_MID(...)                                                                                       \
    TS_LAUNCH(ctx, (k_dft_mid<__VA_ARGS__>), grid, dim3(NT_MID), 0, cols, col_stride, log_len, log_T, row_shift, W, \
              flo, fhi)
        const int plan = sA == 14 ? 2 : (sA == 8 && log_T == 5) ? 1 : 0;
        if (inverse) {
            if (plan == 2) TS_DFT_MID(true, true, 0, 16384);
            else if (plan == 1) TS_DFT_MID(true, true, 1);
            else TS_DFT_MID(true, true, 0);
        } else if (scale) {
            if (plan == 2) TS_DFT_MID(false, true, 0, 16384);
            else if (plan == 1) TS_DFT_MID(false, true, 1);
            else TS_DFT_MID(false, true, 0);
        } else {
            if (plan == 2) TS_DFT_MID(false, false, 0, 16384);
            else if (plan == 1) TS_DFT_MID(false, false, 1);
            else TS_DFT_MID(false, false, 0);
        }
#undef TS_DFT_MID
    };
    if (inverse) {
        if (two_pass) contig();
        mid();
    } else {
        mid();
        if (two_pass) contig();
    }
    TS_HIP(hipGetLastError());
}

void dft_batch(Context& ctx, const uint32_t* in, uint32_t* out, unsigned log_n, uint32_t w, bool inverse,
               uint32_t shift) {
    const uint64_t n = 1ull << log_n;
    DevBuf<uint32_t> cols(&ctx, (size_t)w * n);
    if (inverse) {
        launch_transpose_bitrev(ctx, in, cols.p, log_n, w, n);
        dft_columns(ctx, cols.p, n, w, log_n, true, shift);
        launch_transpose_to_row_major(ctx, cols.p, n, out, n, w);
    } else {
        launch_transpose_plain(ctx, in, cols.p, n, w, n);
        dft_columns(ctx, cols.p, n, w, log_n, false, shift);
        launch_transpose_unbitrev(ctx, cols.p, n, out, log_n, w);
    }
}

void coset_lde_batch(Context& ctx, const uint32_t* in, uint32_t* out, unsigned log_n, uint32_t w, unsigned added_bits,
                     uint32_t shift, bool bit_reversed) {
    const uint64_t n = 1ull << log_n, N = n << added_bits;
    DevBuf<uint32_t> cols(&ctx, (size_t)w * n), lde(&ctx, (size_t)w * N);
    // as Pcs::commit (prover_common.cpp lde_stage): the transpose takes the first inverse round where it can
    const bool r16 = launch_transpose_bitrev_r16(ctx, in, cols.p, log_n, w, n);
    if (!r16) launch_transpose_bitrev(ctx, in, cols.p, log_n, w, n);
    coset_lde(ctx, cols.p, n, w, log_n, added_bits, shift, lde.p, N, 0, 0, r16);
    if (bit_reversed) launch_transpose_to_row_major(ctx, lde.p, N, out, N, w);
    else launch_transpose_unbitrev(ctx, lde.p, N, out, log_n + added_bits, w);
}

}  // namespace ts
