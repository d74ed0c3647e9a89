// Standalone transforms of TwoAdicSubgroupDft on device matrices: dft_batch /
// coset_dft_batch, idft_batch / coset_idft_batch, coset_lde_batch, bit_reverse_rows -- what a caller that
// drives its own flow through the Dft and Pcs traits needs between ts_pcs_commit, ts_quotient_chunks and
// ts_pcs_open, without a trip to the host.
//
// The arithmetic is that of the coset LDE (ntt_lde.hip: block-twiddle radix-2 stages in register rounds of
// up to 16 / 32 elements, the padded LDS image -- ntt_rounds.hpp) under the same pass plan (ntt_plan.hpp).
// The contiguous passes ARE the LDE's: launch_contig_inverse / launch_contig_forward (ntt_lde.hip) run
// k_intt_contig on one matrix and k_lde_fwd_contig on one coset block.  What is new here is the strided pass on
// its own, in one direction:
//   k_dft_mid     the strided stages 0 .. sA-1 of ONE direction on tiles of 2^sA rows x 2^log_T slots,
//                 with the per-coefficient factor of a coset applied where the coefficients are:
//                 forward  x_k *= shift^k on the way in, then stages 0 .. sA-1   (natural in)
//                 inverse  stages sA-1 .. 0, then x_k *= shift^-k / n on the way out (natural, canonical out)
//                 For n <= 4096 it is the whole transform (one tile = one column).
//   k_bit_reverse_rows     row-major -> row-major, rows permuted
// (launch_transpose_unbitrev, ntt.hip: column-major with bit-reversed rows -> row-major with natural rows, the
// output transpose of the forward transforms and of the LDE, and -- on the first 2^log_size rows of a
// committed LDE -- get_evaluations_on_domain.)
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
template <bool INV, bool SCALE, int PLAN, int TILE = TILE_ELEMS, int NTM = NT_MID, class TW = uint32_t>
__global__ void __launch_bounds__(NTM)
k_dft_mid(uint32_t* data, uint64_t col_stride, unsigned log_len, unsigned log_T, unsigned row_shift,
          const TW* __restrict__ W, const uint32_t* __restrict__ f_lo, const uint32_t* __restrict__ f_hi) {
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

// ------------------------------------------------------------------ row permutation
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
// the twiddle form of each instantiation of k_dft_mid, by the rule of ntt_lde.hip (ContigForm / MidForm)
template <bool INV, int PLAN, int TILE> struct DftMidFormOf {
    using type = uint2;
};
// the inverse run-time plan on the 8192-element tile: 61 -> 65 VGPRs, three workgroups per CU instead of four
template <> struct DftMidFormOf<true, 0, TILE_ELEMS> {
    using type = uint32_t;
};
template <bool INV, int PLAN, int TILE> using DftMidForm = typename DftMidFormOf<INV, PLAN, TILE>::type;

// the strided pass of one direction (the whole transform when the plan has one pass); `names`: the kernel-timer
// names of the three variants in NttMid's order, spelled as tools/time_dft.py has always printed them
template <bool INV, bool SCALE>
static void launch_dft_mid_of(Context& ctx, const NttPlan& p, uint32_t* cols, uint64_t col_stride, uint32_t ncols,
                              const uint32_t* f_lo, const uint32_t* f_hi, const char* const (&names)[3]) {
    const TwTables W = INV ? twiddles_inv(ctx) : twiddles_fwd(ctx);
    auto launch = [&](auto kernel) {
        TS_LAUNCH_NAMED(ctx, names[(int)p.mid], kernel, dim3(p.tiles, ncols), dim3(NT_MID), 0, cols, col_stride,
                        p.log_len, p.log_T, p.row_shift, W, f_lo, f_hi);
    };
    if (p.mid == NttMid::TILE16384) launch(k_dft_mid<INV, SCALE, 0, 16384, NT_MID, DftMidForm<INV, 0, 16384>>);
    else if (p.mid == NttMid::FIXED256) launch(k_dft_mid<INV, SCALE, 1, TILE_ELEMS, NT_MID, DftMidForm<INV, 1, TILE_ELEMS>>);
    else launch(k_dft_mid<INV, SCALE, 0, TILE_ELEMS, NT_MID, DftMidForm<INV, 0, TILE_ELEMS>>);
}

static void launch_dft_mid(Context& ctx, const NttPlan& p, uint32_t* cols, uint64_t col_stride, uint32_t ncols,
                           bool inverse, bool scale, const uint32_t* f_lo, const uint32_t* f_hi) {
    if (inverse)
        launch_dft_mid_of<true, true>(ctx, p, cols, col_stride, ncols, f_lo, f_hi,
                                      {"(k_dft_mid<true, true, 0>)", "(k_dft_mid<true, true, 1>)",
                                       "(k_dft_mid<true, true, 0, 16384>)"});
    else if (scale)
        launch_dft_mid_of<false, true>(ctx, p, cols, col_stride, ncols, f_lo, f_hi,
                                       {"(k_dft_mid<false, true, 0>)", "(k_dft_mid<false, true, 1>)",
                                        "(k_dft_mid<false, true, 0, 16384>)"});
    else
        launch_dft_mid_of<false, false>(ctx, p, cols, col_stride, ncols, f_lo, f_hi,
                                        {"(k_dft_mid<false, false, 0>)", "(k_dft_mid<false, false, 1>)",
                                         "(k_dft_mid<false, false, 0, 16384>)"});
}

void dft_columns(Context& ctx, uint32_t* cols, uint64_t col_stride, uint32_t ncols, unsigned log_n, bool inverse,
                 uint32_t shift) {
    if (ncols == 0) return;
    TS_REQUIRE(shift != 0 && shift < P, TS_ERR_INVALID, "dft: the coset shift must be in [1, p)");
    const NttPlan p = ntt_plan(log_n);
    ntt_require_shape(p, ncols, col_stride, 0, false);
    ctx.ensure_twiddles(log_n == 0 ? 1 : log_n);
    ctx.ensure_plant_twiddles(log_n == 0 ? 1 : log_n, log_n == 0 ? 1 : log_n);

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
    if (inverse) {
        if (p.two_pass) launch_contig_inverse(ctx, p, cols, col_stride, ncols);
        launch_dft_mid(ctx, p, cols, col_stride, ncols, true, true, lo.p, hi.p);
    } else {
        launch_dft_mid(ctx, p, cols, col_stride, ncols, false, scale, lo.p, hi.p);
        if (p.two_pass) launch_contig_forward(ctx, p, cols, col_stride, ncols, 1, 0, 0);
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
    // as Pcs::commit (prover_common.cpp lde_stage): the transpose takes the first inverse round where it can --
    // unless the input is one of the LDE's blocks (lde_batch: shift 1), which coset_lde then copies from `cols`
    const bool r16 = lde_own_coset_used(log_n, added_bits, shift) < 0 &&
                     launch_transpose_bitrev_r16(ctx, in, cols.p, log_n, w, n);
    if (!r16) launch_transpose_bitrev(ctx, in, cols.p, log_n, w, n);
    coset_lde(ctx, cols.p, n, w, log_n, added_bits, shift, lde.p, N, 0, 0, r16);
    if (bit_reversed) launch_transpose_to_row_major(ctx, lde.p, N, out, N, w);
    else launch_transpose_unbitrev(ctx, lde.p, N, out, log_n + added_bits, w);
}

}  // namespace ts
