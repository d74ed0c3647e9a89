// Device helpers the opening kernels share (open.hip: one table, one statement; open_multi.hip: the height
// classes of a multi-table proof): the row's domain point, the lazily accumulated alpha-power row dot, the
// pair of inverse denominators with one base-field inversion, and one workgroup's share of a barycentric
// finishing pass.  Device code only.
#pragma once
#include "kernels.hpp"

namespace ts {

// omega_{2^L}^bitrev_L(r) in Montgomery form from the block-twiddle table
__device__ __forceinline__ uint32_t root_bitrev(const uint32_t* __restrict__ W, unsigned L, uint64_t r) {
    if (L == 0) return R_MOD_P;
    uint32_t w = W[((uint64_t)1 << (L - 1)) + (r >> 1)];
    return (r & 1) ? neg(w) : w;
}

// out[j] = sum over blocks of partial[block][j]  (mod p); one workgroup per 4 output words (BaryFinishJob,
// kernels.hpp): one workgroup's four output words of one job
__device__ __forceinline__ void bary_finish_group(const uint32_t* __restrict__ partial, uint32_t* __restrict__ out,
                                                  uint32_t n_blocks, uint32_t n_words, uint32_t group) {
    __shared__ uint32_t red[4][4];
    const uint32_t j = group * 4 + (threadIdx.x & 3);
    uint32_t v = 0;
    if (j < n_words) {
        // eight loads in flight (as one load and one add per trip every trip waited for its own load: with
        // 2048 partial blocks that was 32 round trips to L2, 10-14 us for a kernel that moves kilobytes)
        uint32_t b = threadIdx.x >> 2;
        for (; b + 7 * 64 < n_blocks; b += 8 * 64) {
            uint32_t x[8];
#pragma unroll
            for (int k = 0; k < 8; k++) x[k] = partial[(uint64_t)(b + 64 * k) * n_words + j];
#pragma unroll
            for (int k = 0; k < 8; k++) v = add(v, x[k]);
        }
        for (; b < n_blocks; b += 64) v = add(v, partial[(uint64_t)b * n_words + j]);
    }
    // reduce over the 64 threads that share (threadIdx.x & 3): lanes 4 apart within a wave, 4 waves
#pragma unroll
    for (int off = 32; off >= 4; off >>= 1) v = add(v, __shfl_down(v, off, 64));
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane < 4) red[wv][lane] = v;
    __syncthreads();
    if (threadIdx.x < 4 && j < n_words)
        out[j] = add(add(red[0][threadIdx.x], red[1][threadIdx.x]),
                     add(red[2][threadIdx.x], red[3][threadIdx.x]));
}

// acc[0..3] += sum_i w_i * p_i[X] over `width` columns (lazy: acc stays below p*2^32 between calls)
__device__ __forceinline__ void row_dot_acc(uint64_t (&acc)[4], const uint32_t* __restrict__ m,
                                            uint64_t col_stride, uint32_t width, uint64_t X,
                                            const uint32_t* __restrict__ weights) {
    uint64_t a0 = acc[0], a1 = acc[1], a2 = acc[2], a3 = acc[3];
    // batches of 8 columns: the 8 loads are issued back to back (one load per iteration with a
    // wait behind it left the kernel latency-bound), then 32 MACs with a range fix every 2 columns
    constexpr int B = 8;
    const uint32_t* col = m + X;
    uint32_t i = 0;
    for (; i + B <= width; i += B) {
        uint32_t v[B];
#pragma unroll
        for (int k = 0; k < B; k++) v[k] = col[(uint64_t)(i + k) * col_stride];
#pragma unroll
        for (int k = 0; k < B; k++) {
            const uint32_t* ap = weights + 4 * (i + k);
            a0 = lazy_mac(a0, v[k], ap[0]);
            a1 = lazy_mac(a1, v[k], ap[1]);
            a2 = lazy_mac(a2, v[k], ap[2]);
            a3 = lazy_mac(a3, v[k], ap[3]);
            if (k & 1) {
                a0 = lazy_fix(a0);
                a1 = lazy_fix(a1);
                a2 = lazy_fix(a2);
                a3 = lazy_fix(a3);
            }
        }
    }
    // tail (< 8 columns): same pattern, predicated loads
    if (i < width) {
        uint32_t v[B];
#pragma unroll
        for (int k = 0; k < B; k++) v[k] = i + k < width ? col[(uint64_t)(i + k) * col_stride] : 0u;
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (i + k < width) {
                const uint32_t* ap = weights + 4 * (i + k);
                a0 = lazy_mac(a0, v[k], ap[0]);
                a1 = lazy_mac(a1, v[k], ap[1]);
                a2 = lazy_mac(a2, v[k], ap[2]);
                a3 = lazy_mac(a3, v[k], ap[3]);
            }
            if (k & 1) {
                a0 = lazy_fix(a0);
                a1 = lazy_fix(a1);
                a2 = lazy_fix(a2);
                a3 = lazy_fix(a3);
            }
        }
    }
    acc[0] = a0; acc[1] = a1; acc[2] = a2; acc[3] = a3;
}
// S(X) = sum_i alpha^i * p_i[X]  (dot_ext_powers, :375), canonical; alpha powers are wave-uniform
__device__ __forceinline__ Ef row_dot_alpha(const uint32_t* __restrict__ m, uint64_t col_stride,
                                            uint32_t width, uint64_t X,
                                            const uint32_t* __restrict__ alpha_pows) {
    uint64_t acc[4] = {0, 0, 0, 0};
    row_dot_acc(acc, m, col_stride, width, X, alpha_pows);
    return Ef{{lazy_finish(acc[0]), lazy_finish(acc[1]), lazy_finish(acc[2]), lazy_finish(acc[3])}};
}

// 1/(x - z_p) for NP points with one shared base-field inversion (Montgomery)
template <int NP>
__device__ __forceinline__ void inv_denoms(uint32_t x_mont, const Ef* z_mont, Ef* out) {
    Ef num[NP];
    uint32_t nrm[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const Ef z = z_mont[p];
        Ef u = Ef{{sub(x_mont, z.c[0]), neg(z.c[1]), neg(z.c[2]), neg(z.c[3])}};  // x - z
        ef_inv_parts(u, num[p], nrm[p]);
    }
    if (NP == 2) {
        uint32_t inv = mont_inv(mont_mul(nrm[0], nrm[NP - 1]));
        out[0] = ef_mul_base(num[0], mont_mul(inv, nrm[NP - 1]));
        out[NP - 1] = ef_mul_base(num[NP - 1], mont_mul(inv, nrm[0]));
    } else {
        out[0] = ef_mul_base(num[0], mont_inv(nrm[0]));
    }
}

}  // namespace ts
