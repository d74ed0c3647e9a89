// The register-radix rounds and the padded LDS image of the NTT kernels, shared by the coset LDE
// (ntt_lde.hip, whose header describes the image and the plan) and the standalone transforms
// (ntt_dft.hip).  Device code only: include from a .hip file.  The pass plan itself -- chunk size, tile
// shape, kernel variant -- is host code: ntt_plan.hpp.
#pragma once
#include "kernels.hpp"
#include "ntt_plan.hpp"

namespace ts {

constexpr int NT_MID = 512;        // threads per workgroup, middle kernel
// threads per workgroup of the contiguous kernels: 16 elements per thread at LM = 12, 32 above
constexpr int chunk_threads(int lm) { return lm == 14 ? 512 : 256; }

__device__ __forceinline__ uint32_t pad(uint32_t i) { return i + (i >> 5); }
constexpr int padded(int n) { return n + (n >> 5); }

// The LDS image `s` (padded) holds 2^log_total elements: a transform of 2^log_len points whose
// element e occupies the 2^log_T consecutive slots [e << log_T, (e+1) << log_T) (log_T = 0 for a
// contiguous chunk; for a strided tile the 2^log_T slots are independent side-by-side transforms
// that share their twiddles).  Local stage u (distance 2^(log_total-1-u) slots) is global stage
// s_base + u, whose block `blk` uses W[2^(s_base+u) + (c << u) + blk].
//
// One round = K consecutive stages u0 .. u0+K-1 on register groups of 2^K elements spaced by the
// distance 2^log_dl of the round's last stage.  LOG_DL >= 0 fixes that distance at compile time
// (LDS addresses become base + immediate offsets); LOG_DL = -1 takes it from the arguments.
// The K stages of one register group v[0 .. 2^K): global stages s_base + u0 .. + K - 1 on the group
// whose block index at stage u0 is `hi` (chunk c).
//
// The twiddle table's element type selects the product, and with it the ranges (stated here, once):
//   const uint32_t*  Montgomery words (Context::d_twiddle_fwd / _inv).  Forward and inverse: inputs and outputs
//                    in the lazy range [0, 2p), right mod p.  10 VALU instructions per multiplied butterfly
//                    (forward 2 + 5 + 1 + 2: a -> [0, p), t = mont_mul in [0, p), a + t, a - t + p; inverse
//                    4 + 1 + 2 + 3 with the product left in [0, 2p)).
//   const uint2*     Plantard words {low, high} (Context::d_plant_fwd / _inv; bb.hpp plant_mul: any 32-bit
//                    operand in, canonical product out, 3 instructions).  8 per multiplied butterfly.
//                    Forward: inputs and outputs in [0, 2p) as above (2 + 3 + 1 + 2).
//                    Inverse: inputs CANONICAL, outputs canonical: add(a, b) and plant_mul(a - b + p)
//                    (3 + 2 + 3; a twiddle-1 butterfly of a TOP round is add and sub).  Nothing needs reducing
//                    between the passes of an inverse transform; a producer that leaves lazy values (a
//                    Montgomery pass) has to be reduced on load by the pass that takes this form.
// mul: canonical product; mul_lazy: product in [0, 2p) where that is cheaper (Montgomery)
template <class TW> struct TwForm;
template <> struct TwForm<uint32_t> {
    static constexpr bool plantard = false;
    static __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t w) { return mont_mul(a, w); }
    static __device__ __forceinline__ uint32_t mul_lazy(uint32_t a, uint32_t w) { return mont_mul_lazy(a, w); }
};
template <> struct TwForm<uint2> {
    static constexpr bool plantard = true;
    static __device__ __forceinline__ uint32_t mul(uint32_t a, uint2 w) { return plant_mul(a, w.x, w.y); }
    static __device__ __forceinline__ uint32_t mul_lazy(uint32_t a, uint2 w) { return mul(a, w); }
};

// Host side: both tables of one direction; the parameter type of the kernel launched picks its own.
struct TwTables {
    const uint32_t* mont;
    const uint2* plant;
    operator const uint32_t*() const { return mont; }
    operator const uint2*() const { return plant; }
};
inline TwTables twiddles_fwd(const Context& ctx) { return TwTables{ctx.d_twiddle_fwd, ctx.d_plant_fwd}; }
inline TwTables twiddles_inv(const Context& ctx) { return TwTables{ctx.d_twiddle_inv, ctx.d_plant_inv}; }

template <int K, bool INV, bool TOP, class TW>
__device__ __forceinline__ void radix_butterflies(uint32_t (&v)[1 << K], unsigned s_base, unsigned u0,
                                                  uint32_t c, uint32_t hi,
                                                  const TW* __restrict__ W) {
    using F = TwForm<TW>;
    constexpr int R = 1 << K;
    if (!INV) {
#pragma unroll
        for (int d = 0; d < K; d++) {
            const int half = R >> (d + 1);
            // ONE address per stage: the 2^d twiddles of this group are consecutive words, read at
            // immediate offsets from wp (indexing W[wb + j] made the compiler rebuild a 64-bit
            // address for every j: ~3 VALU instructions per twiddle, 8 % of a contiguous pass)
            const TW* __restrict__ wp = W + ((1u << (s_base + u0 + d)) + (c << (u0 + d)) + (hi << d));
#pragma unroll
            for (int q = 0; q < R; q++) {
                if ((q & half) == 0) {
                    // a -> [0, p), t in [0, p), a + t and a - t + p in [0, 2p) (2p < 2^32)
                    const uint32_t a = red2p(v[q]);
                    uint32_t t = v[q + half];
                    if (TOP && (q >> (K - d)) == 0) t = red2p(t);
                    else t = F::mul(t, wp[q >> (K - d)]);
                    v[q] = a + t;
                    v[q + half] = a - t + P;
                }
            }
        }
    } else {
#pragma unroll
        for (int d = K - 1; d >= 0; d--) {
            const int half = R >> (d + 1);
            const TW* __restrict__ wp = W + ((1u << (s_base + u0 + d)) + (c << (u0 + d)) + (hi << d));
#pragma unroll
            for (int q = 0; q < R; q++) {
                if ((q & half) == 0) {
                    const bool one = TOP && (q >> (K - d)) == 0;  // twiddle 1
                    if (F::plantard) {
                        const uint32_t a = v[q], b = v[q + half];
                        v[q] = add(a, b);
                        v[q + half] = one ? sub(a, b) : F::mul(a - b + P, wp[q >> (K - d)]);
                    } else {
                        // lazy range [0, 2p) in and out: the product is left uncorrected
                        const uint32_t a = red2p(v[q]), b = red2p(v[q + half]);
                        v[q] = a + b;
                        uint32_t dlt = a - b + P;
                        if (!one) dlt = F::mul_lazy(dlt, wp[q >> (K - d)]);
                        v[q + half] = dlt;
                    }
                }
            }
        }
    }
}

// TOP = true: the round starts at global stage 0 of a whole transform (s_base = u0 = c = 0, one group
// block): block 0 of every stage has the twiddle w^0 = 1, i.e. butterflies with q < 2^(K-d) at local
// stage d need no multiplication (all of stage 0, half of stage 1, ...: 47 % of a radix-16 round).
template <int K, bool INV, int LOG_DL, int NTH, bool TOP = false, class TW>
__device__ __forceinline__ void radix_round(uint32_t* s, unsigned log_total, unsigned u0,
                                            unsigned s_base, uint32_t c,
                                            const TW* __restrict__ W) {
    constexpr int R = 1 << K;
    const unsigned log_dl = LOG_DL >= 0 ? (unsigned)LOG_DL : log_total - u0 - K;
    const uint32_t n_groups = 1u << (log_total - K);
    for (uint32_t g0 = threadIdx.x; g0 < n_groups; g0 += NTH) {
        uint32_t g = g0;
        if (LOG_DL == 4 && K < 5) {
            // distance 16: lanes 0-15 of a half-wave are the 16 `lo` of one block, lanes 16-31 those
            // of the block 2^(5-K) further (header comment): swap bits 4 and 9-K of the group index
            constexpr uint32_t B = 9 - K;
            const uint32_t x = ((g >> 4) ^ (g >> B)) & 1u;
            g ^= (x << 4) | (x << B);
        }
        const uint32_t lo = g & ((1u << log_dl) - 1);
        const uint32_t hi = g >> log_dl;  // block index at stage u0
        const uint32_t base = (hi << (K + log_dl)) + lo;
        const uint32_t pbase = pad(base);
        uint32_t addr[R];
#pragma unroll
        for (int q = 0; q < R; q++) {
            if (LOG_DL >= 5)  // base + (q << d) with d >= 5: the pad grows by q << (d - 5)
                addr[q] = pbase + (uint32_t)q * ((1u << (LOG_DL >= 5 ? LOG_DL : 5)) +
                                                 (1u << (LOG_DL >= 5 ? LOG_DL - 5 : 0)));
            else if (LOG_DL == 4)  // lo < 16 and the block offset is a multiple of 32
                addr[q] = pbase + 16u * (uint32_t)q + ((uint32_t)q >> 1);
            else if (LOG_DL == 0 && K == 4)  // the group's 16 words share one pad value
                addr[q] = pbase + (uint32_t)q;
            else
                addr[q] = pad(base + ((uint32_t)q << log_dl));
        }
        uint32_t v[R];
#pragma unroll
        for (int q = 0; q < R; q++) v[q] = s[addr[q]];
        radix_butterflies<K, INV, TOP>(v, s_base, u0, c, hi, W);
#pragma unroll
        for (int q = 0; q < R; q++) s[addr[q]] = v[q];
    }
    __syncthreads();
}

template <bool INV, int NTH, class TW>
__device__ __forceinline__ void radix_round_rt(int k, uint32_t* s, unsigned log_total, unsigned u0,
                                               unsigned s_base, uint32_t c,
                                               const TW* __restrict__ W) {
    switch (k) {
        case 4: radix_round<4, INV, -1, NTH>(s, log_total, u0, s_base, c, W); break;
        case 3: radix_round<3, INV, -1, NTH>(s, log_total, u0, s_base, c, W); break;
        case 2: radix_round<2, INV, -1, NTH>(s, log_total, u0, s_base, c, W); break;
        default: radix_round<1, INV, -1, NTH>(s, log_total, u0, s_base, c, W); break;
    }
}

// Generic plan: log_len stages in ceil(log_len/4) rounds of nearly equal size (10 = 4+3+3): the
// first `rem` rounds take q+1 stages, the others q.
template <int NTH, class TW>
__device__ __forceinline__ void tile_forward_rt(uint32_t* s, unsigned log_len, unsigned log_T,
                                                unsigned s_base, uint32_t c,
                                                const TW* __restrict__ W) {
    if (log_len == 0) return;
    const unsigned nr = (log_len + 3) / 4, q = log_len / nr, rem = log_len % nr;
    unsigned u = 0;
    for (unsigned r = 0; r < nr; r++) {
        const unsigned k = q + (r < rem ? 1u : 0u);
        radix_round_rt<false, NTH>((int)k, s, log_len + log_T, u, s_base, c, W);
        u += k;
    }
}
template <int NTH, class TW>
__device__ __forceinline__ void tile_inverse_rt(uint32_t* s, unsigned log_len, unsigned log_T,
                                                unsigned s_base, uint32_t c,
                                                const TW* __restrict__ Winv) {
    if (log_len == 0) return;
    const unsigned nr = (log_len + 3) / 4, q = log_len / nr, rem = log_len % nr;
    unsigned u = log_len;
    for (int r = (int)nr - 1; r >= 0; r--) {
        const unsigned k = q + ((unsigned)r < rem ? 1u : 0u);
        u -= k;
        radix_round_rt<true, NTH>((int)k, s, log_len + log_T, u, s_base, c, Winv);
    }
}

// ------------------------------------------------------------------ contiguous passes (static plan)
// 2^LM-element chunk: LM = 12: 3 radix-16 rounds (last-stage distances 256, 16, 1); LM = 13: radix-32
// (distance 256), radix-16 (16), radix-16 (1); LM = 14: radix-32 (512), radix-32 (16), radix-16 (1).
template <int LM>
__device__ __forceinline__ void chunk_load(uint32_t* s, const uint32_t* __restrict__ g) {
    constexpr int NT = chunk_threads(LM);
    const uint4* g4 = reinterpret_cast<const uint4*>(g);
    uint4 v[(1 << LM) / 4 / NT];
#pragma unroll
    for (int k = 0; k < (1 << LM) / 4 / NT; k++) v[k] = g4[threadIdx.x + (uint32_t)k * NT];
#pragma unroll
    for (int k = 0; k < (1 << LM) / 4 / NT; k++) {
        const uint32_t i4 = threadIdx.x + (uint32_t)k * NT;
        const uint32_t a = 4 * i4 + (i4 >> 3);  // pad(4*i4); the 4 words stay inside one 32-group
        s[a] = v[k].x;
        s[a + 1] = v[k].y;
        s[a + 2] = v[k].z;
        s[a + 3] = v[k].w;
    }
    __syncthreads();
}
// The butterflies leave values in [0, 2p).  CANON: canonical form on the way to HBM (the LDE itself).
// Between the passes of one transform the next pass reduces its inputs anyway (red2p on `a`, a
// product with b < 2p is still < p 2^32), so intermediate images stay lazy: 2 VALU instructions per
// element less, in kernels that are bound by VALU issue.
template <int LM, bool CANON>
__device__ __forceinline__ void chunk_store(const uint32_t* s, uint32_t* __restrict__ g) {
    constexpr int NT = chunk_threads(LM);
    uint4* g4 = reinterpret_cast<uint4*>(g);
#pragma unroll
    for (int k = 0; k < (1 << LM) / 4 / NT; k++) {
        const uint32_t i4 = threadIdx.x + (uint32_t)k * NT;
        const uint32_t a = 4 * i4 + (i4 >> 3);
        if (CANON)
            g4[i4] = make_uint4(red2p(s[a]), red2p(s[a + 1]), red2p(s[a + 2]), red2p(s[a + 3]));
        else
            g4[i4] = make_uint4(s[a], s[a + 1], s[a + 2], s[a + 3]);
    }
}

// the LM local stages of a chunk, forward (u = 0 .. LM-1) or inverse (backwards)
// SKIP_R16 (inverse only): the round at distance 1 was done by k_transpose_bitrev_r16 already.
template <int LM, bool INV, bool SKIP_R16 = false, class TW>
__device__ __forceinline__ void chunk_rounds(uint32_t* s, unsigned sb, uint32_t c, const TW* __restrict__ W) {
    constexpr int NT = chunk_threads(LM);
    constexpr int K0 = LM == 12 ? 4 : 5;   // stages 0 .. K0-1, distance 2^(LM - K0)
    constexpr int K1 = LM == 14 ? 5 : 4;   // stages K0 .. K0+K1-1, distance 16
    static_assert(K0 + K1 + 4 == LM, "chunk plan");
    if (!INV) {
        radix_round<K0, false, LM - K0, NT>(s, LM, 0, sb, c, W);
        radix_round<K1, false, 4, NT>(s, LM, K0, sb, c, W);
        radix_round<4, false, 0, NT>(s, LM, K0 + K1, sb, c, W);
    } else {
        if (!SKIP_R16) radix_round<4, true, 0, NT>(s, LM, K0 + K1, sb, c, W);
        radix_round<K1, true, 4, NT>(s, LM, K0, sb, c, W);
        radix_round<K0, true, LM - K0, NT>(s, LM, 0, sb, c, W);
    }
}

}  // namespace ts
