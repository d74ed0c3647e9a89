// Coset LDE kernels (see the header of ntt.hip for the block-twiddle formulation).
//
// Execution: up to 4 stages at a time are done in registers (a thread owns the 16 elements of a
// radix-16 group), with one LDS exchange between such rounds.  LDS image: element i lives at word
// i + (i >> 5).  On gfx950 a ds_read_b32 / ds_write_b32 is served in two 32-lane groups over 32
// banks ((byte address / 4) mod 32), so an access is conflict-free when the 32 lanes of a half-wave
// hit 32 distinct words mod 32.  With one pad word per 32:
//   - 32 consecutive elements from a multiple of 32 (tile loads, rounds at distance >= 32): one pad
//     value for the run -> 32 consecutive banks;
//   - the 16 g + q pattern of the distance-1 round (lane = group g): 16 g + (g >> 1) mod 32 takes
//     every value once over 32 consecutive g;
//   - the distance-16 round (16 lanes = consecutive elements, the other 16 = another block `hi`):
//     a block step moves the bank by 2^(K-1) mod 32, so the two halves of a half-wave take blocks
//     2^(5-K) apart (radix_round swaps two bits of the lane -> group map for that);
//   - the 16-byte chunk loads / stores (lane t: words 4 t + j): 4 t + j + (t >> 3) mod 32, distinct.
// (Rounds 1-3 padded one word per 16, right for 16-lane groups: rocprofv3 showed
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.33 / 0.50 / 0.40 for the three big kernels,
// profiles/r03_config3_sq_counters.txt -- lanes 0 and 31 of every 32-element run met on one bank.)
// Three kernels:
//   k_intt_contig    stages log_n-1 .. sA of the inverse on 2^LM-element chunks   (only n > 2^LM)
//   k_lde_mid        the strided stages of the inverse (sA-1 .. 0), coefficient k scaled once by
//                    shift^k / n, then for every coset the strided stages of the forward transform,
//                    writing coset block beta -- the coefficients never touch HBM
//   k_lde_fwd_contig stages sA .. log_n-1 of the forward transform, in place on 2^LM-element chunks
// For n <= 4096 k_lde_mid alone does everything.
//
// COSET TWIDDLES.  Block beta of the LDE holds the values on s_beta H_n, s_beta = shift w_N^bitrev_b(beta)
// (N = n 2^b): the n-point forward transform of the coefficients times s_beta^k.  The coset's own part of that
// factor, w_N^(bitrev_b(beta) k), is what the N-point transform of the zero-padded coefficients applies on the
// way to block beta: its first b stages only copy, and stage s + b uses, on block (beta << s) + blk,
//     W[2^(s+b) + (beta << s) + blk] = w_{2^(s+1)}^bitrev_s(blk) * w_{2^(s+b+1)}^bitrev_b(beta)
// -- the n-point twiddle of local stage s times the factor's ratio across that stage's distance.  So the forward
// rounds of coset beta run with the ordinary table, stage base s_base = b and chunk index c = beta (plus the
// chunk's own bits in the contiguous pass): the index form radix_butterflies has anyway.  What is left of the
// factor, shift^k / n, does not depend on the coset and is applied once, after the inverse rounds, from a table of
// n words per (n, shift) (coset_scale_table; the constant 1/n for shift 1) -- no per-coset table of n 2^b words
// (16 MB at 2^20 x 4 cosets, 268 MB at 2^22 x 16), no multiply and no table load inside the coset loop.  The
// forward tables reach log_n + b for it (Context::ensure_lde_twiddles); the inverse Plantard table stays at log_n.
//
// The contiguous chunk is 2^LM elements, LM = 12 except for n = 2^21 and 2^22, where it grows to
// 2^13 / 2^14 (LM = log_n - 8) so that the strided pass keeps the shape it has at n = 2^20 -- 8
// strided stages on 256-row x 128-byte tiles, two 512-thread workgroups per CU, one LDS round per
// coset (PLAN 1) -- instead of 9 / 10 stages on tiles whose rows are 64 bytes wide and whose
// 1024-thread workgroup has a CU to itself (round 2, 2^22 x 64 at log_blowup 4: that pass ran at VALU
// busy 0.67 with 44 % of its wave-cycles parked at barriers and scale-table loads).  The extra one
// or two stages go to the contiguous passes as radix-32 register rounds (13 = 5+4+4, 14 = 5+5+4):
// still three LDS round trips per chunk.
//
// Those decisions are made in one place, ntt_plan(log_n) (ntt_plan.hpp, host only); the launchers at the end
// of this file turn a plan into grids.  The two contiguous kernels also serve the standalone transforms
// (ntt_dft.hip) through launch_contig_inverse / launch_contig_forward: an inverse pass on one matrix, a
// forward pass on one coset block.
#include <stdlib.h>

#include <algorithm>
#include <optional>
#include <type_traits>

#include "ntt_rounds.hpp"

namespace ts {

// chunk `c` of column blockIdx.y: global stages log_n-1 .. log_n-LM of the inverse (n > 2^LM)
template <int LM, bool SKIP_R16 = false, class TW = uint32_t>
__global__ void __launch_bounds__(chunk_threads(LM))
k_intt_contig(uint32_t* __restrict__ data, uint64_t col_stride, unsigned log_n,
              const TW* __restrict__ Winv, uint32_t* __restrict__ data2, uint32_t gw) {
    __shared__ uint32_t s[padded(1 << LM)];
    const uint32_t c = blockIdx.x;
    // columns gw .. of a two-matrix launch live in the second matrix (coset_lde: evals2)
    uint32_t* col = blockIdx.y < gw ? data + (uint64_t)blockIdx.y * col_stride
                                    : data2 + (uint64_t)(blockIdx.y - gw) * col_stride;
    uint32_t* g = col + ((uint64_t)c << LM);
    chunk_load<LM>(s, g);
    chunk_rounds<LM, true, SKIP_R16>(s, log_n - LM, c, Winv);
    chunk_store<LM, false>(s, g);  // read next by k_lde_mid's inverse rounds (Plantard form: canonical as they are)
}

// The transpose of a row-major trace (src[r][c], natural rows -> dst[c][p], p = bitrev(r)) with the
// first round of the inverse transform folded in.  That round works on groups of 16 consecutive p,
// i.e. on the source rows bitrev(16 G + q): whole 256-byte row pieces whatever the group, so the
// thread that owns (group, column) loads its 16 values coalesced across the 64 columns of the tile,
// runs the four stages in registers and hands the results to the 64 x 64 LDS tile the transpose goes
// through anyway.  The transpose alone is bound by memory (its VALU idles); k_intt_contig then has
// two rounds and two LDS round trips left instead of three.
__global__ void __launch_bounds__(256)
k_transpose_bitrev_r16(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, unsigned log_n,
                       uint32_t w, uint64_t dst_col_stride, uint32_t src_width,
                       const uint2* __restrict__ Winv) {
    __shared__ uint32_t tile[64][65];
    const uint32_t p0 = blockIdx.x << 6;
    const uint32_t c0 = blockIdx.y * 64;
    const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    // bitrev(p0 + i) = bitrev(p0) + (bitrev6(i) << (log_n - 6)): p0 is a multiple of 64
    const uint32_t rb = bitrev32(p0, log_n);
    const uint64_t row_step = (uint64_t)src_width << (log_n - 6);
    uint32_t v[16];
    if (c0 + tx < w) {
        const uint32_t* sp = src + (uint64_t)rb * src_width + c0 + tx;
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] = sp[(uint64_t)(__brev(16 * ty + (uint32_t)q) >> 26) * row_step];
    } else {
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] = 0;
    }
    // global stages log_n-1 .. log_n-4 on group (p0 >> 4) + ty (Plantard form: canonical words in, canonical out)
    radix_butterflies<4, true, false>(v, log_n - 4, 0, 0, (p0 >> 4) + ty, Winv);
#pragma unroll
    for (int q = 0; q < 16; q++) tile[16 * ty + q][tx] = v[q];
    __syncthreads();
    uint32_t t[16];
#pragma unroll
    for (int k = 0; k < 16; k++) t[k] = tile[tx][ty + 4 * k];
    uint32_t* dp = dst + (uint64_t)(c0 + ty) * dst_col_stride + p0 + tx;
#pragma unroll
    for (int k = 0; k < 16; k++)
        if (c0 + ty + 4 * k < w) dp[(uint64_t)(4 * k) * dst_col_stride] = t[k];
}

// in place on chunk `c` of block `bl` of column blockIdx.y, coset beta = beta0 + bl of an LDE of blowup 2^log_b:
// forward stages sA .. log_n-1 of the n-point transform with the coset's own factor folded into the twiddles,
// i.e. stages sA + log_b .. of the N-point transform on block beta (the header's "coset twiddles"); a standalone
// transform is log_b = 0, beta = 0.
// CPW > 1: a workgroup takes CPW consecutive chunks and loads chunk i+1 into registers while the
// rounds of chunk i run (the 16384-element chunk leaves room for two workgroups per CU only, and with
// 16 waves per CU nothing else covers a chunk's load latency: rocprofv3 SQ counters on 2^22 x 64,
// log_blowup 4 showed VALU busy 0.86 with 28 % of the wave-cycles parked).
template <int LM, int CPW, class TW>
__device__ __forceinline__ void lde_fwd_contig_block(uint32_t* __restrict__ out, uint64_t out_col_stride, unsigned log_n,
                                                     const TW* __restrict__ W, const uint32_t bl, unsigned log_b,
                                                     uint32_t beta0) {
    __shared__ uint32_t s[padded(1 << LM)];
    constexpr int NT = chunk_threads(LM);
    constexpr int NV = (1 << LM) / 4 / NT;
    uint32_t* col = out + (uint64_t)blockIdx.y * out_col_stride + ((uint64_t)bl << log_n);
    const unsigned sb = log_n - LM + log_b;                 // the chunk's first stage in the N-point transform
    const uint32_t cb = (beta0 + bl) << (log_n - LM);       // block beta's first chunk there
    if constexpr (CPW == 1) {
        const uint32_t c = blockIdx.x;
        uint32_t* o = col + ((uint64_t)c << LM);
        chunk_load<LM>(s, o);
        chunk_rounds<LM, false>(s, sb, cb + c, W);
        chunk_store<LM, true>(s, o);
    } else {
        const uint32_t c0 = blockIdx.x * CPW;
        uint4 v[NV];
        {
            const uint4* g4 = reinterpret_cast<const uint4*>(col + ((uint64_t)c0 << LM));
#pragma unroll
            for (int k = 0; k < NV; k++) v[k] = g4[threadIdx.x + (uint32_t)k * NT];
        }
#pragma unroll 1
        for (int i = 0; i < CPW; i++) {
            const uint32_t c = c0 + i;
#pragma unroll
            for (int k = 0; k < NV; k++) {
                const uint32_t i4 = threadIdx.x + (uint32_t)k * NT;
                const uint32_t a = 4 * i4 + (i4 >> 3);
                s[a] = v[k].x;
                s[a + 1] = v[k].y;
                s[a + 2] = v[k].z;
                s[a + 3] = v[k].w;
            }
            __syncthreads();
            if (i + 1 < CPW) {
                const uint4* g4 = reinterpret_cast<const uint4*>(col + ((uint64_t)(c + 1) << LM));
#pragma unroll
                for (int k = 0; k < NV; k++) v[k] = g4[threadIdx.x + (uint32_t)k * NT];
            }
            chunk_rounds<LM, false>(s, sb, cb + c, W);
            chunk_store<LM, true>(s, col + ((uint64_t)c << LM));
            __syncthreads();  // the image is rewritten at the top of the loop
        }
    }
}

template <int LM, int CPW = 1, class TW = uint32_t>
__global__ void __launch_bounds__(chunk_threads(LM), CPW > 1 ? 4 : 1)  // CPW > 1: keep two 512-thread groups per CU
k_lde_fwd_contig(uint32_t* __restrict__ out, uint64_t out_col_stride, unsigned log_n,
                 const TW* __restrict__ W, unsigned log_b, uint32_t beta0) {
    lde_fwd_contig_block<LM, CPW>(out, out_col_stride, log_n, W, blockIdx.z, log_b, beta0);
}

// The same on all blocks but one per column, the block that is its matrix's input (own_a for the columns below
// gw, own_b from gw on: coset_lde).  The grid's z is one short and no workgroup is launched for that block.
template <int LM, int CPW = 1, class TW = uint32_t>
__global__ void __launch_bounds__(chunk_threads(LM), CPW > 1 ? 4 : 1)
k_lde_fwd_contig_own(uint32_t* __restrict__ out, uint64_t out_col_stride, unsigned log_n,
                     const TW* __restrict__ W, unsigned log_b, uint32_t beta0, uint32_t gw, uint32_t own_a,
                     uint32_t own_b) {
    const uint32_t own = blockIdx.y < gw ? own_a : own_b;
    lde_fwd_contig_block<LM, CPW>(out, out_col_stride, log_n, W, blockIdx.z + (blockIdx.z >= own ? 1u : 0u), log_b,
                                  beta0);
}

// ------------------------------------------------------------------ middle kernel
// Tile = slots {row << row_shift + j2_0 + jj : row < 2^log_len, jj < 2^log_T} of one column
// (row_shift = LOG_M for n > 4096, where rows are 4096 apart; 0 for n <= 4096 with log_T = 0, where
// the tile is the whole column).  Finishes the inverse transform (stages log_len-1 .. 0), multiplies
// coefficient k by shift^k / n -- once: the factor does not depend on the coset -- and then for each coset
// runs forward stages 0 .. log_len-1 with block beta's twiddles of the N-point transform (s_base = log_b,
// c = beta: the header's "coset twiddles") -> block beta of `out`.
// scale_a / scale_b: the table shift^k / n of the columns below / from gw (coset_scale_table), or nullptr
// where the shift is 1 and the factor is the constant inv_n for every k.
// PLAN 0: generic (runtime round plan).  PLAN 1: log_len = 8, log_T = 5 (n = 2^(LM + 8): 2^20 with
// 4096-element chunks, 2^21 / 2^22 with LM = 13 / 14): two radix-16 rounds with compile-time
// distances 2^9 and 2^5.
// OWN (coset_lde on every coset, beta0 = 0): block own_a of the first matrix's columns and own_b of the second's
// is the matrix itself and has been copied; the coset loop steps over it.
template <int PLAN, int TILE = TILE_ELEMS, int NTM = NT_MID, int LM = LOG_M, bool OWN = false, class TWF = uint32_t,
          class TWI = uint32_t>
__global__ void __launch_bounds__(NTM)
k_lde_mid(const uint32_t* __restrict__ evals, uint64_t in_col_stride, uint32_t* __restrict__ out,
          uint64_t out_col_stride, unsigned log_n, unsigned log_len, unsigned log_T,
          unsigned row_shift, unsigned log_b, unsigned beta0, unsigned n_cosets, const TWF* __restrict__ W,
          const TWI* __restrict__ Winv, const uint32_t* __restrict__ scale_a,
          const uint32_t* __restrict__ evals2, const uint32_t* __restrict__ scale_b, uint32_t inv_n, uint32_t gw,
          uint32_t own_a, uint32_t own_b) {
    __shared__ uint32_t s[padded(TILE)];
    constexpr int PER_THREAD = TILE / NTM;
    if (PLAN == 1) {
        log_len = 8;
        log_T = 5;
    }
    // Tiles narrower than 128 B (log_T < 5) share every cache line they touch with their neighbours:
    // neighbouring tiles go to workgroups of the same XCD (ids 8 apart), whose L2 then merges the
    // pieces of a line (measured on 2^22 x 64, log_blowup 4: 19.6 -> 15.7 ms at 32 B, 14.5 -> 13.8 at 64 B)
    const bool remap = PLAN == 0 && log_T < 5 && gridDim.x >= 8;
    uint32_t bx = remap ? (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    uint32_t col_id = blockIdx.y;
    if constexpr (PLAN == 1) {
        // 1-D grid in the order (32 tiles, all columns, next 32 tiles, ...): the workgroups that use
        // one tile's slice of the scale table (and its twiddles) run close together and -- 32 being
        // a multiple of the 8 XCDs -- on the same XCD, so its L2 serves the slice to every column
        // instead of the Infinity Cache (measured fetch + write traffic 1.39x -> 1.11x of the
        // algorithmic bytes, same kernel time, 3.03-3.06 -> 3.00 ms/step for whole proofs)
        const uint32_t ncols = gridDim.x >> (LM - 5);  // 2^(LM - 5) tiles per column (128 at LM = 12)
        bx = (blockIdx.x & 31) + 32 * (blockIdx.x / (32 * ncols));  // < 2^(LM - 5)
        col_id = (blockIdx.x >> 5) % ncols;
    }
    const uint32_t j2_0 = bx << log_T;
    // a two-matrix launch (coset_lde: evals2): columns gw .. come from the second matrix and take its
    // shift's scale table; the output columns follow each other either way
    const uint32_t* g = (col_id < gw ? evals + (uint64_t)col_id * in_col_stride
                                     : evals2 + (uint64_t)(col_id - gw) * in_col_stride) + j2_0;
    const uint32_t* __restrict__ scale = col_id < gw ? scale_a : scale_b;
    const uint32_t own = OWN ? (col_id < gw ? own_a : own_b) : 0xffffffffu;  // one value per workgroup
    const uint32_t total = 1u << (log_len + log_T);
    const uint32_t tmask = (1u << log_T) - 1;
    if constexpr (PLAN == 1) {
        // fixed shape: PER_THREAD loads issued back to back (the generic loop below is a run-time
        // loop whose iterations the compiler keeps in order: load, wait, LDS store)
        uint32_t t[PER_THREAD];
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) {
            const uint32_t i = threadIdx.x + (uint32_t)k * NTM;
            t[k] = g[((uint64_t)(i >> log_T) << row_shift) + (i & tmask)];
        }
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) s[pad(threadIdx.x + (uint32_t)k * NTM)] = t[k];
    } else {
        for (uint32_t i = threadIdx.x; i < total; i += NTM)
            s[pad(i)] = g[((uint64_t)(i >> log_T) << row_shift) + (i & tmask)];
    }
    // the factors of the coefficients this thread will keep (slot i = threadIdx.x + k NTM is coefficient
    // off(i) + j2_0): asked for here, used after the inverse rounds, which cover the loads
    uint32_t scv[PER_THREAD];
    if (scale != nullptr) {  // one value per workgroup
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) {
            const uint32_t i = threadIdx.x + (uint32_t)k * NTM;
            scv[k] = i < total ? scale[((uint64_t)(i >> log_T) << row_shift) + (i & tmask) + j2_0] : 0u;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) scv[k] = inv_n;
    }
    __syncthreads();
    if (PLAN == 1) {
        radix_round<4, true, 5, NTM>(s, 13, 4, 0, 0, Winv);
        // the last inverse round (distance 2^9) works on elements tid + 512 q: exactly the share of
        // the tile this thread keeps as coefficients, so it runs in registers (below)
    } else {
        tile_inverse_rt<NTM>(s, log_len, log_T, 0, 0, Winv);
    }
    // natural-order coefficients (times n): keep this thread's share in registers
    uint32_t coef[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; k++) {
        const uint32_t i = threadIdx.x + (uint32_t)k * NTM;
        coef[k] = i < total ? s[pad(i)] : 0u;
    }
    // PLAN 1: the radix-16 round at the largest distance (TILE/16) has TILE/16 groups, GP =
    // PER_THREAD/16 per thread, and group j of a thread is {tid + (j + GP q) NTM : q < 16}: its own
    // coefficients coef[j + GP q].  That round therefore runs in registers on either side.
    constexpr int GP = PER_THREAD / 16;
    if constexpr (PLAN == 1) {
#pragma unroll
        for (int j = 0; j < GP; j++) {
            uint32_t v[16];
#pragma unroll
            for (int q = 0; q < 16; q++) v[q] = coef[j + GP * q];
            radix_butterflies<4, true, true>(v, 0, 0, 0, 0, Winv);
#pragma unroll
            for (int q = 0; q < 16; q++) coef[j + GP * q] = v[q];
        }
    }
    // shift^k / n, once for every coset (lazy product: the butterflies that follow take [0, 2p) -- two
    // instructions fewer per coefficient).  What is left of s_beta^k, w_N^(bitrev_b(beta) k), is the difference
    // between the n-point twiddles and block beta's of the N-point transform, which the forward rounds take.
#pragma unroll
    for (int k = 0; k < PER_THREAD; k++) coef[k] = mont_mul_lazy(coef[k], scv[k]);
    // cosets beta0 .. beta0 + n_cosets - 1 go to blocks 0 .. n_cosets - 1 of `out` (a rank of a
    // sharded prover owns a contiguous range of cosets)
    // (nontemporal stores of the coset blocks changed nothing at 2^22 x 64, log_blowup 4: 7.92 against
    // 7.90 ms per launch.  Nor did two LDS images used in turn, which make the barrier at the top of the
    // coset loop unnecessary (3 -> 2 barriers per coset, but more VGPRs and run-time image addresses): 0.61
    // against 0.59-0.60 ms at C3, 8.19 against 7.9-8.1.)
    for (uint32_t bl = 0; bl < n_cosets; bl++) {
        if (OWN && bl == own) continue;
        const uint32_t beta = beta0 + bl;
        __syncthreads();
        if constexpr (PLAN == 1) {
            // the first forward round (the thread's own elements) stays in registers; LDS is written
            // once, for the following rounds.  No twiddle-1 shortcut: block beta's twiddles are 1 for
            // beta = 0 only, and a second copy of the loop body for that coset is not worth its code.
#pragma unroll
            for (int j = 0; j < GP; j++) {
                uint32_t v[16];
#pragma unroll
                for (int q = 0; q < 16; q++) v[q] = coef[j + GP * q];
                radix_butterflies<4, false, false>(v, log_b, 0, beta, 0, W);
#pragma unroll
                for (int q = 0; q < 16; q++) s[pad(threadIdx.x + (uint32_t)(j + GP * q) * NTM)] = v[q];
            }
            __syncthreads();
            uint32_t* og = out + (uint64_t)col_id * out_col_stride + ((uint64_t)bl << log_n) + j2_0;
            // (writing this round's results straight to HBM from registers was tried twice: 137 VGPRs
            // -- one workgroup per CU -- and 0.85 ms against 0.64, later 123 VGPRs and 0.584-0.591 ms per
            // proof against 0.588-0.601: within the noise of whole proofs, so the LDS round stays)
            radix_round<4, false, 5, NTM>(s, 13, 4, log_b, beta, W);
            // lazy values: k_lde_fwd_contig reads them next.  Unrolled: 16 LDS reads in flight, then
            // 16 stores whose addresses differ by constants (as a run-time loop each iteration
            // cost 7 VALU instructions and waited for its own LDS read)
            uint32_t t[PER_THREAD];
#pragma unroll
            for (int k = 0; k < PER_THREAD; k++) t[k] = s[pad(threadIdx.x + (uint32_t)k * NTM)];
            uint32_t* ot = og + ((uint64_t)(threadIdx.x >> 5) << LM) + (threadIdx.x & 31);
#pragma unroll
            for (int k = 0; k < PER_THREAD; k++) ot[(uint64_t)k * (NTM >> 5) << LM] = t[k];
            continue;  // stored; the barrier at the top of the loop protects the LDS image
        } else {
#pragma unroll
            for (int k = 0; k < PER_THREAD; k++) {
                const uint32_t i = threadIdx.x + (uint32_t)k * NTM;
                if (i < total) s[pad(i)] = coef[k];
            }
            __syncthreads();
            tile_forward_rt<NTM>(s, log_len, log_T, log_b, beta, W);
        }
        uint32_t* o = out + (uint64_t)col_id * out_col_stride + ((uint64_t)bl << log_n) + j2_0;
        if (row_shift != 0) {  // n > 4096: k_lde_fwd_contig follows and takes lazy values
            for (uint32_t i = threadIdx.x; i < total; i += NTM)
                o[((uint64_t)(i >> log_T) << row_shift) + (i & tmask)] = s[pad(i)];
        } else {  // the whole transform was done here: canonical output
            for (uint32_t i = threadIdx.x; i < total; i += NTM)
                o[((uint64_t)(i >> log_T) << row_shift) + (i & tmask)] = red2p(s[pad(i)]);
        }
    }
}

// ------------------------------------------------------------------ the block that is the input
// out block own_a (columns below gw, from evals) / own_b (from gw on, from evals2) <- the column itself: what
// the three passes would recompute there (ntt_plan.hpp lde_own_coset).  The words are copied as they are: every
// producer of an LDE input stores canonical words (the quotient kernels end in mont_mul, k_reduce_low in an
// add of two reduced products, the transposes move what a caller uploaded under the ABI's canonical rule).
// VEC (two-pass plans: n a multiple of 4096, columns 16-byte aligned): 4096 elements per workgroup.
template <bool VEC>
__global__ void __launch_bounds__(256)
k_lde_own_copy(const uint32_t* __restrict__ evals, uint64_t in_col_stride, uint32_t* __restrict__ out,
               uint64_t out_col_stride, unsigned log_n, const uint32_t* __restrict__ evals2, uint32_t gw,
               uint32_t own_a, uint32_t own_b) {
    const uint32_t col = blockIdx.y;
    const uint32_t* src = col < gw ? evals + (uint64_t)col * in_col_stride
                                   : evals2 + (uint64_t)(col - gw) * in_col_stride;
    uint32_t* dst = out + (uint64_t)col * out_col_stride + ((uint64_t)(col < gw ? own_a : own_b) << log_n);
    if constexpr (VEC) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src) + (uint64_t)blockIdx.x * 1024 + threadIdx.x;
        uint4* d4 = reinterpret_cast<uint4*>(dst) + (uint64_t)blockIdx.x * 1024 + threadIdx.x;
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = s4[256 * k];
#pragma unroll
        for (int k = 0; k < 4; k++) d4[256 * k] = v[k];
    } else {
        const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
        if (i < (1ull << log_n)) dst[i] = src[i];
    }
}

// ------------------------------------------------------------------ host drivers
// The pass plan -- chunk size, tile shape, kernel variant, limits -- is ntt_plan.hpp's; the launchers below
// only turn a plan into grids.
//
// KERNEL-TIMER NAMES.  bench.py (its roofline leg), tools/pmc_*.py and tools/rocpd_stats.py find a kernel's
// time and its algorithmic bytes by these strings -- by stem, by "true" (the pass after the fused transpose),
// by "k_lde_mid<1" -- so they are spelled out, here and in launch_lde_mid, parentheses included, and are not
// to be tidied.  The standalone transforms (ntt_dft.hip) launch the same contiguous kernels under the same names.
constexpr const char* INTT_NAME[3] = {"k_intt_contig<12>", "k_intt_contig<13>", "k_intt_contig<14>"};
constexpr const char* INTT_R16_NAME[3] = {"(k_intt_contig<12, true>)", "(k_intt_contig<13, true>)",
                                          "(k_intt_contig<14, true>)"};
constexpr const char* FWD_NAME[3] = {"k_lde_fwd_contig<12>", "k_lde_fwd_contig<13>", "(k_lde_fwd_contig<14, 4>)"};

// THE TWIDDLE FORM OF EACH INSTANTIATION (ntt_rounds.hpp: uint32_t = Montgomery table, uint2 = Plantard table).
// An instantiation takes the Plantard form where, against the Montgomery one, it gains no scratch, loses no
// wave per SIMD and executes fewer VALU instructions (profiles/plantard_kernel_resources.txt has the table).
// Range contract between the passes: every inverse pass here leaves canonical words when it is Plantard and
// lazy ones when it is Montgomery; a Plantard inverse pass behind a Montgomery one would have to reduce on
// load, so ContigForm<LM>::Inv being Plantard is what lets MidForm<..>::Inv of the same plan be.
template <int LM> struct ContigForm {
    using Inv = uint2;
    using Fwd = uint2;
};
// k_lde_fwd_contig<14, 4> on the Plantard table: 121 -> 128 VGPRs and 40 bytes of scratch
template <> struct ContigForm<14> {
    using Inv = uint2;
    using Fwd = uint32_t;
};
template <int PLAN, int TILE> struct MidForm {
    using Inv = uint2;
    using Fwd = uint2;
};
// the run-time plan's forward rounds on the Plantard table: 121 -> 150 VGPRs, one workgroup per CU instead of two
// (128 and 8 bytes of scratch when held to two); its inverse rounds alone: 121, as before
template <> struct MidForm<0, TILE_ELEMS> {
    using Inv = uint2;
    using Fwd = uint32_t;
};
static_assert(std::is_same<ContigForm<12>::Inv, uint2>::value && std::is_same<ContigForm<13>::Inv, uint2>::value &&
                  std::is_same<ContigForm<14>::Inv, uint2>::value,
              "the strided inverse rounds (here and in ntt_dft.hip) take canonical words: a Montgomery k_intt_contig "
              "would have to be reduced on load");

// f(std::integral_constant<int, LM>) for the plan's chunk size
template <class F>
static void with_chunk_log(unsigned LM, F&& f) {
    if (LM == 12) f(std::integral_constant<int, 12>{});
    else if (LM == 13) f(std::integral_constant<int, 13>{});
    else f(std::integral_constant<int, 14>{});
}

bool launch_transpose_bitrev_r16(Context& ctx, const uint32_t* src, uint32_t* dst, unsigned log_n, uint32_t w,
                                 uint64_t dst_col_stride, uint32_t src_width) {
    if (w == 0 || !ntt_plan(log_n).fused_first_round) return false;  // no contiguous inverse pass to shorten
    ctx.ensure_plant_twiddles(0, log_n);
    TS_LAUNCH(ctx, k_transpose_bitrev_r16, dim3(1u << (log_n - 6), (w + 63) / 64), dim3(256), 0, src, dst, log_n, w,
              dst_col_stride, src_width ? src_width : w, (const uint2*)ctx.d_plant_inv);
    TS_HIP(hipGetLastError());
    return true;
}

void launch_contig_inverse(Context& ctx, const NttPlan& p, uint32_t* data, uint64_t col_stride, uint32_t ncols,
                           bool first_round_done, uint32_t* data2, uint32_t gw) {
    const TwTables Winv = twiddles_inv(ctx);
    with_chunk_log(p.LM, [&](auto lm) {
        constexpr int LM = decltype(lm)::value;
        using TW = typename ContigForm<LM>::Inv;
        const dim3 g(p.chunks, ncols), b(chunk_threads(LM));
        if (first_round_done)
            TS_LAUNCH_NAMED(ctx, INTT_R16_NAME[LM - 12], (k_intt_contig<LM, true, TW>), g, b, 0, data, col_stride,
                            p.log_n, Winv, data2, gw);
        else
            TS_LAUNCH_NAMED(ctx, INTT_NAME[LM - 12], (k_intt_contig<LM, false, TW>), g, b, 0, data, col_stride, p.log_n,
                            Winv, data2, gw);
    });
}

// the strided pass of the LDE on cosets beta0 .. beta0 + n_beta - 1 (the whole transform when the plan has
// one pass); two matrices as coset_lde
static void launch_lde_mid(Context& ctx, const NttPlan& p, const uint32_t* evals, uint64_t in_col_stride,
                           uint32_t* out, uint64_t out_col_stride, uint32_t ncols, uint32_t beta0, uint32_t n_beta,
                           unsigned log_blowup, const uint32_t* scale, const uint32_t* evals2, const uint32_t* scale2,
                           uint32_t gw, uint32_t own_a, uint32_t own_b) {
    const TwTables W = twiddles_fwd(ctx), Winv = twiddles_inv(ctx);
    const dim3 grid(p.tiles, ncols), b(NT_MID);
    const dim3 grid1(p.tiles * ncols);  // the fixed plan: 1-D, see the kernel
#define TS_MID_ARGS \
    evals, in_col_stride, out, out_col_stride, p.log_n, p.log_len, p.log_T, p.row_shift, log_blowup, beta0, n_beta, W, \
        Winv, scale, evals2, scale2, lde_inv_n_mont(p.log_n), gw, own_a, own_b
#define TS_MID_K(PLAN, TILE, LM, OWN) \
    (k_lde_mid<PLAN, TILE, NT_MID, LM, OWN, typename MidForm<PLAN, TILE>::Fwd, typename MidForm<PLAN, TILE>::Inv>)
    // (the instantiations that step over a block run under the names of the ones that do not)
    if (own_a != LDE_NO_OWN && p.mid == NttMid::FIXED256 && p.LM == 12)
        TS_LAUNCH_NAMED(ctx, "k_lde_mid<1>", TS_MID_K(1, TILE_ELEMS, 12, true), grid1, b, 0, TS_MID_ARGS);
    else if (own_a != LDE_NO_OWN && p.mid == NttMid::FIXED256 && p.LM == 13)
        TS_LAUNCH_NAMED(ctx, "(k_lde_mid<1, 8192, 512, 13>)", TS_MID_K(1, 8192, 13, true), grid1, b, 0,
                        TS_MID_ARGS);
    else if (own_a != LDE_NO_OWN && p.mid == NttMid::FIXED256)
        TS_LAUNCH_NAMED(ctx, "(k_lde_mid<1, 8192, 512, 14>)", TS_MID_K(1, 8192, 14, true), grid1, b, 0,
                        TS_MID_ARGS);
    else if (own_a != LDE_NO_OWN)
        TS_LAUNCH_NAMED(ctx, "k_lde_mid<0>", TS_MID_K(0, TILE_ELEMS, LOG_M, true), grid, b, 0, TS_MID_ARGS);
    else if (p.mid == NttMid::TILE16384)
        TS_LAUNCH_NAMED(ctx, "(k_lde_mid<0, 16384>)", TS_MID_K(0, 16384, LOG_M, false), grid, b, 0, TS_MID_ARGS);
    else if (p.mid == NttMid::FIXED256 && p.LM == 12)
        TS_LAUNCH_NAMED(ctx, "k_lde_mid<1>", TS_MID_K(1, TILE_ELEMS, LOG_M, false), grid1, b, 0, TS_MID_ARGS);
    else if (p.mid == NttMid::FIXED256 && p.LM == 13)
        TS_LAUNCH_NAMED(ctx, "(k_lde_mid<1, 8192, 512, 13>)", TS_MID_K(1, 8192, 13, false), grid1, b, 0, TS_MID_ARGS);
    else if (p.mid == NttMid::FIXED256)
        TS_LAUNCH_NAMED(ctx, "(k_lde_mid<1, 8192, 512, 14>)", TS_MID_K(1, 8192, 14, false), grid1, b, 0, TS_MID_ARGS);
    else
        TS_LAUNCH_NAMED(ctx, "k_lde_mid<0>", TS_MID_K(0, TILE_ELEMS, LOG_M, false), grid, b, 0, TS_MID_ARGS);
#undef TS_MID_ARGS
#undef TS_MID_K
}

void launch_contig_forward(Context& ctx, const NttPlan& p, uint32_t* data, uint64_t col_stride, uint32_t ncols,
                           uint32_t n_blocks, unsigned log_blowup, uint32_t beta0, uint32_t gw, uint32_t own_a,
                           uint32_t own_b) {
    const TwTables W = twiddles_fwd(ctx);
    with_chunk_log(p.LM, [&](auto lm) {
        constexpr int LM = decltype(lm)::value;
        using TW = typename ContigForm<LM>::Fwd;
        // 4 chunks per workgroup of the 16384-element forward pass: measured 12.22 ms per proof against
        // 12.49 with 1 and 13.34 with 2 (spills)
        constexpr int CPW = LM == 14 ? 4 : 1;
        if (own_a != LDE_NO_OWN)  // one block per column is already there: n_blocks - 1 of them in z
            TS_LAUNCH_NAMED(ctx, FWD_NAME[LM - 12], (k_lde_fwd_contig_own<LM, CPW, TW>),
                            dim3(p.chunks / CPW, ncols, n_blocks - 1), dim3(chunk_threads(LM)), 0, data, col_stride,
                            p.log_n, W, log_blowup, beta0, gw, own_a, own_b);
        else
            TS_LAUNCH_NAMED(ctx, FWD_NAME[LM - 12], (k_lde_fwd_contig<LM, CPW, TW>), dim3(p.chunks / CPW, ncols, n_blocks),
                            dim3(chunk_threads(LM)), 0, data, col_stride, p.log_n, W, log_blowup, beta0);
    });
}

int lde_own_coset_used(unsigned log_n, unsigned log_blowup, uint32_t shift) {
    if (const char* e = getenv("TS_LDE_OWN_COSET"); e && *e && atoi(e) == 0) return -1;
    // one coset only: nothing would be left to launch; n = 2^26: the 16384-element tile has a CU to itself as it is
    if (log_blowup == 0 || log_n + log_blowup > 27 || ntt_plan(log_n).mid == NttMid::TILE16384) return -1;
    return lde_own_coset(log_n, log_blowup, shift);
}

void coset_lde(Context& ctx, uint32_t* evals, uint64_t in_col_stride, uint32_t ncols, unsigned log_n,
               unsigned log_blowup, uint32_t shift, uint32_t* out, uint64_t out_col_stride,
               uint32_t beta0, uint32_t n_beta, bool first_round_done, uint32_t* evals2, uint32_t shift2,
               uint32_t gw, bool stage_timers) {
    if (ncols == 0) return;
    TS_REQUIRE(evals2 == nullptr || (gw >= 1 && gw < ncols && shift2 != 0), TS_ERR_INVALID,
               "coset_lde: second matrix needs its first column and its shift");
    if (evals2 == nullptr) gw = 0xffffffffu;
    TS_REQUIRE(log_n + log_blowup <= 27, TS_ERR_INVALID, "coset_lde: log_n + log_blowup > 27");
    const NttPlan p = ntt_plan(log_n);
    ntt_require_shape(p, ncols, in_col_stride, out_col_stride, true);
    TS_REQUIRE(!first_round_done || p.fused_first_round, TS_ERR_INVARIANT,
               "coset_lde: no contiguous inverse pass at this size");
    // the forward passes index block beta of the N-point transform: both forward tables reach log_n + log_blowup
    // (a prover has asked for them already, Context::ensure_lde_twiddles: nothing is rebuilt here inside a proof);
    // the inverse Plantard table stays at log_n
    ctx.ensure_lde_twiddles(std::max(1u, log_n + log_blowup));
    ctx.ensure_plant_twiddles(0, std::max(1u, log_n));

    // scale table shift^k / n (cached per context: the trace's is the same every proof; none for shift 1)
    const uint32_t n_cosets = 1u << log_blowup;
    if (n_beta == 0) n_beta = n_cosets - beta0;
    TS_REQUIRE(beta0 < n_cosets && n_beta <= n_cosets - beta0, TS_ERR_INVALID, "coset_lde: coset range");
    const uint32_t* scale = coset_scale_table(ctx, log_n, shift);
    const uint32_t* scale2 = evals2 ? coset_scale_table(ctx, log_n, shift2) : nullptr;

    // A whole LDE whose input lies on one of its cosets (the quotient chunks, the reduced opening): that block is
    // copied -- now, the inverse pass works in place -- and the passes leave it out.  Every matrix of the launch
    // must have one; an input the transpose has already run a round on is no longer the block.
    uint32_t own_a = LDE_NO_OWN, own_b = LDE_NO_OWN;
    if (beta0 == 0 && n_beta == n_cosets && !first_round_done && ctx.lde_pass_mask == 7u) {
        const int a = lde_own_coset_used(log_n, log_blowup, shift);
        const int b = evals2 ? lde_own_coset_used(log_n, log_blowup, shift2) : a;
        if (a >= 0 && b >= 0) {
            own_a = (uint32_t)a;
            own_b = (uint32_t)b;
            const uint64_t n = 1ull << log_n;
            if (p.two_pass)
                TS_LAUNCH_NAMED(ctx, "k_lde_own_copy", k_lde_own_copy<true>, dim3((unsigned)(n >> 12), ncols), dim3(256), 0,
                                (const uint32_t*)evals, in_col_stride, out, out_col_stride, log_n,
                                (const uint32_t*)evals2, gw, own_a, own_b);
            else
                TS_LAUNCH_NAMED(ctx, "k_lde_own_copy", k_lde_own_copy<false>, dim3((unsigned)((n + 255) / 256), ncols),
                                dim3(256), 0, (const uint32_t*)evals, in_col_stride, out, out_col_stride, log_n,
                                (const uint32_t*)evals2, gw, own_a, own_b);
        }
    }

    if (!p.two_pass) {
        launch_lde_mid(ctx, p, evals, in_col_stride, out, out_col_stride, ncols, beta0, n_beta, log_blowup, scale, evals2,
                       scale2, gw, own_a, own_b);
    } else {
        // (ctx.lde_pass_mask: measurement only -- ts_bench_stage runs one of the three passes alone, on
        // whatever the buffers hold, to sample its clock and power; every product path leaves it at 7)
        if (ctx.lde_pass_mask & 1u) {
            // (stage names: the sharded prover reports where a rank's time goes)
            std::optional<StageTimer> t;
            if (stage_timers) t.emplace(&ctx, "lde: inverse NTT, contiguous stages");
            launch_contig_inverse(ctx, p, evals, in_col_stride, ncols, first_round_done, evals2, gw);
        }
        std::optional<StageTimer> t_rest;
        if (stage_timers) t_rest.emplace(&ctx, "lde: strided pass + forward NTT of the owned cosets");
        if (ctx.lde_pass_mask & 2u)
            launch_lde_mid(ctx, p, evals, in_col_stride, out, out_col_stride, ncols, beta0, n_beta, log_blowup, scale,
                           evals2, scale2, gw, own_a, own_b);
        if (ctx.lde_pass_mask & 4u) launch_contig_forward(ctx, p, out, out_col_stride, ncols, n_beta, log_blowup, beta0, gw, own_a,
                                                          own_b);
    }
    TS_HIP(hipGetLastError());
}

}  // namespace ts
