// Opening kernels (reference fri/src/two_adic_pcs.rs:260-389 `open`):
//   :358-369  ys = interpolate_coset(BitRev(first n rows), 31, z)     -> bary_weights + bary_dots
//   :678-720  inv_denoms[X] = 1/(x_X - z), x_X = 31 * w_N^bitrev(X)   -> computed on the fly
//   :371-381  ro[X] += alpha^offset * (sum_i alpha^i p_i[X] - reduced_ys) * inv_denom[X]  -> reduce
// All matrices are column-major with bit-reversed rows, so "row X" is a coalesced read per column.
// Dot products are accumulated lazily: 64-bit multiply-adds (one v_mad_u64_u32 each) with a cheap
// range fix every two terms and a single Montgomery reduction at the end.
#include "kernels.hpp"
#include "open_dev.hpp"  // root_bitrev, row_dot_acc / row_dot_alpha, inv_denoms, bary_finish_group

namespace ts {

// ------------------------------------------------------------------ barycentric weights
// out[p][t] = x_t / (z_p - x_t), x_t = 31 * omega_n^bitrev(t)   (Montgomery EF4)
constexpr int BW_ROWS = 4;

__global__ void __launch_bounds__(256)
k_bary_weights(unsigned log_n, const uint32_t* __restrict__ W, uint32_t gen_mont, Ef z0, Ef z1,
               uint32_t n_points, Ef* __restrict__ out) {
    const uint64_t n = 1ull << log_n;
    const uint64_t t0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * BW_ROWS;
    if (t0 >= n) return;
    Ef num[2 * BW_ROWS];
    uint32_t nrm[2 * BW_ROWS], pre[2 * BW_ROWS], xs[BW_ROWS];
    uint32_t run = R_MOD_P;
#pragma unroll
    for (int k = 0; k < BW_ROWS; k++) {
        const bool ok = t0 + k < n;
        uint32_t x = ok ? mont_mul(gen_mont, root_bitrev(W, log_n, t0 + k)) : R_MOD_P;
        xs[k] = x;
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const Ef z = p == 0 ? z0 : z1;
            Ef u = Ef{{sub(z.c[0], x), z.c[1], z.c[2], z.c[3]}};  // z - x
            if (p < (int)n_points && ok) {
                ef_inv_parts(u, num[2 * k + p], nrm[2 * k + p]);
            } else {
                num[2 * k + p] = ef_zero();
                nrm[2 * k + p] = R_MOD_P;
            }
            pre[2 * k + p] = run;
            run = mont_mul(run, nrm[2 * k + p]);
        }
    }
    uint32_t inv = mont_inv(run);
#pragma unroll
    for (int j = 2 * BW_ROWS - 1; j >= 0; j--) {
        uint32_t ninv = mont_mul(inv, pre[j]);
        inv = mont_mul(inv, nrm[j]);
        const int k = j >> 1, p = j & 1;
        if (p < (int)n_points && t0 + k < n)
            out[(uint64_t)p * n + t0 + k] = ef_mul_base(num[j], mont_mul(ninv, xs[k]));
    }
}

void launch_bary_weights(Context& ctx, unsigned log_n, const Ef* points_mont, uint32_t n_points,
                         Ef* out, uint32_t coset_gen) {
    TS_REQUIRE(n_points >= 1 && n_points <= 2, TS_ERR_INVALID, "bary_weights: 1 or 2 points");
    ctx.ensure_twiddles(log_n == 0 ? 1 : log_n);
    const uint64_t threads = (((uint64_t)1 << log_n) + BW_ROWS - 1) / BW_ROWS;
    Ef z0 = points_mont[0], z1 = n_points > 1 ? points_mont[1] : points_mont[0];
    TS_LAUNCH(ctx, k_bary_weights, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, log_n,
              ctx.d_twiddle_fwd, to_mont(coset_gen ? coset_gen : GENERATOR), z0, z1, n_points, out);
    TS_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ barycentric dot products
// acc[col][p][k] += sum_t m[col][t] * weights[p][t].c[k]  over the first n rows (a skinny product
// [w x n].[n x 4 NP]).  A workgroup streams tiles of COLS columns x TR rows through LDS (loads
// coalesced along rows, all in flight at once); then each lane owns one column and one row subset
// and reads the tile's weights as LDS broadcasts.  COLS = 64 for wide matrices, 8 for the width-4
// quotient chunks (so that all 64 lanes stay busy).  Per-workgroup sums go to a partial buffer
// [block][col][NP*4] that k_bary_finish adds up.
template <int NP, int COLS>
__global__ void __launch_bounds__(256)
k_bary_dots(const uint32_t* __restrict__ m, uint64_t col_stride, uint32_t width, unsigned log_n,
            const Ef* __restrict__ weights, uint32_t* __restrict__ partial, uint32_t rows_per_block) {
    constexpr int RS = 64 / COLS;        // row subsets per wave
    constexpr int TR = 16 * 4 * RS;      // tile rows: 16 per (wave, row subset)
    constexpr int PER_THREAD = COLS * TR / 256;  // = 16
    // tile element (column c, row t = 16*sub + rr) lives at rr*257 + sub*COLS + c: the compute
    // phase reads it conflict-free (lanes = (sub, c)), the store phase with small conflicts only
    __shared__ uint32_t tile[16 * 257];
    __shared__ uint32_t wts[TR][NP * 4];
    __shared__ uint32_t red[4 * RS][COLS][NP * 4];
    const uint64_t n = 1ull << log_n;
    const uint32_t c0 = blockIdx.y * COLS;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t cl = lane % COLS, rs = lane / COLS;
    const uint32_t sub = wv * RS + rs;  // which 16-row slice of the tile this thread reduces
    const uint64_t row_begin = (uint64_t)blockIdx.x * rows_per_block;
    const uint64_t row_end = row_begin + rows_per_block < n ? row_begin + rows_per_block : n;
    uint64_t acc[NP * 4];
#pragma unroll
    for (int j = 0; j < NP * 4; j++) acc[j] = 0;
    for (uint64_t row0 = row_begin; row0 < row_end; row0 += TR) {
        uint32_t v[PER_THREAD];
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) {
            const uint32_t e = threadIdx.x + (uint32_t)k * 256;
            const uint32_t c = c0 + e / TR;
            const uint64_t t = row0 + e % TR;
            v[k] = (c < width && t < row_end) ? m[(uint64_t)c * col_stride + t] : 0u;
        }
        for (uint32_t e = threadIdx.x; e < (uint32_t)(TR * NP); e += 256) {
            const uint32_t p = e / TR, tt = e % TR;
            const uint64_t t = row0 + tt;
            Ef w = ef_zero();
            if (t < row_end) w = weights[(uint64_t)p * n + t];
            wts[tt][p * 4 + 0] = w.c[0];
            wts[tt][p * 4 + 1] = w.c[1];
            wts[tt][p * 4 + 2] = w.c[2];
            wts[tt][p * 4 + 3] = w.c[3];
        }
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) {
            const uint32_t e = threadIdx.x + (uint32_t)k * 256;
            const uint32_t t = e % TR;
            tile[(t & 15) * 257 + (t >> 4) * COLS + e / TR] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 16; rr++) {
            const uint32_t tt = sub * 16 + rr;
            const uint32_t x = tile[rr * 257 + sub * COLS + cl];
#pragma unroll
            for (int j = 0; j < NP * 4; j++) acc[j] = lazy_mac(acc[j], x, wts[tt][j]);
            if (rr & 1) {
#pragma unroll
                for (int j = 0; j < NP * 4; j++) acc[j] = lazy_fix(acc[j]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NP * 4; j++) red[sub][cl][j] = lazy_finish(acc[j]);
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < (uint32_t)(COLS * NP * 4); idx += 256) {
        const uint32_t c = idx / (NP * 4), j = idx % (NP * 4);
        uint32_t sum = 0;
#pragma unroll
        for (int q = 0; q < 4 * RS; q++) sum = add(sum, red[q][c][j]);
        if (c0 + c < width)
            partial[((uint64_t)blockIdx.x * width + c0 + c) * (NP * 4) + j] = sum;
    }
}

// out[j] = sum over blocks of partial[block][j]  (mod p); one workgroup per 4 output words
// (bary_finish_group, open_dev.hpp).  Up to N jobs in one launch, by value (the trace's sums and the quotient
// chunks'; with a key, its columns' first; with an aux round, that one's second): the first groups[0]
// workgroups take job 0, the next groups[1] job 1, and so on.
template <int N>
struct BaryFinishArgs {
    BaryFinishJob j[N];
    uint32_t groups[N];
};
template <int N>
__global__ void __launch_bounds__(256)
k_bary_finish(BaryFinishArgs<N> a) {
    BaryFinishJob j = a.j[0];
    uint32_t group = blockIdx.x, first = 0;
#pragma unroll
    for (int k = 1; k < N; k++) {
        first += a.groups[k - 1];
        if (blockIdx.x >= first) {
            j = a.j[k];
            group = blockIdx.x - first;
        }
    }
    bary_finish_group(j.partial, j.out, j.n_blocks, j.n_words, group);
}

template <int N>
static void launch_bary_finish_n(Context& ctx, const char* name, const BaryPending& pend) {
    BaryFinishArgs<N> a{};
    uint32_t total = 0;
    for (uint32_t i = 0; i < pend.n; i++) {
        a.j[i] = BaryFinishJob{pend.partial[i].p, pend.out[i], pend.n_blocks[i], pend.n_words[i]};
        a.groups[i] = (pend.n_words[i] + 3) / 4;
        total += a.groups[i];
    }
    TS_LAUNCH_NAMED(ctx, name, k_bary_finish<N>, dim3(total), dim3(256), 0, a);
}

// the finishing pass of the pending launch_bary_dots(..., pending) calls
void launch_bary_finish(Context& ctx, BaryPending& pend) {
    if (pend.n == 0) return;
    if (pend.n == 4)
        launch_bary_finish_n<4>(ctx, "k_bary_finish<4>", pend);
    else if (pend.n == 3)
        launch_bary_finish_n<3>(ctx, "k_bary_finish<3>", pend);
    else
        launch_bary_finish_n<2>(ctx, "k_bary_finish<2>", pend);
    TS_HIP(hipGetLastError());
    for (uint32_t i = 0; i < pend.n; i++) pend.partial[i].reset();
    pend.n = 0;
}

void launch_bary_dots(Context& ctx, const ColMat& m, unsigned log_n, const Ef* weights,
                      uint32_t n_points, Ef* out, BaryPending* pending) {
    const uint64_t n = 1ull << log_n;
    const bool narrow = m.width <= 8;
    const uint32_t tr = narrow ? 512 : 64;
    uint32_t n_blocks = (uint32_t)((n + tr - 1) / tr);
    if (n_blocks > 2048) n_blocks = 2048;
    uint32_t rows_per_block = (uint32_t)(((n + n_blocks - 1) / n_blocks + tr - 1) / tr * tr);
    n_blocks = (uint32_t)((n + rows_per_block - 1) / rows_per_block);
    const uint32_t n_words = m.width * n_points * 4;
    DevBuf<uint32_t> partial(&ctx, (size_t)n_blocks * n_words);
    const uint32_t* md = m.d;
    if (narrow) {
        dim3 grid(n_blocks, (m.width + 7) / 8);
        if (n_points == 2)
            TS_LAUNCH(ctx, (k_bary_dots<2, 8>), grid, dim3(256), 0, md, m.col_stride, m.width, log_n,
                      weights, partial.p, rows_per_block);
        else
            TS_LAUNCH(ctx, (k_bary_dots<1, 8>), grid, dim3(256), 0, md, m.col_stride, m.width, log_n,
                      weights, partial.p, rows_per_block);
    } else {
        dim3 grid(n_blocks, (m.width + 63) / 64);
        if (n_points == 2)
            TS_LAUNCH(ctx, (k_bary_dots<2, 64>), grid, dim3(256), 0, md, m.col_stride, m.width, log_n,
                      weights, partial.p, rows_per_block);
        else
            TS_LAUNCH(ctx, (k_bary_dots<1, 64>), grid, dim3(256), 0, md, m.col_stride, m.width, log_n,
                      weights, partial.p, rows_per_block);
    }
    TS_HIP(hipGetLastError());
    BaryPending own;
    BaryPending& pend = pending ? *pending : own;
    if (pend.n == pend.capacity) launch_bary_finish(ctx, pend);
    pend.partial[pend.n] = std::move(partial);
    pend.out[pend.n] = reinterpret_cast<uint32_t*>(out);
    pend.n_blocks[pend.n] = n_blocks;
    pend.n_words[pend.n] = n_words;
    pend.n++;
    if (!pending) launch_bary_finish(ctx, pend);
}

// ------------------------------------------------------------------ reduce (generic)
// S(X) = sum_i alpha^i * p_i[X]  (dot_ext_powers, :375), canonical: row_dot_alpha; the pair of inverse
// denominators: inv_denoms (both open_dev.hpp)
template <int NP>
__global__ void __launch_bounds__(256)
k_reduce(const uint32_t* __restrict__ m, uint64_t col_stride, uint32_t width, unsigned log_h,
         const uint32_t* __restrict__ W, uint32_t gen_mont, const uint32_t* __restrict__ alpha_pows,
         ReduceArgs args, Ef* __restrict__ ro) {
    const uint64_t h = 1ull << log_h;
    const uint64_t X = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= h) return;
    const Ef S = row_dot_alpha(m, col_stride, width, X, alpha_pows);
    // x_X = 31 * omega_h^bitrev(X)  (:698-705), Montgomery
    const uint32_t x = mont_mul(gen_mont, root_bitrev(W, log_h, X));
    Ef inv_d[NP];
    inv_denoms<NP>(x, args.z_mont, inv_d);
    Ef acc = args.accumulate ? ro[X] : ef_zero();
#pragma unroll
    for (int p = 0; p < NP; p++) {
        Ef t = ef_mul(ef_sub(S, args.rys[p]), args.off_mont[p]);  // canonical
        acc = ef_add(acc, ef_mul(t, inv_d[p]));                   // canonical
    }
    ro[X] = acc;
}

void launch_reduce(Context& ctx, const ColMat& m, unsigned log_h, const uint32_t* d_alpha_pows_mont,
                   const ReduceArgs& args, Ef* ro) {
    TS_REQUIRE(args.n_points >= 1 && args.n_points <= 2, TS_ERR_INVALID, "reduce: 1 or 2 points");
    ctx.ensure_twiddles(log_h == 0 ? 1 : log_h);
    const uint64_t h = 1ull << log_h;
    dim3 grid((unsigned)((h + 255) / 256));
    if (args.n_points == 2)
        TS_LAUNCH(ctx, k_reduce<2>, grid, dim3(256), 0, (const uint32_t*)m.d, m.col_stride, m.width,
                  log_h, (const uint32_t*)ctx.d_twiddle_fwd, to_mont(GENERATOR), d_alpha_pows_mont, args,
                  ro);
    else
        TS_LAUNCH(ctx, k_reduce<1>, grid, dim3(256), 0, (const uint32_t*)m.d, m.col_stride, m.width,
                  log_h, (const uint32_t*)ctx.d_twiddle_fwd, to_mont(GENERATOR), d_alpha_pows_mont, args,
                  ro);
    TS_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ reduce, prove() shape, one pass
// ro[X] = inv(x - zeta)      * [ off_t0 (S_t - rys_t0) + sum_c off_c (S_c - rys_c) ]
//       + inv(x - zeta omega) *   off_t1 (S_t - rys_t1)
// where S_t is shared by the two trace openings (two_adic_pcs.rs:344-387 visits the trace twice).
// Evaluated as  g0 = off_t0 S_t + D - k0,  g1 = off_t1 S_t - k1,  D = one dot product over every
// chunk column with the folded weights alpha^k off_c (FusedReduceArgs): four EF4 products per row
// instead of 5 + n_chunks -- this kernel, too, is bound by VALU issue, not by its 4 TB/s.
//
// EXTRA leading matrices (the key's preprocessed columns, then the aux trace's) are opened at the same two
// points BEFORE the trace: g0 += off_m0 S_m, g1 += off_m1 S_m, with S_m shared by its two openings exactly as
// S_t is (the constants off_m rys_m are in k0, k1).
//
// LOW: the same sums on the low coset only.  The reduced opening is a polynomial of degree < n, so its n values
// on one coset of H_n determine the other N - n: the kernel computes them on the low coset (rows t < n,
// x_t = 31 omega_n^bitrev(t)) and the caller extends them with the coset LDE (prover.cpp).  The two inverses are
// not computed but read:  k_bary_weights left weights[p][t] = x_t / (z_p - x_t), hence
// 1/(x_t - z_p) = -weights[p][t] / x_t, and 1/x_t is one product of the inverse coset generator with an inverse
// twiddle (W and gen_mont are then the inverse table and 1/31, log_h is log_n).  Output: four base-field columns
// of n rows (an n x 4 COL_MAJOR_BITREV matrix, canonical), the shape of a quotient chunk, instead of one EF4.
//
// The chunk-column loop stays in this body: as a helper function it cost the EXTRA = 0 form 20 VGPRs, whether
// the helper took the by-value struct or its members.
template <int EXTRA>
struct ExtraReduceArgs {
    struct {
        const uint32_t* d;
        uint64_t stride;
        uint32_t width;
        Ef off[2];  // alpha^num_reduced at the matrix's two visits (Montgomery)
    } m[EXTRA ? EXTRA : 1];  // in opening order
};

template <int EXTRA, bool LOW>
__global__ void __launch_bounds__(256)
k_reduce_fused(const uint32_t* __restrict__ trace, uint64_t trace_stride, uint32_t width, unsigned log_h,
               const uint32_t* __restrict__ W, uint32_t gen_mont, const uint32_t* __restrict__ alpha_pows,
               FusedReduceArgs a, ExtraReduceArgs<EXTRA> e, const Ef* __restrict__ weights,
               uint32_t* __restrict__ out) {
    const uint64_t X = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // local row
    if (X >= a.rows) return;
    const Ef St = row_dot_alpha(trace, trace_stride, width, X, alpha_pows);
    Ef inv_d[2];
    if constexpr (!LOW) {
        const uint32_t x = mont_mul(gen_mont, root_bitrev(W, log_h, a.row0 + X));
        inv_denoms<2>(x, a.z_mont, inv_d);
    }
    uint64_t acc[4] = {0, 0, 0, 0};
    uint32_t c = 0;
    for (; c + 2 <= a.n_chunks; c += 2) {
        // two width-4 chunks = one full batch of eight columns (their weights are consecutive): eight
        // loads in flight, 32 multiply-adds, 16 range fixes -- as two 4-column tails it cost twice that
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = a.chunk[c + (k >> 2)][(uint64_t)(k & 3) * a.chunk_stride + X];
        const uint32_t* ap = a.chunk_w + 16 * c;
#pragma unroll
        for (int k = 0; k < 8; k++) {
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] = lazy_mac(acc[j], v[k], ap[4 * k + j]);
            if (k & 1) {
#pragma unroll
                for (int j = 0; j < 4; j++) acc[j] = lazy_fix(acc[j]);
            }
        }
    }
    for (; c < a.n_chunks; c++) row_dot_acc(acc, a.chunk[c], a.chunk_stride, 4, X, a.chunk_w + 16 * c);
    const Ef D{{lazy_finish(acc[0]), lazy_finish(acc[1]), lazy_finish(acc[2]), lazy_finish(acc[3])}};
    if constexpr (LOW) {
        // -1/x_t = -(1/gen) omega_n^-bitrev(t)
        const uint32_t nxi = neg(mont_mul(gen_mont, root_bitrev(W, log_h, X)));
        inv_d[0] = ef_mul_base(weights[X], nxi);
        inv_d[1] = ef_mul_base(weights[a.rows + X], nxi);
    }
    Ef g0 = ef_add(ef_mul(St, a.off_t[0]), D), g1 = ef_mul(St, a.off_t[1]);
#pragma unroll
    for (int i = 0; i < EXTRA; i++) {
        const Ef S = row_dot_alpha(e.m[i].d, e.m[i].stride, e.m[i].width, X, alpha_pows);
        g0 = ef_add(g0, ef_mul(S, e.m[i].off[0]));
        g1 = ef_add(g1, ef_mul(S, e.m[i].off[1]));
    }
    const Ef r = ef_add(ef_mul(ef_sub(g0, a.k0), inv_d[0]), ef_mul(ef_sub(g1, a.k1), inv_d[1]));
    if constexpr (LOW) {
#pragma unroll
        for (int k = 0; k < 4; k++) out[(uint64_t)k * a.rows + X] = r.c[k];
    } else {
        *reinterpret_cast<uint4*>(out + 4 * X) = make_uint4(r.c[0], r.c[1], r.c[2], r.c[3]);
    }
}

template <int EXTRA>
static void launch_reduce_fused_n(Context& ctx, const char* name, const ColMat& trace, unsigned log_h,
                                  const uint32_t* d_alpha_pows_mont, const FusedReduceArgs& a,
                                  const LeadingMats& lead, Ef* ro) {
    ExtraReduceArgs<EXTRA> e{};
    for (int i = 0; i < EXTRA; i++) {
        e.m[i].d = lead.m[i]->d;
        e.m[i].stride = lead.m[i]->col_stride;
        e.m[i].width = lead.m[i]->width;
        e.m[i].off[0] = lead.off[i][0];
        e.m[i].off[1] = lead.off[i][1];
    }
    TS_LAUNCH_NAMED(ctx, name, (k_reduce_fused<EXTRA, false>), dim3((unsigned)((a.rows + 255) / 256)), dim3(256), 0,
                    (const uint32_t*)trace.d, trace.col_stride, trace.width, log_h,
                    (const uint32_t*)ctx.d_twiddle_fwd, to_mont(GENERATOR), d_alpha_pows_mont, a, e,
                    (const Ef*)nullptr, reinterpret_cast<uint32_t*>(ro));
}

void launch_reduce_fused(Context& ctx, const ColMat& trace, unsigned log_h,
                         const uint32_t* d_alpha_pows_mont, const FusedReduceArgs& args, Ef* ro,
                         const LeadingMats& lead) {
    TS_REQUIRE(args.n_chunks <= (uint32_t)MAX_QUOTIENT_CHUNKS, TS_ERR_INVALID, "reduce_fused: too many chunks");
    ctx.ensure_twiddles(log_h == 0 ? 1 : log_h);
    FusedReduceArgs a = args;
    if (a.rows == 0) {
        a.row0 = 0;
        a.rows = 1ull << log_h;
    }
    TS_REQUIRE(a.row0 + a.rows <= (1ull << log_h), TS_ERR_INVALID, "reduce_fused: row range");
    TS_REQUIRE(lead.n <= 2, TS_ERR_INVARIANT, "reduce_fused: more than two leading matrices");
    for (uint32_t i = 0; i < lead.n; i++) {
        const ColMat* m = lead.m[i];
        TS_REQUIRE(m && m->d && a.row0 == 0 && m->height == a.rows && m->col_stride >= a.rows, TS_ERR_INVALID,
                   "reduce_fused: preprocessed or aux matrix shape");
    }
    if (lead.n == 2)
        launch_reduce_fused_n<2>(ctx, "k_reduce_fused_pre_aux", trace, log_h, d_alpha_pows_mont, a, lead, ro);
    else if (lead.n == 1)
        launch_reduce_fused_n<1>(ctx, "k_reduce_fused_pre", trace, log_h, d_alpha_pows_mont, a, lead, ro);
    else
        launch_reduce_fused_n<0>(ctx, "k_reduce_fused", trace, log_h, d_alpha_pows_mont, a, lead, ro);
    TS_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ reduce on the low coset
void launch_reduce_low(Context& ctx, const ColMat& trace, unsigned log_n, const uint32_t* d_alpha_pows_mont,
                       const FusedReduceArgs& args, const Ef* weights, uint32_t* out) {
    TS_REQUIRE(args.n_chunks <= (uint32_t)MAX_QUOTIENT_CHUNKS, TS_ERR_INVALID, "reduce_low: too many chunks");
    const uint64_t n = 1ull << log_n;
    TS_REQUIRE(args.row0 == 0 && trace.height >= n && trace.col_stride >= n && args.chunk_stride >= n, TS_ERR_INVALID,
               "reduce_low: the matrices must start with the low coset");
    ctx.ensure_twiddles(log_n == 0 ? 1 : log_n);
    FusedReduceArgs a = args;
    a.rows = n;
    TS_LAUNCH_NAMED(ctx, "k_reduce_low", (k_reduce_fused<0, true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                    (const uint32_t*)trace.d, trace.col_stride, trace.width, log_n, (const uint32_t*)ctx.d_twiddle_inv,
                    to_mont(inv_canon(GENERATOR)), d_alpha_pows_mont, a, ExtraReduceArgs<0>{}, weights, out);
    TS_HIP(hipGetLastError());
}

// out[X] = (cols[0][X], cols[1][X], cols[2][X], cols[3][X]): four base-field columns -> the array of EF4 that
// the FRI commit phase takes; one lane per row, one 16-byte store
__global__ void __launch_bounds__(256)
k_ef_interleave(const uint32_t* __restrict__ cols, uint64_t col_stride, uint64_t rows, Ef* __restrict__ out) {
    const uint64_t X = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= rows) return;
    *reinterpret_cast<uint4*>(out + X) = make_uint4(cols[X], cols[col_stride + X], cols[2 * col_stride + X],
                                                    cols[3 * col_stride + X]);
}

void launch_ef_interleave(Context& ctx, const uint32_t* cols, uint64_t col_stride, uint64_t rows, Ef* out) {
    TS_REQUIRE(col_stride >= rows, TS_ERR_INVALID, "ef_interleave: column stride below the row count");
    TS_LAUNCH(ctx, k_ef_interleave, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, cols, col_stride, rows, out);
    TS_HIP(hipGetLastError());
}

}  // namespace ts
