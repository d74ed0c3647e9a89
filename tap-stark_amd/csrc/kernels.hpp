// Host-callable launchers of the HIP kernels (one translation unit per kernel family).
#pragma once
#include <stdint.h>

#include "bb.hpp"
#include "context.hpp"
#include "ntt_plan.hpp"

namespace ts {

// Column-major device matrix: element (row r, column c) at d[c * col_stride + r].
struct ColMat {
    uint32_t* d = nullptr;
    uint64_t height = 0;
    uint32_t width = 0;
    uint64_t col_stride = 0;
};

// ---- ntt.hip, ntt_lde.hip --------------------------------------------------------------------
void launch_build_twiddles(Context& ctx, uint32_t* W, uint32_t* Winv, unsigned log_size);
// the same table in Plantard form, one direction: WP[m + i] = plant_const(w_{2m}^(+-bitrev(i))) as {low, high}
void launch_build_plant_twiddles(Context& ctx, uint2* WP, unsigned log_size, bool inverse);
// per-coset scale tables: lo[beta][j] = s_beta^j * scale (j < 1024), hi[beta][j] = s_beta^(1024 j)
void launch_build_shift_tables(Context& ctx, uint32_t* lo, uint32_t* hi, uint32_t n_hi,
                               uint32_t n_cosets, uint32_t shift_mont, unsigned log_N,
                               unsigned log_blowup, uint32_t scale_mont);
// T[k] = shift^k / n (Montgomery), k < n: the factor the LDE applies to coefficient k, once, before the
// forward transforms of its cosets (the coset's own part, w_N^(bitrev_b(beta) k), is in the N-point twiddles
// those transforms take: ntt_lde.hip).  Cached per context.  nullptr for shift 1: the factor is the constant
// lde_inv_n_mont(log_n), which coset_lde hands its kernel as a value.
const uint32_t* coset_scale_table(Context& ctx, unsigned log_n, uint32_t shift);
inline uint32_t lde_inv_n_mont(unsigned log_n) { return to_mont(inv_canon((uint32_t)((1ull << log_n) % P))); }
// src: row-major n x w (natural rows)  ->  dst: column-major, rows in bit-reversed order
// src_width (0 = w): the row length of `src` when only w of its columns (starting at `src`) are taken
void launch_transpose_bitrev(Context& ctx, const uint32_t* src, uint32_t* dst, unsigned log_n,
                             uint32_t w, uint64_t dst_col_stride, uint32_t src_width = 0);
// The same with the first round (four stages) of the inverse transform folded in, for a matrix that
// goes to coset_lde next (ntt_lde.hip).  Returns false -- and does nothing -- where coset_lde has no
// contiguous inverse pass to shorten (small n): call launch_transpose_bitrev then; if true, pass
// first_round_done = true to coset_lde.
bool launch_transpose_bitrev_r16(Context& ctx, const uint32_t* src, uint32_t* dst, unsigned log_n, uint32_t w,
                                 uint64_t dst_col_stride, uint32_t src_width = 0);
// same without the bit reversal (rows stay where they are): BFMmcs::commit on given matrices
void launch_transpose_plain(Context& ctx, const uint32_t* src, uint32_t* dst, uint64_t n, uint32_t w,
                            uint64_t dst_col_stride);
// dst row-major (h x w)  <-  src column-major; used by debug downloads and row gathers
void launch_transpose_to_row_major(Context& ctx, const uint32_t* src, uint64_t col_stride,
                                   uint32_t* dst, uint64_t h, uint32_t w);
// dst row-major (2^log_h x w, natural rows)  <-  src column-major, rows p < 2^log_h in bit-reversed order
void launch_transpose_unbitrev(Context& ctx, const uint32_t* src, uint64_t col_stride, uint32_t* dst,
                               unsigned log_h, uint32_t w);
// Coset low-degree extension of `ncols` columns (reference fri/src/two_adic_pcs.rs:233-241):
//   in : evals[c][p] = column value at subgroup index bitrev(p)   (n per column, DESTROYED)
//   out: out[c][beta*n + t] = p_c(shift * w_N^bitrev(beta*n+t)),  N = n << log_blowup
// With a coset range (beta0, n_beta > 0) only the row blocks beta0 .. beta0+n_beta-1 are produced,
// at out[c][(beta - beta0)*n + t]: the slab of a rank that owns those cosets (sharded prover).
// Two matrices of one height in ONE set of launches (the two quotient chunks: each is four columns, and a
// launch set of its own left the chip a quarter full three times over): evals2 != nullptr holds columns
// gw .. ncols-1 (same column stride), extended on its own coset shift2; `out` takes all ncols columns.
// stage_timers = false: the passes record no "lde: ..." stage of their own (an extension that belongs to
// another stage's time: the reduced opening's, prover.cpp).
// A call for every coset whose input lies on one of them (lde_own_coset_used: every matrix of the call, and
// first_round_done = false) copies the input to that block and computes the others.
void coset_lde(Context& ctx, uint32_t* evals, uint64_t in_col_stride, uint32_t ncols, unsigned log_n,
               unsigned log_blowup, uint32_t shift, uint32_t* out, uint64_t out_col_stride,
               uint32_t beta0 = 0, uint32_t n_beta = 0, bool first_round_done = false,
               uint32_t* evals2 = nullptr, uint32_t shift2 = 0, uint32_t gw = 0, bool stage_timers = true);

// The block of a whole LDE that coset_lde copies from its input: ntt_plan.hpp lde_own_coset, or -1 where the
// passes compute every block -- TS_LDE_OWN_COSET=0 (read on every call: the A/B and the tests), a blowup of 1,
// the 2^26-row plan.  A caller that could hand coset_lde a half-transformed input (launch_transpose_bitrev_r16)
// asks here first.
constexpr uint32_t LDE_NO_OWN = 0xffffffffu;
int lde_own_coset_used(unsigned log_n, unsigned log_blowup, uint32_t shift);

// The pass launchers of both (ntt_plan.hpp decides the shapes; twiddles must be there, the Montgomery tables and
// the Plantard ones: Context::ensure_twiddles and ensure_plant_twiddles -- for log_n, and in the forward
// direction for log_n + log_blowup).  Each refuses what the plan cannot run with the caller's wording (`lde`).
inline void ntt_require_shape(const NttPlan& p, uint32_t ncols, uint64_t stride_a, uint64_t stride_b, bool lde) {
    if (const char* why = ntt_plan_refusal(p, ncols, stride_a, stride_b, lde)) throw Error(TS_ERR_INVALID, why);
}
// inverse stages log_n-1 .. sA on the chunks of `ncols` columns, in place (two-pass plans; canonical words in and,
// every chunk size taking the Plantard inverse form, canonical words out: ntt_lde.hip ContigForm);
// first_round_done: k_transpose_bitrev_r16 did the first round; data2: columns gw .. live in a second matrix
void launch_contig_inverse(Context& ctx, const NttPlan& p, uint32_t* data, uint64_t col_stride, uint32_t ncols,
                           bool first_round_done = false, uint32_t* data2 = nullptr, uint32_t gw = 0xffffffffu);
// forward stages sA .. log_n-1 on the chunks of `n_blocks` consecutive 2^log_n-row blocks of every column, in
// place, canonical values out (two-pass plans).  own_a != LDE_NO_OWN: n_blocks counts a block per column that
// is left as it is, own_a for the columns below gw and own_b from gw on.
// Block bl is coset beta0 + bl of an LDE of blowup 2^log_blowup and takes that block's stages of the
// (n << log_blowup)-point transform; a standalone transform passes 0 and 0.
void launch_contig_forward(Context& ctx, const NttPlan& p, uint32_t* data, uint64_t col_stride, uint32_t ncols,
                           uint32_t n_blocks, unsigned log_blowup, uint32_t beta0, uint32_t gw = 0xffffffffu,
                           uint32_t own_a = LDE_NO_OWN, uint32_t own_b = LDE_NO_OWN);

// ---- ntt_dft.hip -----------------------------------------------------------------------------
// TwoAdicSubgroupDft on its own.  Row-major matrices are 2^log_n x w, natural rows,
// canonical; `in` is only read, `out` is another buffer.
// In place on `ncols` column-major columns: forward = natural coefficients -> evaluations over shift * H_n
// in bit-reversed order; inverse = bit-reversed evaluations over shift * H_n -> natural coefficients (1/n
// included).  Heights up to 2^26.
void dft_columns(Context& ctx, uint32_t* cols, uint64_t col_stride, uint32_t ncols, unsigned log_n, bool inverse,
                 uint32_t shift);
// coset_dft_batch (inverse = false: out row k = sum_j in[j] (shift w_n^k)^j) / coset_idft_batch
void dft_batch(Context& ctx, const uint32_t* in, uint32_t* out, unsigned log_n, uint32_t w, bool inverse,
               uint32_t shift);
// coset_lde_batch: out ((n << added_bits) x w) row j = the interpolant of `in` over H_n at shift * w_N^j, or
// row bitrev(j) with bit_reversed (then the rows of Pcs::commit's LDE for shift = 31 / domain shift)
void coset_lde_batch(Context& ctx, const uint32_t* in, uint32_t* out, unsigned log_n, uint32_t w, unsigned added_bits,
                     uint32_t shift, bool bit_reversed);
// bit_reverse_rows().to_row_major_matrix(): dst[r] = src[bitrev(r)], both row-major 2^log_h x w
void launch_bit_reverse_rows(Context& ctx, const uint32_t* src, uint32_t* dst, unsigned log_h, uint32_t w);

// ---- merkle.hip ------------------------------------------------------------------------------
constexpr int MAX_BATCH_MATS = 64;
struct LeafMats {
    const uint32_t* d[MAX_BATCH_MATS];
    uint64_t col_stride[MAX_BATCH_MATS];
    uint32_t width[MAX_BATCH_MATS];
    // row of matrix i opened for leaf index r: r >> row_shift[i] (log_max_height - log_height_i;
    // basic/src/mmcs/bf_mmcs.rs:37-42)
    uint8_t row_shift[MAX_BATCH_MATS];
    uint32_t n_mats;
    uint32_t total_width;
    // device array of total_width column base pointers (column c of the concatenated row), so
    // that the leaf kernel addresses a row element with one uniform pointer load
    const uint32_t* const* cols;
};
// leaf digests (8 words each) of `height` rows: Blake3(row of mat 0 || row of mat 1 || ...)
void launch_leaf_hash(Context& ctx, const LeafMats& mats, uint64_t height, uint32_t* digests);
// leaf digests of an array-of-EF4 vector taken as rows of two elements (FRI commit-phase matrix)
void launch_leaf_hash_ef_pairs(Context& ctx, const uint32_t* vec, uint64_t n_rows, uint32_t* digests);
// builds every upper level of the tree; `tree` holds level l at offset level_off(l) (in digests)
// If `ch` is given, the kernel that produces the root also observes it on the device challenger
// and writes the root and the sampled challenge (returns false if no kernel could do it, i.e. the
// tree is a single leaf).
struct DevChallenger;
bool launch_merkle_levels(Context& ctx, uint32_t* tree, unsigned log_leaves,
                          DevChallenger* ch = nullptr, uint32_t* root_out = nullptr,
                          Ef* beta_out = nullptr);
// the whole-tree kernel on the levels from `first_level` up (first_level's nodes are in the tree; between
// 2 and 2^22 of them): what launch_merkle_levels ends in, and the second launch of a tall leaf tree
void launch_merkle_tree_from(Context& ctx, uint32_t* tree, unsigned log_leaves, unsigned first_level,
                             DevChallenger* ch, uint32_t* root_out, Ef* beta_out);
// Leaf digests AND every level in one launch where the shape allows (leaf_tree.hpp; 2^8 leaves and
// up, rows of at most 256 elements; TS_LEAF_TREE=0 or another shape: launch_leaf_hash +
// launch_merkle_levels).  root_out != nullptr: the kernel that makes the root writes it there as well.
bool leaf_tree_enabled(unsigned log_leaves);
void launch_commit_tree(Context& ctx, const LeafMats& mats, unsigned log_leaves, uint32_t* tree,
                        uint32_t* root_out = nullptr);
// mixed-height batches: one level at a time, with the digests of the rows of the matrices whose
// height equals the level's node count compressed into the nodes (node = Blake3(node || inj))
// sharded trees: the G sub-tree roots (gathered, rank order) -> the log2(G) top levels.  `top`
// receives 2G-1 digests (the G roots first, the tree root last).  With `ch` the root is observed
// and the next challenge sampled, as in launch_merkle_levels.
void launch_shard_top(Context& ctx, const uint32_t* subroots, uint32_t G, uint32_t* top,
                      DevChallenger* ch, uint32_t* root_out, Ef* beta_out);
void launch_merkle_one_level(Context& ctx, const uint32_t* children, uint32_t* parents,
                             uint64_t n_parents);
void launch_merkle_inject(Context& ctx, uint32_t* nodes, const uint32_t* inj, uint64_t n);
inline uint64_t merkle_level_offset(unsigned log_leaves, unsigned level) {
    // levels are stored back to back: leaves first
    uint64_t off = 0;
    for (unsigned l = 0; l < level; l++) off += (uint64_t)1 << (log_leaves - l);
    return off;
}
inline uint64_t merkle_total_digests(unsigned log_leaves) { return ((uint64_t)2 << log_leaves) - 1; }

// ---- quotient.hip ----------------------------------------------------------------------------
struct AirProgram;  // air.hpp
// is_first | is_last | is_transition on the quotient domain shift * H_{n qd} in storage (bit-reversed) order,
// qn = 2^(log_n + log_qd) words each, Montgomery form.  Cached per context (Context::sel_tables).
const uint32_t* selector_table(Context& ctx, unsigned log_n, unsigned log_qd, uint32_t shift);
// quotient chunks, each written column-major (4 columns x n) with bit-reversed rows:
// coefficient k of chunk c at chunk[c][k * n + pos]
constexpr int MAX_QUOTIENT_CHUNKS = 64;  // quotient_degree <= 64 (log_quotient_degree <= log_blowup <= 8)
struct QuotOut {
    uint32_t* chunk[MAX_QUOTIENT_CHUNKS];
};
// Rows [row_begin, row_end) of the quotient domain only (row_end = 0: all); trace_lde.d must then
// be such that d[c * col_stride + r] is valid for those rows r and their `next` rows (a sharded
// prover passes its slab pointer minus the slab's first row; whole cosets keep `next` local).
// `shift`: the domain is shift * H_{n qd}; the selectors come from selector_table for the same shift.
// The side matrices of an AIR (AirProgram::n_side of them, in its order: key first, then aux), as the quotient
// reads them: committed LDEs, column-major and bit-reversed like the trace's and of its height, each with its own
// base and stride.  One of them runs the interpreter timed as k_quotient_pre, two as k_quotient_pre_aux, or
// specialised kernels with one (pointer, stride) parameter pair per matrix; none launches what a plain AIR does.
constexpr uint32_t MAX_SIDE_MATS = 2;
struct SideLdes {
    uint32_t n = 0;
    const ColMat* m[MAX_SIDE_MATS] = {nullptr, nullptr};
};
void launch_quotient(Context& ctx, const AirProgram& air, const ColMat& trace_lde, unsigned log_n,
                     unsigned log_qd, const uint32_t* d_consts_mont, const uint32_t* d_alpha_pows_mont,
                     const QuotOut& out, uint64_t row_begin = 0, uint64_t row_end = 0,
                     uint32_t shift = GENERATOR, const SideLdes& side = SideLdes());
// sharded.cpp "local quotient": in place on the slab LDEs of the qd chunk matrices (4 columns each),
// out[c] = sum_c' mix[c * qd + c'] * in[c'] per row and per column (mix: Montgomery form, device)
void launch_chunk_mix(Context& ctx, uint32_t* const* d_chunk_ptrs, uint32_t qd, uint64_t rows, uint64_t col_stride,
                      const uint32_t* d_mix_mont);

// check_constraints.rs:11-39 on the row-major trace; *d_violation (preset to ~0) receives
// row * 2^16 + constraint index of the first violated constraint
// `side`: the same side matrices as their values, row-major: matrix i is n x width[i] words at d[i] (one is
// timed as k_check_constraints_pre, two as k_check_pre_aux).  Passed to the kernel by value.
struct SideRows {
    uint32_t n = 0;
    const uint32_t* d[MAX_SIDE_MATS] = {nullptr, nullptr};
    uint32_t width[MAX_SIDE_MATS] = {0, 0};
};
void launch_check_constraints(Context& ctx, const AirProgram& air, const uint32_t* trace_row_major,
                              uint64_t n, const uint32_t* d_consts_mont,
                              unsigned long long* d_violation, const SideRows& side = SideRows());

// ---- open.hip --------------------------------------------------------------------------------
// d[p][i] = x_i / (z_p - x_i) (Montgomery EF4) for the low coset 31*H_n in bit-reversed order,
// for up to 2 points; out layout [point][n] of Ef
// coset_gen (canonical, 0 = 31): the weights of the coset coset_gen * H_n instead (any coset of
// the LDE determines the polynomial, so a sharded prover interpolates on one it owns)
void launch_bary_weights(Context& ctx, unsigned log_n, const Ef* points_mont, uint32_t n_points,
                         Ef* out, uint32_t coset_gen = 0);
// out[col][p] = sum_i m[col][i] * d[p][i]   (canonical EF4), i over the first n rows
// `pending` != nullptr: the finishing pass (partial sums -> out) is left to launch_bary_finish, which takes
// up to `capacity` pending products in one launch (2; 3 for a proof with a second committed matrix, 4 with a third)
struct BaryPending {
    DevBuf<uint32_t> partial[4];
    uint32_t* out[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t n_blocks[4] = {0, 0, 0, 0}, n_words[4] = {0, 0, 0, 0};
    uint32_t n = 0, capacity = 2;
};
void launch_bary_dots(Context& ctx, const ColMat& m, unsigned log_n, const Ef* weights,
                      uint32_t n_points, Ef* out, BaryPending* pending = nullptr);
void launch_bary_finish(Context& ctx, BaryPending& pending);
// ro[X] (+)= sum_p off_p * (S(X) - rys_p) / (x_X - z_p),  S(X) = sum_i alpha^i m[i][X]
struct ReduceArgs {
    Ef z_mont[2];
    Ef off_mont[2];  // alpha^num_reduced (Montgomery)
    Ef rys[2];       // reduced opened values (canonical)
    uint32_t n_points;
    uint32_t accumulate;  // 0: ro = ..., 1: ro += ...
};
void launch_reduce(Context& ctx, const ColMat& m, unsigned log_h, const uint32_t* d_alpha_pows_mont,
                   const ReduceArgs& args, Ef* ro);
// the prove() shape in one pass: trace opened at (zeta, zeta*omega), n_chunks width-4 matrices at zeta
struct FusedReduceArgs {
    Ef z_mont[2];
    Ef off_t[2];   // alpha^0, alpha^w            (Montgomery)
    // The chunk terms sum_c off_c (S_c - rys_c), off_c = alpha^(2w + 4c), are folded on the host:
    // column k of chunk c is weighted with alpha^k off_c (chunk_w, device memory, Montgomery, 4 EF4
    // per chunk) so that ONE dot product over all chunk columns gives sum_c off_c S_c, and every
    // constant goes into k0 = off_t0 rys_t0 + sum_c off_c rys_c, k1 = off_t1 rys_t1 (canonical).
    Ef k0, k1;
    const uint32_t* chunk_w;
    const uint32_t* chunk[MAX_QUOTIENT_CHUNKS];
    uint64_t chunk_stride;
    uint32_t n_chunks;
    // slab of a sharded prover: global rows [row0, row0 + rows) live at local rows [0, rows) of
    // every matrix and of `ro` (rows = 0: the whole domain)
    uint64_t row0, rows;
};
// The matrices opened at the same two points BEFORE the trace, in opening order: the LDE of the key's
// preprocessed columns (one: timed as k_reduce_fused_pre), then the aux trace's (two: k_reduce_fused_pre_aux).
// Each is a whole LDE of the trace's height.  off[i] = alpha^num_reduced at matrix i's two visits (Montgomery);
// args.off_t then start after them, args.k0 / k1 hold their constants too, and d_alpha_pows_mont covers
// max(every width, 4) powers.
struct LeadingMats {
    uint32_t n = 0;
    const ColMat* m[2] = {nullptr, nullptr};
    Ef off[2][2];
};
void launch_reduce_fused(Context& ctx, const ColMat& trace, unsigned log_h,
                         const uint32_t* d_alpha_pows_mont, const FusedReduceArgs& args, Ef* ro,
                         const LeadingMats& lead = LeadingMats());
// The same reduced opening on the low coset only (rows t < n = 2^log_n of matrices that hold the whole LDE, no
// leading matrices): out = four base-field columns of n rows (stride n, canonical), to be extended by
// coset_lde with shift 1 like a quotient chunk on 31 H_n.  `weights` = launch_bary_weights' output for
// args.z_mont on the coset 31 H_n ([2][n]); no inversion runs.  args.rows is not used.
void launch_reduce_low(Context& ctx, const ColMat& trace, unsigned log_n, const uint32_t* d_alpha_pows_mont,
                       const FusedReduceArgs& args, const Ef* weights, uint32_t* out);
// out[X] = (cols[k * col_stride + X])_{k < 4}, X < rows
void launch_ef_interleave(Context& ctx, const uint32_t* cols, uint64_t col_stride, uint64_t rows, Ef* out);

// ---- open_multi.hip --------------------------------------------------------------------------
// The opening of a multi-table proof (prove_multi.cpp), one pass per height class: every committed matrix of
// LDE height 2^log_h, of both rounds, is opened at z0 = zeta, and the trace matrices among them at
// z1 = zeta omega_n as well.  One matrix of a class, as the kernel reads it from a table in device memory:
struct ClassJob {
    const uint32_t* d;       // column-major, bit-reversed rows, 2^log_h of them
    uint64_t col_stride;
    uint32_t width;
    uint32_t has_next;       // 1: a trace matrix, opened at both points; 0: a quotient chunk, at z0 only
    // has_next: the column weights are the alpha powers and off[p] = alpha^num_reduced at its (matrix, point)
    // visit (two_adic_pcs.rs:371,383; Montgomery).  Otherwise `weights` holds alpha^k off_0 per column k
    // (device memory, Montgomery, 4 words each): the chunks of a class then cost one dot product in all.
    const uint32_t* weights;
    Ef off[2];
};
struct ClassReduceArgs {
    Ef z_mont[2];
    Ef k0, k1;  // sum over the class of off_p * reduced_ys_p (canonical), folded on the host
};
// ro[X] = inv(x_X - z0) (sum_m off_{m,0} S_m(X) - k0) + inv(x_X - z1) (sum_{m trace} off_{m,1} S_m(X) - k1) for
// every row X of the class; one store per row, `ro` is never read.  d_jobs: n_jobs >= 1 entries, device memory.
void launch_reduce_class(Context& ctx, const ClassJob* d_jobs, uint32_t n_jobs, unsigned log_h,
                         const uint32_t* d_alpha_pows_mont, const ClassReduceArgs& args, Ef* ro);
// The finishing pass of any number of launch_bary_dots products in one launch (k_bary_finish<N> takes up to
// four by value): out[j] = sum over blocks of partial[block][j].  d_jobs: the jobs; d_groups: per workgroup
// {job, group of four output words within it}; both device memory.
struct BaryFinishJob {
    const uint32_t* partial;
    uint32_t* out;
    uint32_t n_blocks, n_words;
};
void launch_bary_finish_jobs(Context& ctx, const BaryFinishJob* d_jobs, const uint2* d_groups, uint32_t n_groups);

// ---- fri.hip ---------------------------------------------------------------------------------
// out[i] = fold(in[2i], in[2i+1]; beta) (reference two_adic_pcs.rs:116-147); h = output length.
// If next_digests != nullptr (h >= 2) also writes the h/2 leaf digests of the next round.
void launch_fri_fold(Context& ctx, const Ef* in, uint64_t h, Ef beta_canonical, Ef* out,
                     uint32_t* next_digests);
// same with beta read from device memory (written by the round's transcript step)
// slab form: `in`/`out` hold global outputs [row0, row0 + h) of a fold whose output has h_global
// rows (h_global = 0: the whole vector, h_global = h, row0 = 0)
void launch_fri_fold_dev(Context& ctx, const Ef* in, uint64_t h, const Ef* d_beta, Ef* out,
                         uint32_t* next_digests, uint64_t h_global = 0, uint64_t row0 = 0);
// One commit-phase round (fri/src/prover.rs:113-116): leaves (cur[2i], cur[2i+1]) hashed, the whole tree
// built and -- with `ch` -- the root observed on the device transcript (chal_dev.hpp) and the next challenge
// sampled, in as few launches as the shape allows; the launcher owns that choice (fri.hip).
struct FriRoundLaunch {
    // != nullptr: cur (2h elements) is first computed as the fold of prev (4h elements) with the challenge
    // at d_beta_prev, and stored
    const Ef* prev = nullptr;
    const Ef* d_beta_prev = nullptr;
    Ef* cur = nullptr;
    uint64_t h = 0;  // leaves
    uint32_t* tree = nullptr;
    // the transcript step; nullptr: the tree only (the sub-tree of a sharded prover's slab, whose root the
    // top kernel makes: launch_shard_top)
    DevChallenger* ch = nullptr;
    uint32_t* root_out = nullptr;
    Ef* beta_out = nullptr;
    // slab form as launch_fri_fold_dev, in LEAVES: `cur`/`tree` hold leaves [row0, row0 + h) of a round of
    // h_global leaves
    uint64_t h_global = 0, row0 = 0;
};
void launch_fri_commit_round(Context& ctx, const FriRoundLaunch& r);
// all remaining commit-phase rounds once the vector has <= 2^FRI_TAIL_LOG elements, one workgroup
constexpr int FRI_TAIL_LOG = 10;
// pow_out != nullptr: the kernel also grinds (fri/src/prover.rs:43) -- *pow_out = the smallest witness
// below 4096 that passes pow_bits on the transcript as the last round leaves it, FRI_POW_NONE if it
// cannot tell (pending transcript input, the test permutation) or none passes
constexpr uint32_t FRI_POW_NONE = 0xffffffffu;
void launch_fri_tail(Context& ctx, const Ef* in, uint32_t L0, uint32_t blowup, DevChallenger* ch,
                     Ef* tail_vecs, uint32_t* tail_trees, uint32_t* roots_out, Ef* betas_out,
                     Ef* final_out, uint32_t pow_bits = 0, uint32_t* pow_out = nullptr,
                     const Ef* beta_in = nullptr);
// (beta_in != nullptr: `in` holds 2 L0 elements, the previous round's vector, and the kernel starts by
// folding it with *beta_in)
void launch_vec_add(Context& ctx, Ef* acc, const Ef* other, uint64_t n);
// The whole query phase of one proof in ONE launch (after the host's sync the stream is empty, and
// every launch on an empty stream costs the ~4 us it takes to reach the GPU: five launches were 16 us
// of a 3.4 ms proof); driven by QueryGather (prover_internal.hpp).  Row jobs: the opened rows of a committed
// batch.  Descriptor jobs: per query the row of two values and its Merkle path (a FRI round opening), where
// vec == nullptr means "path only" (the batch's Merkle path) and log_leaves == 0 "values only" (a pass-through
// input).  Both tables are device arrays.
struct FriGatherDesc {
    const uint32_t* vec;   // committed vector as words (8 per row)
    const uint32_t* tree;  // its Merkle tree
    uint32_t log_leaves;
    uint32_t shift;        // row = index >> shift
    uint64_t out_vals;     // word offset of [query][8] in `out`
    uint64_t out_path;     // word offset of [query][log_leaves][8] in `out`
};
struct RowGatherJob {
    LeafMats mats;
    uint32_t shift;  // row = index >> shift (>> row_shift[i] per matrix)
    uint32_t pad;
    uint64_t out;    // word offset of [query][total_width] in `out`
};
void launch_gather_queries(Context& ctx, const RowGatherJob* d_rows, uint32_t n_rows, uint32_t max_row_width,
                           const FriGatherDesc* d_descs, uint32_t n_descs, uint32_t max_log_leaves,
                           const uint32_t* d_indices, uint32_t n_idx, uint32_t* out);

// ---- alubench.hip ---------------------------------------------------------------------------
// whole-chip rate of NTT butterflies (kind 0) or Blake3 compressions (kind 1), no memory traffic
double alu_ceiling(Context& ctx, int kind);
// (prover_common.cpp) mean ms of one repetition of one stage of the path, on resident, arbitrary data:
// stage 0 coset_lde of a 2^log_n x width matrix, 1 the commit hashing of its LDE, 2 .. 4 one LDE pass alone
double bench_stage(Context& ctx, int stage, unsigned log_n, uint32_t width, unsigned log_blowup, uint32_t reps);

// ---- tracegen.hip ----------------------------------------------------------------------------
// row-major traces generated in place (no H2D): Fibonacci (uni-stark/tests/fib_air.rs:59-78) and the
// build-defined SynthMulAir-w trace (airs.py generate_synth_mul_trace)
void launch_trace_fibonacci(Context& ctx, uint32_t* out, uint32_t a, uint32_t b, uint64_t n);
void launch_trace_synth_mul(Context& ctx, uint32_t* out, uint64_t n, uint32_t width, uint64_t seed);
// build-defined SynthExt-w trace (airs.py generate_synth_ext_trace; config 5's stand-in)
void launch_trace_synth_ext(Context& ctx, uint32_t* out, uint64_t n, uint32_t width, uint64_t seed);

// ---- ingest.hip ------------------------------------------------------------------------------
// A trace as the host holds it (include/tapstark.h ts_trace_format) -> the row-major canonical matrix.
enum : uint8_t { COL_U32 = 0, COL_U16 = 1, COL_U8 = 2, COL_MONTY32 = 3, COL_MONTY31 = 4 };  // = TS_COL_*
struct IngestPlan {
    bool planar = false;
    uint64_t height = 0;
    uint32_t width = 0;
    uint64_t stride = 0;  // rows layout: bytes from one row to the next
    uint64_t bytes = 0;   // of the whole source buffer
    // the one kind of a uniform 4-byte format in tight rows (the source is then the matrix word for word:
    // copied straight into it, launch_scale_words for a Montgomery kind), else -1
    int uniform4 = -1;
    // per column (byte offset << 3) | kind; the offset within a row (rows layout) or of the column within
    // the buffer (planar)
    std::vector<uint64_t> table;
};
// The one place a format's offsets and size are worked out; host only, no device is touched.  Throws
// TS_ERR_INVALID for an unknown kind, n_kinds neither 1 nor width, a stride below a row's bytes (or given for
// planar), a height that is no power of two or above 2^27.
IngestPlan ingest_plan(const uint8_t* kinds, uint32_t n_kinds, bool planar, uint64_t row_stride, uint64_t height,
                       uint32_t width);
// src: plan.bytes device bytes, 16-byte aligned, only read -> out: height x width row-major canonical words
void launch_ingest(Context& ctx, const IngestPlan& plan, const uint8_t* src, uint32_t* out);
// out[i] = in[i] * mult * 2^-32 mod p (canonical; in place allowed; 16-byte aligned): a Montgomery word to its
// value with mult = monty_ingest_factor(kind), a value to its Montgomery word with mult = 2^(32 + radix) mod p
void launch_scale_words(Context& ctx, const uint32_t* in, uint32_t* out, uint64_t n, uint32_t mult);
uint32_t monty_ingest_factor(uint32_t kind);

}  // namespace ts
