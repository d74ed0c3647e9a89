// prove() and TwoAdicFriPcs on the device.  Transcript order, proof structure and every index
// convention follow the reference:
//   uni-stark/src/prover.rs:25-119      prove
//   fri/src/two_adic_pcs.rs:227-245     commit
//   fri/src/two_adic_pcs.rs:247-258     get_evaluations_on_domain (fused into the quotient kernel)
//   fri/src/two_adic_pcs.rs:260-419     open
//   fri/src/prover.rs:19-141            bf_prove / bf_commit_phase / bf_answer_query
// The GPU owns the data from the uploaded trace to the opened rows; the host owns the transcript
// (one 32-byte root down, one challenge up per commitment).
#include <string.h>

#include <algorithm>

#include "logup.hpp"
#include "prover_internal.hpp"

namespace ts {

// ------------------------------------------------------------------ BFMmcs::commit
// basic/src/mmcs/bf_mmcs.rs:22-35 on matrices already resident (column-major): builds the Blake3
// Merkle tree over data.ldes (data.log_height = log2 of the tallest) and leaves the root in data.root.
void mmcs_commit(Context& ctx, PcsData& data) {
    const unsigned log_H = data.log_height;
    const uint64_t N = 1ull << log_H;
    bool uniform = true;
    for (auto& cm : data.ldes) uniform = uniform && cm.height == N;
    {
        StageTimer t(&ctx, "merkle_commit");
        data.tree = DevBuf<uint32_t>(&ctx, merkle_total_digests(log_H) * 8);
        // column pointers grouped by height (tallest first), commit order inside a group
        std::vector<const uint32_t*> cols;
        struct Group { uint64_t height; size_t first; uint32_t total; };
        std::vector<Group> groups;
        for (unsigned lh = log_H + 1; lh-- > 0;) {
            const std::vector<const uint32_t*> gc = column_pointers(data.ldes, 1ull << lh);
            if (!gc.empty()) groups.push_back(Group{1ull << lh, cols.size(), (uint32_t)gc.size()});
            cols.insert(cols.end(), gc.begin(), gc.end());
        }
        data.col_table = DevBuf<const uint32_t*>(&ctx, cols.size());
        data.col_table_uploaded = false;
        auto group_mats = [&](const Group& g) {
            LeafMats lm;
            memset(&lm, 0, sizeof lm);
            lm.cols = data.col_table.p + g.first;
            lm.total_width = g.total;
            // one matrix -- or several lying back to back with one stride -- lets the leaf kernel address
            // the columns by stride (rows of at most 256 elements)
            ColMat one;
            if (columns_as_one_matrix(data.ldes, g.height, 256, one)) {
                lm.n_mats = 1;
                lm.d[0] = one.d;
                lm.col_stride[0] = one.col_stride;
                lm.width[0] = one.width;
            } else if (!data.col_table_uploaded) {
                // only the pointer-table leaf kernels (several scattered matrices, rows wider than 256) read it
                h2d(ctx, data.col_table.p, cols.data(), cols.size() * sizeof(const uint32_t*));
                data.col_table_uploaded = true;
            }
            return lm;
        };
        auto group_leaves = [&](const Group& g, uint32_t* digests) {
            launch_leaf_hash(ctx, group_mats(g), g.height, digests);
        };
        uint32_t* mail = nullptr;
        if (uniform) {  // leaves and every level in one launch (leaf_tree.hpp)
            // the kernel that makes the root writes it into the context's mailbox (host memory) as well:
            // no copy kernel between the tree and the host's next transcript step
            if (log_H >= 1) mail = ctx.mailbox(8);
            launch_commit_tree(ctx, group_mats(groups[0]), log_H, data.tree.p, mail);
        } else {
            group_leaves(groups[0], data.tree.p);
            DevBuf<uint32_t> inj(&ctx, 8 * (N / 2));
            size_t gi = 1;
            for (unsigned l = 1; l <= log_H; l++) {
                uint32_t* children = data.tree.p + 8 * merkle_level_offset(log_H, l - 1);
                uint32_t* parents = data.tree.p + 8 * merkle_level_offset(log_H, l);
                const uint64_t n_par = N >> l;
                launch_merkle_one_level(ctx, children, parents, n_par);
                if (gi < groups.size() && groups[gi].height == n_par) {
                    group_leaves(groups[gi], inj.p);
                    launch_merkle_inject(ctx, parents, inj.p, n_par);
                    gi++;
                }
            }
        }
        if (mail) {
            ctx.sync_point(mail, 32);
            memcpy(data.root, mail, 32);
        } else {
            d2h_sync(ctx, data.root, data.tree.p + 8 * (merkle_total_digests(log_H) - 1), 32);
        }
    }
}

// ------------------------------------------------------------------ commit
// Matrices of different heights share one tree (basic/src/mmcs/bf_mmcs.rs:22-35 commits a mixed batch;
// the tree itself is build-defined, see merkle.hip): leaves hash the rows of the tallest matrices,
// and the rows of the matrices of height h are compressed into the level that has h nodes.
std::unique_ptr<PcsData> TwoAdicFriPcs::commit(std::vector<DeviceMatrix>& evals,
                                               const std::vector<uint32_t>& domain_shifts, bool build_tree,
                                               bool keep_row_major) {
    auto data = std::make_unique<PcsData>();
    lde_stage(ctx_, fri_, evals, domain_shifts, 0, 0, /*allow_pair=*/true, *data, keep_row_major);
    if (build_tree) mmcs_commit(ctx_, *data);
    return data;
}

// ------------------------------------------------------------------ quotient
void check_side_matrix(const PcsData& data, const AirProgram& air, uint32_t i, uint64_t lde_height) {
    const bool aux = air.side_is_aux(i);
    const std::string what = aux ? "aux data" : "preprocessed key";
    TS_REQUIRE(data.ldes.size() == 1, TS_ERR_INVALID, what + ": exactly one committed matrix expected");
    TS_REQUIRE(i < air.n_side() && data.ldes[0].width == air.side_width(i), TS_ERR_INVALID,
               what + ": width differs from the AIR's " + (aux ? "aux" : "preprocessed") + " width");
    TS_REQUIRE(data.ldes[0].height == lde_height, TS_ERR_INVALID,
               what + ": LDE height is not the trace height << log_blowup");
}

std::vector<DeviceMatrix> TwoAdicFriPcs::quotient_chunks(const PcsData& trace_data,
                                                         const AirProgram& air,
                                                         const std::vector<uint32_t>& pis, Ef alpha,
                                                         const SideData& side) {
    TS_REQUIRE(trace_data.ldes.size() >= 1, TS_ERR_INVALID, "quotient: no trace matrix");
    TS_REQUIRE(trace_data.log_height >= fri_.log_blowup, TS_ERR_INVALID, "quotient: bad trace data");
    TS_REQUIRE(side.size() <= MAX_SIDE_MATS, TS_ERR_INVALID, "quotient: more than two committed side matrices");
    SideLdes ldes;
    for (const PcsData* d : side) {
        check_side_matrix(*d, air, ldes.n, trace_data.ldes[0].height);
        ldes.m[ldes.n++] = &d->ldes[0];
    }
    return quotient_chunks_slab(trace_data.ldes[0], trace_data.log_height - fri_.log_blowup, Slab{}, air,
                                pis, alpha, GENERATOR, ldes);
}

std::vector<DeviceMatrix> TwoAdicFriPcs::quotient_chunks_slab(const ColMat& lde_slab, unsigned log_n,
                                                              const Slab& slab, const AirProgram& air,
                                                              const std::vector<uint32_t>& pis, Ef alpha,
                                                              uint32_t domain_shift, const SideLdes& side) {
    StageTimer t(&ctx_, "compute quotient polynomial");
    TS_REQUIRE(side.n == air.n_side(), TS_ERR_INVALID,
               "quotient: an AIR needs the committed key of its preprocessed columns and the committed aux trace of "
               "its aux columns, and only such an AIR takes them");
    TS_REQUIRE(side.n == 0 || slab.rows == 0, TS_ERR_UNSUPPORTED, "quotient: preprocessed or aux columns on a slab");
    TS_REQUIRE(lde_slab.width == air.width, TS_ERR_INVALID, "quotient: trace width != AIR width");
    TS_REQUIRE(pis.size() == air.n_public_slots(), TS_ERR_INVALID, "quotient: wrong number of public values");
    const unsigned lqd = air.log_quotient_degree;
    // two_adic_pcs.rs:256: assert!(lde.height() >= domain.size())
    TS_REQUIRE(lqd <= fri_.log_blowup, TS_ERR_INVARIANT,
               "quotient domain larger than the committed LDE (log_quotient_degree > log_blowup)");
    const uint64_t n = 1ull << log_n, qn = n << lqd;
    const uint32_t qd = 1u << lqd;
    // rows of the quotient domain (the first qn bit-reversed rows of the LDE) inside the slab
    const uint64_t slab_rows = slab.rows ? slab.rows : lde_slab.height;
    const uint64_t row_begin = std::min<uint64_t>(slab.row0, qn);
    const uint64_t row_end = std::min<uint64_t>(slab.row0 + slab_rows, qn);
    // whole cosets only: `next` (natural index + qd) stays inside a coset of H_n
    TS_REQUIRE(row_begin % n == 0 && row_end % n == 0, TS_ERR_INVALID, "quotient: slab must hold whole cosets");

    // constants / public values, then alpha^(K-1-i): folder.rs:60-64 unrolled (acc = acc*alpha + c_i).  One
    // upload for both (a small host-to-device copy is a launch of its own on the stream)
    std::vector<uint32_t> consts = air_consts_mont(air, pis.data(), pis.size());
    consts.resize((consts.size() + 3) & ~(size_t)3, 0);  // the powers stay 16-byte aligned
    const size_t n_consts = consts.size();
    const uint32_t K = air.n_constraints;
    const std::vector<uint32_t> pw = alpha_powers_mont(alpha, K);
    consts.resize(n_consts + std::max<size_t>(4 * (size_t)K, 4), 0);
    for (uint32_t i = 0; i < K; i++) memcpy(&consts[n_consts + 4 * (size_t)(K - 1 - i)], &pw[4 * (size_t)i], 16);
    DevBuf<uint32_t> d_consts(&ctx_, consts.size());
    h2d(ctx_, d_consts.p, consts.data(), consts.size() * 4);

    std::vector<DeviceMatrix> chunks(qd);
    QuotOut qo;
    memset(&qo, 0, sizeof qo);
    for (uint32_t c = 0; c < qd; c++) {
        chunks[c].buf = DevBuf<uint32_t>(&ctx_, 4 * n);
        chunks[c].height = n;
        chunks[c].width = 4;
        chunks[c].layout = DeviceMatrix::COL_MAJOR_BITREV;
        qo.chunk[c] = chunks[c].buf.p;
    }
    if (row_begin < row_end) {
        ColMat lde = lde_slab;
        lde.d = lde_slab.d - slab.row0;  // global row r of the slab's range lives at d[r]
        launch_quotient(ctx_, air, lde, log_n, lqd, d_consts.p, d_consts.p + n_consts, qo, row_begin, row_end,
                        domain_shift, side);
    }
    return chunks;  // (the staged uploads live in the context's pinned arena: no sync needed)
}

// ------------------------------------------------------------------ open
DevBuf<Ef> TwoAdicFriPcs::open_reduce(const PcsData& trace_data, const PcsData& quotient_data, Ef zeta,
                                      Ef alpha, std::vector<Ef>& opened_values, const SideData& side) {
    TS_REQUIRE(trace_data.log_height == quotient_data.log_height, TS_ERR_INVALID,
               "open: trace and quotient LDE heights differ");
    return open_reduce_slab(trace_data, quotient_data, trace_data.log_height, Slab{}, zeta, alpha,
                            opened_values, side);
}

// `slab` (rows != 0): the two PcsData hold only global rows [row0, row0 + rows) of the LDEs, which
// start with the whole coset beta0 (sharded prover).  The opened values are interpolated on that
// coset -- any coset of the LDE determines the polynomials, so every rank gets the same values.
DevBuf<Ef> TwoAdicFriPcs::open_reduce_slab(const PcsData& trace_data, const PcsData& quotient_data,
                                           unsigned log_N, const Slab& slab, Ef zeta, Ef alpha,
                                           std::vector<Ef>& opened_values, const SideData& side) {
    TS_REQUIRE(trace_data.ldes.size() == 1, TS_ERR_UNSUPPORTED, "open: one trace matrix expected");
    // The rounds opened before the trace, at the trace's points, in opening order = the side matrices' order: a
    // preprocessed round (the key), then an aux round (four rounds with both: key, aux, trace, chunks).  Each is
    // one matrix of the trace's height, whole LDE; its 2 width values lead the opened values and its columns the
    // offsets (two_adic_pcs.rs:371,383).
    TS_REQUIRE(side.size() <= MAX_SIDE_MATS, TS_ERR_INVALID, "open: more than two rounds before the trace's");
    LeadingMats lead;
    for (const PcsData* d : side) {
        TS_REQUIRE(slab.rows == 0 && d->ldes.size() == 1 && d->ldes[0].height == trace_data.ldes[0].height,
                   TS_ERR_INVALID, "open: preprocessed or aux round shape");
        lead.m[lead.n++] = &d->ldes[0];
    }
    const unsigned log_n = log_N - fri_.log_blowup;
    const uint64_t n = 1ull << log_n;
    const uint64_t N = slab.rows ? slab.rows : 1ull << log_N;  // rows held here
    TS_REQUIRE(N >= n && trace_data.ldes[0].height == N, TS_ERR_INVALID, "open: slab shape");
    // x of local row t < n: coset_gen * omega_n^bitrev(t), coset_gen = 31 * omega_N^bitrev_b(beta0)
    const uint32_t coset_gen =
        mul(GENERATOR, pow_canon(two_adic_generator(log_N), bitrev32(slab.beta0, fri_.log_blowup)));
    const ColMat& tr = trace_data.ldes[0];
    const uint32_t w = tr.width;
    const uint32_t qd = (uint32_t)quotient_data.ldes.size();
    for (auto& m : quotient_data.ldes)
        TS_REQUIRE(m.width == 4, TS_ERR_INVALID, "open: quotient chunks must have width 4");
    ctx_.ensure_lde_twiddles(std::max(1u, log_N));
    // the matrices opened at both points, in opening order: the leading ones, then the trace.  Raw sums and
    // opened values are laid out in that order, 2 width words each, and the 4 qd of the chunks behind them
    const ColMat* two_point[3];
    uint32_t n_two = 0, max_w = 4;
    size_t chunks_at = 0;
    for (uint32_t i = 0; i < lead.n; i++) two_point[n_two++] = lead.m[i];
    two_point[n_two++] = &tr;
    for (uint32_t i = 0; i < n_two; i++) {
        chunks_at += 2 * (size_t)two_point[i]->width;
        max_w = std::max(max_w, two_point[i]->width);
    }

    // prover.rs:92 zeta_next = trace_domain.next_point(zeta) = zeta * omega_n
    const Ef zeta_next = efc_mul_base(zeta, two_adic_generator(log_n));
    const Ef pts_mont[2] = {ef_to_mont(zeta), ef_to_mont(zeta_next)};

    // ---- opened values: barycentric interpolation on the low coset (two_adic_pcs.rs:358-369)
    std::vector<Ef> raw(chunks_at + 4 * (size_t)qd);  // [col][point] per matrix
    DevBuf<Ef> weights(&ctx_, 2 * n);  // x_t / (z_p - x_t): the low-coset reduce below divides by them again
    {
        StageTimer t(&ctx_, "compute opened values with Lagrange interpolation");
        launch_bary_weights(ctx_, log_n, pts_mont, 2, weights.p, coset_gen);
        // the last kernels of the stage write the sums straight into the context's mailbox (host memory)
        Ef* const mail = reinterpret_cast<Ef*>(ctx_.mailbox(4 * raw.size()));
        BaryPending pend;  // every matrix's partial sums are added up in one launch
        pend.capacity = n_two + 1;
        Ef* sums = mail;
        for (uint32_t i = 0; i < n_two; i++) {
            launch_bary_dots(ctx_, *two_point[i], log_n, weights.p, 2, sums, &pend);
            sums += 2 * (size_t)two_point[i]->width;
        }
        ColMat all;  // lde_stage lays the chunk LDEs back to back (no width limit: the dot products take any)
        if (qd > 1 && columns_as_one_matrix(quotient_data.ldes, quotient_data.ldes[0].height, 0, all) &&
            all.width == 4 * qd) {
            launch_bary_dots(ctx_, all, log_n, weights.p, 1, sums, &pend);
        } else {
            for (uint32_t c = 0; c < qd; c++)
                launch_bary_dots(ctx_, quotient_data.ldes[c], log_n, weights.p, 1, sums + 4 * c, &pend);
        }
        launch_bary_finish(ctx_, pend);
        ctx_.sync_point(mail, raw.size() * sizeof(Ef));
        memcpy(raw.data(), mail, raw.size() * sizeof(Ef));
    }
    // p(z) = ((z/s)^n - 1)/n * sum_i p_i x_i/(z - x_i) on the coset s*H_n (s = 31 unless sharded)
    const Ef scale[2] = {bary_scale(zeta, coset_gen, n), bary_scale(zeta_next, coset_gen, n)};
    opened_values.assign(raw.size(), ef_zero());
    size_t at = 0;
    for (uint32_t i = 0; i < n_two; i++) {  // local, then next
        opened_from_raw(&raw[at], two_point[i]->width, 2, scale, &opened_values[at]);
        at += 2 * (size_t)two_point[i]->width;
    }
    opened_from_raw(&raw[at], 4 * qd, 1, scale, &opened_values[at]);

    // ---- reduce (two_adic_pcs.rs:371-383)
    StageTimer t(&ctx_, "reduce rows");
    // The reduced opening has degree < n: on wide proofs it is computed on the low coset only, where the
    // inverses are the barycentric weights, and extended like a quotient chunk on 31 H_n (open.hip)
    const bool low = slab.rows == 0 && lead.n == 0 && reduce_low_wanted(w + 4 * qd);
    if (!low) weights.reset();
    DevBuf<Ef> ro(&ctx_, N);
    TS_REQUIRE(qd <= (uint32_t)MAX_QUOTIENT_CHUNKS, TS_ERR_UNSUPPORTED, "open: more than 64 quotient chunks");
    FusedReduceArgs a;
    memset(&a, 0, sizeof a);
    a.z_mont[0] = pts_mont[0];
    a.z_mont[1] = pts_mont[1];
    a.n_chunks = qd;
    a.chunk_stride = N;
    a.row0 = slab.row0;
    a.rows = N;
    // every matrix shares log_height here: one height of the ledger, visited in opening order
    AlphaLedger ledger(alpha, max_w);
    const Ef* ys = opened_values.data();
    for (uint32_t i = 0; i < n_two; i++) {
        const uint32_t mw = two_point[i]->width;
        Ef* const off = i < lead.n ? lead.off[i] : a.off_t;
        for (int p = 0; p < 2; p++, ys += mw) off[p] = ledger.visit(log_N, ys, mw, p).off;
    }
    // the alpha powers and, behind them, the chunk weights: one copy on the stream instead of two
    std::vector<uint32_t> words = ledger.powers();
    const size_t n_apow = words.size();
    for (uint32_t c = 0; c < qd; c++, ys += 4) {
        TS_REQUIRE(quotient_data.ldes[c].col_stride == N, TS_ERR_INVALID, "open: chunk stride");
        a.chunk[c] = quotient_data.ldes[c].d;
        ledger.fold_weights(ledger.visit(log_N, ys, 4, 0).off, 4, words);  // alpha^k off_c: column k of chunk c
    }
    a.k0 = ledger.k(log_N, 0);
    a.k1 = ledger.k(log_N, 1);
    DevBuf<uint32_t> d_apow(&ctx_, words.size());
    h2d(ctx_, d_apow.p, words.data(), words.size() * 4);
    a.chunk_w = d_apow.p + n_apow;
    if (low) {
        DevBuf<uint32_t> ro_low(&ctx_, 4 * n), ro_cols(&ctx_, 4 * N);
        launch_reduce_low(ctx_, tr, log_n, d_apow.p, a, weights.p, ro_low.p);
        // the chunk-0 call of lde_stage (domain shift 31, so coset_lde's shift is 1), without its stage
        // timers: the launches belong to "reduce rows"
        coset_lde(ctx_, ro_low.p, n, 4, log_n, fri_.log_blowup, 1, ro_cols.p, N, 0, 0, false, nullptr, 0, 0,
                  /*stage_timers=*/false);
        launch_ef_interleave(ctx_, ro_cols.p, N, N, ro.p);
    } else {
        launch_reduce_fused(ctx_, tr, log_N, d_apow.p, a, ro.p, lead);
    }
    return ro;
}

// ------------------------------------------------------------------ open_batch
void TwoAdicFriPcs::open_batch(const PcsData& d, uint64_t index, std::vector<uint32_t>& rows,
                               std::vector<uint32_t>& path) {
    TS_REQUIRE(index < (1ull << d.log_height), TS_ERR_INVALID, "open_batch: index out of range");
    QueryGather qg(ctx_);
    const unsigned li = qg.add_indices({(uint32_t)index});
    const QueryGather::Slot o_rows = qg.add_rows(li, d.leaf_mats(), 0), o_path = qg.add_path(li, d.tree.p, d.log_height, 0);
    qg.run();
    rows.assign(qg.data(o_rows, 0), qg.data(o_rows, 0) + o_rows.words);
    path.assign(qg.data(o_path, 0), qg.data(o_path, 0) + o_path.words);
}

// ------------------------------------------------------------------ bf_prove
// fri/src/prover.rs:19-141 (bf_prove, bf_commit_phase, bf_answer_query) with the open_input closure
// of two_adic_pcs.rs:399-414.  `inputs` are the reduced openings by strictly descending height.
// Appends the FriProof to `pf`.
void TwoAdicFriPcs::fri_prove(std::vector<DevBuf<Ef>>& inputs, const std::vector<unsigned>& log_lens,
                              BfChallenger& challenger,
                              const std::vector<const PcsData*>& input_rounds,
                              std::vector<uint32_t>& pf, bool pass_through) {
    Context& ctx = ctx_;
    const FriConfig& fri = fri_;
    TS_REQUIRE(!inputs.empty() && inputs.size() == log_lens.size(), TS_ERR_INVALID, "FRI: no input");
    // pass-through input proof (fri/tests/fri.rs:109-118): the literal reduced openings; the input
    // vectors stay alive (and unmodified) in the commit state until the queries are answered
    std::vector<const Ef*> in_ptr;
    for (auto& v : inputs) in_ptr.push_back(v.p);
    if (pass_through)
        TS_REQUIRE(input_rounds.empty() && log_lens.back() >= 1, TS_ERR_INVALID,
                   "FRI: pass-through input proof takes no committed batches");
    for (size_t k = 1; k < log_lens.size(); k++)
        TS_REQUIRE(log_lens[k] < log_lens[k - 1], TS_ERR_INVALID, "FRI: inputs must descend in height");
    const unsigned log_max_height = log_lens[0];  // prover.rs:30
    TS_REQUIRE(log_lens.back() >= fri.log_blowup, TS_ERR_INVALID, "FRI: vector shorter than the blowup");
    for (const PcsData* d : input_rounds)
        TS_REQUIRE(d->log_height <= log_max_height, TS_ERR_INVALID,
                   "FRI: a committed batch is taller than every opened matrix");

    FriCommit st;
    Ef final_poly;
    {
        StageTimer t(&ctx, "FRI commit phase");
        fri_commit_begin(ctx, fri, log_max_height, challenger, st);
        fri_commit_rounds(ctx, fri, std::move(inputs[0]), 1ull << log_max_height, inputs, log_lens, 1, st);
        final_poly = fri_commit_finish(ctx, fri, challenger, st);
    }
    std::vector<FriRound>& rounds = st.rounds;
    const uint32_t R = (uint32_t)rounds.size();

    // :43 proof of work
    uint32_t pow_witness;
    {
        StageTimer t(&ctx, "grind for proof-of-work witness");
        pow_witness = fri_pow_witness(ctx, challenger, fri.proof_of_work_bits, st);
    }

    // ---- query phase :45-59
    StageTimer tq(&ctx, "query phase");
    const uint32_t Q = fri.num_queries;
    std::vector<uint32_t> indices(Q);
    for (uint32_t q = 0; q < Q; q++) indices[q] = (uint32_t)challenger.sample_bits(log_max_height);

    // The whole query phase is ONE upload, ONE launch and ONE D2H (QueryGather): the opened rows and the Merkle
    // path of every committed batch (two_adic_pcs.rs:403-409: bits_reduced = log_global_max_height -
    // log_max_height(batch)), bf_answer_query :69-90 for every commit round (index_i = index >> i >> 1) and
    // the pass-through inputs (values only: the pair holding element index >> shift).
    const size_t n_in_rounds = input_rounds.size();
    QueryGather qg(ctx);
    const unsigned li = qg.add_indices(indices);
    std::vector<QueryGather::Slot> o_rows(n_in_rounds), o_path(n_in_rounds);
    for (size_t k = 0; k < n_in_rounds; k++) {
        const unsigned lh = input_rounds[k]->log_height;
        o_rows[k] = qg.add_rows(li, input_rounds[k]->leaf_mats(), log_max_height - lh);
        o_path[k] = qg.add_path(li, input_rounds[k]->tree.p, lh, log_max_height - lh);
    }
    std::vector<QueryGather::Opening> o_round(R);
    for (uint32_t r = 0; r < R; r++)
        o_round[r] = qg.add_round(li, rounds[r].vec, rounds[r].tree, rounds[r].log_leaves, r + 1);
    std::vector<QueryGather::Slot> o_pass(pass_through ? in_ptr.size() : 0);
    for (size_t k = 0; k < o_pass.size(); k++)
        o_pass[k] = qg.add_values(li, in_ptr[k], log_max_height - log_lens[k] + 1);
    qg.run();

    // ---- FriProof (fri/src/proof.rs)
    std::vector<ProofWriter::Batch> batches;
    for (const PcsData* d : input_rounds) batches.push_back({&d->ldes, d->log_height});
    std::vector<unsigned> round_depths;
    for (auto& r : rounds) round_depths.push_back(r.log_leaves);
    pf.reserve(pf.size() + 16 + 8 * (size_t)R +
               (size_t)Q * ProofWriter::words_per_query(batches, round_depths, o_pass.size()));
    ProofWriter pw(pf);
    pw.begin_rounds(R);
    for (uint32_t r = 0; r < R; r++) pw.commitment(rounds[r].root, 8);
    pw.begin_queries(Q);
    for (uint32_t q = 0; q < Q; q++) {
        pw.begin_input_proof((uint32_t)(pass_through ? in_ptr.size() : n_in_rounds));
        for (size_t k = 0; k < o_pass.size(); k++) {
            const uint32_t half = (indices[q] >> (log_max_height - log_lens[k])) & 1;
            pw.pass_through_value(log_lens[k], qg.data(o_pass[k], q) + 4 * half);
        }
        for (size_t k = 0; k < n_in_rounds; k++) {
            const unsigned lh = input_rounds[k]->log_height;
            pw.batch_opening(input_rounds[k]->ldes, qg.data(o_rows[k], q), lh, {{qg.data(o_path[k], q), lh}});
        }
        for (uint32_t r = 0; r < R; r++)
            pw.round_opening(qg.data(o_round[r].vals, q), rounds[r].log_leaves,
                             {{qg.data(o_round[r].path, q), rounds[r].log_leaves}});
    }
    pw.finish(final_poly, pow_witness);
}

// ------------------------------------------------------------------ Pcs::open, any shape
// two_adic_pcs.rs:260-419.  Opened values come back in (round, matrix, point, column) order.
std::vector<uint32_t> TwoAdicFriPcs::open(const std::vector<OpenRound>& rounds, BfChallenger& challenger,
                                          std::vector<Ef>& opened_values) {
    TS_REQUIRE(!rounds.empty(), TS_ERR_INVALID, "open: no rounds");
    const Ef alpha = challenger.sample();  // :312
    uint32_t max_w = 1;
    unsigned log_global_max = 0;
    for (auto& r : rounds) {
        TS_REQUIRE(r.data && r.points.size() == r.data->ldes.size(), TS_ERR_INVALID,
                   "open: one point list per committed matrix");
        for (auto& m : r.data->ldes) max_w = std::max(max_w, m.width);
        log_global_max = std::max(log_global_max, r.data->log_height);  // :319-326
    }
    ctx_.ensure_twiddles(std::max(1u, log_global_max));
    AlphaLedger ledger(alpha, max_w);  // :332 num_reduced by log_height
    DevBuf<uint32_t> d_apow(&ctx_, ledger.powers().size());
    h2d(ctx_, d_apow.p, ledger.powers().data(), ledger.powers().size() * 4);

    opened_values.clear();
    DevBuf<Ef> ro[AlphaLedger::MAX_LOG_HEIGHT];  // :331 reduced_openings by log_height
    for (auto& r : rounds) {
        for (size_t mi = 0; mi < r.data->ldes.size(); mi++) {
            const ColMat& m = r.data->ldes[mi];
            const unsigned log_h = log2_strict(m.height);
            TS_REQUIRE(log_h >= fri_.log_blowup, TS_ERR_INVALID, "open: matrix shorter than the blowup");
            const unsigned log_n = log_h - fri_.log_blowup;
            const uint64_t n = 1ull << log_n;
            const uint32_t w = m.width;
            const auto& pts = r.points[mi];
            for (size_t p0 = 0; p0 < pts.size(); p0 += 2) {
                const uint32_t np = (uint32_t)std::min<size_t>(2, pts.size() - p0);
                Ef pts_mont[2] = {ef_to_mont(pts[p0]), ef_to_mont(pts[p0 + np - 1])};
                // :358-369 interpolate_coset on the low coset (first n bit-reversed rows)
                std::vector<Ef> raw((size_t)w * np);
                {
                    StageTimer t(&ctx_, "compute opened values with Lagrange interpolation");
                    DevBuf<Ef> weights(&ctx_, (size_t)np * n);
                    launch_bary_weights(ctx_, log_n, pts_mont, np, weights.p);
                    DevBuf<Ef> sums(&ctx_, raw.size());
                    launch_bary_dots(ctx_, m, log_n, weights.p, np, sums.p);  // [col][point]
                    d2h_sync(ctx_, raw.data(), sums.p, raw.size() * sizeof(Ef));
                }
                StageTimer t(&ctx_, "reduce rows");
                Ef scale[2];
                for (uint32_t p = 0; p < np; p++) scale[p] = bary_scale(pts[p0 + p], GENERATOR, n);  // low coset: s = 31
                const size_t first = opened_values.size();
                opened_values.resize(first + raw.size());
                opened_from_raw(raw.data(), w, np, scale, &opened_values[first]);
                ReduceArgs a;
                memset(&a, 0, sizeof a);
                a.n_points = np;
                for (uint32_t p = 0; p < np; p++) {
                    const AlphaLedger::Visit v = ledger.visit(log_h, &opened_values[first + (size_t)p * w], w, (int)p);
                    a.z_mont[p] = pts_mont[p];
                    a.off_mont[p] = v.off;  // :371
                    a.rys[p] = v.rys;       // :372
                }
                a.accumulate = ro[log_h].p ? 1 : 0;
                if (!ro[log_h].p) ro[log_h] = DevBuf<Ef>(&ctx_, m.height);
                launch_reduce(ctx_, m, log_h, d_apow.p, a, ro[log_h].p);  // :375-381
            }
        }
    }
    // :389-393 fri_input: the reduced openings by descending height
    std::vector<DevBuf<Ef>> inputs;
    std::vector<unsigned> log_lens;
    for (int lh = 31; lh >= 0; lh--)
        if (ro[lh].p) {
            inputs.push_back(std::move(ro[lh]));
            log_lens.push_back((unsigned)lh);
        }
    TS_REQUIRE(!inputs.empty(), TS_ERR_INVALID, "open: nothing to open");
    TS_REQUIRE(log_lens[0] == log_global_max, TS_ERR_UNSUPPORTED,
               "open: the tallest committed matrix must be opened at one point at least");
    std::vector<const PcsData*> datas;
    for (auto& r : rounds) datas.push_back(r.data);
    std::vector<uint32_t> pf;
    fri_prove(inputs, log_lens, challenger, datas, pf);
    return pf;
}

// ------------------------------------------------------------------ prove
// One body for the four proof formats.  uni-stark/src/prover.rs:25-119 is the case without
// side matrices; the key and the challenge phase are build-defined (the reference's prove stops at preprocessed
// width 0, prover.rs:46, and has one trace phase).
//   `preprocessed`: the committed key of the AIR's preprocessed columns, null exactly for an AIR without any.  The
//     key is part of the statement: its root is observed first and is not in the proof.
//   `aux_source`: null exactly for an AIR without aux columns.  After the trace's commit come n_challenges
//     samples, [the aux source], the aux root and every exposed word; then alpha and on as without them.
// The quotient reads the side matrices (key, then aux) beside the trace; the opening has one round for each
// before the trace's and the chunks', in that order.
// `proof_version` 1 and 3: the header ends with the preprocessed width (v3 only), and an AIR with a challenge
// phase is refused; 4 and 5: with the aux width, n_challenges, n_exposed and, v5 only, the preprocessed width, and v4
// refuses preprocessed columns.  (The C ABI's admission refuses both first; nothing is consumed before them.)
std::vector<uint32_t> prove(TwoAdicFriPcs& pcs, const AirProgram& air, BfChallenger& challenger, DeviceMatrix trace,
                            const std::vector<uint32_t>& public_values, const PcsData* preprocessed,
                            const AuxSource& aux_source, uint32_t proof_version) {
    TS_REQUIRE(proof_version >= 4 || (air.aux_width == 0 && air.n_challenges == 0 && air.n_exposed == 0), TS_ERR_INVALID,
               "prove: the AIR has a challenge phase (aux columns, challenges or exposed words); prove_aux proves it");
    TS_REQUIRE(proof_version != 4 || air.preprocessed_width == 0, TS_ERR_UNSUPPORTED,
               "prove_aux: preprocessed columns together with aux columns are proved by prove_pre_aux (TSPF v5)");
    const Statement st = check_statement(pcs.fri(), air, trace.width, trace.height, public_values.size());
    TS_REQUIRE((preprocessed != nullptr) == (air.preprocessed_width > 0), TS_ERR_INVALID,
               "prove: an AIR with preprocessed columns needs their committed key, and only such an AIR takes one");
    const uint32_t aw = air.aux_width;
    TS_REQUIRE((aux_source != nullptr) == (aw > 0), TS_ERR_INVALID,
               "prove_aux: an AIR with aux columns needs an aux source, and only such an AIR takes one");
    TS_REQUIRE(aw > 0 || air.n_exposed == 0, TS_ERR_INVALID, "prove_aux: exposed words without aux columns");
    TS_REQUIRE(!aw || trace.layout == DeviceMatrix::ROW_MAJOR, TS_ERR_INVALID,
               "prove_aux: the trace must be row-major (it is handed to the aux source after its commit)");
    SideData side;
    if (preprocessed) {
        check_side_matrix(*preprocessed, air, 0, 1ull << st.log_N);
        challenger.observe_commitment(preprocessed->root);
        side.push_back(preprocessed);
    }
    pcs.ctx().ensure_lde_twiddles(std::max(1u, st.log_N));
    const uint64_t n = trace.height;

    // :50-53 commit to trace data (natural domain: shift 1)
    std::vector<DeviceMatrix> tv;
    tv.push_back(std::move(trace));
    // the LDE stage transposes a row-major trace into a buffer of its own and never writes the input: kept, not copied
    std::unique_ptr<PcsData> trace_data = pcs.commit(tv, {1u}, true, /*keep_row_major=*/aw > 0);
    challenger.observe_commitment(trace_data->root);  // :60
    std::vector<uint32_t> pis = public_values;
    for (uint32_t k = 0; k < air.n_challenges; k++) {
        const Ef c = challenger.sample();
        pis.insert(pis.end(), c.c, c.c + 4);
    }
    std::unique_ptr<PcsData> aux_data;
    std::vector<uint32_t> exposed(air.n_exposed, 0);
    if (aw) {
        DeviceMatrix aux = aux_source(tv[0], pis.data() + public_values.size(), exposed.data());
        tv[0].buf.reset();  // the trace's rows are not read again
        TS_REQUIRE(aux.buf.p && aux.buf.ctx == &pcs.ctx(), TS_ERR_INVALID,
                   "prove_aux: the aux matrix is consumed or was made on another context");
        TS_REQUIRE(aux.height == n && aux.width == aw, TS_ERR_INVALID,
                   "prove_aux: the aux matrix must have the trace's height and the AIR's aux width");
        for (uint32_t e : exposed) TS_REQUIRE(e < P, TS_ERR_INVALID, "prove_aux: non-canonical exposed word");
        std::vector<DeviceMatrix> av;
        av.push_back(std::move(aux));
        aux_data = pcs.commit(av, {1u});
        challenger.observe_commitment(aux_data->root);
        for (uint32_t e : exposed) challenger.observe(e);
        side.push_back(aux_data.get());
    }
    pis.insert(pis.end(), exposed.begin(), exposed.end());
    const Ef alpha = challenger.sample();  // :63

    // :65-80 quotient on the disjoint domain, flattened and split into qd chunks
    std::vector<DeviceMatrix> chunks = pcs.quotient_chunks(*trace_data, air, pis, alpha, side);
    std::unique_ptr<PcsData> quotient_data =
        pcs.commit(chunks, chunk_domain_shifts(GENERATOR, st.log_degree, st.lqd));  // :80-83
    challenger.observe_commitment(quotient_data->root);                             // :84
    const Ef zeta = challenger.sample();                                            // :91

    // :94-104 open; two_adic_pcs.rs:312 batch-combination challenge first.  Same result as
    // pcs.open({trace: [zeta, zeta_next]}, {chunks: [zeta]}), through the one-pass reduce kernel.
    const Ef batch_alpha = challenger.sample();
    std::vector<Ef> opened;
    std::vector<DevBuf<Ef>> inputs;
    inputs.push_back(pcs.open_reduce(*trace_data, *quotient_data, zeta, batch_alpha, opened, side));

    // ---- Proof (prover.rs:105-118)
    const bool challenge_phase = proof_version >= 4;
    std::vector<uint32_t> pf;
    pf.reserve(64 + exposed.size() + opened.size() * 4);
    ProofWriter pw(pf);
    pw.header(proof_version, st.log_degree, st.w, st.qd, challenge_phase ? aw : air.preprocessed_width);
    const uint32_t more[3] = {air.n_challenges, air.n_exposed, air.preprocessed_width};
    if (challenge_phase) pw.words(more, proof_version == 5 ? 3 : 2);
    pw.commitment(trace_data->root, 8);
    if (aw) {
        pw.commitment(aux_data->root, 8);
        pw.words(exposed.data(), exposed.size());
    }
    pw.commitment(quotient_data->root, 8);
    pw.opened_values(opened);
    std::vector<const PcsData*> rounds = side;
    rounds.push_back(trace_data.get());
    rounds.push_back(quotient_data.get());
    pcs.fri_prove(inputs, {st.log_N}, challenger, rounds, pf);
    return pf;
}

// ------------------------------------------------------------------ a lookup proof inside a batch lane
// A TSPF v5 prove with its two lookup steps run by the library on the lane's stream instead of by the host: the
// multiplicity fills before the commit, the LogUp builder as the aux source.  Same launches in the same order as
// the solo calls, so the proof is theirs word for word.
std::string logup_miss_text(const LogupMultResult& r, uint32_t n_lookups) {
    return "logup multiplicities: the tuple of row " + std::to_string(r.first_missing / n_lookups) + ", lookup " +
           std::to_string(r.first_missing % n_lookups) + " is in no table row (" + std::to_string(r.n_missing) +
           " such lookups)";
}

AuxSource logup_aux_source(Context& ctx, LogupSpec spec, const DeviceMatrix* table) {
    return [&ctx, spec = std::move(spec), table](const DeviceMatrix& live, const uint32_t* challenges, uint32_t* exposed) {
        try {
            return logup_aux_build(ctx, spec, live, challenges, exposed, table, /*takes_table=*/true);
        } catch (const Error& e) {
            // the builder's one invariant: a zero denominator, read back after its kernels finished
            if (e.code == TS_ERR_INVARIANT) throw LookupDataError(e.code, e.what());
            throw;
        }
    };
}

std::vector<uint32_t> prove_lookup(TwoAdicFriPcs& pcs, const AirProgram& air, BfChallenger& challenger,
                                   DeviceMatrix trace, const std::vector<uint32_t>& public_values, const PcsData* key,
                                   const AuxSource& aux_source, const std::vector<LogupMultSpec>& fills,
                                   const DeviceMatrix* table, LogupMultResult* miss) {
    *miss = LogupMultResult{0, ~0ull};
    for (const LogupMultSpec& f : fills) {
        const LogupMultResult r = logup_multiplicities(pcs.ctx(), f, trace, table);
        if (r.n_missing) {
            *miss = r;
            throw LookupDataError(TS_ERR_INVARIANT, logup_miss_text(r, (uint32_t)f.weights.size()));
        }
    }
    return prove(pcs, air, challenger, std::move(trace), public_values, key, aux_source, 5);
}

}  // namespace ts

