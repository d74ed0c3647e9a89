// prove() over the reference's own MMCS: `TapTreeMmcs` (basic/src/mmcs/taptree_mmcs.rs:24-119) as the
// input MMCS of `TwoAdicFriPcs` and as the FRI MMCS, the configuration of uni-stark/tests/fib_air.rs:
// 117-131.  Same numeric pipeline as prover.cpp (LDE, quotient, opened values, reduce, fold); what
// changes is the commitment:
//   - a commitment is num_queries taptrees (tcs/mod.rs:284-292), built on the device from the LDE
//     columns and the caller's lock scripts (taptree.hip k_tapleaf_template);
//   - `challenger.observe(commit)` observes all num_queries roots (challenger/mod.rs:211-223);
//   - query q opens every commitment in tree q (fri/src/prover.rs:50-56, two_adic_pcs.rs:399-414:
//     open_batch(query_times_index = q, ...)).
// The transcript runs on the host here (one root download per commitment): hashing a level of
// kilobyte-sized script leaves dwarfs the round trip.  Proof: TSPF v2 = v1 with a sixth header word
// (num_queries) and num_queries x 8 words per commitment; a digest is 8 words = its 32 bytes read
// little-endian (chan_field.rs:87-95 u256_to_u32).
#include <string.h>

#include <algorithm>

#include "prover_internal.hpp"
#include "taptree.hpp"

namespace ts {

namespace {

// which of the Q trees of every commitment this rank builds: [q0, q0 + cnt), `per` = trees per rank
// (the last ranks may own fewer, or none when there are more ranks than queries)
struct TreeShare {
    uint32_t Q = 0, per = 0, q0 = 0, cnt = 0;
    const Comm* comm = nullptr;
    TreeShare(uint32_t num_queries, const Comm* c) : Q(num_queries), comm(c) {
        const uint32_t G = c ? (uint32_t)c->world : 1u, g = c ? (uint32_t)c->rank : 0u;
        per = (Q + G - 1) / G;
        q0 = std::min(Q, g * per);
        cnt = std::min(Q, q0 + per) - q0;
    }
    bool owns(uint32_t q) const { return q >= q0 && q < q0 + cnt; }
};

struct TapCommit {
    DevBuf<uint32_t> trees;        // [cnt][2N-1][8] state words: the trees this rank owns
    std::vector<uint32_t> roots;   // Q x 8 words (bytes read little-endian), every tree's
    unsigned log_height = 0;
};

void observe_roots(BfChallenger& ch, const std::vector<uint32_t>& roots) {
    for (size_t q = 0; q < roots.size() / 8; q++) ch.observe_commitment(&roots[8 * q]);
}

// the rank's trees over the padded row described by cols / shifts / elem_stride, then the roots of
// all Q trees (exchange: per x 32 bytes from every rank, rank order = tree order)
TapCommit commit_trees(Context& ctx, const TreeShare& sh, const std::vector<const uint32_t*>& cols,
                       const std::vector<uint8_t>& shifts, uint32_t elem_stride, unsigned log_height,
                       uint32_t u32_size, const TapLocks& locks, size_t& cursor) {
    const size_t n_seg = 1 + cols.size() / u32_size;
    TapCommit tc;
    tc.log_height = log_height;
    std::vector<uint32_t> mine;
    if (sh.cnt)
        tc.trees = tap_build_trees(ctx, cols, shifts, elem_stride, log_height, u32_size, sh.cnt, locks,
                                   cursor + (size_t)sh.q0 * n_seg, mine);
    cursor += (size_t)sh.Q * n_seg;
    if (!sh.comm) {
        tc.roots = std::move(mine);
        return tc;
    }
    const size_t seg = (size_t)sh.per * 8, G = (size_t)sh.comm->world;
    mine.resize(seg, 0);
    DevBuf<uint32_t> d_send(&ctx, seg), d_recv(&ctx, seg * G);
    h2d(ctx, d_send.p, mine.data(), seg * 4);
    sh.comm->all_gather(d_send.p, d_recv.p, seg * 4, ctx.stream);
    std::vector<uint32_t> all(seg * G);
    d2h_sync(ctx, all.data(), d_recv.p, all.size() * 4);
    tc.roots.assign(all.begin(), all.begin() + (size_t)sh.Q * 8);  // tree q sits at q: ranges are contiguous
    return tc;
}

TapCommit commit_columns(Context& ctx, const TreeShare& sh, const PcsData& data, const TapLocks& locks,
                         size_t& cursor) {
    for (auto& cm : data.ldes)
        TS_REQUIRE(cm.height == (1ull << data.log_height), TS_ERR_UNSUPPORTED,
                   "prove over taptrees: matrices of one height per commitment");
    const std::vector<const uint32_t*> cols = column_pointers(data.ldes);
    const std::vector<uint8_t> shifts(cols.size(), 0);
    return commit_trees(ctx, sh, cols, shifts, 1, data.log_height, 1, locks, cursor);
}

}  // namespace

// comm == nullptr: one GPU.  Otherwise every rank holds the WHOLE trace and repeats the numeric
// pipeline (milliseconds), while the commitments -- the seconds: kilobytes of SHA-256 per leaf, times
// num_queries trees -- are split by TREE: rank g builds trees [g per, (g+1) per) of every commitment,
// the roots are all-gathered (32 bytes per tree) so that every transcript observes all of them, and
// query q is answered by the rank that owns tree q.  Trees are independent, so nothing else moves.
std::vector<uint32_t> prove_tap(TwoAdicFriPcs& pcs, const AirProgram& air, BfChallenger& challenger,
                                DeviceMatrix trace, const std::vector<uint32_t>& public_values,
                                const TapLocks& locks, const Comm* comm) {
    Context& ctx = pcs.ctx();
    const FriConfig& fri = pcs.fri();
    const Statement st = check_statement(fri, air, trace.width, trace.height, public_values.size());
    TS_REQUIRE(locks.bytes && locks.offsets, TS_ERR_INVALID, "prove over taptrees: no lock-script table");
    TS_REQUIRE(!comm || (comm->world >= 1 && comm->rank >= 0 && comm->rank < comm->world), TS_ERR_INVALID,
               "prove over taptrees: bad communicator");
    const uint32_t w = st.w, qd = st.qd, Q = fri.num_queries;
    const unsigned log_n = st.log_degree, log_N = st.log_N;
    const uint64_t N = 1ull << log_N;
    const uint32_t R = log_N - fri.log_blowup;
    TS_REQUIRE(locks.n_scripts >= (size_t)Q * ((1 + w) + (1 + 4 * (size_t)qd) + 3 * (size_t)R), TS_ERR_INVALID,
               "prove over taptrees: the lock-script table is shorter than Q ((1+w) + (1+4 qd) + 3 log2(n))");
    const TreeShare sh(Q, comm && comm->world > 1 ? comm : nullptr);
    size_t cursor = 0;

    // ---- prover.rs:50-63 commit to the trace, alpha
    std::vector<DeviceMatrix> tv;
    tv.push_back(std::move(trace));
    std::unique_ptr<PcsData> trace_data = pcs.commit(tv, {1u}, /*build_tree=*/false);
    TapCommit trace_commit = commit_columns(ctx, sh, *trace_data, locks, cursor);
    observe_roots(challenger, trace_commit.roots);
    const Ef alpha = challenger.sample();

    // ---- :65-84 quotient chunks, their commitment, zeta
    std::vector<DeviceMatrix> chunks = pcs.quotient_chunks(*trace_data, air, public_values, alpha);
    std::unique_ptr<PcsData> quotient_data = pcs.commit(chunks, chunk_domain_shifts(GENERATOR, log_n, st.lqd), false);
    TapCommit quotient_commit = commit_columns(ctx, sh, *quotient_data, locks, cursor);
    observe_roots(challenger, quotient_commit.roots);
    const Ef zeta = challenger.sample();

    // ---- :94-104 open: opened values + reduced openings (needs the LDEs only)
    const Ef batch_alpha = challenger.sample();
    std::vector<Ef> opened;
    DevBuf<Ef> folded = pcs.open_reduce(*trace_data, *quotient_data, zeta, batch_alpha, opened);

    // ---- bf_commit_phase, fri/src/prover.rs:93-141 (host transcript)
    struct Round {
        DevBuf<Ef> vec;
        TapCommit commit;
    };
    std::vector<Round> rounds;
    uint64_t len = N;
    DevBuf<Ef> d_beta(&ctx, 1);
    while (len > fri.blowup()) {
        const uint64_t h = len / 2;
        Round r;
        // RowMajorMatrix::new(folded, 2): row i = (f[2i], f[2i+1]) = 8 consecutive words
        std::vector<const uint32_t*> cols(8);
        for (int c = 0; c < 8; c++) cols[c] = reinterpret_cast<const uint32_t*>(folded.p) + c;
        r.commit = commit_trees(ctx, sh, cols, std::vector<uint8_t>(8, 0), 8, log2_strict(h), 4, locks, cursor);
        observe_roots(challenger, r.commit.roots);  // :114
        const Ef beta = challenger.sample();        // :116
        DevBuf<Ef> out(&ctx, h);
        h2d(ctx, d_beta.p, &beta, sizeof(Ef));
        launch_fri_fold_dev(ctx, folded.p, h, d_beta.p, out.p, nullptr);  // :119
        r.vec = std::move(folded);
        rounds.push_back(std::move(r));
        folded = std::move(out);
        len = h;
    }
    std::vector<Ef> finals(fri.blowup());
    d2h_sync(ctx, finals.data(), folded.p, finals.size() * sizeof(Ef));
    for (auto& e : finals)  // :130-134
        TS_REQUIRE(memcmp(e.c, finals[0].c, 16) == 0, TS_ERR_INVARIANT, "FRI: final polynomial is not constant");
    const Ef final_poly = finals[0];
    const uint32_t pow_witness = challenger.grind(fri.proof_of_work_bits);  // :43

    // ---- query phase :45-59: query q opens every commitment in tree q, i.e. on the rank that owns it
    std::vector<uint32_t> indices(Q);
    for (uint32_t q = 0; q < Q; q++) indices[q] = (uint32_t)challenger.sample_bits(log_N);
    PcsData* in_data[2] = {trace_data.get(), quotient_data.get()};
    const TapCommit* in_commit[2] = {&trace_commit, &quotient_commit};
    std::vector<unsigned> round_depths(R);
    for (uint32_t r = 0; r < R; r++) round_depths[r] = rounds[r].commit.log_height;
    const size_t wpq =
        ProofWriter::words_per_query({{&trace_data->ldes, log_N}, {&quotient_data->ldes, log_N}}, round_depths);
    const uint32_t nq = sh.cnt;  // queries answered here: q0 .. q0 + nq - 1, in local trees 0 .. nq - 1
    std::vector<uint32_t> answers((size_t)(sh.comm ? sh.per : Q) * wpq, 0);
    if (nq) {
        // rows and round values through the shared gather: one upload, one launch, and the one sync of this phase
        const std::vector<uint32_t> idx(indices.begin() + sh.q0, indices.begin() + sh.q0 + nq);
        QueryGather qg(ctx);
        const unsigned li = qg.add_indices(idx);
        QueryGather::Slot o_rows[2];
        // (the row gather reads the columns through the table, which this flow has not built so far)
        for (int k = 0; k < 2; k++) o_rows[k] = qg.add_rows(li, in_data[k]->leaf_mats_with_table(ctx), 0);
        std::vector<QueryGather::Slot> o_vals(R);
        for (uint32_t r = 0; r < R; r++) o_vals[r] = qg.add_values(li, rounds[r].vec.p, r + 1);
        // The paths stay with launch_tap_gather_paths (its trees are addressed per query): the two input batches,
        // then the rounds, launch after launch into one buffer.  Leaf indices from ONE uploaded table: row t =
        // index >> t (row 0 for the batches; row r + 1 for round r, bf_answer_query :69-90: it opens row
        // index >> r >> 1 of its h x 2 matrix, in tree q), then the local tree numbers.
        const size_t n_tab = (size_t)(R + 1) * nq;
        std::vector<uint64_t> tab(n_tab + (nq + 1) / 2);
        uint32_t* tree_of = reinterpret_cast<uint32_t*>(&tab[n_tab]);
        for (uint32_t j = 0; j < nq; j++) {
            for (uint32_t t = 0; t <= R; t++) tab[(size_t)t * nq + j] = idx[j] >> t;
            tree_of[j] = j;
        }
        DevBuf<uint64_t> d_tab(&ctx, tab.size());
        h2d(ctx, d_tab.p, tab.data(), tab.size() * 8);
        std::vector<size_t> o_tpath(2 + R + 1, 0);  // [i]: where opening i's [query][depth][8] starts; last: the total
        auto depth = [&](uint32_t i) { return i < 2 ? log_N : rounds[i - 2].commit.log_height; };
        for (uint32_t i = 0; i < 2 + R; i++) o_tpath[i + 1] = o_tpath[i] + (size_t)nq * 8 * depth(i);
        DevBuf<uint32_t> d_paths(&ctx, o_tpath.back());
        for (uint32_t i = 0; i < 2 + R; i++)
            launch_tap_gather_paths(ctx, i < 2 ? in_commit[i]->trees.p : rounds[i - 2].commit.trees.p,
                                    (2ull << depth(i)) - 1, depth(i), reinterpret_cast<const uint32_t*>(d_tab.p + n_tab),
                                    d_tab.p + (size_t)(i < 2 ? 0 : i - 1) * nq, nq, d_paths.p + o_tpath[i]);
        std::vector<uint32_t> paths(o_tpath.back());
        TS_HIP(hipMemcpyAsync(paths.data(), d_paths.p, paths.size() * 4, hipMemcpyDeviceToHost, ctx.stream));
        qg.run();
        std::vector<uint32_t> one;
        ProofWriter pw(one, /*swap_path_bytes=*/true);  // state words -> bytes read little-endian
        for (uint32_t j = 0; j < nq; j++) {
            one.clear();
            pw.begin_input_proof(2);
            for (int k = 0; k < 2; k++)
                pw.batch_opening(in_data[k]->ldes, qg.data(o_rows[k], j), log_N,
                                 {{&paths[o_tpath[k] + (size_t)j * 8 * log_N], log_N}});
            for (uint32_t r = 0; r < R; r++) {
                const unsigned ll = rounds[r].commit.log_height;
                pw.round_opening(qg.data(o_vals[r], j), ll, {{paths.data() + o_tpath[2 + r] + (size_t)j * 8 * ll, ll}});
            }
            TS_REQUIRE(one.size() == wpq, TS_ERR_INVARIANT, "taptree query: segment size");
            memcpy(&answers[(size_t)j * wpq], one.data(), wpq * 4);
        }
    }
    if (sh.comm) {  // collect the answers: per x wpq words from every rank, rank order = query order
        const size_t seg = (size_t)sh.per * wpq, G = (size_t)sh.comm->world;
        DevBuf<uint32_t> d_send(&ctx, seg), d_recv(&ctx, seg * G);
        h2d(ctx, d_send.p, answers.data(), seg * 4);
        sh.comm->all_gather(d_send.p, d_recv.p, seg * 4, ctx.stream);
        answers.resize(seg * G);
        d2h_sync(ctx, answers.data(), d_recv.p, answers.size() * 4);
    }

    // ---- Proof (uni-stark/src/prover.rs:105-118), TSPF v2
    std::vector<uint32_t> pf;
    ProofWriter pw(pf);
    pw.header(2, log_n, w, qd, Q);
    pw.commitment(trace_commit.roots.data(), trace_commit.roots.size());
    pw.commitment(quotient_commit.roots.data(), quotient_commit.roots.size());
    pw.opened_values(opened);
    pw.begin_rounds(R);
    for (uint32_t r = 0; r < R; r++) pw.commitment(rounds[r].commit.roots.data(), rounds[r].commit.roots.size());
    pw.begin_queries(Q);
    pw.words(answers.data(), (size_t)Q * wpq);  // query q sits at q: the ranks' ranges are contiguous
    pw.finish(final_poly, pow_witness);
    return pf;
}

}  // namespace ts
