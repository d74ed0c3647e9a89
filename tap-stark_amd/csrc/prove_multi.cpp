// prove_multi: T plain AIR tables of mixed heights in one proof.  Build-defined (the reference's prove takes one
// trace, uni-stark/src/prover.rs:25-119); every stage is the single-table prover's, batched:
//   1. observe T, then log_degree_t for every table (base words): the heights are part of the statement
//   2. ONE commit of all traces on their natural domains, table order (two_adic_pcs.rs:227-245 takes mixed
//      heights); observe the root; sample alpha
//   3. per table the quotient chunks over that table's LDE inside the batch, constraints folded from alpha^0
//   4. ONE commit of all chunks, table-major, chunk-minor, chunk c of table t on chunk_domain_shifts(31,
//      log_degree_t, lqd_t)[c]; observe the root; sample zeta
//   5. Pcs::open over two rounds: trace t at {zeta, zeta omega_{n_t}}, every chunk at {zeta}
// Proof = TSPF v6.  Step 5 runs one pass per height class (open_multi.hip) or, with
// TS_MULTI_OPEN_GENERIC=1, TwoAdicFriPcs::open; the words are the same.
//
// prove_multi_bus: the same with a challenge phase ACROSS the tables, a LogUp bus (TSPF v7).  After the trace root
// gamma and beta are sampled ONCE for every table; every table with aux columns gets its LogUp matrix
// (logup_aux_build_multi: all tables in three launches), ONE commit holds them in table order; its root and the
// exposed sums (four words per aux table) are observed before alpha.  A table's quotient reads (aux LDE, trace LDE)
// and the public vector pis ++ gamma ++ beta ++ its exposed words.  The opening has three rounds, in the order of
// TSPF v4: aux matrices and traces at {zeta, zeta omega_{n_t}}, chunks at {zeta}.
//
// prove_multi_key: prove_multi_bus against a commit-once key of preprocessed matrices (MultiKey, logup.hpp; TSPF v8).
// The key's root is observed after the shapes and is not in the proof; the i-th
// table with preprocessed columns reads key matrix i: its LDE is the first side matrix of that table's quotient
// and the key is the first opened round, in the order of TSPF v5.  A LogUp spec may read the key's kept values
// (kind-2 terms).  Without any table with aux columns the challenge phase is skipped whole: three rounds.
//
// The three are one body (prove_multi_versioned) behind one statement walk (check_multi_statement): the rounds a
// statement has -- a key or none, aux tables or none -- select the paths, and the header's version is all that tells a
// v6 proof from a v7 body without aux tables, which the statement walk refuses.
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "logup.hpp"
#include "prover_internal.hpp"

namespace ts {

bool multi_open_generic() {
    const char* e = getenv("TS_MULTI_OPEN_GENERIC");
    return e && *e && atoi(e) != 0;
}

namespace {

// one committed matrix of the two rounds, in the visiting order of TwoAdicFriPcs::open: round, matrix
struct OpenMat {
    const ColMat* m;
    unsigned round;  // of `rounds` in open_rounds
    unsigned log_n;
    bool has_next; // opened at zeta omega_n as well: a trace or an aux matrix (a ClassJob with has_next)
    size_t first;  // of its opened values (and of its raw sums) in (round, matrix, point, column) order
};

// Step 5 on the per-class kernels: the opened values of every matrix with ONE host wait, then one
// k_reduce_class launch per LDE height.  `batch_alpha` is already sampled.
void open_classes(TwoAdicFriPcs& pcs, const std::vector<OpenMat>& mats, Ef zeta, Ef batch_alpha,
                  std::vector<Ef>& opened, std::vector<DevBuf<Ef>>& inputs, std::vector<unsigned>& log_lens) {
    Context& ctx = pcs.ctx();
    const unsigned log_blowup = pcs.fri().log_blowup;
    size_t n_opened = 0;
    uint32_t max_w = 4;
    for (const OpenMat& om : mats) {
        n_opened = om.first + (size_t)om.m->width * (om.has_next ? 2 : 1);
        max_w = std::max(max_w, om.m->width);
    }

    // ---- opened values: barycentric interpolation on each matrix's low coset (two_adic_pcs.rs:358-369)
    struct Points { Ef z[2]; Ef scale[2]; DevBuf<Ef> weights; };
    std::map<unsigned, Points> by_log_n;  // one weight table per trace height, two points each
    std::vector<Ef> raw(n_opened);
    {
        StageTimer t(&ctx, "compute opened values with Lagrange interpolation");
        for (const OpenMat& om : mats) {
            if (by_log_n.count(om.log_n)) continue;
            Points& pt = by_log_n[om.log_n];
            const uint64_t n = 1ull << om.log_n;
            pt.z[0] = zeta;
            pt.z[1] = efc_mul_base(zeta, two_adic_generator(om.log_n));  // prover.rs:92 next_point
            for (int p = 0; p < 2; p++) pt.scale[p] = bary_scale(pt.z[p], GENERATOR, n);
            const Ef pts_mont[2] = {ef_to_mont(pt.z[0]), ef_to_mont(pt.z[1])};
            pt.weights = DevBuf<Ef>(&ctx, 2 * n);
            launch_bary_weights(ctx, om.log_n, pts_mont, 2, pt.weights.p);
        }
        // every finishing job writes its sums straight into the context's mailbox (host memory)
        Ef* const mail = reinterpret_cast<Ef*>(ctx.mailbox(4 * n_opened));
        std::vector<DevBuf<uint32_t>> partials;
        std::vector<BaryFinishJob> jobs;
        std::vector<uint2> groups;
        for (const OpenMat& om : mats) {
            BaryPending pend;  // the dot kernel's partial sums are taken over, its own finishing pass is not run
            launch_bary_dots(ctx, *om.m, om.log_n, by_log_n[om.log_n].weights.p, om.has_next ? 2 : 1, mail + om.first,
                             &pend);
            jobs.push_back(BaryFinishJob{pend.partial[0].p, pend.out[0], pend.n_blocks[0], pend.n_words[0]});
            for (uint32_t g = 0; g < (pend.n_words[0] + 3) / 4; g++)
                groups.push_back(make_uint2((uint32_t)jobs.size() - 1, g));
            partials.push_back(std::move(pend.partial[0]));
            pend.n = 0;
        }
        // both tables in one upload
        static_assert(sizeof(BaryFinishJob) % sizeof(uint2) == 0, "the group table follows the jobs, aligned");
        std::vector<char> tab(jobs.size() * sizeof(BaryFinishJob) + groups.size() * sizeof(uint2));
        memcpy(tab.data(), jobs.data(), jobs.size() * sizeof(BaryFinishJob));
        memcpy(tab.data() + jobs.size() * sizeof(BaryFinishJob), groups.data(), groups.size() * sizeof(uint2));
        DevBuf<uint64_t> d_tab(&ctx, tab.size() / 8);
        h2d(ctx, d_tab.p, tab.data(), tab.size());
        launch_bary_finish_jobs(ctx, reinterpret_cast<const BaryFinishJob*>(d_tab.p),
                                reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(d_tab.p) +
                                                               jobs.size() * sizeof(BaryFinishJob)),
                                (uint32_t)groups.size());
        ctx.sync_point(mail, n_opened * sizeof(Ef));
        memcpy((void*)raw.data(), mail, n_opened * sizeof(Ef));
    }
    // p(z) = ((z/31)^n - 1)/n * sum_i p_i x_i/(z - x_i); the dot kernel left [col][point]
    opened.assign(n_opened, ef_zero());
    for (const OpenMat& om : mats)
        opened_from_raw(raw.data() + om.first, om.m->width, om.has_next ? 2 : 1, by_log_n[om.log_n].scale,
                        opened.data() + om.first);

    // ---- reduce (two_adic_pcs.rs:371-383), one launch per height class
    StageTimer t(&ctx, "reduce rows");
    AlphaLedger ledger(batch_alpha, max_w);
    std::vector<uint32_t> words = ledger.powers();  // and behind them alpha^k off_0 per chunk column: one upload
    struct Class {
        std::vector<ClassJob> jobs;
        std::vector<size_t> weights_at;  // per job: word offset of its folded weights in `words`
        ClassReduceArgs args;
    };
    std::map<unsigned, Class> classes;  // by LDE log-height
    for (const OpenMat& om : mats) {
        const unsigned log_h = om.log_n + log_blowup;
        const bool fresh = !classes.count(log_h);
        Class& cl = classes[log_h];
        if (fresh) {
            const Points& pt = by_log_n[om.log_n];
            cl.args.z_mont[0] = ef_to_mont(pt.z[0]);
            cl.args.z_mont[1] = ef_to_mont(pt.z[1]);
        }
        const uint32_t w = om.m->width;
        ClassJob j;
        memset(&j, 0, sizeof j);
        j.d = om.m->d;
        j.col_stride = om.m->col_stride;
        j.width = w;
        j.has_next = om.has_next ? 1 : 0;
        j.off[0] = ledger.visit(log_h, &opened[om.first], w, 0).off;
        if (om.has_next) j.off[1] = ledger.visit(log_h, &opened[om.first + w], w, 1).off;
        cl.weights_at.push_back(words.size());
        if (!om.has_next) ledger.fold_weights(j.off[0], w, words);
        cl.jobs.push_back(j);
    }
    DevBuf<uint32_t> d_apow(&ctx, words.size());
    h2d(ctx, d_apow.p, words.data(), words.size() * 4);
    std::vector<ClassJob> all_jobs;
    for (auto& [log_h, cl] : classes) {
        cl.args.k0 = ledger.k(log_h, 0);
        cl.args.k1 = ledger.k(log_h, 1);
        for (size_t k = 0; k < cl.jobs.size(); k++) {
            if (!cl.jobs[k].has_next) cl.jobs[k].weights = d_apow.p + cl.weights_at[k];
            all_jobs.push_back(cl.jobs[k]);
        }
    }
    DevBuf<ClassJob> d_jobs(&ctx, all_jobs.size());
    h2d(ctx, d_jobs.p, all_jobs.data(), all_jobs.size() * sizeof(ClassJob));
    // :389-393 fri_input: the reduced openings by descending height
    std::vector<size_t> first_job;
    size_t at = 0;
    for (auto& [log_h, cl] : classes) {
        first_job.push_back(at);
        at += cl.jobs.size();
    }
    size_t ci = classes.size();
    for (auto it = classes.rbegin(); it != classes.rend(); ++it) {
        ci--;
        const unsigned log_h = it->first;
        DevBuf<Ef> ro(&ctx, 1ull << log_h);
        launch_reduce_class(ctx, d_jobs.p + first_job[ci], (uint32_t)it->second.jobs.size(), log_h, d_apow.p,
                            it->second.args, ro.p);
        inputs.push_back(std::move(ro));
        log_lens.push_back(log_h);
    }
}

// Step 5 of both provers: `mats` in the visiting order of Pcs::open over `rounds`; samples the batch challenge,
// fills `opened` in (round, matrix, point, column) order and returns the FriProof words.  The per-class kernels,
// or TwoAdicFriPcs::open with TS_MULTI_OPEN_GENERIC=1: the same words.
std::vector<uint32_t> open_rounds(TwoAdicFriPcs& pcs, BfChallenger& challenger, const std::vector<const PcsData*>& rounds,
                                  const std::vector<OpenMat>& mats, Ef zeta, std::vector<Ef>& opened) {
    std::vector<uint32_t> fri_words;
    if (multi_open_generic()) {
        std::vector<TwoAdicFriPcs::OpenRound> rs(rounds.size());
        for (size_t r = 0; r < rounds.size(); r++) rs[r].data = rounds[r];
        for (const OpenMat& om : mats) {
            std::vector<Ef> pts{zeta};
            if (om.has_next) pts.push_back(efc_mul_base(zeta, two_adic_generator(om.log_n)));
            rs[om.round].points.push_back(std::move(pts));
        }
        fri_words = pcs.open(rs, challenger, opened);
    } else {
        const Ef batch_alpha = challenger.sample();  // two_adic_pcs.rs:312
        std::vector<DevBuf<Ef>> inputs;
        std::vector<unsigned> log_lens;
        open_classes(pcs, mats, zeta, batch_alpha, opened, inputs, log_lens);
        pcs.fri_prove(inputs, log_lens, challenger, rounds, fri_words);
    }
    return fri_words;
}

}  // namespace

bool multi_logup_per_table() {
    const char* e = getenv("TS_MULTI_LOGUP_PER_TABLE");
    return e && *e && atoi(e) != 0;
}

MultiCall multi_call(uint32_t version, const FriConfig* fri) {
    switch (version) {
        case 6: return {"prove_multi", MultiRound::NEVER, MultiRound::NEVER, fri};
        case 7: return {"prove_multi_bus", MultiRound::NEVER, MultiRound::ALWAYS, fri};
        case 8: return {"prove_multi_key", MultiRound::ALWAYS, MultiRound::AS_TABLES_HAVE, fri};
        default: return {"check_multi", MultiRound::AS_TABLES_HAVE, MultiRound::AS_TABLES_HAVE, nullptr};
    }
}

void check_multi_statement(const MultiCall& call, const std::vector<MultiBusTable>& tables, const MultiKey* key) {
    const std::string name = call.name;
    TS_REQUIRE(!tables.empty() && tables.size() <= MAX_MULTI_TABLES, TS_ERR_INVALID, name + ": between 1 and 64 tables");
    uint32_t n_chunks = 0;
    size_t n_pre = 0, n_aux = 0;
    for (const MultiBusTable& t : tables) {
        TS_REQUIRE(t.air, TS_ERR_INVALID, name + ": null AIR");
        n_pre += t.air->preprocessed_width ? 1 : 0;
        n_aux += t.air->aux_width ? 1 : 0;
    }
    // the key round (a call without one is handed no key and refuses preprocessed columns table by table)
    if (call.key == MultiRound::ALWAYS)
        TS_REQUIRE(key && key->data && n_pre > 0, TS_ERR_INVALID,
                   name + ": a null key, or no table has preprocessed columns; tables without a key are proved by "
                          "ts_prove_multi_bus (TSPF v7) or ts_prove_multi (TSPF v6)");
    if (call.key == MultiRound::AS_TABLES_HAVE)
        TS_REQUIRE((key != nullptr) == (n_pre > 0), TS_ERR_INVALID,
                   name + (n_pre ? ": a null key and a table with preprocessed columns"
                                 : ": a key was given and no table has preprocessed columns"));
    if (key) {
        TS_REQUIRE(key->data && key->heights.size() == n_pre, TS_ERR_INVALID,
                   name + ": the key holds " + std::to_string(key->heights.size()) + " matrices and " +
                       std::to_string(n_pre) + " tables have preprocessed columns");
        TS_REQUIRE(!call.fri || key->log_blowup == call.fri->log_blowup, TS_ERR_INVALID,
                   name + ": the key was committed with another log_blowup");
    }
    size_t ki = 0;
    for (size_t k = 0; k < tables.size(); k++) {
        const MultiBusTable& t = tables[k];
        const std::string w = name + ": table " + std::to_string(k);
        const uint32_t pw = t.air->preprocessed_width, aw = t.air->aux_width;
        if (call.aux == MultiRound::NEVER)
            TS_REQUIRE(pw == 0 && aw == 0, TS_ERR_UNSUPPORTED,
                       name + ": a table's AIR has preprocessed or challenge-phase (aux) columns; only plain AIRs "
                              "share a multi-table proof");
        else if (call.key == MultiRound::NEVER)
            TS_REQUIRE(pw == 0, TS_ERR_UNSUPPORTED,
                       w + ": the AIR has preprocessed columns; a multi-table proof has no key round");
        if (!call.fri) {  // (with a FriConfig check_statement below says the same)
            TS_REQUIRE(t.trace.width == t.air->width, TS_ERR_INVALID, w + ": the trace has not the AIR's width");
            TS_REQUIRE(t.public_values.size() == t.air->n_public, TS_ERR_INVALID, w + ": wrong number of public values");
        }
        if (pw) {
            TS_REQUIRE(key->heights[ki] == t.trace.height && key->widths[ki] == pw, TS_ERR_INVALID,
                       w + ": key matrix " + std::to_string(ki) + " has not the table's height and the AIR's preprocessed width");
            // (the constraint check reads the rows of every key matrix, the builder those a spec names)
            TS_REQUIRE(call.fri || key->values[ki], TS_ERR_INVALID, w + ": the key was made without keep_values");
        }
        // the table's challenge phase; its kind-2 terms read a key matrix and are refused without one
        bool reads_key = false;
        if (aw) {
            TS_REQUIRE(t.air->n_challenges == 2 && t.air->n_exposed == 4, TS_ERR_INVALID,
                       w + ": an AIR on the bus has 2 challenges (gamma, beta) and 4 exposed words (its sum)");
            TS_REQUIRE(t.logup, TS_ERR_INVALID, w + ": the AIR has aux columns and no logup spec");
            TS_REQUIRE(logup_aux_width(*t.logup, pw ? 2 : 1) == aw, TS_ERR_INVALID,
                       w + ": the logup spec's aux width is not the AIR's");
            for (const LogupInteraction& it : t.logup->interactions) {
                std::vector<LogupTerm> terms = it.values;
                terms.push_back(it.multiplicity);
                for (const LogupTerm& tm : terms) {
                    TS_REQUIRE(tm.kind == 2 ? tm.value < pw : tm.kind ? tm.value < t.trace.width : tm.value < P,
                               TS_ERR_INVALID,
                               w + (pw ? ": the logup spec reads a column outside the trace or the key matrix, or has a "
                                         "non-canonical constant"
                                       : ": the logup spec reads a column outside the trace, or has a non-canonical constant"));
                    reads_key = reads_key || tm.kind == 2;
                }
            }
            TS_REQUIRE(t.trace.layout == DeviceMatrix::ROW_MAJOR, TS_ERR_INVALID,
                       w + ": the trace of a table with aux columns must be row-major (the LogUp builder reads its rows)");
        } else if (call.aux != MultiRound::NEVER) {
            TS_REQUIRE(t.air->n_challenges == 0 && t.air->n_exposed == 0, TS_ERR_INVALID,
                       w + ": challenges or exposed words without aux columns");
            TS_REQUIRE(!t.logup, TS_ERR_INVALID, w + ": a logup spec for an AIR without aux columns");
        }
        TS_REQUIRE(!reads_key || (pw && key->values[ki]), TS_ERR_INVALID,
                   w + ": the logup spec reads preprocessed columns and the key was made without keep_values");
        ki += pw ? 1 : 0;
        if (call.fri)
            n_chunks += check_statement(*call.fri, *t.air, t.trace.width, t.trace.height, t.public_values.size()).qd;
        else
            TS_REQUIRE(t.trace.layout == DeviceMatrix::ROW_MAJOR, TS_ERR_INVALID, w + ": the trace must be row-major");
    }
    TS_REQUIRE(n_chunks <= (uint32_t)MAX_BATCH_MATS, TS_ERR_INVALID,
               name + ": more than 64 quotient chunks over all tables (the limit of one committed batch)");
    TS_REQUIRE(call.aux != MultiRound::ALWAYS || n_aux > 0, TS_ERR_INVALID,
               name + ": no table has aux columns; plain tables are proved by ts_prove_multi (TSPF v6)");
}

// One body for TSPF v6 (no key, no table with aux columns), v7 (no key, at least one aux table) and v8 (a key; the
// challenge phase only if some table has aux columns): the rounds the statement has select the paths, `version` is
// the header's.
static std::vector<uint32_t> prove_multi_versioned(TwoAdicFriPcs& pcs, BfChallenger& challenger,
                                                   std::vector<MultiBusTable>& tables, const MultiKey* key,
                                                   uint32_t version) {
    const MultiCall call = multi_call(version, &pcs.fri());
    check_multi_statement(call, tables, key);
    const std::string name = call.name;  // of the running call, in front of the invariant texts
    Context& ctx = pcs.ctx();
    const size_t T = tables.size();
    std::vector<Statement> st;
    unsigned log_max = 0;
    for (const MultiBusTable& t : tables) {
        st.push_back(check_statement(pcs.fri(), *t.air, t.trace.width, t.trace.height, t.public_values.size()));
        log_max = std::max(log_max, st.back().log_N);
    }
    ctx.ensure_lde_twiddles(std::max(1u, log_max));

    // the statement's shape: a prover must not choose the heights after the fact
    challenger.observe((uint32_t)T);
    for (const Statement& s : st) challenger.observe(s.log_degree);
    // the key is part of the statement: its root is observed and is not in the proof, as prove_pre does
    std::vector<size_t> key_of(T, ~(size_t)0);
    if (key) {
        size_t ki = 0;
        for (size_t t = 0; t < T; t++)
            if (tables[t].air->preprocessed_width) key_of[t] = ki++;
        challenger.observe_commitment(key->data->root);
    }
    std::vector<size_t> aux_of(T, ~(size_t)0), aux_tables;
    for (size_t t = 0; t < T; t++)
        if (tables[t].air->aux_width) {
            aux_of[t] = aux_tables.size();
            aux_tables.push_back(t);
        }
    const size_t A = aux_tables.size();  // 0: no samples, no aux commitment

    // one commit of every trace on its natural domain (shift 1); with an aux table the row-major ones stay alive for
    // the LogUp builder (the LDE stage only reads them)
    std::vector<DeviceMatrix> tv;
    for (MultiBusTable& t : tables) tv.push_back(std::move(t.trace));
    std::unique_ptr<PcsData> trace_data = pcs.commit(tv, std::vector<uint32_t>(T, 1u), true, /*keep_row_major=*/A > 0);
    for (size_t t = 0; t < T; t++)
        if (!tables[t].air->aux_width) tv[t].buf.reset();  // a plain table's rows are not read again
    challenger.observe_commitment(trace_data->root);
    uint32_t challenges[8] = {0};
    for (int k = 0; A && k < 2; k++) {  // gamma, beta: one tuple encoding on the whole bus
        const Ef c = challenger.sample();
        memcpy(challenges + 4 * k, c.c, 16);
    }

    // the LogUp matrices of the tables that have one, then ONE commit of them in table order
    std::vector<uint32_t> exposed(4 * A, 0);
    std::vector<DeviceMatrix> av;
    auto key_values = [&](size_t t) -> const DeviceMatrix* {
        return key_of[t] != ~(size_t)0 ? key->values[key_of[t]] : nullptr;
    };
    if (A == 0) {
    } else if (multi_logup_per_table()) {
        for (size_t a = 0; a < A; a++) {
            const size_t t = aux_tables[a];
            try {
                av.push_back(logup_aux_build(ctx, *tables[t].logup, tv[t], challenges, &exposed[4 * a], key_values(t),
                                             /*takes_table=*/key != nullptr));
            } catch (const Error& e) {  // the single call names row and interaction: add the table
                if (e.code != TS_ERR_INVARIANT) throw;
                throw Error(TS_ERR_INVARIANT, "table " + std::to_string(t) + ": " + e.what());
            }
        }
    } else {
        std::vector<const LogupSpec*> specs;
        std::vector<const DeviceMatrix*> traces, pre;
        for (size_t t : aux_tables) {
            specs.push_back(tables[t].logup);
            traces.push_back(&tv[t]);
            pre.push_back(key_values(t));
        }
        std::vector<uint32_t> ids(aux_tables.begin(), aux_tables.end());  // a report names the proof's table
        av = logup_aux_build_multi(ctx, specs, traces, challenges, exposed.data(), ids.data(), key ? &pre : nullptr);
    }
    for (DeviceMatrix& m : tv) m.buf.reset();  // no trace row is read again
    std::unique_ptr<PcsData> aux_data;
    if (A) {
        aux_data = pcs.commit(av, std::vector<uint32_t>(A, 1u));
        challenger.observe_commitment(aux_data->root);
        for (uint32_t e : exposed) challenger.observe(e);
    }
    const Ef alpha = challenger.sample();

    // the chunks of every table over (its key LDE, its aux LDE, its trace LDE) in the batches, each side matrix where
    // the table has one, then one commit of all of them
    std::vector<DeviceMatrix> chunks;
    std::vector<uint32_t> shifts;
    for (size_t t = 0; t < T; t++) {
        std::vector<uint32_t> pis = tables[t].public_values;
        SideLdes side;
        if (key_of[t] != ~(size_t)0) {
            const ColMat& m = key->data->ldes[key_of[t]];
            TS_REQUIRE(m.width == tables[t].air->preprocessed_width && m.height == (1ull << st[t].log_N), TS_ERR_INVARIANT,
                       name + ": a key matrix has another shape than its table's");
            side.m[side.n++] = &m;
        }
        if (aux_of[t] != ~(size_t)0) {
            pis.insert(pis.end(), challenges, challenges + 8);
            pis.insert(pis.end(), &exposed[4 * aux_of[t]], &exposed[4 * aux_of[t]] + 4);
            const ColMat& m = aux_data->ldes[aux_of[t]];
            TS_REQUIRE(m.width == tables[t].air->aux_width && m.height == (1ull << st[t].log_N), TS_ERR_INVARIANT,
                       name + ": a committed aux matrix has another shape than its table's");
            side.m[side.n++] = &m;
        }
        std::vector<DeviceMatrix> c = pcs.quotient_chunks_slab(trace_data->ldes[t], st[t].log_degree, TwoAdicFriPcs::Slab{},
                                                               *tables[t].air, pis, alpha, GENERATOR, side);
        const std::vector<uint32_t> sh = chunk_domain_shifts(GENERATOR, st[t].log_degree, st[t].lqd);
        for (auto& m : c) chunks.push_back(std::move(m));
        shifts.insert(shifts.end(), sh.begin(), sh.end());
    }
    std::unique_ptr<PcsData> quotient_data = pcs.commit(chunks, shifts);
    challenger.observe_commitment(quotient_data->root);
    const Ef zeta = challenger.sample();

    // the rounds in the visiting order of Pcs::open: [key,] [aux,] traces, chunks
    std::vector<OpenMat> mats;
    std::vector<const PcsData*> rounds;
    size_t first = 0, qi = 0;
    if (key) {
        for (size_t t = 0; t < T; t++)
            if (key_of[t] != ~(size_t)0) {
                const ColMat& m = key->data->ldes[key_of[t]];
                mats.push_back(OpenMat{&m, (unsigned)rounds.size(), st[t].log_degree, true, first});
                first += 2 * (size_t)m.width;
            }
        rounds.push_back(key->data.get());
    }
    if (A) {
        for (size_t a = 0; a < A; a++) {
            const size_t t = aux_tables[a];
            mats.push_back(OpenMat{&aux_data->ldes[a], (unsigned)rounds.size(), st[t].log_degree, true, first});
            first += 2 * (size_t)aux_data->ldes[a].width;
        }
        rounds.push_back(aux_data.get());
    }
    for (size_t t = 0; t < T; t++) {
        mats.push_back(OpenMat{&trace_data->ldes[t], (unsigned)rounds.size(), st[t].log_degree, true, first});
        first += 2 * (size_t)st[t].w;
    }
    rounds.push_back(trace_data.get());
    for (size_t t = 0; t < T; t++)
        for (uint32_t c = 0; c < st[t].qd; c++, qi++) {
            const ColMat& m = quotient_data->ldes[qi];
            TS_REQUIRE(m.width == 4 && m.height == (1ull << st[t].log_N), TS_ERR_INVARIANT,
                       name + ": a committed chunk has another shape than its table's");
            mats.push_back(OpenMat{&m, (unsigned)rounds.size(), st[t].log_degree, false, first});
            first += 4;
        }
    rounds.push_back(quotient_data.get());
    std::vector<Ef> opened;
    const std::vector<uint32_t> fri_words = open_rounds(pcs, challenger, rounds, mats, zeta, opened);

    std::vector<uint32_t> pf;
    pf.reserve(32 + 5 * T + exposed.size() + opened.size() * 4 + fri_words.size());
    ProofWriter pw(pf);
    std::vector<ProofWriter::TableShape> shapes;
    for (size_t t = 0; t < T; t++)
        shapes.push_back({st[t].log_degree, st[t].w, st[t].qd, tables[t].air->aux_width, tables[t].air->n_exposed,
                          tables[t].air->preprocessed_width});
    pw.header_multi(shapes, version);
    pw.commitment(trace_data->root, 8);
    if (A) {
        pw.commitment(aux_data->root, 8);
        pw.words(exposed.data(), exposed.size());
    }
    pw.commitment(quotient_data->root, 8);
    pw.opened_values(opened);
    pw.words(fri_words.data(), fri_words.size());
    return pf;
}

std::vector<uint32_t> prove_multi(TwoAdicFriPcs& pcs, BfChallenger& challenger, std::vector<MultiBusTable>& tables) {
    return prove_multi_versioned(pcs, challenger, tables, nullptr, 6);
}

std::vector<uint32_t> prove_multi_bus(TwoAdicFriPcs& pcs, BfChallenger& challenger, std::vector<MultiBusTable>& tables) {
    return prove_multi_versioned(pcs, challenger, tables, nullptr, 7);
}

std::vector<uint32_t> prove_multi_key(TwoAdicFriPcs& pcs, BfChallenger& challenger, std::vector<MultiBusTable>& tables,
                                      const MultiKey& key) {
    return prove_multi_versioned(pcs, challenger, tables, &key, 8);
}

}  // namespace ts
