// Native verifier (host only): accepts exactly the proofs the
// reference's verifier accepts, for the Blake3-Merkle MMCS of this build.
//   uni-stark/src/verifier.rs:19-161   verify
//   fri/src/two_adic_pcs.rs:421-534    Pcs::verify (reduced openings per query)
//   fri/src/verifier.rs:20-60          verify_shape_and_sample_challenges
//   fri/src/verifier.rs:62-98          verify_challenges
//   fri/src/verifier.rs:100-165        verify_query
//   fri/src/two_adic_pcs.rs:87-114     fold_row
//   uni-stark/src/folder.rs:101-105    VerifierConstraintFolder::assert_zero
// Proofs are read in the TSPF v1 wire format.
#include <string.h>

#include <vector>

#include "blake3.hpp"
#include "prover_internal.hpp"

namespace ts {

namespace {

// canonical-domain EF helpers (host scalars only)
Ef c_mul(Ef a, Ef b) { return ef_mul(a, ef_to_mont(b)); }
Ef c_mul_base(Ef a, uint32_t b) { return ef_mul_base(a, to_mont(b)); }
Ef c_inv(Ef a) { return ef_from_mont(ef_inv(ef_to_mont(a))); }
Ef c_pow(Ef a, uint64_t e) { return ef_from_mont(ef_pow(ef_to_mont(a), e)); }
Ef c_one() { return Ef{{1, 0, 0, 0}}; }
Ef c_sub_base(Ef a, uint32_t b) { a.c[0] = sub(a.c[0], b); return a; }
Ef c_add_base(Ef a, uint32_t b) { a.c[0] = add(a.c[0], b); return a; }

struct Reader {
    const uint32_t* w;
    size_t len, pos = 0;
    bool bad = false;
    uint32_t get() {
        if (pos >= len) { bad = true; return 0; }
        return w[pos++];
    }
    const uint32_t* take(size_t n) {
        if (n > len - pos || pos > len) { bad = true; return nullptr; }
        const uint32_t* p = w + pos;
        pos += n;
        return p;
    }
};

void hash_words(const uint32_t* w, size_t n, uint32_t out[8]) {
    // Blake3 over n words, any length (multi-chunk rows included)
    b3::hash_stream([w](uint64_t i) { return w[i]; }, n, out);
}
void compress2(const uint32_t* l, const uint32_t* r, uint32_t out[8]) {
    uint32_t m[16];
    memcpy(m, l, 32);
    memcpy(m + 8, r, 32);
    b3::hash64(m, out);
}

// BFMmcs::verify_batch for the Blake3 Merkle MMCS (mixed heights: rows of a shorter matrix are
// injected at the layer of its height).  rows = concatenated opened rows in matrix order.
bool mmcs_verify(const std::vector<uint64_t>& heights, const std::vector<uint32_t>& widths,
                 uint64_t index, const uint32_t* rows, const uint32_t* path, size_t path_len,
                 const uint32_t root[8]) {
    uint64_t max_h = 0;
    for (size_t i = 0; i < heights.size(); i++) max_h = std::max(max_h, heights[i]);
    unsigned log_max = 0;
    while ((1ull << log_max) < max_h) log_max++;
    if (path_len != log_max || (index >> log_max) != 0) return false;
    auto hash_height = [&](uint64_t h, uint32_t out[8]) -> bool {
        std::vector<uint32_t> buf;
        size_t off = 0;
        for (size_t i = 0; i < heights.size(); i++) {
            if (heights[i] == h) buf.insert(buf.end(), rows + off, rows + off + widths[i]);
            off += widths[i];
        }
        if (buf.empty()) return false;
        hash_words(buf.data(), buf.size(), out);
        return true;
    };
    uint32_t cur[8];
    if (!hash_height(max_h, cur)) return false;
    uint64_t idx = index;
    for (unsigned l = 0; l < log_max; l++) {
        uint32_t nxt[8];
        if (idx & 1) compress2(path + 8 * l, cur, nxt);
        else compress2(cur, path + 8 * l, nxt);
        idx >>= 1;
        uint32_t inj[8];
        if (hash_height(max_h >> (l + 1), inj)) compress2(nxt, inj, cur);
        else memcpy(cur, nxt, 32);
    }
    return memcmp(cur, root, 32) == 0;
}

// two_adic_pcs.rs:87-114
Ef fold_row(uint64_t index, unsigned log_height, Ef beta, Ef e0, Ef e1) {
    const uint32_t s = pow_canon(two_adic_generator(log_height + 1), bitrev32((uint32_t)index, log_height));
    const uint32_t x0 = s, x1 = neg(s);
    Ef num = c_mul(c_sub_base(beta, x0), ef_sub(e1, e0));
    return ef_add(e0, c_mul_base(num, inv_canon(sub(x1, x0))));
}

// tape evaluation over EF4 (verifier side: opened values are extension elements)
// (prep_local / prep_next: the opened preprocessed rows of a version-2 AIR, aux_local / aux_next: the opened aux
// rows of a version-3 AIR; unread otherwise)
void eval_tape_ext(const AirProgram& air, const Ef* prep_local, const Ef* prep_next, const Ef* aux_local,
                   const Ef* aux_next, const Ef* local, const Ef* next,
                   const std::vector<uint32_t>& pis, Ef is_first, Ef is_last, Ef is_trans,
                   std::vector<Ef>& v) {
    const uint32_t n_nodes = air.tape[4];
    const uint32_t* nodes = air.tape_nodes();
    v.resize(n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) {
        const uint32_t op = nodes[3 * i], a = nodes[3 * i + 1], b = nodes[3 * i + 2];
        switch (op) {
            case T_CONST: v[i] = ef_from_base(a); break;
            case T_MAIN: v[i] = a ? next[b] : local[b]; break;
            case T_PREP: v[i] = a ? prep_next[b] : prep_local[b]; break;
            case T_PUBLIC: v[i] = ef_from_base(pis[a]); break;
            // version 3: `pis` is public values ++ challenges ++ exposed
            case T_AUX: v[i] = a ? aux_next[b] : aux_local[b]; break;
            case T_CHALLENGE: v[i] = ef_from_base(pis[air.n_public + a]); break;
            case T_EXPOSED: v[i] = ef_from_base(pis[air.n_public + 4 * air.n_challenges + a]); break;
            case T_IS_FIRST: v[i] = is_first; break;
            case T_IS_LAST: v[i] = is_last; break;
            case T_IS_TRANSITION: v[i] = is_trans; break;
            case T_ADD: v[i] = ef_add(v[a], v[b]); break;
            case T_SUB: v[i] = ef_sub(v[a], v[b]); break;
            case T_NEG: v[i] = ef_neg(v[a]); break;
            default: v[i] = c_mul(v[a], v[b]); break;
        }
    }
}

}  // namespace

// Pcs::verify, fri/src/two_adic_pcs.rs:421-534, with verify_shape_and_sample_challenges and
// verify_challenges / verify_query of fri/src/verifier.rs:20-165, for any rounds x matrices x points.
// `words` = the FriProof (TSPF v1 order, from the commit-phase round count on).  Returns 0 or the
// error code of include/tapstark.h ts_verify.
// `tap` != nullptr: every commitment is num_queries taptree roots (8 words each, `root` points at
// the first) and the MMCS checks are TapTreeMmcs::verify_batch in tree q (taptree_mmcs.rs:77-99)
static int fri_verify_impl(const FriConfig& fri, BfChallenger& challenger,
                           const std::vector<PcsRoundClaim>& rounds, bool pass_through,
                           const uint32_t* words, size_t n_words, const TapLocks* tap = nullptr);

int pcs_verify(const FriConfig& fri, BfChallenger& challenger, const std::vector<PcsRoundClaim>& rounds,
               const uint32_t* words, size_t n_words) {
    return fri_verify_impl(fri, challenger, rounds, false, words, n_words);
}
int fri_verify_pass_through(const FriConfig& fri, BfChallenger& challenger, const uint32_t* words,
                            size_t n_words) {
    return fri_verify_impl(fri, challenger, {}, true, words, n_words);
}

static int fri_verify_impl(const FriConfig& fri, BfChallenger& challenger,
                           const std::vector<PcsRoundClaim>& rounds, bool pass_through,
                           const uint32_t* words, size_t n_words, const TapLocks* tap) {
    const size_t n_roots = tap ? fri.num_queries : 1, cw = 8 * n_roots;
    Reader rb{words, n_words};
    unsigned log_global_max_height = 0;  // two_adic_pcs.rs:447-455
    for (auto& r : rounds)
        for (auto& m : r.mats) {
            if (m.log_height > 27 || m.log_height < fri.log_blowup || m.points.size() != m.values.size())
                return 1;
            for (auto& v : m.values)
                if (v.size() != m.width) return 1;
            log_global_max_height = std::max(log_global_max_height, m.log_height);
        }
    const Ef batch_alpha = pass_through ? c_one() : challenger.sample();  // :443
    const uint32_t R = rb.get();
    if (rb.bad || R > 31) return 9;
    const uint32_t* commits = rb.take(cw * (size_t)R);
    if (rb.bad) return 9;
    std::vector<Ef> betas(R);
    for (uint32_t r = 0; r < R; r++) {  // fri/src/verifier.rs:32-39
        for (size_t k = 0; k < n_roots; k++) challenger.observe_commitment(commits + cw * r + 8 * k);
        betas[r] = challenger.sample();
    }
    // taptree: first lock script of every commitment (commit order: input rounds, then FRI rounds)
    std::vector<size_t> lock_base(rounds.size());
    size_t fri_lock_base = 0;
    for (size_t r = 0; r < rounds.size(); r++) {
        size_t tw = 0;
        for (auto& m : rounds[r].mats) tw += m.width;
        lock_base[r] = fri_lock_base;
        fri_lock_base += n_roots * (1 + tw);
    }
    if (tap && tap->n_scripts < fri_lock_base + (size_t)R * n_roots * 3) return 1;
    const uint32_t Q = rb.get();
    if (rb.bad) return 9;
    if (Q != fri.num_queries) return 2;  // :39-41 InvalidProofShape
    const unsigned log_max_height = R + fri.log_blowup;
    // BabyBear's two-adicity is 27: a taller domain does not exist, and `have`/`ro` below,
    // sample_bits and two_adic_generator all assume it (both paths; R comes from untrusted input).
    if (log_max_height > 27) return pass_through ? 9 : 1;
    if (!pass_through && log_max_height != log_global_max_height) return 1;
    if (pass_through) log_global_max_height = log_max_height;
    // the PoW witness follows the queries in the buffer: locate it with a dry parse
    const size_t save = rb.pos;
    for (uint32_t q = 0; q < Q && !rb.bad; q++) {
        const uint32_t nb = rb.get();
        for (uint32_t k = 0; k < nb && !rb.bad; k++) {
            if (pass_through) {  // (log_height, value)
                rb.take(5);
                continue;
            }
            const uint32_t nm = rb.get();
            for (uint32_t i = 0; i < nm && !rb.bad; i++) rb.take(rb.get());
            rb.take(8 * (size_t)rb.get());
        }
        for (uint32_t r = 0; r < R && !rb.bad; r++) {
            rb.take(8);
            rb.take(8 * (size_t)rb.get());
        }
    }
    const uint32_t* tail = rb.take(5);
    if (rb.bad) return 9;
    if (rb.pos != rb.len) return 9;
    for (int k = 0; k < 4; k++)
        if (tail[k] >= P) return 9;
    const Ef final_poly = Ef{{tail[0], tail[1], tail[2], tail[3]}};
    const uint32_t pow_witness = tail[4];
    rb.pos = save;
    if (!challenger.check_witness(fri.proof_of_work_bits, pow_witness)) return 3;  // :44-46
    std::vector<uint64_t> indices(Q);
    for (uint32_t q = 0; q < Q; q++) indices[q] = challenger.sample_bits(log_max_height);  // :50-52

    for (uint32_t q = 0; q < Q; q++) {  // verify_challenges, fri/src/verifier.rs:62-98
        const uint64_t index = indices[q];
        // ---- open_input, two_adic_pcs.rs:457-528: the reduced opening of every height
        Ef ro[32], alpha_pow[32];
        bool have[32] = {false};
        for (int i = 0; i < 32; i++) {
            ro[i] = ef_zero();
            alpha_pow[i] = c_one();
        }
        if (pass_through) {  // fri.rs:126-140: the input proof IS the reduced openings
            const uint32_t n_in = rb.get();
            if (rb.bad || n_in > 32) return 9;
            unsigned prev = 32;
            for (uint32_t k = 0; k < n_in; k++) {
                const uint32_t* e = rb.take(5);
                if (rb.bad) return 9;
                const unsigned lh = e[0];
                if (lh >= prev || lh > log_max_height) return 1;  // sorted by descending height
                prev = lh;
                for (int j = 1; j < 5; j++)
                    if (e[j] >= P) return 9;
                ro[lh] = Ef{{e[1], e[2], e[3], e[4]}};
                have[lh] = true;
            }
        } else if (rb.get() != rounds.size()) {
            return 1;  // one BatchOpening per commit round
        }
        for (auto& round : rounds) {
            const uint32_t nm = rb.get();
            if (rb.bad || nm != round.mats.size()) return 1;
            std::vector<uint32_t> rows;
            std::vector<uint64_t> heights;
            std::vector<uint32_t> widths;
            unsigned log_batch_max = 0;
            for (uint32_t i = 0; i < nm; i++) {
                const uint32_t wd = rb.get();
                if (rb.bad || wd != round.mats[i].width) return 1;
                const uint32_t* vals = rb.take(wd);
                if (rb.bad) return 9;
                for (uint32_t c = 0; c < wd; c++)
                    if (vals[c] >= P) return 9;
                rows.insert(rows.end(), vals, vals + wd);
                heights.push_back(1ull << round.mats[i].log_height);
                widths.push_back(wd);
                log_batch_max = std::max(log_batch_max, round.mats[i].log_height);
            }
            const uint32_t plen = rb.get();
            const uint32_t* path = rb.take(8 * (size_t)plen);
            if (rb.bad) return 9;
            // :470-486 reduced_index = index >> (log_global_max_height - log_batch_max_height)
            const uint64_t reduced_index = index >> (log_global_max_height - log_batch_max);
            if (tap) {
                // taptree_mmcs.rs:68-72: the opened rows must come tallest matrix first
                for (size_t i = 1; i < heights.size(); i++)
                    if (heights[i] > heights[i - 1]) return 4;
                const size_t ri = (size_t)(&round - rounds.data());
                const uint32_t n_evals = (uint32_t)rows.size();
                if (plen != log_batch_max ||
                    !tap_verify_words(*tap, lock_base[ri] + (size_t)q * (1 + n_evals), n_evals, 1, reduced_index,
                                      rows.data(), path, plen, round.root + 8 * (size_t)q))
                    return 4;
            } else if (!mmcs_verify(heights, widths, reduced_index, rows.data(), path, plen, round.root)) {
                return 4;  // InputError
            }
            size_t off = 0;
            for (uint32_t i = 0; i < nm; i++) {  // :490-523
                const PcsMatClaim& m = round.mats[i];
                const unsigned lh = m.log_height;
                const uint64_t rev = bitrev32((uint32_t)(index >> (log_global_max_height - lh)), lh);
                const uint32_t x = mul(GENERATOR, pow_canon(two_adic_generator(lh), rev));
                have[lh] = true;
                for (size_t p = 0; p < m.points.size(); p++) {
                    Ef acc = ef_zero();
                    for (uint32_t c = 0; c < m.width; c++) {
                        Ef diff = c_add_base(ef_neg(m.values[p][c]), rows[off + c]);
                        acc = ef_add(acc, c_mul(alpha_pow[lh], diff));
                        alpha_pow[lh] = c_mul(alpha_pow[lh], batch_alpha);
                    }
                    const Ef den = c_add_base(ef_neg(m.points[p]), x);
                    ro[lh] = ef_add(ro[lh], c_mul(acc, c_inv(den)));
                }
                off += m.width;
            }
        }
        // ---- verify_query, fri/src/verifier.rs:100-165
        Ef folded_eval = ef_zero();
        uint64_t query_index = index;
        for (uint32_t r = 0; r < R; r++) {
            const unsigned log_folded_height = log_max_height - 1 - r;
            const uint64_t point_index = query_index & 1;
            const uint64_t index_pair = query_index >> 1;
            if (have[log_folded_height + 1]) folded_eval = ef_add(folded_eval, ro[log_folded_height + 1]);  // :127-130
            const uint32_t* vals = rb.take(8);
            const uint32_t plen = rb.get();
            const uint32_t* path = rb.take(8 * (size_t)plen);
            if (rb.bad) return 9;
            for (int k = 0; k < 8; k++)
                if (vals[k] >= P) return 9;
            const Ef e0 = Ef{{vals[0], vals[1], vals[2], vals[3]}}, e1 = Ef{{vals[4], vals[5], vals[6], vals[7]}};
            const Ef committed = point_index ? e1 : e0;
            // :139-141 asserts this from the second round on; checking the first round as well is a
            // strict superset (the reduced opening must be what was committed)
            if (!ef_eq(folded_eval, committed)) return 8;
            std::vector<uint64_t> hh{1ull << log_folded_height};
            std::vector<uint32_t> ww{8};
            if (tap) {
                if (plen != log_folded_height ||
                    !tap_verify_words(*tap, fri_lock_base + ((size_t)r * n_roots + q) * 3, 2, 4, index_pair, vals,
                                      path, plen, commits + cw * r + 8 * (size_t)q))
                    return 5;
            } else if (!mmcs_verify(hh, ww, index_pair, vals, path, plen, commits + 8 * r)) {
                return 5;  // :143-146
            }
            query_index = index_pair;
            folded_eval = fold_row(query_index, log_folded_height, betas[r], e0, e1);  // :149-154
        }
        if (!ef_eq(folded_eval, final_poly)) return 6;  // :92-94 FinalPolyMismatch
    }
    return 0;
}

static bool ood_holds(const AirProgram& air, unsigned degree_bits, Ef zeta, Ef alpha, const Ef* pl, const Ef* pn,
                      const Ef* al, const Ef* an, const Ef* tl, const Ef* tn, const std::vector<Ef>& qc,
                      const std::vector<uint32_t>& pis);

// 0 = accept; otherwise the reference's error (see include/tapstark.h ts_verify).  One body for TSPF v1 to v5, keyed
// on `version` (host.hpp): `tap` (v2), `prep_root` (v3, v5) and `exposed_out` (v4, v5) are the data of those
// versions, not switches.
int verify(uint32_t version, const FriConfig& fri, const AirProgram& air, BfChallenger& challenger,
           const uint32_t* proof, size_t n_words, const std::vector<uint32_t>& pis_in, const uint32_t* prep_root,
           std::vector<uint32_t>* exposed_out, const TapLocks* tap) {
    if (pis_in.size() != air.n_public) return 1;
    // keyed: the key's round leads; phased: the second matrix is the aux trace, committed in the proof
    const bool v3 = version == 3, v5 = version == 5;
    const bool keyed = v3 || v5, phased = version >= 4;
    if (version != 2) tap = nullptr;
    if ((!keyed && air.preprocessed_width) || (!phased && air.aux_width)) return 1;
    Reader rb{proof, n_words};
    if (rb.get() != 0x46505354u || rb.get() != version) return 9;
    const unsigned degree_bits = rb.get();
    const uint32_t pw = rb.get(), pqd = rb.get();
    if (tap && rb.get() != fri.num_queries) return 1;  // TSPF v2: roots per commitment
    const uint32_t P_w = air.preprocessed_width;       // the key's round (v3, v5)
    const uint32_t A_w = air.aux_width;                // the aux trace's round (v4, v5)
    if (v3 && rb.get() != P_w) return 1;               // TSPF v3: the preprocessed width
    if (phased && (rb.get() != A_w || rb.get() != air.n_challenges || rb.get() != air.n_exposed)) return 1;
    if (v5 && rb.get() != P_w) return 1;               // TSPF v5: the v4 header, then the preprocessed width
    if (phased && !A_w && air.n_exposed) return 1;
    if (rb.bad || degree_bits > 27) return 9;
    const size_t n_roots = tap ? fri.num_queries : 1, cw = 8 * n_roots;
    const unsigned lqd = air.log_quotient_degree;
    const uint32_t qd = 1u << lqd, w = air.width;
    // verifier.rs:49-59 valid_shape
    if (pw != w || pqd != qd) return 1;
    const uint32_t* trace_root = rb.take(cw);
    const uint32_t* aux_root = nullptr;
    const uint32_t* exposed = nullptr;
    if (A_w) {  // v4 order: trace root, aux root, exposed words, quotient root
        aux_root = rb.take(8);
        exposed = rb.take(air.n_exposed);
    }
    const uint32_t* quot_root = rb.take(cw);
    const uint32_t* prep_local = rb.take(4 * (size_t)P_w);  // v3 order: the preprocessed rows lead
    const uint32_t* prep_next = rb.take(4 * (size_t)P_w);
    const uint32_t* aux_local = rb.take(4 * (size_t)A_w);   // then the aux rows
    const uint32_t* aux_next = rb.take(4 * (size_t)A_w);
    const uint32_t* trace_local = rb.take(4 * (size_t)w);
    const uint32_t* trace_next = rb.take(4 * (size_t)w);
    const uint32_t* qchunks = rb.take(16 * (size_t)qd);
    if (rb.bad) return 9;
    // (the proof is a word stream: Ef is 16-byte aligned, the words are not)
    std::vector<Ef> pl(P_w), pn(P_w), al(A_w), an(A_w), tl(w), tn(w), qc(4 * (size_t)qd);
    if (P_w) memcpy((void*)pl.data(), prep_local, 16 * (size_t)P_w);
    if (P_w) memcpy((void*)pn.data(), prep_next, 16 * (size_t)P_w);
    if (A_w) memcpy((void*)al.data(), aux_local, 16 * (size_t)A_w);
    if (A_w) memcpy((void*)an.data(), aux_next, 16 * (size_t)A_w);
    memcpy((void*)tl.data(), trace_local, 16 * (size_t)w);
    memcpy((void*)tn.data(), trace_next, 16 * (size_t)w);
    memcpy((void*)qc.data(), qchunks, 64 * (size_t)qd);
    for (auto* vec : {&pl, &pn, &al, &an, &tl, &tn, &qc})
        for (auto& e : *vec)
            for (int k = 0; k < 4; k++)
                if (e.c[k] >= P) return 9;

    for (uint32_t e = 0; exposed && e < air.n_exposed; e++)
        if (exposed[e] >= P) return 9;

    // the key is part of the statement: observed before anything of the proof (prover.cpp prove)
    if (P_w) challenger.observe_commitment(prep_root);
    // verifier.rs:69-75
    for (size_t k = 0; k < n_roots; k++) challenger.observe_commitment(trace_root + 8 * k);
    // v4, v5 (prover.cpp prove_aux): the challenges, then the aux root and the exposed words; the constraints read
    // public values ++ challenge words ++ exposed words
    std::vector<uint32_t> pis = pis_in;
    if (phased) {
        for (uint32_t k = 0; k < air.n_challenges; k++) {
            const Ef c = challenger.sample();
            pis.insert(pis.end(), c.c, c.c + 4);
        }
        if (A_w) {
            challenger.observe_commitment(aux_root);
            for (uint32_t e = 0; e < air.n_exposed; e++) challenger.observe(exposed[e]);
            pis.insert(pis.end(), exposed, exposed + air.n_exposed);
        }
    }
    const Ef alpha = challenger.sample();
    for (size_t k = 0; k < n_roots; k++) challenger.observe_commitment(quot_root + 8 * k);
    const Ef zeta = challenger.sample();
    const uint32_t gn = two_adic_generator(degree_bits);
    const Ef zeta_next = c_mul_base(zeta, gn);

    // ---- pcs.verify, two_adic_pcs.rs:421-534 (verifier.rs:77-101 builds these claims)
    PcsRoundClaim r0, r1;
    r0.root = trace_root;
    r0.mats.push_back(PcsMatClaim{degree_bits + fri.log_blowup, w, {zeta, zeta_next}, {tl, tn}});
    r1.root = quot_root;
    for (uint32_t c = 0; c < qd; c++) {
        std::vector<Ef> vals(qc.begin() + 4 * (size_t)c, qc.begin() + 4 * (size_t)c + 4);
        r1.mats.push_back(PcsMatClaim{degree_bits + fri.log_blowup, 4, {zeta}, {vals}});
    }
    std::vector<PcsRoundClaim> claims{r0, r1};
    if (A_w) {  // the aux trace's round comes before the trace's, opened at the trace's points
        PcsRoundClaim ra;
        ra.root = aux_root;
        ra.mats.push_back(PcsMatClaim{degree_bits + fri.log_blowup, A_w, {zeta, zeta_next}, {al, an}});
        claims.insert(claims.begin(), ra);
    }
    if (P_w) {  // the key's round comes first of all
        PcsRoundClaim rp;
        rp.root = prep_root;
        rp.mats.push_back(PcsMatClaim{degree_bits + fri.log_blowup, P_w, {zeta, zeta_next}, {pl, pn}});
        claims.insert(claims.begin(), rp);
    }
    Reader fr{proof + rb.pos, n_words - rb.pos};
    const int rc = fri_verify_impl(fri, challenger, claims, false, fr.w, fr.len, tap);
    if (rc) return rc;

    if (!ood_holds(air, degree_bits, zeta, alpha, pl.data(), pn.data(), al.data(), an.data(), tl.data(), tn.data(),
                   qc, pis))
        return 7;  // :157 OodEvaluationMismatch
    if (phased) exposed_out->assign(pis.end() - (A_w ? air.n_exposed : 0), pis.end());
    return 0;
}

// verifier.rs:103-157: the constraints folded at zeta over the opened rows, divided by the zeroifier, against the
// quotient recomposed from its opened chunks (qc: 4 values per chunk)
static bool ood_holds(const AirProgram& air, unsigned degree_bits, Ef zeta, Ef alpha, const Ef* pl, const Ef* pn,
                      const Ef* al, const Ef* an, const Ef* tl, const Ef* tn, const std::vector<Ef>& qc,
                      const std::vector<uint32_t>& pis) {
    const unsigned lqd = air.log_quotient_degree;
    const uint32_t qd = 1u << lqd;
    const uint32_t gn = two_adic_generator(degree_bits);
    // ---- verifier.rs:103-132 quotient recombination
    const std::vector<uint32_t> shifts = chunk_domain_shifts(GENERATOR, degree_bits, lqd);
    Ef quotient = ef_zero();
    for (uint32_t i = 0; i < qd; i++) {
        Ef zp = c_one();
        for (uint32_t j = 0; j < qd; j++) {
            if (j == i) continue;
            const uint32_t sj_inv = inv_canon(shifts[j]);
            // zp_at_point(z) = (z/shift)^(2^log_n) - 1
            Ef a = c_sub_base(c_pow(c_mul_base(zeta, sj_inv), 1ull << degree_bits), 1);
            const uint32_t bden = sub(pow_canon(mul(shifts[i], sj_inv), 1ull << degree_bits), 1);
            zp = c_mul(zp, c_mul_base(a, inv_canon(bden)));
        }
        for (int e = 0; e < 4; e++) {
            Ef mono = ef_zero();
            mono.c[e] = 1;
            quotient = ef_add(quotient, c_mul(c_mul(zp, mono), qc[4 * (size_t)i + e]));
        }
    }
    // :136 selectors_at_point (trace domain shift 1)
    const Ef zh = c_sub_base(c_pow(zeta, 1ull << degree_bits), 1);
    const uint32_t gn_inv = inv_canon(gn);
    const Ef is_first = c_mul(zh, c_inv(c_sub_base(zeta, 1)));
    const Ef is_last = c_mul(zh, c_inv(c_sub_base(zeta, gn_inv)));
    const Ef is_trans = c_sub_base(zeta, gn_inv);
    const Ef inv_zeroifier = c_inv(zh);
    // :138-153 fold the constraints at zeta
    std::vector<Ef> v;
    eval_tape_ext(air, pl, pn, al, an, tl, tn, pis, is_first, is_last, is_trans, v);
    const uint32_t* cons = air.tape_constraints();
    Ef acc = ef_zero();
    for (uint32_t c = 0; c < air.n_constraints; c++) acc = ef_add(c_mul(acc, alpha), v[cons[c]]);
    return ef_eq(c_mul(acc, inv_zeroifier), quotient);
}

// ------------------------------------------------------------------ verify, several tables in one proof
// The verifier of the multi-table provers (prove_multi.cpp), one body for three formats:
//   TSPF v6 (prove_multi): [magic, 6, T], T x [log_degree, width, qd], trace root, quotient root, the opened values
//     in (round, matrix, point, column) order over (traces, chunks), the FriProof.  Plain tables only.
//   TSPF v7 (prove_multi_bus): T x [.., aux_width, n_exposed]; behind the trace root the aux root and the exposed
//     words (four per aux table, table order); the aux matrices' round before the traces'.  No preprocessed columns,
//     at least one aux table.
//   TSPF v8 (prove_multi_key): a sixth header word per table (the preprocessed width), the key root observed after
//     the shapes (it is not in the proof), the key's round first of all.  At least one table with preprocessed
//     columns; without an aux table the proof holds no aux root and no exposed words, and no challenge is sampled
//     before alpha.
// Replays the transcript -- with aux tables the challenge phase of verify: gamma and beta once for every table,
// the aux root and the exposed words -- runs the out-of-domain check of verify per table on that table's domain
// over (key, aux, trace) with pis ++ challenges ++ that table's exposed words, then Pcs::verify over the rounds.
// `exposed` receives the proof's exposed words and `bus_sum` their EF4 sum over the tables on acceptance; whether
// the bus balances (bus_sum == 0) is the caller's statement, as the single-table verifier leaves it.
static int verify_multi_impl(const FriConfig& fri, BfChallenger& challenger, uint32_t version, const uint32_t* key_root,
                             const std::vector<const AirProgram*>& airs,
                             const std::vector<std::vector<uint32_t>>& public_values, const uint32_t* proof,
                             size_t n_words, std::vector<uint32_t>& exposed, uint32_t bus_sum[4]) {
    const size_t T = airs.size();
    const size_t SW = version == 6 ? 3 : version == 7 ? 5 : 6;  // header words per table
    if (T == 0 || T > MAX_MULTI_TABLES || public_values.size() != T) return 1;
    size_t A = 0, K = 0;
    for (size_t t = 0; t < T; t++) {
        if (!airs[t] || public_values[t].size() != airs[t]->n_public) return 1;
        const AirProgram& a = *airs[t];
        if (version > 6 && (a.aux_width ? (a.n_challenges != 2 || a.n_exposed != 4) : (a.n_challenges || a.n_exposed)))
            return 1;
        A += a.aux_width ? 1 : 0;
        K += a.preprocessed_width ? 1 : 0;
    }
    if (version == 6 ? (A || K) : version == 7 ? (K || !A) : !K) return 1;
    Reader rb{proof, n_words};
    if (rb.get() != TSPF_MAGIC || rb.get() != version) return 9;
    const uint32_t pT = rb.get();
    if (rb.bad) return 9;
    if (pT != T) return 1;
    const uint32_t* shapes = rb.take(SW * T);
    if (rb.bad) return 9;
    size_t n_vals = 0;  // opened EF4 values
    unsigned log_max = 0;
    for (size_t t = 0; t < T; t++) {
        const uint32_t* sh = shapes + SW * t;
        if (sh[0] > 27) return 9;
        if (sh[1] != airs[t]->width || sh[2] != (1u << airs[t]->log_quotient_degree) ||
            (SW > 3 && (sh[3] != airs[t]->aux_width || sh[4] != airs[t]->n_exposed)) ||
            (SW > 5 && sh[5] != airs[t]->preprocessed_width))
            return 1;
        n_vals += 2 * (size_t)airs[t]->preprocessed_width + 2 * (size_t)airs[t]->aux_width + 2 * (size_t)airs[t]->width +
                  4 * (size_t)sh[2];
        log_max = std::max<unsigned>(log_max, sh[0]);
    }
    const uint32_t* trace_root = rb.take(8);
    const uint32_t* aux_root = A ? rb.take(8) : nullptr;
    const uint32_t* exp_words = rb.take(4 * A);
    const uint32_t* quot_root = rb.take(8);
    const uint32_t* vals = rb.take(4 * n_vals);
    if (rb.bad) return 9;
    for (size_t k = 0; k < 4 * A; k++)
        if (exp_words[k] >= P) return 9;
    for (size_t k = 0; k < 4 * n_vals; k++)
        if (vals[k] >= P) return 9;
    // (the proof is a word stream: Ef is 16-byte aligned, the words are not)
    std::vector<Ef> ov(n_vals);
    memcpy((void*)ov.data(), vals, 16 * n_vals);

    challenger.observe((uint32_t)T);
    for (size_t t = 0; t < T; t++) challenger.observe(shapes[SW * t]);
    if (key_root) challenger.observe_commitment(key_root);
    challenger.observe_commitment(trace_root);
    uint32_t challenges[8] = {0};
    if (A) {  // the challenge phase, skipped whole by a proof without aux tables
        for (int k = 0; k < 2; k++) {
            const Ef c = challenger.sample();
            memcpy(challenges + 4 * k, c.c, 16);
        }
        challenger.observe_commitment(aux_root);
        for (size_t k = 0; k < 4 * A; k++) challenger.observe(exp_words[k]);
    }
    const Ef alpha = challenger.sample();
    challenger.observe_commitment(quot_root);
    const Ef zeta = challenger.sample();

    PcsRoundClaim rk, ra, r0, r1;
    rk.root = key_root;
    ra.root = aux_root;
    r0.root = trace_root;
    r1.root = quot_root;
    // the values in round order: every key matrix's, then every aux matrix's, every trace's, every chunk's
    size_t kat = 0, aat = 0, at = 0, qat = 0, ai = 0;
    for (size_t t = 0; t < T; t++) aat += 2 * (size_t)airs[t]->preprocessed_width;
    at = aat;
    for (size_t t = 0; t < T; t++) at += 2 * (size_t)airs[t]->aux_width;
    qat = at;
    for (size_t t = 0; t < T; t++) qat += 2 * (size_t)airs[t]->width;
    Ef sum = ef_zero();
    for (size_t t = 0; t < T; t++) {
        const unsigned degree_bits = shapes[SW * t];
        const uint32_t w = airs[t]->width, qd = shapes[SW * t + 2], aw = airs[t]->aux_width, kw = airs[t]->preprocessed_width;
        const Ef zeta_next = c_mul_base(zeta, two_adic_generator(degree_bits));
        const std::vector<Ef> kl(ov.begin() + kat, ov.begin() + kat + kw), kn(ov.begin() + kat + kw, ov.begin() + kat + 2 * kw);
        const std::vector<Ef> al(ov.begin() + aat, ov.begin() + aat + aw), an(ov.begin() + aat + aw, ov.begin() + aat + 2 * aw);
        const std::vector<Ef> tl(ov.begin() + at, ov.begin() + at + w), tn(ov.begin() + at + w, ov.begin() + at + 2 * w);
        const std::vector<Ef> qc(ov.begin() + qat, ov.begin() + qat + 4 * (size_t)qd);
        std::vector<uint32_t> pis = public_values[t];
        if (kw) rk.mats.push_back(PcsMatClaim{degree_bits + fri.log_blowup, kw, {zeta, zeta_next}, {kl, kn}});
        if (aw) {
            pis.insert(pis.end(), challenges, challenges + 8);
            pis.insert(pis.end(), exp_words + 4 * ai, exp_words + 4 * ai + 4);
            sum = ef_add(sum, Ef{{exp_words[4 * ai], exp_words[4 * ai + 1], exp_words[4 * ai + 2], exp_words[4 * ai + 3]}});
            ra.mats.push_back(PcsMatClaim{degree_bits + fri.log_blowup, aw, {zeta, zeta_next}, {al, an}});
            ai++;
        }
        if (!ood_holds(*airs[t], degree_bits, zeta, alpha, kl.data(), kn.data(), al.data(), an.data(), tl.data(), tn.data(),
                       qc, pis))
            return 7;
        r0.mats.push_back(PcsMatClaim{degree_bits + fri.log_blowup, w, {zeta, zeta_next}, {tl, tn}});
        for (uint32_t c = 0; c < qd; c++)
            r1.mats.push_back(PcsMatClaim{degree_bits + fri.log_blowup, 4, {zeta},
                                          {std::vector<Ef>(qc.begin() + 4 * (size_t)c, qc.begin() + 4 * (size_t)c + 4)}});
        kat += 2 * (size_t)kw;
        aat += 2 * (size_t)aw;
        at += 2 * (size_t)w;
        qat += 4 * (size_t)qd;
    }
    // the counts that lead the FriProof belong to the shape this format fixes (verdict 1, like the header's): R
    // commit-phase roots for the tallest table, then num_queries answers
    Reader fr{proof + rb.pos, n_words - rb.pos};
    const uint32_t R = fr.get();
    if (fr.bad) return 9;
    if (R != log_max) return 1;
    fr.take(8 * (size_t)R);
    const uint32_t Q = fr.get();
    if (fr.bad) return 9;
    if (Q != fri.num_queries) return 1;
    std::vector<PcsRoundClaim> claims;
    if (key_root) claims.push_back(rk);
    if (A) claims.push_back(ra);
    claims.push_back(r0);
    claims.push_back(r1);
    const int rc = fri_verify_impl(fri, challenger, claims, false, proof + rb.pos, n_words - rb.pos);
    if (rc) return rc;
    exposed.assign(exp_words, exp_words + 4 * A);
    memcpy(bus_sum, sum.c, 16);
    return 0;
}

int verify_multi(const FriConfig& fri, BfChallenger& challenger, const std::vector<const AirProgram*>& airs,
                 const std::vector<std::vector<uint32_t>>& public_values, const uint32_t* proof, size_t n_words) {
    std::vector<uint32_t> exposed;  // none in a v6 proof
    uint32_t bus_sum[4];
    return verify_multi_impl(fri, challenger, 6, nullptr, airs, public_values, proof, n_words, exposed, bus_sum);
}

int verify_multi_bus(const FriConfig& fri, BfChallenger& challenger, const std::vector<const AirProgram*>& airs,
                     const std::vector<std::vector<uint32_t>>& public_values, const uint32_t* proof, size_t n_words,
                     std::vector<uint32_t>& exposed, uint32_t bus_sum[4]) {
    return verify_multi_impl(fri, challenger, 7, nullptr, airs, public_values, proof, n_words, exposed, bus_sum);
}

int verify_multi_key(const FriConfig& fri, BfChallenger& challenger, const uint32_t key_root[8],
                     const std::vector<const AirProgram*>& airs, const std::vector<std::vector<uint32_t>>& public_values,
                     const uint32_t* proof, size_t n_words, std::vector<uint32_t>& exposed, uint32_t bus_sum[4]) {
    if (!key_root) return 1;
    return verify_multi_impl(fri, challenger, 8, key_root, airs, public_values, proof, n_words, exposed, bus_sum);
}

}  // namespace ts
