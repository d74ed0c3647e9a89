// extern "C" boundary (include/tapstark.h): plain pointers and sizes, status codes, no exceptions
// across the ABI.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <memory>
#include <string>
#include <vector>

#include "abi_types.hpp"
#include "blake3.hpp"
#include "collect.hpp"
#include "expand.hpp"
#include "group.hpp"
#include "derive.hpp"
#include "jit.hpp"
#include "join.hpp"
#include "logup.hpp"
#include "prover_internal.hpp"
#include "scan.hpp"
#include "sort.hpp"

// the program as the prover sees it; the handle is const in the prove calls, adopting a finished specialisation is not
static const ts::AirProgram& ready_prog(const ts_air* air) { return const_cast<ts_air*>(air)->a.ready(); }

struct ts_challenger {
    ts::BfChallenger c;
    ts_challenger(int perm, bool ext) : c(perm, ext) {}
};

namespace {

thread_local std::string g_create_error;

// set_device = false: argument checks that must fail before anything touches a device
template <class F>
ts_status guard(ts_ctx* ctx, F&& f, bool set_device = true) {
    try {
        if (ctx && set_device) TS_HIP(hipSetDevice(ctx->ctx.device));
        f();
        return TS_OK;
    } catch (const ts::Error& e) {
        if (ctx) ctx->ctx.last_error = e.what();
        else g_create_error = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        if (ctx) ctx->ctx.last_error = "host allocation failed";
        return TS_ERR_OOM;
    } catch (const std::exception& e) {
        if (ctx) ctx->ctx.last_error = e.what();
        return TS_ERR_INVALID;
    }
}

ts::Ef load_ef(const uint32_t w[4]) {
    for (int i = 0; i < 4; i++)
        TS_REQUIRE(w[i] < ts::P, ts::TS_ERR_INVALID, "non-canonical extension-field element");
    return ts::Ef{{w[0], w[1], w[2], w[3]}};
}

ts::FriConfig load_cfg(const ts_fri_config* cfg) {
    TS_REQUIRE(cfg != nullptr, ts::TS_ERR_INVALID, "null FriConfig");
    TS_REQUIRE(cfg->log_blowup >= 1 && cfg->log_blowup <= 8, ts::TS_ERR_INVALID,
               "FriConfig.log_blowup must be in [1, 8]");
    TS_REQUIRE(cfg->num_queries >= 1 && cfg->num_queries <= 4096, ts::TS_ERR_INVALID,
               "FriConfig.num_queries must be in [1, 4096]");
    TS_REQUIRE(cfg->proof_of_work_bits <= 31, ts::TS_ERR_INVALID, "FriConfig.proof_of_work_bits > 31");
    ts::FriConfig f;
    f.log_blowup = cfg->log_blowup;
    f.num_queries = cfg->num_queries;
    f.proof_of_work_bits = cfg->proof_of_work_bits;
    return f;
}

// ------------------------------------------------------------------ arguments of the prove / verify calls
std::vector<uint32_t> public_inputs(const uint32_t* values, uint32_t n) {
    std::vector<uint32_t> pis;
    if (n) {
        TS_REQUIRE(values, ts::TS_ERR_INVALID, "null public values");
        pis.assign(values, values + n);
    }
    return pis;
}

// The four single-table formats.  The operations of a format are "ts_<operation><suffix>": prove, verify,
// quotient_chunks, check_constraints.  DESIGN.md section 5 has the table of what each takes and refuses.
struct SingleCall {
    uint32_t version;    // the TSPF version its prove call writes and its verify call takes
    const char* suffix;  // of the entry points' names
    bool key;            // takes a preprocessed key (prove, quotient_chunks), its root (verify), the matrix (check)
    bool aux;            // takes an aux source (prove), aux data (quotient_chunks), the matrix (check); verify hands
                         // back the exposed words
    // Three differences between the formats, kept as they are ("Kept differences"):
    bool any_context;          // prove does not refuse a trace made on another context
    bool own_height_text;      // prove words its key-height refusal itself; the others leave it to check_side_matrix
    bool anonymous_key_texts;  // the AIR-kind and key refusals of prove and quotient_chunks do not name the entry point

    std::string name(const char* op) const { return std::string("ts_") + op + suffix; }
    std::string keyed_name(const char* op) const {
        return anonymous_key_texts ? "a call that takes a preprocessed key" : name(op);
    }
};
constexpr SingleCall PLAIN{1, "", false, false, true, false, false}, PRE{3, "_pre", true, false, true, true, true},
    AUX{4, "_aux", false, true, false, false, false}, PRE_AUX{5, "_pre_aux", true, true, false, false, false};

// The one admission of an AIR to a single-table call (`call` names it in the texts), before anything is consumed or
// launched: a call without an aux argument refuses aux columns, a call without a key argument preprocessed ones.
void admit_air(const SingleCall& sc, const ts_air* air, const std::string& call) {
    const ts::AirProgram& p = air->a.prog();
    TS_REQUIRE(sc.aux || !p.aux_width, ts::TS_ERR_UNSUPPORTED,
               call + ": the AIR has challenge-phase (aux) columns; prove it with ts_prove_aux" +
                   (sc.key ? "" : " (and ts_quotient_chunks_aux, ts_check_constraints_aux, ts_verify_aux)"));
    // (aux columns together with a key would be a third matrix in the kernels of the ts_*_aux calls)
    TS_REQUIRE(sc.key || !p.preprocessed_width, ts::TS_ERR_UNSUPPORTED,
               call + (sc.aux ? ": preprocessed columns together with aux columns are not supported yet"
                              : ": the AIR has preprocessed columns; prove it with ts_prove_pre (and "
                                "ts_quotient_chunks_pre, ts_check_constraints_pre, ts_verify_pre)"));
}
// public values ++ challenge words ++ exposed words, as the lowered program of a version-3 AIR indexes them
std::vector<uint32_t> public_slots(const ts::AirProgram& p, const uint32_t* values, uint32_t n, const uint32_t* challenges,
                                   const uint32_t* exposed) {
    TS_REQUIRE(n == p.n_public, ts::TS_ERR_INVALID, "wrong number of public values");
    std::vector<uint32_t> pis = public_inputs(values, n);
    TS_REQUIRE((challenges || !p.n_challenges) && (exposed || !p.n_exposed), ts::TS_ERR_INVALID,
               "null challenges or exposed words for an AIR that has them");
    pis.insert(pis.end(), challenges, challenges + 4 * (size_t)p.n_challenges);
    pis.insert(pis.end(), exposed, exposed + p.n_exposed);
    for (uint32_t v : pis) TS_REQUIRE(v < ts::P, ts::TS_ERR_INVALID, "non-canonical public value, challenge or exposed word");
    return pis;
}

// The key of the calls that take one (`call` names it in the texts): null exactly when the AIR has no preprocessed
// columns, else one committed matrix of the AIR's preprocessed width, made on this context.  (Its height is
// checked against the trace's where both are known: ts::check_side_matrix.)  Returns the PcsData or null.
const ts::PcsData* preprocessed_key_any(ts_ctx* ctx, const ts_air* air, const ts_pcs_data* key, const char* call) {
    const uint32_t pw = air->a.prog().preprocessed_width;
    TS_REQUIRE((key != nullptr) == (pw > 0), ts::TS_ERR_INVALID,
               std::string(call) + (pw ? ": null preprocessed key for an AIR with preprocessed columns"
                                       : ": a preprocessed key was given for an AIR without preprocessed columns"));
    if (!key) return nullptr;
    TS_REQUIRE(key->d && key->d->ldes.size() == 1, ts::TS_ERR_INVALID,
               "preprocessed key: exactly one committed matrix expected");
    TS_REQUIRE(key->d->ldes[0].width == pw, ts::TS_ERR_INVALID,
               "preprocessed key: width differs from the AIR's preprocessed width");
    TS_REQUIRE(key->d->tree.ctx == &ctx->ctx, ts::TS_ERR_INVALID, "preprocessed key was made on another context");
    return key->d.get();
}

// The committed aux trace of the calls that take one: null exactly when the AIR has no aux columns, else one
// committed matrix of the AIR's aux width, made on this context.  Returns the PcsData or null.
const ts::PcsData* committed_aux(ts_ctx* ctx, const ts::AirProgram& p, const ts_pcs_data* aux_data) {
    TS_REQUIRE((aux_data != nullptr) == (p.aux_width > 0), ts::TS_ERR_INVALID,
               p.aux_width ? "null aux data for an AIR with aux columns"
                           : "aux data was given for an AIR without aux columns");
    if (!aux_data) return nullptr;
    TS_REQUIRE(aux_data->d && aux_data->d->ldes.size() == 1 && aux_data->d->ldes[0].width == p.aux_width,
               ts::TS_ERR_INVALID, "aux data: exactly one committed matrix of the AIR's aux width expected");
    TS_REQUIRE(aux_data->d->tree.ctx == &ctx->ctx, ts::TS_ERR_INVALID, "aux data was made on another context");
    return aux_data->d.get();
}

// A row-major matrix beside the trace of a ts_check_constraints* call (`what`: "preprocessed" or "aux"): null
// exactly when the AIR has no such columns (`width` of them), else on this context, of that width and the trace's
// height.  Appended to `side`: the caller adds the preprocessed matrix before the aux one.
void add_side_rows(ts_ctx* ctx, const ts_matrix* m, uint32_t width, const std::string& what, const ts_matrix* trace,
                   ts::SideRows& side) {
    TS_REQUIRE((m != nullptr) == (width > 0), ts::TS_ERR_INVALID,
               "check_constraints: the " + what + " matrix is needed exactly by an AIR with " + what + " columns");
    if (!m) return;
    TS_REQUIRE(m->m.buf.p && m->m.layout == ts::DeviceMatrix::ROW_MAJOR && m->m.buf.ctx == &ctx->ctx &&
                   m->m.width == width && m->m.height == trace->m.height,
               ts::TS_ERR_INVALID, "check_constraints: the " + what + " matrix must be on this context, row-major, of "
                                   "the AIR's " + what + " width and the trace's height");
    side.d[side.n] = m->m.buf.p;
    side.width[side.n++] = width;
}

// the trace is consumed, like the reference's moved RowMajorMatrix
ts::DeviceMatrix take_trace(ts_matrix* trace) {
    TS_REQUIRE(trace->m.buf.p, ts::TS_ERR_INVALID, "trace matrix was already consumed");
    return std::move(trace->m);
}

// *n_words_out is set before the size check: a caller told TS_ERR_BUFFER learns the size it needs
void copy_proof(const std::vector<uint32_t>& words, uint32_t* out, size_t cap, size_t* n_words_out) {
    *n_words_out = words.size();
    TS_REQUIRE(words.size() <= cap, ts::TS_ERR_BUFFER, "proof buffer too small");
    memcpy(out, words.data(), words.size() * 4);
}

ts::TapLocks tap_locks(const uint8_t* bytes, const uint64_t* offsets, size_t n_scripts) {
    ts::TapLocks locks;
    locks.bytes = bytes;
    locks.offsets = offsets;
    locks.n_scripts = n_scripts;
    return locks;
}

// a rank leaving the protocol on an error makes the peers' pending collectives fail instead of hang
template <class F>
auto abort_on_throw(const ts_comm& cb, F&& fn) -> decltype(fn()) {
    try {
        return fn();
    } catch (...) {
        if (cb.abort) cb.abort(cb.user);
        throw;
    }
}

// ------------------------------------------------------------------ lanes of ts_prove_stream / ts_prove_batch
// The refusals every lane call shares, made before any lane starts: pointer comparisons only, so no context
// is dereferenced.  A context on two lanes would have two threads driving one Context (pool, stream,
// last_error).
bool check_lanes(ts_ctx* const* ctxs, const ts_air* const* airs, uint32_t n_lanes, const ts_fri_config* cfg,
                 ts::FriConfig& fri) {
    if (!ctxs || !airs || n_lanes == 0 || n_lanes > 64) return false;
    for (uint32_t l = 0; l < n_lanes; l++) {
        if (!ctxs[l] || !airs[l]) return false;
        for (uint32_t k = 0; k < l; k++)
            if (ctxs[k] == ctxs[l]) return false;
    }
    try {
        fri = load_cfg(cfg);
    } catch (const ts::Error&) {
        return false;
    }
    return true;
}

// The call's clock and its start gate: no two proofs start within gap ms of each other.  enter() stamps the
// start inside the critical section, so sorted stamps are at least gap apart.
struct StartGate {
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    const double gap;
    std::mutex m;
    double last = -1e300;

    explicit StartGate(double gate_ms) : gap(gate_ms > 0 ? gate_ms : 0) {}
    double now_ms() const {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
    double enter() {
        if (gap <= 0) return now_ms();
        std::lock_guard<std::mutex> g(m);
        for (double wait; (wait = last + gap - now_ms()) > 0;)
            std::this_thread::sleep_for(std::chrono::microseconds((long)std::min(wait * 1e3, 200.0)));
        return last = now_ms();
    }
};

// fn(l) for every lane: lanes 1 .. n_lanes-1 on threads of their own, lane 0 on the caller's.  If a thread
// cannot be created, no further lane starts (lane 0 neither), the running ones finish and are joined, and
// the call gets TS_ERR_OOM instead of an exception through the C ABI.
template <class F>
ts_status run_lanes(uint32_t n_lanes, const F& fn) {
    std::vector<std::thread> threads;
    ts_status st = TS_OK;
    try {
        threads.reserve(n_lanes - 1);
        for (uint32_t l = 1; l < n_lanes; l++) threads.emplace_back(fn, l);
    } catch (...) {  // std::system_error, std::bad_alloc
        st = TS_ERR_OOM;
    }
    if (st == TS_OK) fn(0);
    for (std::thread& t : threads) t.join();
    return st;
}

// a lane's device trace: made on the lane's context, of the AIR's width and unconsumed, all checked before it
// is moved out
ts::DeviceMatrix lane_trace(ts_matrix* trace, ts_ctx* ctx, const ts::AirProgram& prog) {
    TS_REQUIRE(trace->m.buf.ctx == &ctx->ctx, ts::TS_ERR_INVALID, "trace was not made on the lane's context");
    TS_REQUIRE(trace->m.width == prog.width, ts::TS_ERR_INVALID, "trace width differs from the lane's AIR");
    return take_trace(trace);
}

// ---- the lane body of ts_prove_batch and ts_prove_batch_lookup: ONE owner of the per-item argument checks, the
// upload on the lane's stream, the gate, the proof copy, the digest and the state export.  `Item` has
// ts_batch_item's fields under the same names; a call supplies what differs through BatchCall's three hooks.
struct ItemOutcome {
    bool lane_goes_on = false;  // the failure says something about the item's data, not about the context
    ts_status status = TS_OK;   // non-zero: replaces the item's status (an aux callback's own status)
};
template <class Item>
struct BatchCall {
    const char* name = "";  // the entry point, in texts that name it
    const char* what = "";  // the prefix of the per-item refusals
    ts_ctx* const* ctxs = nullptr;
    const ts_air* const* airs = nullptr;
    // the item's outputs beyond ts_batch_item's, before anything runs
    void reset(Item&) const {}
    // refusals that depend on the lane's AIR alone: before any other check of the item
    void refuse(uint32_t) const {}
    // refusals that need the trace's shape: after the shared checks, before the trace is taken or uploaded
    // (`trace`: the device handle's matrix, null for a host trace)
    void admit(uint32_t, Item&, const ts::AirProgram&, uint64_t, const ts::DeviceMatrix*) const {}
};

template <class Call, class Item>
ts_status run_batch(const Call& call, uint32_t n_lanes, const ts::FriConfig& fri, Item* items, uint32_t n_items,
                    double gate_ms, uint32_t flags) {
    for (uint32_t i = 0; i < n_items; i++) {
        Item& it = items[i];
        it.status = -1;
        it.n_words = 0;
        it.start_ms = it.wall_ms = 0;
        memset(it.proof_blake3, 0, sizeof it.proof_blake3);
        memset(it.final_state, 0, sizeof it.final_state);
        call.reset(it);
    }
    // items no lane can take, or whose trace handle an earlier item already names (two lane threads would
    // race for it), fail here
    std::vector<std::pair<const ts_matrix*, uint32_t>> handles;
    for (uint32_t i = 0; i < n_items; i++) {
        if (items[i].lane >= n_lanes) items[i].status = TS_ERR_INVALID;
        else if (items[i].trace) handles.emplace_back(items[i].trace, i);
    }
    std::sort(handles.begin(), handles.end());
    for (size_t k = 1; k < handles.size(); k++)
        if (handles[k].first == handles[k - 1].first) items[handles[k].second].status = TS_ERR_INVALID;

    const std::string what = call.what;
    StartGate gate(gate_ms);
    auto lane_main = [&](uint32_t l) {
        ts_ctx* ctx = call.ctxs[l];
        const ts_air* air = call.airs[l];
        std::unique_ptr<ts::TwoAdicFriPcs> pcs;
        for (uint32_t i = 0; i < n_items; i++) {
            Item& it = items[i];
            if (it.lane != l || it.status != -1) continue;
            ItemOutcome outcome;
            it.status = guard(ctx, [&] {
                call.refuse(l);
                const ts::AirProgram& prog = ready_prog(air);
                TS_REQUIRE((it.trace != nullptr) != (it.host_trace != nullptr), ts::TS_ERR_INVALID,
                           what + ": exactly one of trace / host_trace must be set");
                TS_REQUIRE(it.proof_out, ts::TS_ERR_INVALID, what + ": null proof_out");
                TS_REQUIRE(it.n_public == prog.n_public, ts::TS_ERR_INVALID,
                           what + ": n_public differs from the lane's AIR");
                const std::vector<uint32_t> pis = public_inputs(it.public_values, it.n_public);
                if (!it.trace) {
                    TS_REQUIRE(it.height >= 1 && (it.height & (it.height - 1)) == 0 && it.height <= (1ull << 27),
                               ts::TS_ERR_INVALID, what + ": host trace height must be a power of two <= 2^27");
                    TS_REQUIRE(it.width == prog.width, ts::TS_ERR_INVALID,
                               what + ": host trace width differs from the lane's AIR");
                }
                call.admit(l, it, prog, it.trace ? it.trace->m.height : it.height, it.trace ? &it.trace->m : nullptr);
                ts::DeviceMatrix trace;
                if (it.trace) trace = lane_trace(it.trace, ctx, prog);
                ts::BfChallenger chal = it.challenger ? it.challenger->c : ts::BfChallenger(0, true);
                if (!pcs) pcs = std::make_unique<ts::TwoAdicFriPcs>(ctx->ctx, fri);
                const double t0 = gate.enter();
                if (!it.trace) {  // H2D on the lane's stream: ordered before the proof's kernels, no host wait here
                    trace.buf = ts::DevBuf<uint32_t>(&ctx->ctx, (size_t)it.height * it.width);
                    trace.height = it.height;
                    trace.width = it.width;
                    trace.layout = ts::DeviceMatrix::ROW_MAJOR;
                    TS_HIP(hipMemcpyAsync(trace.buf.p, it.host_trace, (size_t)it.height * it.width * 4,
                                          hipMemcpyHostToDevice, ctx->ctx.stream));
                }
                std::vector<uint32_t> proof = call.prove(l, it, *pcs, prog, chal, std::move(trace), pis, outcome);
                it.start_ms = t0;
                it.wall_ms = gate.now_ms() - t0;
                chal.export_state(it.final_state);
                copy_proof(proof, it.proof_out, it.cap_words, &it.n_words);
                if (flags & TS_BATCH_DIGEST)
                    ts::b3::hash_stream([&](uint64_t k) { return proof[k]; }, proof.size(), it.proof_blake3);
            });
            if (outcome.status != TS_OK) it.status = outcome.status;
            // a device fault leaves the lane's context in doubt: its later items stay unattempted
            if (!outcome.lane_goes_on &&
                (it.status == TS_ERR_HIP || it.status == TS_ERR_OOM || it.status == TS_ERR_INVARIANT))
                break;
        }
    };
    if (run_lanes(n_lanes, lane_main) != TS_OK) return TS_ERR_OOM;
    for (uint32_t i = 0; i < n_items; i++)
        if (items[i].status != TS_OK) return items[i].status;
    return TS_OK;
}

}  // namespace

extern "C" {

ts_status ts_pcs_verify(const ts_fri_config* cfg, ts_challenger* chal, uint32_t n_rounds,
                        const uint32_t* commitments, const uint32_t* mats_per_round,
                        const uint32_t* log_degrees, const uint32_t* widths, const uint32_t* n_points,
                        const uint32_t* points, const uint32_t* opened_values,
                        const uint32_t* fri_proof, size_t n_words, int* verdict) {
    if (!chal || !commitments || !mats_per_round || !log_degrees || !widths || !n_points || !fri_proof ||
        !verdict || n_rounds == 0)
        return TS_ERR_INVALID;
    *verdict = 9;
    return guard(nullptr, [&] {
        const ts::FriConfig fri = load_cfg(cfg);
        std::vector<ts::PcsRoundClaim> rounds(n_rounds);
        size_t k = 0, pw = 0, ow = 0;
        auto load_checked = [&](const uint32_t* p) {
            for (int j = 0; j < 4; j++) TS_REQUIRE(p[j] < ts::P, ts::TS_ERR_INVALID, "non-canonical element");
            return load_ef(p);
        };
        for (uint32_t r = 0; r < n_rounds; r++) {
            rounds[r].root = commitments + 8 * (size_t)r;
            TS_REQUIRE(mats_per_round[r] >= 1 && mats_per_round[r] <= 16, ts::TS_ERR_INVALID, "mats per round");
            for (uint32_t i = 0; i < mats_per_round[r]; i++, k++) {
                ts::PcsMatClaim m;
                TS_REQUIRE(log_degrees[k] + fri.log_blowup <= 27, ts::TS_ERR_INVALID, "matrix too tall");
                m.log_height = log_degrees[k] + fri.log_blowup;
                m.width = widths[k];
                TS_REQUIRE(n_points[k] == 0 || (points && opened_values), ts::TS_ERR_INVALID, "null points");
                for (uint32_t p = 0; p < n_points[k]; p++, pw += 4) {
                    m.points.push_back(load_checked(points + pw));
                    std::vector<ts::Ef> vals(m.width);
                    for (uint32_t c = 0; c < m.width; c++, ow += 4) vals[c] = load_checked(opened_values + ow);
                    m.values.push_back(std::move(vals));
                }
                rounds[r].mats.push_back(std::move(m));
            }
        }
        *verdict = ts::pcs_verify(fri, chal->c, rounds, fri_proof, n_words);
    });
}

ts_status ts_proof_to_postcard(const uint32_t* proof, size_t n_words, uint8_t* out, size_t cap_bytes,
                               size_t* n_bytes_out) {
    if (!proof || !out || !n_bytes_out) return TS_ERR_INVALID;
    *n_bytes_out = 0;
    return guard(nullptr, [&] {
        std::vector<uint8_t> b;
        // the reference's OpenedValues has no preprocessed fields (uni-stark/src/proof.rs): no postcard form of v3
        TS_REQUIRE(!(n_words >= 2 && proof[0] == ts::TSPF_MAGIC && proof[1] == 3), ts::TS_ERR_UNSUPPORTED,
                   "TSPF v3 proofs (ts_prove_pre) have no postcard form");
        TS_REQUIRE(!(n_words >= 2 && proof[0] == ts::TSPF_MAGIC && proof[1] == 4), ts::TS_ERR_UNSUPPORTED,
                   "TSPF v4 proofs (ts_prove_aux) have no postcard form");
        TS_REQUIRE(!(n_words >= 2 && proof[0] == ts::TSPF_MAGIC && proof[1] == 5), ts::TS_ERR_UNSUPPORTED,
                   "TSPF v5 proofs (ts_prove_pre_aux) have no postcard form");
        TS_REQUIRE(!(n_words >= 2 && proof[0] == ts::TSPF_MAGIC && proof[1] == 6), ts::TS_ERR_UNSUPPORTED,
                   "TSPF v6 proofs (ts_prove_multi) have no postcard form");
        TS_REQUIRE(!(n_words >= 2 && proof[0] == ts::TSPF_MAGIC && proof[1] == 7), ts::TS_ERR_UNSUPPORTED,
                   "TSPF v7 proofs (ts_prove_multi_bus) have no postcard form");
        TS_REQUIRE(!(n_words >= 2 && proof[0] == ts::TSPF_MAGIC && proof[1] == 8), ts::TS_ERR_UNSUPPORTED,
                   "TSPF v8 proofs (ts_prove_multi_key) have no postcard form");
        TS_REQUIRE(ts::tspf_to_postcard(proof, n_words, b), ts::TS_ERR_INVALID, "not a TSPF v1 proof");
        *n_bytes_out = b.size();
        TS_REQUIRE(b.size() <= cap_bytes, ts::TS_ERR_BUFFER, "postcard buffer too small");
        memcpy(out, b.data(), b.size());
    });
}
ts_status ts_proof_from_postcard(const uint8_t* bytes, size_t n_bytes, uint32_t* proof_out,
                                 size_t cap_words, size_t* n_words_out) {
    return ts_proof_from_postcard_v(bytes, n_bytes, 0, proof_out, cap_words, n_words_out);
}
ts_status ts_proof_from_postcard_v(const uint8_t* bytes, size_t n_bytes, int tspf_version,
                                   uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    if (!bytes || !proof_out || !n_words_out || tspf_version < 0 || tspf_version > 2) return TS_ERR_INVALID;
    *n_words_out = 0;
    return guard(nullptr, [&] {
        std::vector<uint32_t> w;
        TS_REQUIRE(ts::postcard_to_tspf(bytes, n_bytes, w, tspf_version), ts::TS_ERR_INVALID,
                   "malformed postcard proof (or not of the TSPF version asked for)");
        copy_proof(w, proof_out, cap_words, n_words_out);
    });
}

uint32_t ts_abi_version(void) { return 5; }  // 5: ts_shard_options (struct_size first, the dead column_sharded_inverse gone), ts_air_program / _jit_*

int ts_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

ts_status ts_ctx_create(int device, ts_ctx** out) {
    if (!out) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(nullptr, [&] { *out = new ts_ctx(device); });
}
void ts_ctx_destroy(ts_ctx* ctx) { delete ctx; }
const char* ts_last_error(const ts_ctx* ctx) {
    return ctx ? ctx->ctx.last_error.c_str() : g_create_error.c_str();
}
ts_status ts_ctx_synchronize(ts_ctx* ctx) {
    if (!ctx) return TS_ERR_INVALID;
    return guard(ctx, [&] { ctx->ctx.sync(); });
}
void* ts_ctx_stream(ts_ctx* ctx) { return ctx ? (void*)ctx->ctx.stream : nullptr; }
ts_status ts_ctx_set_timing(ts_ctx* ctx, int enabled) {
    if (!ctx) return TS_ERR_INVALID;
    ctx->ctx.timing = enabled != 0;
    ctx->ctx.stage_ms.clear();
    return TS_OK;
}
ts_status ts_ctx_take_timings(ts_ctx* ctx, char* buf, size_t cap) {
    if (!ctx || !buf || cap == 0) return TS_ERR_INVALID;
    std::string s;
    for (auto& kv : ctx->ctx.stage_ms) {
        char tmp[160];
        snprintf(tmp, sizeof tmp, "%s=%.6f;", kv.first.c_str(), kv.second);
        s += tmp;
    }
    ctx->ctx.stage_ms.clear();
    if (s.size() + 1 > cap) return TS_ERR_BUFFER;
    memcpy(buf, s.c_str(), s.size() + 1);
    return TS_OK;
}

ts_status ts_ctx_set_replay(ts_ctx* ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return TS_ERR_INVALID;
    return guard(ctx, [&] {
        ctx->ctx.sync();
        if (mode == 1) ctx->ctx.replay_log.clear();
        ctx->ctx.replay_pos = 0;
        ctx->ctx.replay_mode = mode;
    });
}
ts_status ts_ctx_set_kernel_timing(ts_ctx* ctx, int enabled) {
    if (!ctx) return TS_ERR_INVALID;
    return guard(ctx, [&] {
        ctx->ctx.take_kernel_timings();  // drop anything pending
        ctx->ctx.kernel_timing = enabled != 0;
    });
}
ts_status ts_ctx_take_kernel_timings(ts_ctx* ctx, char* buf, size_t cap) {
    if (!ctx || !buf || cap == 0) return TS_ERR_INVALID;
    return guard(ctx, [&] {
        std::string s;
        for (auto& kv : ctx->ctx.take_kernel_timings()) {
            char tmp[200];
            snprintf(tmp, sizeof tmp, "%s=%llu:%.6f;", kv.first.c_str(),
                     (unsigned long long)kv.second.first, kv.second.second);
            s += tmp;
        }
        TS_REQUIRE(s.size() + 1 <= cap, ts::TS_ERR_BUFFER, "timing buffer too small");
        memcpy(buf, s.c_str(), s.size() + 1);
    });
}

ts_status ts_ctx_graph_stats(ts_ctx* ctx, uint64_t out[4]) {
    if (!ctx || !out) return TS_ERR_INVALID;
    out[0] = out[1] = out[2] = 0;  // the retired FRI graph replay's counters
    out[3] = ctx->ctx.bytes_reserved;
    return TS_OK;
}

ts_status ts_ctx_stat(ts_ctx* ctx, int which, uint64_t* out) {
    if (!ctx || !out) return TS_ERR_INVALID;
    switch (which) {
    case 0: case 1: case 2: case 4: *out = 0; break;  // the retired FRI graph replay's counters
    case 3: *out = ctx->ctx.bytes_reserved; break;
    case 5: *out = ctx->ctx.local_quotient_fallbacks; break;
    case 6: *out = ctx->ctx.pow_hints_accepted; break;
    case 7: *out = ctx->ctx.pow_hints_rejected; break;
    case 8: *out = ctx->ctx.pow_host_grinds; break;
    case 9: *out = ctx->ctx.poison_fills; break;
    case 11: *out = ctx->ctx.live_blocks.size(); break;  // (10 stays unknown)
    default: return TS_ERR_INVALID;
    }
    return TS_OK;
}

ts_status ts_bench_alu(ts_ctx* ctx, int kind, double* units_per_second) {
    if (!ctx || !units_per_second) return TS_ERR_INVALID;
    return guard(ctx, [&] { *units_per_second = ts::alu_ceiling(ctx->ctx, kind); });
}

ts_status ts_bench_stage(ts_ctx* ctx, int stage, unsigned log_n, uint32_t width, unsigned log_blowup,
                         uint32_t reps, double* ms_per_rep) {
    if (!ctx || !ms_per_rep) return TS_ERR_INVALID;
    return guard(ctx, [&] { *ms_per_rep = ts::bench_stage(ctx->ctx, stage, log_n, width, log_blowup, reps); });
}

// pinned host memory for traces handed over as host buffers (PCIe at full rate, truly async copies)
ts_status ts_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return TS_ERR_INVALID;
    *out = nullptr;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? TS_OK : TS_ERR_OOM;
}
void ts_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

// ------------------------------------------------------------------ matrices
// a new handle that owns `m`
static ts_matrix* new_matrix(ts::DeviceMatrix m) {
    auto h = std::make_unique<ts_matrix>();
    h->m = std::move(m);
    return h.release();
}
static ts_status matrix_from(ts_ctx* ctx, const uint32_t* src, uint64_t height, uint32_t width,
                             hipMemcpyKind kind, ts_matrix** out, bool sync = true) {
    if (!ctx || !out) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        TS_REQUIRE(src && height >= 1 && width >= 1, ts::TS_ERR_INVALID, "matrix: empty");
        TS_REQUIRE((height & (height - 1)) == 0, ts::TS_ERR_INVALID, "matrix: height must be a power of two");
        TS_REQUIRE(height <= (1ull << 27), ts::TS_ERR_INVALID, "matrix: height > 2^27");
        auto m = std::make_unique<ts_matrix>();
        m->m.buf = ts::DevBuf<uint32_t>(&ctx->ctx, (size_t)height * width);
        m->m.height = height;
        m->m.width = width;
        m->m.layout = ts::DeviceMatrix::ROW_MAJOR;
        TS_HIP(hipMemcpyAsync(m->m.buf.p, src, (size_t)height * width * 4, kind, ctx->ctx.stream));
        if (sync) ctx->ctx.sync();
        *out = m.release();
    });
}
ts_status ts_matrix_upload(ts_ctx* ctx, const uint32_t* host, uint64_t height, uint32_t width,
                           ts_matrix** out) {
    return matrix_from(ctx, host, height, width, hipMemcpyHostToDevice, out);
}
ts_status ts_matrix_upload_async(ts_ctx* ctx, const uint32_t* host_pinned, uint64_t height,
                                 uint32_t width, ts_matrix** out) {
    return matrix_from(ctx, host_pinned, height, width, hipMemcpyHostToDevice, out, false);
}
ts_status ts_matrix_from_device(ts_ctx* ctx, const uint32_t* dev, uint64_t height, uint32_t width,
                                ts_matrix** out) {
    return matrix_from(ctx, dev, height, width, hipMemcpyDeviceToDevice, out);
}
// ---- traces in the host's own form (ts_trace_format; kernels in ingest.hip)
// every check of a format, and its offsets and size; host only
static ts::IngestPlan load_format(const ts_trace_format* f, uint64_t height, uint32_t width) {
    TS_REQUIRE(f != nullptr, ts::TS_ERR_INVALID, "null trace format");
    TS_REQUIRE(f->struct_size == sizeof(ts_trace_format), ts::TS_ERR_INVALID,
               "ts_trace_format.struct_size is not sizeof(ts_trace_format)");
    TS_REQUIRE(f->reserved == 0, ts::TS_ERR_INVALID, "ts_trace_format.reserved must be 0");
    TS_REQUIRE(f->layout == TS_LAYOUT_ROWS || f->layout == TS_LAYOUT_PLANAR, ts::TS_ERR_INVALID,
               "trace format: unknown layout");
    return ts::ingest_plan(f->kinds, f->n_kinds, f->layout == TS_LAYOUT_PLANAR, f->row_stride_bytes, height, width);
}
ts_status ts_trace_format_bytes(const ts_trace_format* format, uint64_t height, uint32_t width, uint64_t* bytes) {
    if (!bytes) return TS_ERR_INVALID;
    *bytes = 0;
    return guard(nullptr, [&] { *bytes = load_format(format, height, width).bytes; });
}
static ts_status matrix_from_packed(ts_ctx* ctx, const void* src, const ts_trace_format* format, uint64_t height,
                                    uint32_t width, hipMemcpyKind kind, ts_matrix** out, bool sync = true) {
    if (!ctx || !out) return TS_ERR_INVALID;
    *out = nullptr;
    ts::IngestPlan plan;
    const ts_status refused = guard(ctx, [&] {
        plan = load_format(format, height, width);
        TS_REQUIRE(src != nullptr, ts::TS_ERR_INVALID, "packed trace: null buffer");
        TS_REQUIRE(((uintptr_t)src & 15) == 0, ts::TS_ERR_INVALID, "packed trace: the buffer is not 16-byte aligned");
    }, false);
    if (refused) return refused;
    return guard(ctx, [&] {
        auto m = std::make_unique<ts_matrix>();
        m->m.buf = ts::DevBuf<uint32_t>(&ctx->ctx, (size_t)height * width);
        m->m.height = height;
        m->m.width = width;
        m->m.layout = ts::DeviceMatrix::ROW_MAJOR;
        if (plan.uniform4 >= 0) {  // the source is the matrix, word for word
            TS_HIP(hipMemcpyAsync(m->m.buf.p, src, plan.bytes, kind, ctx->ctx.stream));
            if (plan.uniform4 != ts::COL_U32)
                ts::launch_scale_words(ctx->ctx, m->m.buf.p, m->m.buf.p, (uint64_t)height * width,
                                       ts::monty_ingest_factor(plan.uniform4));
        } else {
            // a host buffer is staged in the pool; the pool hands a freed block only to later work on this
            // stream, so releasing it at the end of this scope cannot take it from under the kernel
            ts::DevBuf<uint8_t> staging;
            const uint8_t* d_src = static_cast<const uint8_t*>(src);
            if (kind != hipMemcpyDeviceToDevice) {
                staging = ts::DevBuf<uint8_t>(&ctx->ctx, plan.bytes);
                TS_HIP(hipMemcpyAsync(staging.p, src, plan.bytes, kind, ctx->ctx.stream));
                d_src = staging.p;
            }
            ts::launch_ingest(ctx->ctx, plan, d_src, m->m.buf.p);
        }
        if (sync) ctx->ctx.sync();
        *out = m.release();
    });
}
ts_status ts_matrix_upload_packed(ts_ctx* ctx, const void* host, const ts_trace_format* format, uint64_t height,
                                  uint32_t width, ts_matrix** out) {
    return matrix_from_packed(ctx, host, format, height, width, hipMemcpyHostToDevice, out);
}
ts_status ts_matrix_upload_packed_async(ts_ctx* ctx, const void* host_pinned, const ts_trace_format* format,
                                        uint64_t height, uint32_t width, ts_matrix** out) {
    return matrix_from_packed(ctx, host_pinned, format, height, width, hipMemcpyHostToDevice, out, false);
}
ts_status ts_matrix_from_device_packed(ts_ctx* ctx, const void* dev, const ts_trace_format* format, uint64_t height,
                                       uint32_t width, ts_matrix** out) {
    return matrix_from_packed(ctx, dev, format, height, width, hipMemcpyDeviceToDevice, out);
}
static ts_status generated_matrix(ts_ctx* ctx, uint64_t height, uint32_t width, ts_matrix** out,
                                  const std::function<void(uint32_t*)>& fill) {
    if (!ctx || !out || height == 0 || width == 0) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        TS_REQUIRE((height & (height - 1)) == 0, ts::TS_ERR_INVALID, "trace height must be a power of two");
        auto m = std::make_unique<ts_matrix>();
        m->m.buf = ts::DevBuf<uint32_t>(&ctx->ctx, (size_t)height * width);
        m->m.height = height;
        m->m.width = width;
        m->m.layout = ts::DeviceMatrix::ROW_MAJOR;
        fill(m->m.buf.p);
        *out = m.release();
    });
}
ts_status ts_trace_fibonacci(ts_ctx* ctx, uint32_t a, uint32_t b, uint64_t n, ts_matrix** out) {
    return generated_matrix(ctx, n, 2, out,
                            [&](uint32_t* p) { ts::launch_trace_fibonacci(ctx->ctx, p, a, b, n); });
}
ts_status ts_trace_synth_mul(ts_ctx* ctx, uint64_t n, uint32_t width, uint64_t seed, ts_matrix** out) {
    return generated_matrix(ctx, n, width, out,
                            [&](uint32_t* p) { ts::launch_trace_synth_mul(ctx->ctx, p, n, width, seed); });
}
ts_status ts_trace_synth_ext(ts_ctx* ctx, uint64_t n, uint32_t width, uint64_t seed, ts_matrix** out) {
    return generated_matrix(ctx, n, width, out,
                            [&](uint32_t* p) { ts::launch_trace_synth_ext(ctx->ctx, p, n, width, seed); });
}
ts_status ts_matrix_dims(const ts_matrix* m, uint64_t* height, uint32_t* width) {
    if (!m) return TS_ERR_INVALID;
    if (height) *height = m->m.height;
    if (width) *width = m->m.width;
    return TS_OK;
}
ts_status ts_matrix_download(ts_ctx* ctx, const ts_matrix* m, uint32_t* host) {
    if (!ctx || !m || !host) return TS_ERR_INVALID;
    return guard(ctx, [&] {
        TS_REQUIRE(m->m.buf.p, ts::TS_ERR_INVALID, "matrix was consumed");
        const size_t words = (size_t)m->m.height * m->m.width;
        if (m->m.layout == ts::DeviceMatrix::ROW_MAJOR) {
            TS_HIP(hipMemcpyAsync(host, m->m.buf.p, words * 4, hipMemcpyDeviceToHost, ctx->ctx.stream));
            ctx->ctx.sync();
        } else {
            // column-major with bit-reversed rows -> row-major natural
            ts::DevBuf<uint32_t> rm(&ctx->ctx, words);
            ts::launch_transpose_to_row_major(ctx->ctx, m->m.buf.p, m->m.height, rm.p, m->m.height,
                                              m->m.width);
            std::vector<uint32_t> tmp(words);
            TS_HIP(hipMemcpyAsync(tmp.data(), rm.p, words * 4, hipMemcpyDeviceToHost, ctx->ctx.stream));
            ctx->ctx.sync();
            unsigned bits = 0;
            while ((1ull << bits) < m->m.height) bits++;
            for (uint64_t r = 0; r < m->m.height; r++) {
                uint64_t nat = ts::bitrev32((uint32_t)r, bits);
                memcpy(host + nat * m->m.width, tmp.data() + r * m->m.width, (size_t)m->m.width * 4);
            }
        }
    });
}
void ts_matrix_free(ts_ctx* ctx, ts_matrix* m) {
    (void)ctx;
    delete m;
}

// ------------------------------------------------------------------ transforms on device matrices
// (TwoAdicSubgroupDft; kernels in ntt_dft.hip).  The input is only read.
namespace {

std::unique_ptr<ts_matrix> new_row_major(ts_ctx* ctx, uint64_t height, uint32_t width) {
    auto m = std::make_unique<ts_matrix>();
    m->m.buf = ts::DevBuf<uint32_t>(&ctx->ctx, (size_t)height * width);
    m->m.height = height;
    m->m.width = width;
    m->m.layout = ts::DeviceMatrix::ROW_MAJOR;
    return m;
}

// the matrix as row-major words with natural rows: its own buffer, or -- for one made on the device in
// column-major form (quotient chunks) -- a copy in `tmp`
const uint32_t* row_major_words(ts_ctx* ctx, const ts::DeviceMatrix& m, ts::DevBuf<uint32_t>& tmp) {
    TS_REQUIRE(m.buf.p, ts::TS_ERR_INVALID, "matrix was consumed");
    if (m.layout == ts::DeviceMatrix::ROW_MAJOR) return m.buf.p;
    tmp = ts::DevBuf<uint32_t>(&ctx->ctx, (size_t)m.height * m.width);
    ts::launch_transpose_unbitrev(ctx->ctx, m.buf.p, m.height, tmp.p, ts::log2_strict(m.height), m.width);
    return tmp.p;
}

void check_shift(uint32_t shift) {
    TS_REQUIRE(shift != 0 && shift < ts::P, ts::TS_ERR_INVALID, "coset shift must be in [1, p)");
}

}  // namespace

ts_status ts_dft_batch(ts_ctx* ctx, const ts_matrix* in, int inverse, uint32_t shift, ts_matrix** out) {
    if (!ctx || !in || !out) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        check_shift(shift);
        const unsigned log_n = ts::log2_strict(in->m.height);
        TS_REQUIRE(log_n <= 26, ts::TS_ERR_INVALID, "dft: height above 2^26, the tallest matrix ts_pcs_commit accepts");
        ts::DevBuf<uint32_t> tmp;
        const uint32_t* src = row_major_words(ctx, in->m, tmp);
        auto m = new_row_major(ctx, in->m.height, in->m.width);
        if (log_n == 0)  // one point: the polynomial is its value
            TS_HIP(hipMemcpyAsync(m->m.buf.p, src, (size_t)in->m.width * 4, hipMemcpyDeviceToDevice, ctx->ctx.stream));
        else
            ts::dft_batch(ctx->ctx, src, m->m.buf.p, log_n, in->m.width, inverse != 0, shift);
        *out = m.release();
    });
}

ts_status ts_coset_lde_batch(ts_ctx* ctx, const ts_matrix* in, uint32_t added_bits, uint32_t shift, int bit_reversed,
                             ts_matrix** out) {
    if (!ctx || !in || !out) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        check_shift(shift);
        const unsigned log_n = ts::log2_strict(in->m.height);
        TS_REQUIRE(added_bits <= 27 && log_n + added_bits <= 27, ts::TS_ERR_INVALID,
                   "coset_lde_batch: result above 2^27 rows, the tallest LDE ts_pcs_commit makes");
        ts::DevBuf<uint32_t> tmp;
        const uint32_t* src = row_major_words(ctx, in->m, tmp);
        auto m = new_row_major(ctx, in->m.height << added_bits, in->m.width);
        ts::coset_lde_batch(ctx->ctx, src, m->m.buf.p, log_n, in->m.width, added_bits, shift, bit_reversed != 0);
        *out = m.release();
    });
}

ts_status ts_matrix_bit_reverse_rows(ts_ctx* ctx, const ts_matrix* in, ts_matrix** out) {
    if (!ctx || !in || !out) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        const unsigned log_h = ts::log2_strict(in->m.height);
        ts::DevBuf<uint32_t> tmp;
        const uint32_t* src = row_major_words(ctx, in->m, tmp);
        auto m = new_row_major(ctx, in->m.height, in->m.width);
        ts::launch_bit_reverse_rows(ctx->ctx, src, m->m.buf.p, log_h, in->m.width);
        *out = m.release();
    });
}

ts_status ts_matrix_device_ptr(ts_ctx* ctx, ts_matrix* m, const uint32_t** ptr) {
    if (!ctx || !m || !ptr) return TS_ERR_INVALID;
    *ptr = nullptr;
    return guard(ctx, [&] {
        TS_REQUIRE(m->m.buf.p, ts::TS_ERR_INVALID, "matrix was consumed");
        if (m->m.layout != ts::DeviceMatrix::ROW_MAJOR) {
            // made on the device in column-major form: the handle takes the row-major copy (same values)
            ts::DevBuf<uint32_t> tmp;
            row_major_words(ctx, m->m, tmp);
            m->m.buf = std::move(tmp);
            m->m.layout = ts::DeviceMatrix::ROW_MAJOR;
        }
        *ptr = m->m.buf.p;
    });
}

// (after row_major_words: a matrix made on the device in column-major form downloads the same way)
ts_status ts_matrix_download_monty(ts_ctx* ctx, const ts_matrix* m, uint32_t monty_bits, uint32_t* host) {
    if (!ctx || !m || !host) return TS_ERR_INVALID;
    const ts_status refused = guard(ctx, [&] {
        TS_REQUIRE(monty_bits == 31 || monty_bits == 32, ts::TS_ERR_INVALID, "download: monty_bits must be 31 or 32");
    }, false);
    if (refused) return refused;
    return guard(ctx, [&] {
        ts::DevBuf<uint32_t> tmp;
        const uint32_t* src = row_major_words(ctx, m->m, tmp);
        const size_t words = (size_t)m->m.height * m->m.width;
        // value * 2^bits = mont_mul(value, 2^(32 + bits) mod p)
        constexpr uint32_t TWO_63_MOD_P = 0x5eeeeef2u;
        ts::DevBuf<uint32_t> mont(&ctx->ctx, words);
        ts::launch_scale_words(ctx->ctx, src, mont.p, words, monty_bits == 32 ? ts::R2_MOD_P : TWO_63_MOD_P);
        TS_HIP(hipMemcpyAsync(host, mont.p, words * 4, hipMemcpyDeviceToHost, ctx->ctx.stream));
        ctx->ctx.sync();
    });
}

// ------------------------------------------------------------------ AIR
// ctx == NULL: a host-only AIR (no GPU needed), usable by ts_verify
static ts_status air_compile(ts_ctx* ctx, const uint32_t* tape, size_t n_words, uint32_t segment_instr,
                             uint32_t jit_jobs, ts_air** out) {
    if (!out) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] { *out = new ts_air{{ctx ? &ctx->ctx : nullptr, tape, n_words, segment_instr, jit_jobs}}; });
}
ts_status ts_air_compile(ts_ctx* ctx, const uint32_t* tape, size_t n_words, ts_air** out) {
    return air_compile(ctx, tape, n_words, 0, 0, out);
}
ts_status ts_air_compile_opts(ts_ctx* ctx, const uint32_t* tape, size_t n_words, const ts_air_options* opt,
                              ts_air** out) {
    if (opt && (opt->struct_size != sizeof(ts_air_options) || opt->reserved != 0)) return TS_ERR_INVALID;
    return air_compile(ctx, tape, n_words, opt ? opt->segment_instr : 0, opt ? std::min(opt->jit_jobs, 8u) : 0, out);
}
int ts_air_is_jit(const ts_air* air) { return air && const_cast<ts_air*>(air)->a.is_specialised() ? 1 : 0; }
ts_status ts_air_jit_wait(ts_ctx* ctx, ts_air* air, int* state, double* compile_seconds) {
    if (!ctx || !air) return TS_ERR_INVALID;
    return guard(ctx, [&] {
        const auto [st, seconds] = air->a.wait();
        if (state) *state = st;
        if (compile_seconds) *compile_seconds = seconds;
    });
}
ts_status ts_air_info(const ts_air* air, uint32_t* width, uint32_t* n_public,
                      uint32_t* max_constraint_degree, uint32_t* log_quotient_degree) {
    if (!air) return TS_ERR_INVALID;
    if (width) *width = air->a.prog().width;
    if (n_public) *n_public = air->a.prog().n_public;
    if (max_constraint_degree) *max_constraint_degree = air->a.prog().max_degree;
    if (log_quotient_degree) *log_quotient_degree = air->a.prog().log_quotient_degree;
    return TS_OK;
}
ts_status ts_air_preprocessed_width(const ts_air* air, uint32_t* preprocessed_width) {
    if (!air || !preprocessed_width) return TS_ERR_INVALID;
    *preprocessed_width = air->a.prog().preprocessed_width;
    return TS_OK;
}
void ts_air_free(ts_ctx* ctx, ts_air* air) {
    (void)ctx;
    delete air;
}
ts_status ts_air_program(const ts_air* air, uint32_t* out, size_t cap_words, size_t* n_words) {
    if (!air || !n_words) return TS_ERR_INVALID;
    const ts::AirProgram& p = air->a.prog();
    const size_t nc = p.const_canonical.size();
    *n_words = 3 + p.code.size() + 2 * nc;
    if (!out || cap_words < *n_words) return TS_ERR_BUFFER;
    out[0] = p.n_regs;
    out[1] = (uint32_t)(p.code.size() / 4);
    out[2] = (uint32_t)nc;
    std::copy(p.code.begin(), p.code.end(), out + 3);
    std::copy(p.const_canonical.begin(), p.const_canonical.end(), out + 3 + p.code.size());
    std::copy(p.const_public_idx.begin(), p.const_public_idx.end(), out + 3 + p.code.size() + nc);
    return TS_OK;
}
ts_status ts_air_segment_plan(const ts_air* air, uint32_t* out, size_t cap_words, size_t* n_words) {
    if (!air || !n_words || !air->a.seg()) return TS_ERR_INVALID;
    const ts::SegmentPlan& sp = *air->a.seg();
    std::vector<uint32_t> w = {sp.slab_width, (uint32_t)sp.segs.size()};
    for (const auto& sg : sp.segs) {
        w.insert(w.end(), {sg.begin, sg.end, (uint32_t)sg.live_in.size(), (uint32_t)sg.live_out.size(), sg.pressure});
        for (const auto& v : sg.live_in) w.insert(w.end(), {v.def, v.slot});
        for (const auto& v : sg.live_out) w.insert(w.end(), {v.def, v.slot});
    }
    *n_words = w.size();
    if (!out || cap_words < w.size()) return TS_ERR_BUFFER;
    std::copy(w.begin(), w.end(), out);
    return TS_OK;
}
ts_status ts_air_jit_source(const ts_air* air, char* buf, size_t cap, size_t* n_bytes) {
    if (!air || !n_bytes) return TS_ERR_INVALID;
    return guard(nullptr, [&] {
        const std::string src = air->a.source();
        *n_bytes = src.size();
        TS_REQUIRE(buf && cap >= src.size(), ts::TS_ERR_BUFFER, "jit source buffer too small");
        memcpy(buf, src.data(), src.size());
    });
}
ts_status ts_air_jit_compile(const ts_air* air, const char* arch, void* code_out, size_t cap, size_t* n_bytes,
                             double* seconds) {
    if (!air || !arch || !n_bytes) return TS_ERR_INVALID;
    return guard(nullptr, [&] {
        std::vector<char> code;
        std::string log;
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = ts::jit_compile_source(air->a.source(), arch, code, log);
        if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        TS_REQUIRE(ok, ts::TS_ERR_UNSUPPORTED, ("hiprtc: " + log).c_str());
        *n_bytes = code.size();
        TS_REQUIRE(code_out && cap >= code.size(), ts::TS_ERR_BUFFER, "code object buffer too small");
        memcpy(code_out, code.data(), code.size());
    });
}

// ------------------------------------------------------------------ PCS
ts_status ts_pcs_commit(ts_ctx* ctx, const ts_fri_config* cfg, uint32_t n_mats, ts_matrix* const* evals,
                        const uint32_t* domain_shifts, uint32_t root_out[8], ts_pcs_data** out) {
    if (!ctx || !out || !evals || !domain_shifts) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        ts::TwoAdicFriPcs pcs(ctx->ctx, load_cfg(cfg));
        TS_REQUIRE(n_mats >= 1 && n_mats <= (uint32_t)ts::MAX_BATCH_MATS, ts::TS_ERR_INVALID,
                   "commit: between 1 and 64 matrices");
        std::vector<ts::DeviceMatrix> ms;
        for (uint32_t i = 0; i < n_mats; i++) {
            TS_REQUIRE(evals[i] && evals[i]->m.buf.p, ts::TS_ERR_INVALID, "commit: null or consumed matrix");
            ms.push_back(std::move(evals[i]->m));
        }
        std::vector<uint32_t> shifts(domain_shifts, domain_shifts + n_mats);
        auto d = std::make_unique<ts_pcs_data>();
        d->d = pcs.commit(ms, shifts);
        if (root_out) memcpy(root_out, d->d->root, 32);
        *out = d.release();
    });
}
ts_status ts_mmcs_commit(ts_ctx* ctx, uint32_t n_mats, ts_matrix* const* mats, uint32_t root_out[8],
                         ts_pcs_data** out) {
    if (!ctx || !out || !mats) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        TS_REQUIRE(n_mats >= 1 && n_mats <= (uint32_t)ts::MAX_BATCH_MATS, ts::TS_ERR_INVALID,
                   "mmcs commit: between 1 and 64 matrices");
        auto d = std::make_unique<ts_pcs_data>();
        d->d = std::make_unique<ts::PcsData>();
        uint64_t max_h = 0;
        for (uint32_t i = 0; i < n_mats; i++) {
            TS_REQUIRE(mats[i] && mats[i]->m.buf.p, ts::TS_ERR_INVALID, "mmcs commit: null or consumed matrix");
            TS_REQUIRE(mats[i]->m.layout == ts::DeviceMatrix::ROW_MAJOR, ts::TS_ERR_INVALID,
                       "mmcs commit: row-major (uploaded) matrices expected");
            max_h = std::max(max_h, mats[i]->m.height);
        }
        d->d->log_height = ts::log2_strict(max_h);
        for (uint32_t i = 0; i < n_mats; i++) {
            ts::DeviceMatrix& m = mats[i]->m;
            ts::DevBuf<uint32_t> cmaj(&ctx->ctx, (size_t)m.height * m.width);
            ts::launch_transpose_plain(ctx->ctx, m.buf.p, cmaj.p, m.height, m.width, m.height);
            ts::ColMat cm;
            cm.d = cmaj.p;
            cm.height = m.height;
            cm.width = m.width;
            cm.col_stride = m.height;
            d->d->ldes.push_back(cm);
            d->d->lde_storage.push_back(std::move(cmaj));
            m.buf.reset();  // consumed, like the moved RowMajorMatrix arguments
        }
        ts::mmcs_commit(ctx->ctx, *d->d);
        if (root_out) memcpy(root_out, d->d->root, 32);
        *out = d.release();
    });
}
ts_status ts_pcs_data_info(const ts_pcs_data* d, uint32_t* n_mats, uint32_t* log_height) {
    if (!d || !d->d) return TS_ERR_INVALID;
    if (n_mats) *n_mats = (uint32_t)d->d->ldes.size();
    if (log_height) *log_height = d->d->log_height;
    return TS_OK;
}
ts_status ts_pcs_data_lde(ts_ctx* ctx, const ts_pcs_data* d, uint32_t idx, uint32_t* host) {
    if (!ctx || !d || !d->d || !host) return TS_ERR_INVALID;
    return guard(ctx, [&] {
        TS_REQUIRE(idx < d->d->ldes.size(), ts::TS_ERR_INVALID, "lde index out of range");
        const ts::ColMat& cm = d->d->ldes[idx];
        const size_t words = (size_t)cm.height * cm.width;
        ts::DevBuf<uint32_t> rm(&ctx->ctx, words);
        ts::launch_transpose_to_row_major(ctx->ctx, cm.d, cm.col_stride, rm.p, cm.height, cm.width);
        TS_HIP(hipMemcpyAsync(host, rm.p, words * 4, hipMemcpyDeviceToHost, ctx->ctx.stream));
        ctx->ctx.sync();
    });
}
ts_status ts_pcs_data_evaluations_on_domain(ts_ctx* ctx, const ts_pcs_data* d, uint32_t idx, uint32_t log_size,
                                            ts_matrix** out) {
    if (!ctx || !d || !d->d || !out) return TS_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        TS_REQUIRE(idx < d->d->ldes.size(), ts::TS_ERR_INVALID, "evaluations_on_domain: matrix index out of range");
        const ts::ColMat& cm = d->d->ldes[idx];
        // two_adic_pcs.rs:256: assert!(lde.height() >= domain.size())
        TS_REQUIRE(log_size <= 27 && (1ull << log_size) <= cm.height, ts::TS_ERR_INVALID,
                   "evaluations_on_domain: domain larger than the committed LDE");
        auto m = new_row_major(ctx, 1ull << log_size, cm.width);
        // :257 lde.split_rows(domain.size()).0.bit_reverse_rows()
        ts::launch_transpose_unbitrev(ctx->ctx, cm.d, cm.col_stride, m->m.buf.p, log_size, cm.width);
        *out = m.release();
    });
}
ts_status ts_pcs_data_matrix_info(const ts_pcs_data* d, uint32_t idx, uint64_t* height, uint32_t* width) {
    if (!d || !d->d || idx >= d->d->ldes.size()) return TS_ERR_INVALID;
    if (height) *height = d->d->ldes[idx].height;
    if (width) *width = d->d->ldes[idx].width;
    return TS_OK;
}
ts_status ts_pcs_data_digests(ts_ctx* ctx, const ts_pcs_data* d, uint32_t level, uint32_t* host) {
    if (!ctx || !d || !d->d || !host) return TS_ERR_INVALID;
    return guard(ctx, [&] {
        TS_REQUIRE(level <= d->d->log_height, ts::TS_ERR_INVALID, "digest level out of range");
        const uint64_t off = ts::merkle_level_offset(d->d->log_height, level);
        const uint64_t cnt = 1ull << (d->d->log_height - level);
        TS_HIP(hipMemcpyAsync(host, d->d->tree.p + 8 * off, cnt * 32, hipMemcpyDeviceToHost, ctx->ctx.stream));
        ctx->ctx.sync();
    });
}
ts_status ts_pcs_open_batch(ts_ctx* ctx, const ts_pcs_data* d, uint64_t index, uint32_t* rows_out,
                            uint32_t* path_out) {
    if (!ctx || !d || !d->d || !rows_out || !path_out) return TS_ERR_INVALID;
    return guard(ctx, [&] {
        ts::TwoAdicFriPcs pcs(ctx->ctx, ts::FriConfig{});
        std::vector<uint32_t> rows, path;
        pcs.open_batch(*d->d, index, rows, path);
        memcpy(rows_out, rows.data(), rows.size() * 4);
        memcpy(path_out, path.data(), path.size() * 4);
    });
}
void ts_pcs_data_free(ts_ctx* ctx, ts_pcs_data* d) {
    (void)ctx;
    delete d;
}

// What every ts_quotient_chunks* call does after its own admission rule: `side` holds the committed side matrices
// it admitted, key first, then aux; `challenges` and `exposed` are null for a call that takes none.
static void quotient_chunks(ts_ctx* ctx, const ts::AirProgram& p, const ts::SideData& side,
                            const ts_pcs_data* trace_data, uint32_t log_blowup, const uint32_t* public_values,
                            uint32_t n_public, const uint32_t* challenges, const uint32_t* exposed,
                            const uint32_t alpha[4], ts_matrix** chunks_out) {
    ts_fri_config raw{log_blowup, 1, 0};
    ts::TwoAdicFriPcs pcs(ctx->ctx, load_cfg(&raw));  // same [1, 8] bound as everywhere else
    const std::vector<uint32_t> pis = public_slots(p, public_values, n_public, challenges, exposed);
    auto chunks = pcs.quotient_chunks(*trace_data->d, p, pis, load_ef(alpha), side);
    for (size_t c = 0; c < chunks.size(); c++) chunks_out[c] = new_matrix(std::move(chunks[c]));
}
// The head of the four calls: the admission, then the side matrices the format takes, key first (the quotient over
// (key, aux, trace)).  `key`, `aux_data`, `challenges` and `exposed` are null from a call that has no such argument.
static ts_status single_quotient_chunks(const SingleCall& sc, ts_ctx* ctx, const ts_pcs_data* key,
                                        const ts_pcs_data* aux_data, const ts_pcs_data* trace_data, uint32_t log_blowup,
                                        const ts_air* air, const uint32_t* public_values, uint32_t n_public,
                                        const uint32_t* challenges, const uint32_t* exposed, const uint32_t alpha[4],
                                        ts_matrix** chunks_out) {
    if (!ctx || !trace_data || !trace_data->d || !air || !alpha || !chunks_out) {
        if (ctx) ctx->ctx.last_error = sc.name("quotient_chunks") + ": null argument";
        return TS_ERR_INVALID;
    }
    return guard(ctx, [&] {
        const std::string call = sc.keyed_name("quotient_chunks");
        admit_air(sc, air, call);
        ts::SideData side;
        if (const ts::PcsData* k = sc.key ? preprocessed_key_any(ctx, air, key, call.c_str()) : nullptr) side.push_back(k);
        const ts::AirProgram& p = ready_prog(air);
        if (const ts::PcsData* a = sc.aux ? committed_aux(ctx, p, aux_data) : nullptr) side.push_back(a);
        quotient_chunks(ctx, p, side, trace_data, log_blowup, public_values, n_public, challenges, exposed, alpha,
                        chunks_out);
    });
}
ts_status ts_quotient_chunks(ts_ctx* ctx, const ts_pcs_data* trace_data, uint32_t log_blowup,
                             const ts_air* air, const uint32_t* public_values, uint32_t n_public,
                             const uint32_t alpha[4], ts_matrix** chunks_out) {
    return single_quotient_chunks(PLAIN, ctx, nullptr, nullptr, trace_data, log_blowup, air, public_values, n_public,
                                  nullptr, nullptr, alpha, chunks_out);
}
ts_status ts_quotient_chunks_pre(ts_ctx* ctx, const ts_pcs_data* preprocessed, const ts_pcs_data* trace_data,
                                 uint32_t log_blowup, const ts_air* air, const uint32_t* public_values,
                                 uint32_t n_public, const uint32_t alpha[4], ts_matrix** chunks_out) {
    return single_quotient_chunks(PRE, ctx, preprocessed, nullptr, trace_data, log_blowup, air, public_values, n_public,
                                  nullptr, nullptr, alpha, chunks_out);
}
ts_status ts_quotient_chunks_aux(ts_ctx* ctx, const ts_pcs_data* aux_data, const ts_pcs_data* trace_data,
                                 uint32_t log_blowup, const ts_air* air, const uint32_t* public_values,
                                 uint32_t n_public, const uint32_t* challenges, const uint32_t* exposed,
                                 const uint32_t alpha[4], ts_matrix** chunks_out) {
    return single_quotient_chunks(AUX, ctx, nullptr, aux_data, trace_data, log_blowup, air, public_values, n_public,
                                  challenges, exposed, alpha, chunks_out);
}
ts_status ts_quotient_chunks_pre_aux(ts_ctx* ctx, const ts_pcs_data* key, const ts_pcs_data* aux_data,
                                     const ts_pcs_data* trace_data, uint32_t log_blowup, const ts_air* air,
                                     const uint32_t* public_values, uint32_t n_public, const uint32_t* challenges,
                                     const uint32_t* exposed, const uint32_t alpha[4], ts_matrix** chunks_out) {
    return single_quotient_chunks(PRE_AUX, ctx, key, aux_data, trace_data, log_blowup, air, public_values, n_public,
                                  challenges, exposed, alpha, chunks_out);
}

ts_status ts_pcs_open_reduce(ts_ctx* ctx, const ts_fri_config* cfg, const ts_pcs_data* trace_data,
                             const ts_pcs_data* quotient_data, const uint32_t zeta[4],
                             const uint32_t batch_alpha[4], uint32_t* opened_out, uint32_t* reduced_out) {
    if (!ctx || !trace_data || !trace_data->d || !quotient_data || !quotient_data->d || !zeta ||
        !batch_alpha || !opened_out)
        return TS_ERR_INVALID;
    return guard(ctx, [&] {
        ts::TwoAdicFriPcs pcs(ctx->ctx, load_cfg(cfg));
        std::vector<ts::Ef> opened;
        ts::DevBuf<ts::Ef> ro =
            pcs.open_reduce(*trace_data->d, *quotient_data->d, load_ef(zeta), load_ef(batch_alpha), opened);
        memcpy(opened_out, opened.data(), opened.size() * sizeof(ts::Ef));
        if (reduced_out) {
            TS_HIP(hipMemcpyAsync(reduced_out, ro.p, ro.n * sizeof(ts::Ef), hipMemcpyDeviceToHost,
                                  ctx->ctx.stream));
            ctx->ctx.sync();
        }
    });
}

ts_status ts_pcs_open(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal, uint32_t n_rounds,
                      const ts_pcs_data* const* rounds, const uint32_t* n_points,
                      const uint32_t* points, uint32_t* opened_out, size_t opened_cap_words,
                      size_t* n_opened_words, uint32_t* proof_out, size_t proof_cap_words,
                      size_t* n_proof_words) {
    if (!ctx || !chal || !rounds || !n_points || !opened_out || !n_opened_words || !proof_out ||
        !n_proof_words || n_rounds == 0)
        return TS_ERR_INVALID;
    *n_opened_words = *n_proof_words = 0;
    return guard(ctx, [&] {
        ts::TwoAdicFriPcs pcs(ctx->ctx, load_cfg(cfg));
        std::vector<ts::TwoAdicFriPcs::OpenRound> rs(n_rounds);
        size_t k = 0, pw = 0;
        for (uint32_t r = 0; r < n_rounds; r++) {
            TS_REQUIRE(rounds[r] && rounds[r]->d, ts::TS_ERR_INVALID, "open: null round data");
            rs[r].data = rounds[r]->d.get();
            rs[r].points.resize(rs[r].data->ldes.size());
            for (auto& pl : rs[r].points) {
                const uint32_t np = n_points[k++];
                TS_REQUIRE(np == 0 || points, ts::TS_ERR_INVALID, "open: null points");
                for (uint32_t p = 0; p < np; p++, pw += 4) {
                    for (int j = 0; j < 4; j++)
                        TS_REQUIRE(points[pw + j] < ts::P, ts::TS_ERR_INVALID, "open: non-canonical point");
                    pl.push_back(load_ef(points + pw));
                }
            }
        }
        std::vector<ts::Ef> opened;
        std::vector<uint32_t> proof = pcs.open(rs, chal->c, opened);
        *n_opened_words = opened.size() * 4;
        copy_proof(proof, proof_out, proof_cap_words, n_proof_words);
        TS_REQUIRE(opened.size() * 4 <= opened_cap_words, ts::TS_ERR_BUFFER, "opened-values buffer too small");
        memcpy(opened_out, opened.data(), opened.size() * sizeof(ts::Ef));
    });
}

ts_status ts_fri_prove(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal, uint32_t n_inputs,
                       const uint32_t* log_lens, const uint32_t* const* inputs, uint32_t* proof_out,
                       size_t cap_words, size_t* n_words_out) {
    if (!ctx || !chal || !log_lens || !inputs || !proof_out || !n_words_out || n_inputs == 0 || n_inputs > 32)
        return TS_ERR_INVALID;
    *n_words_out = 0;
    return guard(ctx, [&] {
        ts::TwoAdicFriPcs pcs(ctx->ctx, load_cfg(cfg));
        std::vector<ts::DevBuf<ts::Ef>> in;
        std::vector<unsigned> logs;
        for (uint32_t k = 0; k < n_inputs; k++) {
            TS_REQUIRE(inputs[k] && log_lens[k] <= 27, ts::TS_ERR_INVALID, "fri_prove: bad input");
            const size_t len = (size_t)1 << log_lens[k];
            for (size_t i = 0; i < 4 * len; i++)
                TS_REQUIRE(inputs[k][i] < ts::P, ts::TS_ERR_INVALID, "fri_prove: non-canonical element");
            ts::DevBuf<ts::Ef> d(&ctx->ctx, len);
            TS_HIP(hipMemcpyAsync(d.p, inputs[k], len * sizeof(ts::Ef), hipMemcpyHostToDevice, ctx->ctx.stream));
            in.push_back(std::move(d));
            logs.push_back(log_lens[k]);
        }
        ctx->ctx.sync();
        std::vector<uint32_t> pf;
        pcs.fri_prove(in, logs, chal->c, {}, pf, /*pass_through=*/true);
        copy_proof(pf, proof_out, cap_words, n_words_out);
    });
}
ts_status ts_fri_verify(const ts_fri_config* cfg, ts_challenger* chal, const uint32_t* proof,
                        size_t n_words, int* verdict) {
    if (!chal || !proof || !verdict) return TS_ERR_INVALID;
    *verdict = 9;
    return guard(nullptr, [&] {
        *verdict = ts::fri_verify_pass_through(load_cfg(cfg), chal->c, proof, n_words);
    });
}

ts_status ts_fri_fold(ts_ctx* ctx, const uint32_t* in, uint64_t h, const uint32_t beta[4], uint32_t* out) {
    if (!ctx || !in || !beta || !out || h == 0) return TS_ERR_INVALID;
    return guard(ctx, [&] {
        ts::DevBuf<ts::Ef> d_in(&ctx->ctx, 2 * h), d_out(&ctx->ctx, h);
        TS_HIP(hipMemcpyAsync(d_in.p, in, 2 * h * 16, hipMemcpyHostToDevice, ctx->ctx.stream));
        ts::launch_fri_fold(ctx->ctx, d_in.p, h, load_ef(beta), d_out.p, nullptr);
        TS_HIP(hipMemcpyAsync(out, d_out.p, h * 16, hipMemcpyDeviceToHost, ctx->ctx.stream));
        ctx->ctx.sync();
    });
}

ts_status ts_fri_fold_device(ts_ctx* ctx, const uint32_t* in_dev, uint64_t h, const uint32_t beta[4],
                             uint32_t* out_dev) {
    if (!ctx || !in_dev || !beta || !out_dev || h == 0) return TS_ERR_INVALID;
    if (((uintptr_t)in_dev | (uintptr_t)out_dev) & 15) return TS_ERR_INVALID;  // EF4 = 16-byte accesses
    return guard(ctx, [&] {
        ts::launch_fri_fold(ctx->ctx, reinterpret_cast<const ts::Ef*>(in_dev), h, load_ef(beta),
                            reinterpret_cast<ts::Ef*>(out_dev), nullptr);
    });
}

// ------------------------------------------------------------------ challenger
ts_status ts_chal_new(int permutation, int sample_ext, ts_challenger** out) {
    if (!out || (permutation != 0 && permutation != 1)) return TS_ERR_INVALID;
    *out = new (std::nothrow) ts_challenger(permutation, sample_ext != 0);
    return *out ? TS_OK : TS_ERR_OOM;
}
ts_status ts_chal_clone(const ts_challenger* c, ts_challenger** out) {
    if (!c || !out) return TS_ERR_INVALID;
    *out = new (std::nothrow) ts_challenger(*c);
    return *out ? TS_OK : TS_ERR_OOM;
}
void ts_chal_free(ts_challenger* c) { delete c; }
// void/value returns leave no room for a status: a null handle (or out pointer) is a no-op
void ts_chal_observe(ts_challenger* c, uint32_t word) {
    if (c) c->c.observe(word);
}
void ts_chal_observe_commitment(ts_challenger* c, const uint32_t d[8]) {
    if (c && d) c->c.observe_commitment(d);
}
void ts_chal_sample(ts_challenger* c, uint32_t out[4]) {
    if (!c || !out) return;
    ts::Ef e = c->c.sample();
    memcpy(out, e.c, 16);
}
uint64_t ts_chal_sample_bits(ts_challenger* c, uint32_t bits) {
    return c && bits <= 32 ? c->c.sample_bits(bits) : 0;
}
int ts_chal_check_witness(ts_challenger* c, uint32_t bits, uint32_t witness) {
    return c && bits <= 32 && c->c.check_witness(bits, witness) ? 1 : 0;
}
ts_status ts_chal_grind(ts_challenger* c, uint32_t bits, uint32_t* witness) {
    if (!c || !witness || bits > 31) return TS_ERR_INVALID;
    try {
        *witness = c->c.grind(bits);
        return TS_OK;
    } catch (const ts::Error& e) {
        return e.code;
    }
}
void ts_chal_state(const ts_challenger* c, uint32_t out[34]) {
    if (c && out) c->c.export_state(out);
}

// (ts_prove and its three siblings: "prove, the four single-table formats" below, behind the aux callback they share)

// ------------------------------------------------------------------ prove_stream
// Throughput mode as ONE call: n_proofs independent proofs of one AIR on `n_lanes` contexts of a device, one
// host thread per lane INSIDE the call (examples/prove_stream.cpp as an entry point).  Proofs are independent
// objects (uni-stark/src/prover.rs:25-35 takes one trace), so several are kept in flight: one proof's kernels
// fill the gaps the serial transcript of another leaves.  A host whose own threads are cheap (Rust, C++)
// does this itself; a host behind an interpreter lock (the Python binding: bench.py) gets the same loop
// without taking its lock once per proof.
ts_status ts_prove_stream(ts_ctx* const* ctxs, const ts_air* const* airs, uint32_t n_lanes,
                          const ts_fri_config* cfg, ts_matrix* const* traces, const uint32_t* lane_of,
                          uint32_t n_proofs, const uint32_t* public_values, uint32_t n_public, double gate_ms,
                          uint32_t* last_proof_out, size_t cap_words, size_t* n_words_out,
                          double* start_ms_out, double* wall_ms_out) {
    if (!traces || !lane_of || !n_words_out) return TS_ERR_INVALID;
    *n_words_out = 0;
    ts::FriConfig fri;
    if (!check_lanes(ctxs, airs, n_lanes, cfg, fri)) return TS_ERR_INVALID;
    for (uint32_t i = 0; i < n_proofs; i++)
        if (!traces[i] || lane_of[i] >= n_lanes) return TS_ERR_INVALID;
    if (n_public && !public_values) return TS_ERR_INVALID;
    for (uint32_t l = 0; l < n_lanes; l++) {
        const ts_status st = guard(ctxs[l], [&] { admit_air(PLAIN, airs[l], "ts_prove_stream"); }, false);
        if (st != TS_OK) return st;
    }
    const std::vector<uint32_t> pis(public_values, public_values + n_public);
    StartGate gate(gate_ms);
    std::vector<ts_status> status(n_lanes, TS_OK);
    std::vector<std::vector<uint32_t>> last_proof(n_lanes);
    std::vector<uint32_t> last_index(n_lanes, 0);
    std::atomic<bool> stop{false};
    auto lane_main = [&](uint32_t l) {
        ts_ctx* ctx = ctxs[l];
        status[l] = guard(ctx, [&] {
            ts::TwoAdicFriPcs pcs(ctx->ctx, fri);
            for (uint32_t i = 0; i < n_proofs && !stop.load(); i++) {
                if (lane_of[i] != l) continue;
                const ts::AirProgram& prog = ready_prog(airs[l]);
                ts::DeviceMatrix trace = lane_trace(traces[i], ctx, prog);
                ts::BfChallenger chal(0, true);  // a fresh challenger per proof, as prove() is handed
                const double t0 = gate.enter();
                std::vector<uint32_t> proof = ts::prove(pcs, prog, chal, std::move(trace), pis);
                if (start_ms_out) start_ms_out[i] = t0;
                if (wall_ms_out) wall_ms_out[i] = gate.now_ms() - t0;
                last_proof[l] = std::move(proof);
                last_index[l] = i;
            }
        });
        if (status[l] != TS_OK) stop = true;
    };
    if (run_lanes(n_lanes, lane_main) != TS_OK) return TS_ERR_OOM;
    for (uint32_t l = 0; l < n_lanes; l++)
        if (status[l] != TS_OK) return status[l];
    // the proof of the highest index goes back (every proof of a run is checked by the caller's tests, not here)
    uint32_t best = 0;
    bool any = false;
    for (uint32_t l = 0; l < n_lanes; l++)
        if (!last_proof[l].empty() && (!any || last_index[l] > last_index[best])) best = l, any = true;
    if (any && last_proof_out) {
        *n_words_out = last_proof[best].size();
        if (last_proof[best].size() > cap_words) return TS_ERR_BUFFER;
        memcpy(last_proof_out, last_proof[best].data(), last_proof[best].size() * 4);
    }
    return TS_OK;
}

// ------------------------------------------------------------------ prove_batch
// ts_prove_stream's lane loop for n DISTINCT statements (uni-stark/src/prover.rs:25-39: each call has its own
// trace, public values and challenger, and returns its proof): per-item inputs and outputs, host traces
// uploaded on the lane's stream just before their proof, failures confined to the item (or, for a device
// fault, to its lane).  The whole-call refusals, the start gate and the lane threads are shared with the stream.
ts_status ts_prove_batch(ts_ctx* const* ctxs, const ts_air* const* airs, uint32_t n_lanes,
                         const ts_fri_config* cfg, ts_batch_item* items, uint32_t n_items, double gate_ms,
                         uint32_t flags) {
    // whole-call refusals first: nothing is consumed or written before these pass
    ts::FriConfig fri;
    if ((!items && n_items) || !check_lanes(ctxs, airs, n_lanes, cfg, fri)) return TS_ERR_INVALID;
    for (uint32_t i = 0; i < n_items; i++)
        if (items[i].struct_size != sizeof(ts_batch_item)) return TS_ERR_INVALID;
    struct Plain : BatchCall<ts_batch_item> {
        void refuse(uint32_t l) const { admit_air(PLAIN, airs[l], name); }
        std::vector<uint32_t> prove(uint32_t, ts_batch_item&, ts::TwoAdicFriPcs& pcs, const ts::AirProgram& prog,
                                    ts::BfChallenger& chal, ts::DeviceMatrix trace, const std::vector<uint32_t>& pis,
                                    ItemOutcome&) const {
            return ts::prove(pcs, prog, chal, std::move(trace), pis);
        }
    } call;
    call.name = "ts_prove_batch";
    call.what = "prove_batch";
    call.ctxs = ctxs;
    call.airs = airs;
    return run_batch(call, n_lanes, fri, items, n_items, gate_ms, flags);
}

static ts::Comm wrap_comm(const ts_comm& cb) {
    ts::Comm c;
    c.rank = cb.rank;
    c.world = cb.world;
    c.all_gather = [cb](const void* send, void* recv, size_t bytes, hipStream_t stream) {
        if (cb.all_gather(cb.user, send, recv, bytes, (void*)stream) != 0)
            throw ts::Error(ts::TS_ERR_COMM, "all_gather callback failed");
    };
    c.broadcast = [cb](void* buf, size_t bytes, int root, hipStream_t stream) {
        if (cb.broadcast(cb.user, buf, bytes, root, (void*)stream) != 0)
            throw ts::Error(ts::TS_ERR_COMM, "broadcast callback failed");
    };
    return c;
}

ts_status ts_prove_sharded(ts_ctx* ctx, const ts_fri_config* cfg, const ts_comm* comm,
                           const ts_air* air, ts_challenger* chal, ts_matrix* trace_rows,
                           const uint32_t* public_values, uint32_t n_public,
                           const ts_shard_options* options, uint32_t* proof_out, size_t cap_words,
                           size_t* n_words_out) {
    if (!ctx || !comm || !air || !chal || !trace_rows || !proof_out || !n_words_out ||
        !comm->all_gather || !comm->broadcast)
        return TS_ERR_INVALID;
    *n_words_out = 0;
    return guard(ctx, [&] {
        admit_air(PLAIN, air, "ts_prove_sharded");
        ts::TwoAdicFriPcs pcs(ctx->ctx, load_cfg(cfg));
        const std::vector<uint32_t> pis = public_inputs(public_values, n_public);
        const ts_comm cb = *comm;
        ts::Comm c = wrap_comm(cb);
        ts::ShardOptions opt;
        if (options)
            TS_REQUIRE(options->struct_size == sizeof(ts_shard_options), ts::TS_ERR_INVALID,
                       "ts_shard_options.struct_size != sizeof(ts_shard_options): caller built against another ABI");
        if (options && options->min_local_log) {
            TS_REQUIRE(options->min_local_log <= 27, ts::TS_ERR_INVALID, "min_local_log > 27");
            opt.min_local_log = options->min_local_log;
        }
        if (options) opt.trace_replicated = options->trace_replicated != 0;
        if (options) opt.local_quotient = options->local_quotient != 0;
        ts::DeviceMatrix m = take_trace(trace_rows);
        ts::StageTimer t(&ctx->ctx, "prove");
        copy_proof(abort_on_throw(cb, [&] {
                       return ts::prove_sharded(pcs, c, ready_prog(air), chal->c, std::move(m), pis, opt);
                   }),
                   proof_out, cap_words, n_words_out);
    });
}

// ------------------------------------------------------------------ prove / verify over taptrees
ts_status ts_prove_tap(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                       ts_matrix* trace, const uint32_t* public_values, uint32_t n_public,
                       const uint8_t* lock_scripts, const uint64_t* lock_offsets, size_t n_scripts,
                       uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    if (!ctx || !air || !chal || !trace || !proof_out || !n_words_out || !lock_scripts || !lock_offsets)
        return TS_ERR_INVALID;
    *n_words_out = 0;
    return guard(ctx, [&] {
        admit_air(PLAIN, air, "ts_prove_tap");
        ts::TwoAdicFriPcs pcs(ctx->ctx, load_cfg(cfg));
        const std::vector<uint32_t> pis = public_inputs(public_values, n_public);
        const ts::TapLocks locks = tap_locks(lock_scripts, lock_offsets, n_scripts);
        ts::DeviceMatrix m = take_trace(trace);
        ts::StageTimer t(&ctx->ctx, "prove");
        copy_proof(ts::prove_tap(pcs, ready_prog(air), chal->c, std::move(m), pis, locks), proof_out, cap_words,
                   n_words_out);
    });
}

ts_status ts_prove_tap_sharded(ts_ctx* ctx, const ts_fri_config* cfg, const ts_comm* comm, const ts_air* air,
                               ts_challenger* chal, ts_matrix* trace, const uint32_t* public_values,
                               uint32_t n_public, const uint8_t* lock_scripts, const uint64_t* lock_offsets,
                               size_t n_scripts, uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    if (!ctx || !comm || !air || !chal || !trace || !proof_out || !n_words_out || !lock_scripts ||
        !lock_offsets || !comm->all_gather)
        return TS_ERR_INVALID;
    *n_words_out = 0;
    return guard(ctx, [&] {
        admit_air(PLAIN, air, "ts_prove_tap_sharded");
        ts::TwoAdicFriPcs pcs(ctx->ctx, load_cfg(cfg));
        const std::vector<uint32_t> pis = public_inputs(public_values, n_public);
        const ts::TapLocks locks = tap_locks(lock_scripts, lock_offsets, n_scripts);
        const ts_comm cb = *comm;
        ts::Comm c = wrap_comm(cb);
        ts::DeviceMatrix m = take_trace(trace);
        ts::StageTimer t(&ctx->ctx, "prove");
        copy_proof(abort_on_throw(cb, [&] {
                       return ts::prove_tap(pcs, ready_prog(air), chal->c, std::move(m), pis, locks, &c);
                   }),
                   proof_out, cap_words, n_words_out);
    });
}

ts_status ts_verify_tap(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                        const uint32_t* proof, size_t n_words, const uint32_t* public_values,
                        uint32_t n_public, const uint8_t* lock_scripts, const uint64_t* lock_offsets,
                        size_t n_scripts, int* verdict) {
    if (!air || !chal || !proof || !verdict || !lock_scripts || !lock_offsets) return TS_ERR_INVALID;
    *verdict = -1;
    return guard(nullptr, [&] {
        admit_air(PLAIN, air, "ts_verify_tap");
        ts::FriConfig f = load_cfg(cfg);
        const std::vector<uint32_t> pis = public_inputs(public_values, n_public);
        for (size_t i = 0; i < n_scripts; i++)
            TS_REQUIRE(lock_offsets[i + 1] >= lock_offsets[i], ts::TS_ERR_INVALID, "bad lock script offsets");
        const ts::TapLocks locks = tap_locks(lock_scripts, lock_offsets, n_scripts);
        *verdict = ts::verify(2, f, air->a.prog(), chal->c, proof, n_words, pis, nullptr, nullptr, &locks);
    });
}

// ------------------------------------------------------------------ check_constraints
// What every ts_check_constraints* call does after its own admission rule: `side` holds the row-major side
// matrices it admitted (add_side_rows), preprocessed first, then aux; `challenges` and `exposed` are null for a
// call that takes none.
static void check_constraints(ts_ctx* ctx, const ts::AirProgram& p, const ts::SideRows& side, const ts_matrix* trace,
                              const uint32_t* public_values, uint32_t n_public, const uint32_t* challenges,
                              const uint32_t* exposed, int64_t* first_violation) {
    TS_REQUIRE(trace->m.buf.p && trace->m.layout == ts::DeviceMatrix::ROW_MAJOR, ts::TS_ERR_INVALID,
               "check_constraints: needs an uploaded (row-major, unconsumed) trace");
    TS_REQUIRE(trace->m.width == p.width, ts::TS_ERR_INVALID, "check_constraints: width != AIR width");
    const std::vector<uint32_t> pis = public_slots(p, public_values, n_public, challenges, exposed);
    const std::vector<uint32_t> consts = ts::air_consts_mont(p, pis.data(), pis.size());
    ts::DevBuf<uint32_t> d_consts(&ctx->ctx, consts.size());
    ts::DevBuf<unsigned long long> d_v(&ctx->ctx, 1);
    TS_HIP(hipMemcpyAsync(d_consts.p, consts.data(), consts.size() * 4, hipMemcpyHostToDevice, ctx->ctx.stream));
    TS_HIP(hipMemsetAsync(d_v.p, 0xff, 8, ctx->ctx.stream));
    ts::launch_check_constraints(ctx->ctx, p, trace->m.buf.p, trace->m.height, d_consts.p, d_v.p, side);
    unsigned long long v = 0;
    TS_HIP(hipMemcpyAsync(&v, d_v.p, 8, hipMemcpyDeviceToHost, ctx->ctx.stream));
    ctx->ctx.sync();
    *first_violation = v == ~0ull ? -1 : (int64_t)v;
}
// The head of the four calls: the admission, then the row-major side matrices the format takes, preprocessed first.
// `preprocessed`, `aux`, `challenges` and `exposed` are null from a call that has no such argument.
static ts_status single_check_constraints(const SingleCall& sc, ts_ctx* ctx, const ts_air* air,
                                          const ts_matrix* preprocessed, const ts_matrix* aux, const ts_matrix* trace,
                                          const uint32_t* public_values, uint32_t n_public, const uint32_t* challenges,
                                          const uint32_t* exposed, int64_t* first_violation) {
    if (!ctx || !air || !trace || !first_violation) {
        if (ctx) ctx->ctx.last_error = sc.name("check_constraints") + ": null argument";
        return TS_ERR_INVALID;
    }
    *first_violation = -1;
    return guard(ctx, [&] {
        admit_air(sc, air, sc.name("check_constraints"));
        const ts::AirProgram& p = air->a.prog();
        ts::SideRows side;
        if (sc.key) add_side_rows(ctx, preprocessed, p.preprocessed_width, "preprocessed", trace, side);
        if (sc.aux) add_side_rows(ctx, aux, p.aux_width, "aux", trace, side);
        check_constraints(ctx, p, side, trace, public_values, n_public, challenges, exposed, first_violation);
    });
}
ts_status ts_check_constraints(ts_ctx* ctx, const ts_air* air, const ts_matrix* trace,
                               const uint32_t* public_values, uint32_t n_public,
                               int64_t* first_violation) {
    return single_check_constraints(PLAIN, ctx, air, nullptr, nullptr, trace, public_values, n_public, nullptr, nullptr,
                                    first_violation);
}
ts_status ts_check_constraints_pre(ts_ctx* ctx, const ts_air* air, const ts_matrix* preprocessed,
                                   const ts_matrix* trace, const uint32_t* public_values, uint32_t n_public,
                                   int64_t* first_violation) {
    return single_check_constraints(PRE, ctx, air, preprocessed, nullptr, trace, public_values, n_public, nullptr,
                                    nullptr, first_violation);
}
ts_status ts_check_constraints_aux(ts_ctx* ctx, const ts_air* air, const ts_matrix* aux, const ts_matrix* trace,
                                   const uint32_t* public_values, uint32_t n_public, const uint32_t* challenges,
                                   const uint32_t* exposed, int64_t* first_violation) {
    return single_check_constraints(AUX, ctx, air, nullptr, aux, trace, public_values, n_public, challenges, exposed,
                                    first_violation);
}
ts_status ts_check_constraints_pre_aux(ts_ctx* ctx, const ts_air* air, const ts_matrix* preprocessed,
                                       const ts_matrix* aux, const ts_matrix* trace, const uint32_t* public_values,
                                       uint32_t n_public, const uint32_t* challenges, const uint32_t* exposed,
                                       int64_t* first_violation) {
    return single_check_constraints(PRE_AUX, ctx, air, preprocessed, aux, trace, public_values, n_public, challenges,
                                    exposed, first_violation);
}

// ------------------------------------------------------------------ challenge-phase (aux) columns
ts_status ts_air_aux_info(const ts_air* air, uint32_t* aux_width, uint32_t* n_challenges, uint32_t* n_exposed) {
    if (!air) return TS_ERR_INVALID;
    if (aux_width) *aux_width = air->a.prog().aux_width;
    if (n_challenges) *n_challenges = air->a.prog().n_challenges;
    if (n_exposed) *n_exposed = air->a.prog().n_exposed;
    return TS_OK;
}

// The callback's failure, carried through ts::prove as an exception of its own so that its status -- any
// value the host chose -- reaches the caller unchanged.
namespace {
struct AuxCallbackFailed {
    ts_status status;
};

// The aux source around a host's ts_aux_fn, for every call that takes one (`call` names it in the texts).  The
// callback sees the live trace as a ts_matrix of its own: borrowed for the call, handed back after.  A non-zero
// status is left in `cb_status` and leaves as AuxCallbackFailed; callback_failure() is the ts::Error for it.
ts::AuxSource callback_aux_source(ts_ctx* ctx, const ts::AirProgram& p, ts_aux_fn aux_fn, void* user,
                                  ts_status& cb_status, const char* call) {
    return [ctx, &p, aux_fn, user, &cb_status, call](const ts::DeviceMatrix& live, const uint32_t* challenges,
                                                     uint32_t* exposed) {
        ts_matrix view;
        view.m = std::move(const_cast<ts::DeviceMatrix&>(live));
        ts_matrix* out = nullptr;
        const ts_status rc = aux_fn(user, ctx, &view, challenges, p.n_challenges, &out, exposed);
        const_cast<ts::DeviceMatrix&>(live) = std::move(view.m);
        std::unique_ptr<ts_matrix> owned(out);
        if (rc != TS_OK) {
            cb_status = rc;
            throw AuxCallbackFailed{rc};
        }
        TS_REQUIRE(owned, ts::TS_ERR_INVALID, std::string(call) + ": the aux callback returned no matrix");
        return std::move(owned->m);
    };
}
ts::Error callback_failure(ts_ctx* ctx, ts_status cb_status, const char* call) {
    const std::string inner = ctx->ctx.last_error;
    return ts::Error(ts::TS_ERR_INVALID, std::string(call) + ": the aux callback (aux_fn) returned status " +
                                             std::to_string((int)cb_status) + (inner.empty() ? "" : ": " + inner));
}
}  // namespace

// ------------------------------------------------------------------ prove, the four single-table formats
// The key is an ordinary ts_pcs_data, part of the statement, read and never consumed; the aux source is the host's
// callback.  Every refusal is made before the trace is taken and before any device work; the callback's own status
// wins over the call's.
static ts_status single_prove(const SingleCall& sc, ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air,
                              ts_challenger* chal, const ts_pcs_data* key, ts_matrix* trace,
                              const uint32_t* public_values, uint32_t n_public, ts_aux_fn aux_fn, void* user,
                              uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    const std::string call = sc.name("prove");
    if (!ctx || !air || !chal || !trace || !proof_out || !n_words_out) {
        if (ctx) ctx->ctx.last_error = call + ": null argument";
        return TS_ERR_INVALID;
    }
    *n_words_out = 0;
    ts_status cb_status = TS_OK;
    const ts_status st = guard(ctx, [&] {
        const std::string keyed = sc.keyed_name("prove");
        admit_air(sc, air, keyed);
        const ts::PcsData* k = sc.key ? preprocessed_key_any(ctx, air, key, keyed.c_str()) : nullptr;
        const ts::AirProgram& p = ready_prog(air);
        if (sc.aux)
            TS_REQUIRE((aux_fn != nullptr) == (p.aux_width > 0), ts::TS_ERR_INVALID,
                       call + (p.aux_width ? ": null aux_fn for an AIR with aux columns"
                                           : ": an aux_fn was given for an AIR without aux columns"));
        ts::TwoAdicFriPcs pcs(ctx->ctx, load_cfg(cfg));
        // the key's height is known against the trace's before the trace is consumed
        const unsigned log_blowup = pcs.fri().log_blowup;
        if (k && sc.own_height_text)
            TS_REQUIRE(trace->m.buf.p && k->ldes[0].height == trace->m.height << log_blowup, ts::TS_ERR_INVALID,
                       "preprocessed key: LDE height is not the trace height << log_blowup");
        const std::vector<uint32_t> pis = public_inputs(public_values, n_public);
        if (!sc.any_context)
            TS_REQUIRE(trace->m.buf.ctx == &ctx->ctx || !trace->m.buf.p, ts::TS_ERR_INVALID,
                       "trace was made on another context");
        if (k && !sc.own_height_text) {
            TS_REQUIRE(trace->m.buf.p, ts::TS_ERR_INVALID, "trace matrix was already consumed");
            ts::check_side_matrix(*k, p, 0, trace->m.height << log_blowup);
        }
        ts::DeviceMatrix m = take_trace(trace);
        ts::AuxSource source;
        if (aux_fn) source = callback_aux_source(ctx, p, aux_fn, user, cb_status, call.c_str());
        ts::StageTimer t(&ctx->ctx, "prove");
        try {
            copy_proof(ts::prove(pcs, p, chal->c, std::move(m), pis, k, source, sc.version), proof_out, cap_words,
                       n_words_out);
        } catch (const AuxCallbackFailed&) {
            throw callback_failure(ctx, cb_status, call.c_str());
        }
    });
    return cb_status != TS_OK ? cb_status : st;
}
ts_status ts_prove(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                   ts_matrix* trace, const uint32_t* public_values, uint32_t n_public,
                   uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    return single_prove(PLAIN, ctx, cfg, air, chal, nullptr, trace, public_values, n_public, nullptr, nullptr, proof_out,
                        cap_words, n_words_out);
}
ts_status ts_prove_pre(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                       const ts_pcs_data* preprocessed, ts_matrix* trace, const uint32_t* public_values,
                       uint32_t n_public, uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    return single_prove(PRE, ctx, cfg, air, chal, preprocessed, trace, public_values, n_public, nullptr, nullptr,
                        proof_out, cap_words, n_words_out);
}
ts_status ts_prove_aux(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                       ts_matrix* trace, const uint32_t* public_values, uint32_t n_public, ts_aux_fn aux_fn,
                       void* user, uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    return single_prove(AUX, ctx, cfg, air, chal, nullptr, trace, public_values, n_public, aux_fn, user, proof_out,
                        cap_words, n_words_out);
}
ts_status ts_prove_pre_aux(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                           const ts_pcs_data* key, ts_matrix* trace, const uint32_t* public_values, uint32_t n_public,
                           ts_aux_fn aux_fn, void* user, uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    return single_prove(PRE_AUX, ctx, cfg, air, chal, key, trace, public_values, n_public, aux_fn, user, proof_out,
                        cap_words, n_words_out);
}

// ------------------------------------------------------------------ verify, the four single-table formats
// Host only.  A proof of another TSPF version (verdict 9) or with other widths in its header than the AIR's (verdict
// 1) is refused as an argument, TS_ERR_INVALID, with the verdict set; ts_verify alone leaves both to the verifier.
static ts_status single_verify(const SingleCall& sc, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                               const uint32_t* preprocessed_root, const uint32_t* proof, size_t n_words,
                               const uint32_t* public_values, uint32_t n_public, uint32_t* exposed_out,
                               uint32_t cap_exposed, int* verdict) {
    if (verdict) *verdict = -1;
    return guard(nullptr, [&] {
        const std::string call = sc.name("verify");
        TS_REQUIRE(air && chal && proof && verdict, ts::TS_ERR_INVALID, call + ": null argument");
        admit_air(sc, air, call);
        const ts::AirProgram& p = air->a.prog();
        const uint32_t pw = p.preprocessed_width;
        if (sc.key)
            TS_REQUIRE((preprocessed_root != nullptr) == (pw > 0), ts::TS_ERR_INVALID,
                       call + (pw ? ": null preprocessed root for an AIR with preprocessed columns"
                                  : ": a preprocessed root was given for an AIR without preprocessed columns"));
        if (sc.aux)
            TS_REQUIRE(p.n_exposed == 0 || (exposed_out && cap_exposed >= p.n_exposed), ts::TS_ERR_INVALID,
                       call + ": null or short buffer for the exposed words");
        ts::FriConfig f = load_cfg(cfg);
        const std::vector<uint32_t> pis = public_inputs(public_values, n_public);
        // the header behind word 4: v4 and v5 the aux width and the two counts, then v3 and v5 the preprocessed width
        std::vector<uint32_t> widths;
        if (sc.aux) widths = {p.aux_width, p.n_challenges, p.n_exposed};
        if (sc.key) widths.push_back(pw);
        if (sc.version != 1 && n_words >= 2 && proof[0] == ts::TSPF_MAGIC && proof[1] != sc.version) {
            *verdict = 9;
            throw ts::Error(ts::TS_ERR_INVALID, call + ": not a TSPF v" + std::to_string(sc.version) + " proof");
        }
        if (!widths.empty() && n_words >= 5 + widths.size() && proof[0] == ts::TSPF_MAGIC &&
            !std::equal(widths.begin(), widths.end(), proof + 5)) {
            *verdict = 1;
            throw ts::Error(ts::TS_ERR_INVALID,
                            call + ": the proof's " + (sc.aux ? "aux width, challenge or exposed count" : "") +
                                (sc.aux && sc.key ? " or " : "") + (sc.key ? "preprocessed width" : "") +
                                " is not the AIR's");
        }
        std::vector<uint32_t> exposed;
        *verdict = ts::verify(sc.version, f, p, chal->c, proof, n_words, pis, preprocessed_root,
                              sc.aux ? &exposed : nullptr);
        if (*verdict == 0 && !exposed.empty()) memcpy(exposed_out, exposed.data(), exposed.size() * 4);
    });
}
ts_status ts_verify(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                    const uint32_t* proof, size_t n_words, const uint32_t* public_values,
                    uint32_t n_public, int* verdict) {
    return single_verify(PLAIN, cfg, air, chal, nullptr, proof, n_words, public_values, n_public, nullptr, 0, verdict);
}
ts_status ts_verify_pre(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                        const uint32_t preprocessed_root[8], const uint32_t* proof, size_t n_words,
                        const uint32_t* public_values, uint32_t n_public, int* verdict) {
    return single_verify(PRE, cfg, air, chal, preprocessed_root, proof, n_words, public_values, n_public, nullptr, 0,
                         verdict);
}
ts_status ts_verify_aux(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal, const uint32_t* proof,
                        size_t n_words, const uint32_t* public_values, uint32_t n_public, uint32_t* exposed_out,
                        uint32_t cap_exposed, int* verdict) {
    return single_verify(AUX, cfg, air, chal, nullptr, proof, n_words, public_values, n_public, exposed_out, cap_exposed,
                         verdict);
}
ts_status ts_verify_pre_aux(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                            const uint32_t preprocessed_root[8], const uint32_t* proof, size_t n_words,
                            const uint32_t* public_values, uint32_t n_public, uint32_t* exposed_out,
                            uint32_t cap_exposed, int* verdict) {
    return single_verify(PRE_AUX, cfg, air, chal, preprocessed_root, proof, n_words, public_values, n_public, exposed_out,
                         cap_exposed, verdict);
}

// ------------------------------------------------------------------ LogUp aux columns
namespace {
void load_terms(const ts_logup_term* from, size_t count, std::vector<ts::LogupTerm>& to) {
    for (size_t i = 0; i < count; i++) to.push_back(ts::LogupTerm{from[i].kind, from[i].value});
}

ts::LogupSpec load_logup_spec(const ts_logup_spec* spec) {
    TS_REQUIRE(spec && spec->struct_size >= sizeof(ts_logup_spec), ts::TS_ERR_INVALID, "logup: null spec or bad struct_size");
    TS_REQUIRE(spec->n_interactions >= 1 && spec->n_interactions <= ts::LOGUP_MAX_INTERACTIONS && spec->interactions,
               ts::TS_ERR_INVALID, "logup: between 1 and 16 interactions");
    ts::LogupSpec s;
    for (uint32_t i = 0; i < spec->n_interactions; i++) {
        const ts_logup_interaction& it = spec->interactions[i];
        TS_REQUIRE(it.n_values >= 1 && it.n_values <= ts::LOGUP_MAX_VALUES && it.values, ts::TS_ERR_INVALID,
                   "logup: between 1 and 8 values per interaction");
        s.interactions.push_back({ts::LogupTerm{it.multiplicity.kind, it.multiplicity.value}, {}});
        load_terms(it.values, it.n_values, s.interactions.back().values);
    }
    return s;
}

// what ts_logup_mult_spec and ts_logup_mult_bus_spec share: the struct's size and the table's terms
void load_mult_table(bool size_ok, uint32_t n_values, const ts_logup_term* table, std::vector<ts::LogupTerm>& to) {
    TS_REQUIRE(size_ok, ts::TS_ERR_INVALID, "logup multiplicities: bad struct_size");
    TS_REQUIRE(n_values >= 1 && n_values <= ts::LOGUP_MAX_VALUES && table, ts::TS_ERR_INVALID,
               "logup multiplicities: between 1 and 8 values");
    load_terms(table, n_values, to);
}
// and one set of lookups with their weights, n_values terms each
void load_mult_lookups(uint32_t n_lookups, uint32_t n_values, const ts_logup_term* lookups,
                       const ts_logup_term* weights, std::vector<ts::LogupTerm>& l, std::vector<ts::LogupTerm>& w) {
    TS_REQUIRE(n_lookups >= 1 && n_lookups <= ts::LOGUP_MULT_MAX_LOOKUPS && lookups && weights, ts::TS_ERR_INVALID,
               "logup multiplicities: between 1 and 16 lookups, each with its weight");
    load_terms(lookups, (size_t)n_lookups * n_values, l);
    load_terms(weights, n_lookups, w);
}

ts::LogupMultSpec load_mult_spec(const ts_logup_mult_spec* spec) {
    ts::LogupMultSpec s;
    load_mult_table(spec->struct_size == sizeof(ts_logup_mult_spec), spec->n_values, spec->table, s.table);
    load_mult_lookups(spec->n_lookups, spec->n_values, spec->lookups, spec->weights, s.lookups, s.weights);
    s.out_column = spec->out_column;
    s.negate = spec->negate;
    return s;
}
}  // namespace

ts_status ts_logup_aux_width(const ts_logup_spec* spec, uint32_t* aux_width) {
    if (!aux_width) return TS_ERR_INVALID;
    *aux_width = 0;
    return guard(nullptr, [&] { *aux_width = ts::logup_aux_width(load_logup_spec(spec)); });
}

namespace {
ts_status aux_build(ts_ctx* ctx, const char* call, const ts_logup_spec* spec, const ts_matrix* preprocessed,
                    bool takes_table, const ts_matrix* trace, const uint32_t challenges[8], ts_matrix** aux_out,
                    uint32_t exposed_out[4]) {
    if (!ctx || !trace || !challenges || !aux_out || !exposed_out) {
        if (ctx) ctx->ctx.last_error = std::string(call) + ": null argument";
        return TS_ERR_INVALID;
    }
    *aux_out = nullptr;
    return guard(ctx, [&] {
        const ts::LogupSpec s = load_logup_spec(spec);
        *aux_out = new_matrix(ts::logup_aux_build(ctx->ctx, s, trace->m, challenges, exposed_out,
                                                  preprocessed ? &preprocessed->m : nullptr, takes_table));
    });
}
}  // namespace

ts_status ts_logup_aux_build(ts_ctx* ctx, const ts_logup_spec* spec, const ts_matrix* trace,
                             const uint32_t challenges[8], ts_matrix** aux_out, uint32_t exposed_out[4]) {
    return aux_build(ctx, "ts_logup_aux_build", spec, nullptr, false, trace, challenges, aux_out, exposed_out);
}

// ts_logup_aux_build with terms of kind 2: columns of a row-major table of the trace's height (the values of a
// preprocessed key; not consumed)
ts_status ts_logup_aux_build_pre(ts_ctx* ctx, const ts_logup_spec* spec, const ts_matrix* preprocessed,
                                 const ts_matrix* trace, const uint32_t challenges[8], ts_matrix** aux_out,
                                 uint32_t exposed_out[4]) {
    return aux_build(ctx, "ts_logup_aux_build_pre", spec, preprocessed, true, trace, challenges, aux_out, exposed_out);
}

// The multiplicity column of one table, in place in the resident trace (logup_mult.hip).
ts_status ts_logup_multiplicities(ts_ctx* ctx, const ts_logup_mult_spec* spec, const ts_matrix* preprocessed,
                                  ts_matrix* trace, uint64_t* n_missing, uint64_t* first_missing) {
    if (!ctx || !spec || !trace) {
        if (ctx) ctx->ctx.last_error = "ts_logup_multiplicities: null argument";
        return TS_ERR_INVALID;
    }
    if (n_missing) *n_missing = 0;
    if (first_missing) *first_missing = ~0ull;
    return guard(ctx, [&] {
        const ts::LogupMultSpec s = load_mult_spec(spec);
        const ts::LogupMultResult r = ts::logup_multiplicities(ctx->ctx, s, trace->m, preprocessed ? &preprocessed->m : nullptr);
        if (n_missing) *n_missing = r.n_missing;
        if (first_missing) *first_missing = r.first_missing;
        if (!n_missing && r.n_missing) throw ts::Error(ts::TS_ERR_INVARIANT, ts::logup_miss_text(r, spec->n_lookups));
    });
}

// The multiplicity column of a table whose lookups are rows of other traces (logup_mult.hip).
namespace {
ts_status mult_bus(ts_ctx* ctx, const ts_logup_mult_bus_spec* spec, const ts_matrix* table_pre, bool takes_pre,
                   ts_matrix* table_trace, const ts_matrix* const* lookers, uint64_t* n_missing,
                   uint64_t first_missing[3]) {
    if (!ctx) return TS_ERR_INVALID;
    if (n_missing) *n_missing = 0;
    if (first_missing) first_missing[0] = first_missing[1] = first_missing[2] = ~0ull;
    return guard(ctx, [&] {
        TS_REQUIRE(spec && table_trace && lookers, ts::TS_ERR_INVALID, "ts_logup_multiplicities_bus: null argument");
        ts::LogupMultBusSpec s;
        load_mult_table(spec->struct_size == sizeof(ts_logup_mult_bus_spec), spec->n_values, spec->table, s.table);
        TS_REQUIRE(spec->n_lookers >= 1 && spec->n_lookers <= ts::LOGUP_MULT_MAX_LOOKERS && spec->lookers,
                   ts::TS_ERR_INVALID, "logup multiplicities: between 1 and 16 lookers");
        std::vector<const ts::DeviceMatrix*> mats;
        for (uint32_t k = 0; k < spec->n_lookers; k++) {
            const ts_logup_bus_looker& in = spec->lookers[k];
            ts::LogupMultLooker lk;
            load_mult_lookups(in.n_lookups, spec->n_values, in.lookups, in.weights, lk.lookups, lk.weights);
            TS_REQUIRE(lookers[k], ts::TS_ERR_INVALID, "ts_logup_multiplicities_bus: null looker");
            s.lookers.push_back(std::move(lk));
            mats.push_back(&lookers[k]->m);
        }
        s.out_column = spec->out_column;
        s.negate = spec->negate;
        const ts::LogupMultBusResult r = ts::logup_multiplicities_bus(ctx->ctx, s, table_trace->m, mats, table_pre ? &table_pre->m : nullptr, takes_pre);
        if (n_missing) *n_missing = r.n_missing;
        if (first_missing) {
            first_missing[0] = r.looker;
            first_missing[1] = r.row;
            first_missing[2] = r.lookup;
        }
        if (!n_missing && r.n_missing)
            throw ts::Error(ts::TS_ERR_INVARIANT,
                            "logup multiplicities: the tuple of looker " + std::to_string(r.looker) + ", row " +
                                std::to_string(r.row) + ", lookup " + std::to_string(r.lookup) + " is in no table row (" +
                                std::to_string(r.n_missing) + " such lookups)");
    });
}
}  // namespace

ts_status ts_logup_multiplicities_bus(ts_ctx* ctx, const ts_logup_mult_bus_spec* spec, ts_matrix* table_trace,
                                      const ts_matrix* const* lookers, uint64_t* n_missing, uint64_t first_missing[3]) {
    return mult_bus(ctx, spec, nullptr, false, table_trace, lookers, n_missing, first_missing);
}

// The same with kind-2 terms on the table's side: columns of the table's preprocessed matrix (the values of a key).
ts_status ts_logup_multiplicities_bus_pre(ts_ctx* ctx, const ts_logup_mult_bus_spec* spec,
                                          const ts_matrix* table_preprocessed, ts_matrix* table_trace,
                                          const ts_matrix* const* lookers, uint64_t* n_missing,
                                          uint64_t first_missing[3]) {
    return mult_bus(ctx, spec, table_preprocessed, true, table_trace, lookers, n_missing, first_missing);
}

// The rows of a resident matrix in sorted order, and rows gathered through an index column (sort.hip).
ts_status ts_matrix_sort_rows(ts_ctx* ctx, const ts_sort_spec* spec, const ts_matrix* src, ts_matrix** out) {
    if (out) *out = nullptr;
    if (!ctx) return TS_ERR_INVALID;
    const ts_status refused = guard(ctx, [&] {
        TS_REQUIRE(spec && src && out, ts::TS_ERR_INVALID, "ts_matrix_sort_rows: null argument");
        TS_REQUIRE(spec->struct_size == sizeof(ts_sort_spec), ts::TS_ERR_INVALID, "sort rows: bad struct_size");
        TS_REQUIRE(spec->n_keys >= 1 && spec->n_keys <= ts::SORT_MAX_KEYS, ts::TS_ERR_INVALID,
                   "sort rows: between 1 and 4 keys");
    }, false);
    if (refused) return refused;
    return guard(ctx, [&] {
        ts::SortSpec s;
        s.key_columns.assign(spec->key_columns, spec->key_columns + spec->n_keys);
        s.group_keys = spec->group_keys;
        s.flags = spec->flags;
        s.n_live = spec->n_live;
        *out = new_matrix(ts::sort_rows(ctx->ctx, s, src->m));
    });
}

ts_status ts_matrix_gather_rows(ts_ctx* ctx, const ts_matrix* src, const ts_matrix* index, uint32_t index_column,
                                ts_matrix** out) {
    if (out) *out = nullptr;
    if (!ctx) return TS_ERR_INVALID;
    if (!src || !index || !out) {
        ctx->ctx.last_error = "ts_matrix_gather_rows: null argument";
        return TS_ERR_INVALID;
    }
    return guard(ctx, [&] {
        *out = new_matrix(ts::gather_rows(ctx->ctx, src->m, index->m, index_column));
    });
}

// Derived columns: a row program over a resident matrix (derive.hip), its checks and its host evaluation (derive.cpp).
ts_status ts_matrix_derive(ts_ctx* ctx, const uint32_t* program, size_t n_words, const ts_matrix* src, ts_matrix** out) {
    if (out) *out = nullptr;
    if (!ctx) return TS_ERR_INVALID;
    const ts_status refused = guard(ctx, [&] {
        TS_REQUIRE(program && src && out, ts::TS_ERR_INVALID, "ts_matrix_derive: null argument");
    }, false);
    if (refused) return refused;
    return guard(ctx, [&] {
        *out = new_matrix(ts::derive_matrix(ctx->ctx, program, n_words, src->m));
    });
}

ts_status ts_derive_check(const uint32_t* program, size_t n_words, uint32_t src_width, uint32_t* out_width,
                          uint32_t* n_instructions, uint32_t* n_live) {
    if (out_width) *out_width = 0;
    if (n_instructions) *n_instructions = 0;
    if (n_live) *n_live = 0;
    return guard(nullptr, [&] {
        const ts::DeriveProgram prog = ts::derive_lower(program, n_words, src_width);
        if (out_width) *out_width = prog.out_width;
        if (n_instructions) *n_instructions = prog.n_nodes_kept;
        if (n_live) *n_live = prog.n_live;
    });
}

ts_status ts_derive_rows_host(const uint32_t* program, size_t n_words, const uint32_t* src_row_major, uint64_t height,
                              uint32_t src_width, uint32_t* out_row_major, size_t out_cap_words) {
    return guard(nullptr, [&] {
        TS_REQUIRE(program && src_row_major && out_row_major, ts::TS_ERR_INVALID, "ts_derive_rows_host: null argument");
        TS_REQUIRE(height >= 1 && height <= ts::DERIVE_MAX_HEIGHT, ts::TS_ERR_INVALID,
                   "derive: the height of the source must be in [1, 2^27]");
        const ts::DeriveProgram prog = ts::derive_lower(program, n_words, src_width);
        TS_REQUIRE((uint64_t)out_cap_words >= height * prog.out_width, ts::TS_ERR_BUFFER,
                   "ts_derive_rows_host: the output buffer holds fewer than height * out_width words");
        ts::derive_rows_host(prog, src_row_major, height, out_row_major);
    });
}

// Scanned columns: linear recurrences down the rows of a resident matrix (scan.hip), their checks and the sequential
// loop over host rows (scan.cpp).
namespace {
ts::ScanSpec scan_spec(const std::string& call, const ts_scan_spec* spec) {
    TS_REQUIRE(spec->struct_size == sizeof(ts_scan_spec), ts::TS_ERR_INVALID, call + ": bad struct_size");
    TS_REQUIRE(spec->n_columns >= 1 && spec->n_columns <= TS_SCAN_MAX_COLUMNS, ts::TS_ERR_INVALID,
               "scan: n_columns " + std::to_string(spec->n_columns) + " outside [1, 8]");
    ts::ScanSpec s;
    for (uint32_t k = 0; k < spec->n_columns; k++) {
        const ts_scan_column& c = spec->columns[k];
        s.columns.push_back({c.a.kind, c.a.value, c.b.kind, c.b.value, c.init, c.reset_column, c.dst_column, c.flags});
    }
    s.out_width = spec->out_width;
    return s;
}
}  // namespace

ts_status ts_matrix_scan(ts_ctx* ctx, const ts_scan_spec* spec, const ts_matrix* src, ts_matrix** out, uint32_t* finals) {
    if (out) *out = nullptr;
    if (!ctx) return TS_ERR_INVALID;
    const ts_status refused = guard(ctx, [&] {
        TS_REQUIRE(spec && src && out, ts::TS_ERR_INVALID, "ts_matrix_scan: null argument");
    }, false);
    if (refused) return refused;
    return guard(ctx, [&] {
        const ts::ScanSpec s = scan_spec("ts_matrix_scan", spec);
        *out = new_matrix(ts::scan_matrix(ctx->ctx, s, src->m, finals));
    });
}

ts_status ts_scan_rows_host(const ts_scan_spec* spec, const uint32_t* src_row_major, uint64_t height, uint32_t src_width,
                            uint32_t* out_row_major, size_t out_cap_words, uint32_t* finals) {
    return guard(nullptr, [&] {
        TS_REQUIRE(spec && src_row_major && out_row_major, ts::TS_ERR_INVALID, "ts_scan_rows_host: null argument");
        const ts::ScanSpec s = scan_spec("ts_scan_rows_host", spec);
        TS_REQUIRE(height >= 1 && height <= ts::SCAN_MAX_HEIGHT, ts::TS_ERR_INVALID,
                   "scan: the height of the source must be in [1, 2^27]");
        const ts::ScanPlan plan = ts::scan_check(s, src_width);
        TS_REQUIRE((uint64_t)out_cap_words >= height * plan.out_width, ts::TS_ERR_BUFFER,
                   "ts_scan_rows_host: the output buffer holds fewer than height * out_width words");
        ts::scan_rows_host(s, plan, src_row_major, height, out_row_major, finals);
    });
}

// Collected rows: the selected rows of up to four resident matrices as one new matrix (collect.hip), the checks and the
// sequential loop over host rows (collect.cpp).
// The three calls take a second tape form, told apart by its magic: grouped rows, one row per distinct key tuple of ONE
// source (group.hip, group.cpp).  Any other first word is the collect's to judge.
static bool is_group_tape(const uint32_t* spec, size_t n_words) {
    return spec && n_words >= 1 && spec[0] == ts::GROUP_MAGIC;
}

ts_status ts_matrix_collect_rows(ts_ctx* ctx, const uint32_t* spec, size_t n_words, const ts_matrix* const* sources,
                                 uint64_t out_height, ts_matrix** out, uint64_t* n_live) {
    if (out) *out = nullptr;
    if (n_live) *n_live = 0;
    if (!ctx) return TS_ERR_INVALID;
    const ts_status refused = guard(ctx, [&] {
        TS_REQUIRE(spec && sources && out && n_live, ts::TS_ERR_INVALID, "ts_matrix_collect_rows: null argument");
    }, false);
    if (refused) return refused;
    return guard(ctx, [&] {
        if (is_group_tape(spec, n_words)) {
            const ts::GroupPlan plan = ts::group_check(spec, n_words);
            TS_REQUIRE(sources[0], ts::TS_ERR_INVALID, "ts_matrix_collect_rows: null argument");
            uint64_t live = 0;
            *out = new_matrix(ts::group_matrix(ctx->ctx, plan, sources[0]->m, out_height, &live));
            *n_live = live;
            return;
        }
        const ts::CollectPlan plan = ts::collect_check(spec, n_words);  // (and so how many handles `sources` holds)
        const ts::DeviceMatrix* mats[ts::COLLECT_MAX_SOURCES] = {};
        for (uint32_t s = 0; s < plan.n_sources; s++) {
            TS_REQUIRE(sources[s], ts::TS_ERR_INVALID, "ts_matrix_collect_rows: null argument");
            mats[s] = &sources[s]->m;
        }
        uint64_t live = 0;
        *out = new_matrix(ts::collect_matrix(ctx->ctx, plan, mats, out_height, &live));
        *n_live = live;
    });
}

ts_status ts_collect_check(const uint32_t* spec, size_t n_words, uint32_t* n_sources, uint32_t* out_width) {
    if (n_sources) *n_sources = 0;
    if (out_width) *out_width = 0;
    return guard(nullptr, [&] {
        if (is_group_tape(spec, n_words)) {
            const ts::GroupPlan plan = ts::group_check(spec, n_words);
            if (n_sources) *n_sources = 1;
            if (out_width) *out_width = plan.out_width;
            return;
        }
        const ts::CollectPlan plan = ts::collect_check(spec, n_words);
        if (n_sources) *n_sources = plan.n_sources;
        if (out_width) *out_width = plan.out_width;
    });
}

ts_status ts_collect_rows_host(const uint32_t* spec, size_t n_words, const uint32_t* const* src_row_major,
                               const uint64_t* heights, uint64_t out_height, uint32_t* out_row_major,
                               size_t out_cap_words, uint64_t* out_height_used, uint64_t* n_live) {
    if (out_height_used) *out_height_used = 0;
    if (n_live) *n_live = 0;
    return guard(nullptr, [&] {
        TS_REQUIRE(spec && src_row_major && heights && out_row_major && out_height_used && n_live, ts::TS_ERR_INVALID,
                   "ts_collect_rows_host: null argument");
        if (is_group_tape(spec, n_words)) {
            const ts::GroupPlan plan = ts::group_check(spec, n_words);
            TS_REQUIRE(src_row_major[0], ts::TS_ERR_INVALID, "ts_collect_rows_host: null argument");
            TS_REQUIRE(heights[0] >= 1 && heights[0] <= ts::GROUP_MAX_HEIGHT, ts::TS_ERR_INVALID,
                       "group: the height of source 0 must be in [1, 2^27]");
            ts::collect_check_out_height(out_height);
            const std::vector<unsigned long long> records = ts::group_records_host(plan, src_row_major[0], heights[0]);
            const uint64_t live = records.size() / (ts::GROUP_RECORD_HEAD + plan.n_aggregates);
            const uint64_t height = ts::group_height(live, out_height);
            TS_REQUIRE((uint64_t)out_cap_words >= height * plan.out_width, ts::TS_ERR_BUFFER,
                       "ts_collect_rows_host: the output buffer holds fewer than height * out_width words");
            ts::group_rows_host(plan, records, src_row_major[0], height, out_row_major);
            *out_height_used = height;
            *n_live = live;
            return;
        }
        const ts::CollectPlan plan = ts::collect_check(spec, n_words);
        for (uint32_t s = 0; s < plan.n_sources; s++) {
            TS_REQUIRE(src_row_major[s], ts::TS_ERR_INVALID, "ts_collect_rows_host: null argument");
            TS_REQUIRE(heights[s] >= 1 && heights[s] <= ts::COLLECT_MAX_HEIGHT, ts::TS_ERR_INVALID,
                       "collect: the height of source " + std::to_string(s) + " must be in [1, 2^27]");
        }
        ts::collect_check_out_height(out_height);
        const uint64_t live = ts::collect_count_host(plan, src_row_major, heights);
        const uint64_t height = ts::collect_height(live, out_height);
        TS_REQUIRE((uint64_t)out_cap_words >= height * plan.out_width, ts::TS_ERR_BUFFER,
                   "ts_collect_rows_host: the output buffer holds fewer than height * out_width words");
        ts::collect_rows_host(plan, src_row_major, heights, height, out_row_major);
        *out_height_used = height;
        *n_live = live;
    });
}

// Expanded rows: every row of a resident matrix repeated by its own count as one new matrix (expand.hip), the checks and
// the sequential loop over host rows (expand.cpp).
ts_status ts_matrix_expand_rows(ts_ctx* ctx, const uint32_t* spec, size_t n_words, const ts_matrix* src,
                                uint64_t out_height, ts_matrix** out, uint64_t* n_live) {
    if (out) *out = nullptr;
    if (n_live) *n_live = 0;
    if (!ctx) return TS_ERR_INVALID;
    const ts_status refused = guard(ctx, [&] {
        TS_REQUIRE(spec && src && out && n_live, ts::TS_ERR_INVALID, "ts_matrix_expand_rows: null argument");
    }, false);
    if (refused) return refused;
    return guard(ctx, [&] {
        const ts::ExpandPlan plan = ts::expand_check(spec, n_words);
        uint64_t live = 0;
        *out = new_matrix(ts::expand_matrix(ctx->ctx, plan, src->m, out_height, &live));
        *n_live = live;
    });
}

ts_status ts_expand_check(const uint32_t* spec, size_t n_words, uint32_t* src_width, uint32_t* out_width) {
    if (src_width) *src_width = 0;
    if (out_width) *out_width = 0;
    return guard(nullptr, [&] {
        const ts::ExpandPlan plan = ts::expand_check(spec, n_words);
        if (src_width) *src_width = plan.src_width;
        if (out_width) *out_width = plan.out_width;
    });
}

ts_status ts_expand_rows_host(const uint32_t* spec, size_t n_words, const uint32_t* src_row_major, uint64_t height,
                              uint64_t out_height, uint32_t* out_row_major, size_t out_cap_words,
                              uint64_t* out_height_used, uint64_t* n_live) {
    if (out_height_used) *out_height_used = 0;
    if (n_live) *n_live = 0;
    return guard(nullptr, [&] {
        TS_REQUIRE(spec && src_row_major && out_row_major && out_height_used && n_live, ts::TS_ERR_INVALID,
                   "ts_expand_rows_host: null argument");
        const ts::ExpandPlan plan = ts::expand_check(spec, n_words);
        TS_REQUIRE(height >= 1 && height <= ts::EXPAND_MAX_HEIGHT, ts::TS_ERR_INVALID,
                   "expand: the height of the source must be in [1, 2^27]");
        ts::expand_check_out_height(out_height);
        const ts::ExpandTotals totals = ts::expand_count_host(plan, src_row_major, height);
        const uint64_t used = ts::expand_height(plan, totals, out_height);
        TS_REQUIRE((uint64_t)out_cap_words >= used * plan.out_width, ts::TS_ERR_BUFFER,
                   "ts_expand_rows_host: the output buffer holds fewer than height * out_width words");
        ts::expand_rows_host(plan, src_row_major, height, used, out_row_major);
        *out_height_used = used;
        *n_live = totals.total;
    });
}

// Joined rows: columns of the table row with the same key, fetched into a copy of the source (join.hip), the checks and
// the sequential loop over host rows (join.cpp).
namespace {
static_assert(sizeof(ts::JoinTerm) == sizeof(ts_logup_term), "JoinTerm is ts_logup_term");
ts::JoinPlan load_join(const ts_join_spec* spec, uint32_t src_width, uint32_t table_width) {
    TS_REQUIRE(spec, ts::TS_ERR_INVALID, "join: null spec");
    const bool size_ok = spec->struct_size == sizeof(ts_join_spec);
    ts::JoinSpecIn in = {};
    in.size_ok = size_ok;
    if (size_ok) {  // (the fields of another struct are not read)
        in.n_keys = spec->n_keys;
        in.src_keys = reinterpret_cast<const ts::JoinTerm*>(spec->src_keys);
        in.table_keys = reinterpret_cast<const ts::JoinTerm*>(spec->table_keys);
        in.when = ts::JoinTerm{spec->when.kind, spec->when.value};
        in.n_fetch = spec->n_fetch;
        in.table_columns = spec->table_columns;
        in.dst_columns = spec->dst_columns;
        in.defaults = spec->defaults;
        in.flags = spec->flags;
        in.table_rows = spec->table_rows;
    }
    return ts::join_check(in, src_width, table_width);
}
}  // namespace

ts_status ts_matrix_join_rows(ts_ctx* ctx, const ts_join_spec* spec, const ts_matrix* src, const ts_matrix* table,
                              ts_matrix** out, uint64_t* n_missing, uint64_t* first_missing) {
    if (out) *out = nullptr;
    if (n_missing) *n_missing = 0;
    if (first_missing) *first_missing = ~0ull;
    if (!ctx) return TS_ERR_INVALID;
    const ts_status refused = guard(ctx, [&] {
        TS_REQUIRE(spec && src && table && out, ts::TS_ERR_INVALID, "ts_matrix_join_rows: null argument");
    }, false);
    if (refused) return refused;
    return guard(ctx, [&] {
        ts::require_resident(ctx->ctx, src->m, "join", "the source");  // (a consumed matrix has no width to check against)
        ts::require_resident(ctx->ctx, table->m, "join", "the table");
        const ts::JoinPlan plan = load_join(spec, src->m.width, table->m.width);
        uint64_t n = 0, first = ~0ull;
        *out = new_matrix(ts::join_matrix(ctx->ctx, plan, src->m, table->m, n_missing == nullptr, &n, &first));
        if (n_missing) *n_missing = n;
        if (first_missing) *first_missing = first;
    });
}

ts_status ts_join_check(const ts_join_spec* spec, uint32_t src_width, uint32_t table_width, uint32_t* out_width) {
    if (out_width) *out_width = 0;
    return guard(nullptr, [&] {
        const ts::JoinPlan plan = load_join(spec, src_width, table_width);
        if (out_width) *out_width = plan.out_width;
    });
}

ts_status ts_join_rows_host(const ts_join_spec* spec, const uint32_t* src, uint64_t src_height, uint32_t src_width,
                            const uint32_t* table, uint64_t table_height, uint32_t table_width, uint32_t* out,
                            uint64_t out_words, uint64_t* n_missing, uint64_t* first_missing) {
    if (n_missing) *n_missing = 0;
    if (first_missing) *first_missing = ~0ull;
    return guard(nullptr, [&] {
        TS_REQUIRE(spec && src && table && out, ts::TS_ERR_INVALID, "ts_join_rows_host: null argument");
        const ts::JoinPlan plan = load_join(spec, src_width, table_width);
        const uint64_t n_table = ts::join_table_rows(plan, src_height, table_height);
        TS_REQUIRE(out_words >= src_height * plan.out_width, ts::TS_ERR_BUFFER,
                   "ts_join_rows_host: the output buffer holds fewer than height * out_width words");
        std::vector<uint32_t> match;
        uint64_t first = ~0ull;
        const uint64_t n = ts::join_match_host(plan, src, src_height, table, n_table, match, &first);
        if (!n_missing && n) throw ts::Error(ts::TS_ERR_INVARIANT, ts::join_miss_text(n, first));
        ts::join_rows_host(plan, src, src_height, table, match, out);
        if (n_missing) *n_missing = n;
        if (first_missing) *first_missing = first;
    });
}

// The LogUp columns of n traces for one set of challenges, in three launches (logup.hip logup_aux_build_multi).
namespace {
ts_status aux_build_multi(ts_ctx* ctx, const std::string& call, uint32_t n, const ts_logup_spec* const* specs,
                          const ts_matrix* const* preprocessed, bool takes_tables, const ts_matrix* const* traces,
                          const uint32_t challenges[8], ts_matrix** aux_out, uint32_t* exposed_out) {
    if (!ctx) return TS_ERR_INVALID;
    if (aux_out && n >= 1 && n <= ts::LOGUP_MAX_TABLES)
        for (uint32_t k = 0; k < n; k++) aux_out[k] = nullptr;
    return guard(ctx, [&] {
        TS_REQUIRE(specs && traces && challenges && aux_out && exposed_out && (preprocessed || !takes_tables),
                   ts::TS_ERR_INVALID, call + ": null argument");
        TS_REQUIRE(n >= 1 && n <= ts::LOGUP_MAX_TABLES, ts::TS_ERR_INVALID, call + ": between 1 and 64 tables");
        std::vector<ts::LogupSpec> loaded(n);
        std::vector<const ts::LogupSpec*> sp(n);
        std::vector<const ts::DeviceMatrix*> tr(n), pre(n, nullptr);
        for (uint32_t k = 0; k < n; k++) {
            TS_REQUIRE(traces[k], ts::TS_ERR_INVALID, call + ": null trace");
            if (takes_tables && preprocessed[k]) pre[k] = &preprocessed[k]->m;
            loaded[k] = load_logup_spec(specs[k]);
            sp[k] = &loaded[k];
            tr[k] = &traces[k]->m;
        }
        std::vector<uint32_t> exposed(4 * (size_t)n);
        std::vector<ts::DeviceMatrix> aux = ts::logup_aux_build_multi(ctx->ctx, sp, tr, challenges, exposed.data(), nullptr, takes_tables ? &pre : nullptr);
        std::vector<std::unique_ptr<ts_matrix>> handles(n);
        for (uint32_t k = 0; k < n; k++) {
            handles[k] = std::make_unique<ts_matrix>();
            handles[k]->m = std::move(aux[k]);
        }
        for (uint32_t k = 0; k < n; k++) aux_out[k] = handles[k].release();
        memcpy(exposed_out, exposed.data(), exposed.size() * 4);
    });
}
}  // namespace

ts_status ts_logup_aux_build_multi(ts_ctx* ctx, uint32_t n, const ts_logup_spec* const* specs,
                                   const ts_matrix* const* traces, const uint32_t challenges[8], ts_matrix** aux_out,
                                   uint32_t* exposed_out) {
    return aux_build_multi(ctx, "ts_logup_aux_build_multi", n, specs, nullptr, false, traces, challenges, aux_out,
                           exposed_out);
}

// The same with kind-2 terms: table k's read preprocessed[k], the row-major values of its preprocessed columns.
ts_status ts_logup_aux_build_multi_pre(ts_ctx* ctx, uint32_t n, const ts_logup_spec* const* specs,
                                       const ts_matrix* const* preprocessed, const ts_matrix* const* traces,
                                       const uint32_t challenges[8], ts_matrix** aux_out, uint32_t* exposed_out) {
    return aux_build_multi(ctx, "ts_logup_aux_build_multi_pre", n, specs, preprocessed, true, traces, challenges, aux_out,
                           exposed_out);
}

// ------------------------------------------------------------------ prove_multi, prove_multi_bus, prove_multi_key
// Several AIR tables of mixed heights in one proof (prove_multi.cpp): plain ones (TSPF v6), with LogUp aux columns on
// a bus across the tables (v7), against a commit-once key (v8).  Every refusal is made before the first trace is taken.
namespace {
// A table array of the C ABI, read as ts_multi_bus_table: ts_multi_table is that struct without its last field, logup.
struct MultiTables {
    const char* p;
    size_t size;  // of one table
    std::string type;
    uint32_t n;
    MultiTables(const ts_multi_table* t, uint32_t n) : p((const char*)t), size(sizeof *t), type("ts_multi_table"), n(n) {}
    MultiTables(const ts_multi_bus_table* t, uint32_t n)
        : p((const char*)t), size(sizeof *t), type("ts_multi_bus_table"), n(n) {}
    ts_multi_bus_table operator[](uint32_t t) const {
        ts_multi_bus_table v{};
        memcpy(&v, p + t * size, size);
        return v;
    }
};
static_assert(sizeof(ts_multi_table) == offsetof(ts_multi_bus_table, logup) &&
                  offsetof(ts_multi_table, air) == offsetof(ts_multi_bus_table, air) &&
                  offsetof(ts_multi_table, trace) == offsetof(ts_multi_bus_table, trace) &&
                  offsetof(ts_multi_table, public_values) == offsetof(ts_multi_bus_table, public_values),
              "ts_multi_table is a prefix of ts_multi_bus_table");

// the admission of the handles of `call`'s tables, table by table
void admit_multi_tables(ts_ctx* ctx, const std::string& call, const MultiTables& tables) {
    for (uint32_t t = 0; t < tables.n; t++) {
        const ts_multi_bus_table mt = tables[t];
        TS_REQUIRE(mt.struct_size == tables.size, ts::TS_ERR_INVALID,
                   call + ": " + tables.type + ".struct_size is not sizeof(" + tables.type + ")");
        TS_REQUIRE(mt.air && mt.trace, ts::TS_ERR_INVALID, call + ": null AIR or trace");
        TS_REQUIRE(mt.air->a.context() == &ctx->ctx, ts::TS_ERR_INVALID,
                   call + ": an AIR was compiled on another context (or host-only)");
        TS_REQUIRE(mt.trace->m.buf.p, ts::TS_ERR_INVALID, "trace matrix was already consumed");
        TS_REQUIRE(mt.trace->m.buf.ctx == &ctx->ctx, ts::TS_ERR_INVALID, call + ": a trace was made on another context");
        for (uint32_t k = 0; k < t; k++)
            TS_REQUIRE(tables[k].trace != mt.trace, ts::TS_ERR_INVALID, call + ": one trace handle in two tables");
    }
}

// the statement of admitted tables on shapes alone: the matrices stay with their handles until all of it holds.
// `specs` keeps the loaded specs alive.
std::vector<ts::MultiBusTable> multi_table_shapes(const MultiTables& tables, std::vector<ts::LogupSpec>& specs) {
    std::vector<ts::MultiBusTable> mts(tables.n);
    specs.resize(tables.n);
    for (uint32_t t = 0; t < tables.n; t++) {
        const ts_multi_bus_table mt = tables[t];
        mts[t].air = &ready_prog(mt.air);
        mts[t].public_values = public_inputs(mt.public_values, mt.n_public);
        mts[t].trace.width = mt.trace->m.width;
        mts[t].trace.height = mt.trace->m.height;
        mts[t].trace.layout = mt.trace->m.layout;
        if (mt.logup) {
            specs[t] = load_logup_spec(mt.logup);
            mts[t].logup = &specs[t];
        }
    }
    return mts;
}

// `version`: 6 ts_prove_multi, 7 ts_prove_multi_bus (both without a key), 8 ts_prove_multi_key
ts_status prove_multi_call(ts_ctx* ctx, uint32_t version, const ts_fri_config* cfg, ts_challenger* chal,
                           const ts_multi_key* key, const MultiTables& tables, uint32_t* proof_out, size_t cap_words,
                           size_t* n_words_out) {
    if (!ctx) return TS_ERR_INVALID;
    if (n_words_out) *n_words_out = 0;
    return guard(ctx, [&] {
        const std::string call = std::string("ts_") + ts::multi_call(version, nullptr).name;
        TS_REQUIRE(cfg && chal && tables.p && proof_out && n_words_out, ts::TS_ERR_INVALID, call + ": null argument");
        TS_REQUIRE(tables.n >= 1 && tables.n <= ts::MAX_MULTI_TABLES, ts::TS_ERR_INVALID,
                   call + ": between 1 and 64 tables");
        const ts::FriConfig fri = load_cfg(cfg);
        admit_multi_tables(ctx, call, tables);
        std::vector<ts::LogupSpec> specs;
        std::vector<ts::MultiBusTable> mts = multi_table_shapes(tables, specs);
        TS_REQUIRE(!key || key->k.ctx == &ctx->ctx, ts::TS_ERR_INVALID, call + ": the key was made on another context");
        ts::check_multi_statement(ts::multi_call(version, &fri), mts, key ? &key->k : nullptr);
        ts::TwoAdicFriPcs pcs(ctx->ctx, fri);
        for (uint32_t t = 0; t < tables.n; t++) mts[t].trace = take_trace(tables[t].trace);
        ts::StageTimer timer(&ctx->ctx, "prove");
        copy_proof(version == 6   ? ts::prove_multi(pcs, chal->c, mts)
                   : version == 7 ? ts::prove_multi_bus(pcs, chal->c, mts)
                                  : ts::prove_multi_key(pcs, chal->c, mts, key->k),
                   proof_out, cap_words, n_words_out);
    });
}

// The three host-only verify calls: `version` as above.  ts_verify_multi has no exposed or bus outputs (null here);
// ts_verify_multi_key may be handed no exposed buffer where no table has aux columns.
ts_status verify_multi_call(uint32_t version, const ts_fri_config* cfg, ts_challenger* chal, const uint32_t* key_root,
                            const ts_air* const* airs, uint32_t n_tables, const uint32_t* const* public_values,
                            const uint32_t* n_public, const uint32_t* proof, size_t n_words, uint32_t* exposed_out,
                            uint32_t cap_exposed, uint32_t* bus_sum, int* verdict) {
    if (verdict) *verdict = -1;
    return guard(nullptr, [&] {
        const std::string call = version == 6 ? "ts_verify_multi" : version == 7 ? "ts_verify_multi_bus" : "ts_verify_multi_key";
        TS_REQUIRE(cfg && chal && airs && public_values && n_public && proof && verdict && (version == 6 || bus_sum) &&
                       (version != 7 || exposed_out) && (version != 8 || key_root),
                   ts::TS_ERR_INVALID, call + ": null argument");
        TS_REQUIRE(n_tables >= 1 && n_tables <= ts::MAX_MULTI_TABLES, ts::TS_ERR_INVALID,
                   call + ": between 1 and 64 tables");
        const ts::FriConfig fri = load_cfg(cfg);
        std::vector<const ts::AirProgram*> progs(n_tables);
        std::vector<std::vector<uint32_t>> pis(n_tables);
        uint32_t n_aux = 0, n_pre = 0;
        for (uint32_t t = 0; t < n_tables; t++) {
            TS_REQUIRE(airs[t], ts::TS_ERR_INVALID, call + ": null AIR");
            const ts::AirProgram& p = airs[t]->a.prog();
            if (version == 6)
                TS_REQUIRE(!p.preprocessed_width && !p.aux_width, ts::TS_ERR_UNSUPPORTED,
                           call + ": a table's AIR has preprocessed or aux columns");
            else {
                TS_REQUIRE(version == 8 || !p.preprocessed_width, ts::TS_ERR_UNSUPPORTED,
                           call + ": a table's AIR has preprocessed columns");
                TS_REQUIRE(p.aux_width ? p.n_challenges == 2 && p.n_exposed == 4 : !p.n_challenges && !p.n_exposed,
                           ts::TS_ERR_INVALID,
                           call + ": an AIR on the bus has aux columns, 2 challenges and 4 exposed words, " +
                               (version == 8 ? "any other" : "a plain one") + " none of them");
            }
            n_aux += p.aux_width ? 1 : 0;
            n_pre += p.preprocessed_width ? 1 : 0;
            progs[t] = &p;
            pis[t] = public_inputs(public_values[t], n_public[t]);
        }
        TS_REQUIRE(version != 8 || n_pre > 0, ts::TS_ERR_INVALID,
                   call + ": no table has preprocessed columns; ts_verify_multi_bus (TSPF v7) and "
                          "ts_verify_multi (TSPF v6) verify tables without a key");
        TS_REQUIRE(version != 7 || n_aux > 0, ts::TS_ERR_INVALID,
                   call + ": no table has aux columns; ts_verify_multi verifies plain tables (TSPF v6)");
        TS_REQUIRE(n_aux == 0 || (exposed_out && cap_exposed >= 4 * n_aux), ts::TS_ERR_INVALID,
                   call + (version == 8 ? ": null or short" : ": short") +
                       " buffer for the exposed words (4 per table with aux columns)");
        std::vector<uint32_t> exposed;
        uint32_t sum[4] = {0, 0, 0, 0};
        *verdict = version == 6   ? ts::verify_multi(fri, chal->c, progs, pis, proof, n_words)
                   : version == 7 ? ts::verify_multi_bus(fri, chal->c, progs, pis, proof, n_words, exposed, sum)
                                  : ts::verify_multi_key(fri, chal->c, key_root, progs, pis, proof, n_words, exposed, sum);
        if (*verdict == 0 && version != 6) {
            if (!exposed.empty()) memcpy(exposed_out, exposed.data(), exposed.size() * 4);
            memcpy(bus_sum, sum, 16);
        }
    }, false);
}
}  // namespace

ts_status ts_prove_multi(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal, ts_multi_table* tables,
                         uint32_t n_tables, uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    return prove_multi_call(ctx, 6, cfg, chal, nullptr, MultiTables(tables, n_tables), proof_out, cap_words, n_words_out);
}

ts_status ts_verify_multi(const ts_fri_config* cfg, ts_challenger* chal, const ts_air* const* airs, uint32_t n_tables,
                          const uint32_t* const* public_values, const uint32_t* n_public, const uint32_t* proof,
                          size_t n_words, int* verdict) {
    return verify_multi_call(6, cfg, chal, nullptr, airs, n_tables, public_values, n_public, proof, n_words, nullptr, 0,
                             nullptr, verdict);
}

ts_status ts_prove_multi_bus(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal, ts_multi_bus_table* tables,
                             uint32_t n_tables, uint32_t* proof_out, size_t cap_words, size_t* n_words_out) {
    return prove_multi_call(ctx, 7, cfg, chal, nullptr, MultiTables(tables, n_tables), proof_out, cap_words, n_words_out);
}

ts_status ts_verify_multi_bus(const ts_fri_config* cfg, ts_challenger* chal, const ts_air* const* airs, uint32_t n_tables,
                              const uint32_t* const* public_values, const uint32_t* n_public, const uint32_t* proof,
                              size_t n_words, uint32_t* exposed_out, uint32_t cap_exposed, uint32_t bus_sum[4],
                              int* verdict) {
    return verify_multi_call(7, cfg, chal, nullptr, airs, n_tables, public_values, n_public, proof, n_words, exposed_out,
                             cap_exposed, bus_sum, verdict);
}

// ------------------------------------------------------------------ the key of a multi-table proof
// ts_pcs_commit of the matrices on their natural domains; with keep_values the row-major inputs stay alive as handles
// of the key (TwoAdicFriPcs::commit's keep_row_major: no second copy).
ts_status ts_multi_key_commit(ts_ctx* ctx, const ts_fri_config* cfg, uint32_t n_mats, ts_matrix* const* mats,
                              int keep_values, uint32_t root_out[8], ts_multi_key** out) {
    if (!ctx) return TS_ERR_INVALID;
    if (out) *out = nullptr;
    return guard(ctx, [&] {
        TS_REQUIRE(cfg && mats && out, ts::TS_ERR_INVALID, "ts_multi_key_commit: null argument");
        TS_REQUIRE(n_mats >= 1 && n_mats <= (uint32_t)ts::MAX_BATCH_MATS, ts::TS_ERR_INVALID,
                   "ts_multi_key_commit: between 1 and 64 matrices");
        const ts::FriConfig fri = load_cfg(cfg);
        for (uint32_t i = 0; i < n_mats; i++) {
            TS_REQUIRE(mats[i] && mats[i]->m.buf.p, ts::TS_ERR_INVALID, "ts_multi_key_commit: null or consumed matrix");
            TS_REQUIRE(mats[i]->m.buf.ctx == &ctx->ctx, ts::TS_ERR_INVALID,
                       "ts_multi_key_commit: a matrix was made on another context");
            TS_REQUIRE(!keep_values || mats[i]->m.layout == ts::DeviceMatrix::ROW_MAJOR, ts::TS_ERR_INVALID,
                       "ts_multi_key_commit: keep_values needs row-major (uploaded) matrices");
            ts::log2_strict(mats[i]->m.height);
            for (uint32_t k = 0; k < i; k++)
                TS_REQUIRE(mats[k] != mats[i], ts::TS_ERR_INVALID, "ts_multi_key_commit: one matrix handle twice");
        }
        auto key = std::make_unique<ts_multi_key>();
        key->k.ctx = &ctx->ctx;
        key->k.log_blowup = fri.log_blowup;
        std::vector<ts::DeviceMatrix> ms;
        for (uint32_t i = 0; i < n_mats; i++) {
            key->k.heights.push_back(mats[i]->m.height);
            key->k.widths.push_back(mats[i]->m.width);
            ms.push_back(std::move(mats[i]->m));
        }
        ts::TwoAdicFriPcs pcs(ctx->ctx, fri);
        key->k.data = pcs.commit(ms, std::vector<uint32_t>(n_mats, 1u), true, /*keep_row_major=*/keep_values != 0);
        for (uint32_t i = 0; i < n_mats; i++) {
            if (keep_values) {
                key->values.push_back(std::make_unique<ts_matrix>());
                key->values.back()->m = std::move(ms[i]);
                key->k.values.push_back(&key->values.back()->m);
            } else {
                key->k.values.push_back(nullptr);
            }
        }
        if (root_out) memcpy(root_out, key->k.data->root, 32);
        *out = key.release();
    });
}
ts_status ts_multi_key_info(const ts_multi_key* key, uint32_t idx, uint64_t* height, uint32_t* width) {
    if (!key || idx >= key->k.heights.size()) return TS_ERR_INVALID;
    if (height) *height = key->k.heights[idx];
    if (width) *width = key->k.widths[idx];
    return TS_OK;
}
ts_status ts_multi_key_values(const ts_multi_key* key, uint32_t idx, const ts_matrix** out) {
    if (out) *out = nullptr;
    if (!key || !out || idx >= key->k.values.size() || !key->k.values[idx]) return TS_ERR_INVALID;
    *out = key->values[idx].get();
    return TS_OK;
}
ts_status ts_multi_key_free(ts_ctx* ctx, ts_multi_key* key) {
    if (!key) return TS_OK;
    if (!ctx || key->k.ctx != &ctx->ctx) return TS_ERR_INVALID;
    return guard(ctx, [&] { delete key; });
}

// ts_prove_multi_bus against a key: tables with preprocessed columns read the key's matrices in order (TSPF v8).
ts_status ts_prove_multi_key(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal, const ts_multi_key* key,
                             ts_multi_key_table* tables, uint32_t n_tables, uint32_t* proof_out, size_t cap_words,
                             size_t* n_words_out) {
    return prove_multi_call(ctx, 8, cfg, chal, key, MultiTables(tables, n_tables), proof_out, cap_words, n_words_out);
}

ts_status ts_verify_multi_key(const ts_fri_config* cfg, ts_challenger* chal, const uint32_t key_root[8],
                              const ts_air* const* airs, uint32_t n_tables, const uint32_t* const* public_values,
                              const uint32_t* n_public, const uint32_t* proof, size_t n_words, uint32_t* exposed_out,
                              uint32_t cap_exposed, uint32_t bus_sum[4], int* verdict) {
    return verify_multi_call(8, cfg, chal, key_root, airs, n_tables, public_values, n_public, proof, n_words, exposed_out,
                             cap_exposed, bus_sum, verdict);
}

// ------------------------------------------------------------------ before you prove: the bus, exactly
namespace {
void reset_bus_report(ts_bus_report* report, ts_bus_share* shares, uint32_t n) {
    const uint32_t size = report->struct_size;
    memset(report, 0, sizeof *report);
    report->struct_size = size;
    report->first_table = report->first_row = report->first_interaction = ~0u;
    if (shares)
        for (uint32_t k = 0; k < n; k++) shares[k] = ts_bus_share{0, 0, ~0u, ~0u, 0};
}
// the refusals of ts_bus_check and ts_check_multi (`call`) that are made on the arguments alone, in this order, before
// a context is looked at: the text, or empty
std::string bus_report_refusal(const std::string& call, const ts_ctx* ctx, uint32_t n, const ts_bus_report* report) {
    if (!report) return call + ": null report";
    if (n < 1 || n > ts::LOGUP_MAX_TABLES) return call + ": between 1 and 64 tables";
    if (!ctx) return call + ": null context";
    if (report->struct_size != sizeof(ts_bus_report))
        return call + ": ts_bus_report.struct_size is not sizeof(ts_bus_report)";
    return "";
}
}  // namespace

// The balance of a whole bus from the resident traces (bus_check.hip).
ts_status ts_bus_check(ts_ctx* ctx, uint32_t n, const ts_logup_spec* const* specs, const ts_matrix* const* preprocessed,
                       const ts_matrix* const* traces, ts_bus_report* report, ts_bus_share* shares) {
    if (const std::string no = bus_report_refusal("ts_bus_check", ctx, n, report); !no.empty()) {
        (ctx ? ctx->ctx.last_error : g_create_error) = no;
        return TS_ERR_INVALID;
    }
    reset_bus_report(report, shares, n);
    return guard(ctx, [&] {
        TS_REQUIRE(specs && traces, ts::TS_ERR_INVALID, "ts_bus_check: null argument");
        std::vector<ts::LogupSpec> loaded(n);
        std::vector<const ts::LogupSpec*> sp(n, nullptr);
        std::vector<const ts::DeviceMatrix*> tr(n, nullptr), pre(n, nullptr);
        for (uint32_t k = 0; k < n; k++) {
            if (!specs[k]) continue;
            TS_REQUIRE(traces[k], ts::TS_ERR_INVALID, "ts_bus_check: null trace");
            if (preprocessed && preprocessed[k]) pre[k] = &preprocessed[k]->m;
            loaded[k] = load_logup_spec(specs[k]);
            sp[k] = &loaded[k];
            tr[k] = &traces[k]->m;
        }
        const ts::BusReport r = ts::bus_check(ctx->ctx, sp, tr, pre);
        report->n_contributions = r.n_contributions;
        report->n_tuples = r.n_tuples;
        report->n_unbalanced = r.n_unbalanced;
        report->first_table = r.first_table;
        report->first_row = r.first_row;
        report->first_interaction = r.first_interaction;
        report->n_values = r.n_values;
        memcpy(report->tuple, r.tuple, sizeof report->tuple);
        report->sum = r.sum;
        if (shares)
            for (uint32_t k = 0; k < n; k++)
                shares[k] = ts_bus_share{r.shares[k].count, r.shares[k].sum, r.shares[k].first_row,
                                         r.shares[k].first_interaction, 0};
    });
}

// The debug counterpart of ts_prove_multi_bus / ts_prove_multi_key: the builder, the per-table constraint check and
// the bus check over traces that stay with their handles.
ts_status ts_check_multi(ts_ctx* ctx, const ts_multi_key* key, const ts_multi_key_table* tables, uint32_t n_tables,
                         const uint32_t challenges[8], int32_t* bad_table, int64_t* first_violation,
                         ts_bus_report* report, ts_bus_share* shares) {
    if (bad_table) *bad_table = -1;
    if (first_violation) *first_violation = -1;
    if (const std::string no = bus_report_refusal("ts_check_multi", ctx, n_tables, report); !no.empty()) {
        (ctx ? ctx->ctx.last_error : g_create_error) = no;
        return TS_ERR_INVALID;
    }
    reset_bus_report(report, shares, n_tables);
    return guard(ctx, [&] {
        const std::string call = "ts_check_multi";
        TS_REQUIRE(tables && challenges && bad_table && first_violation, ts::TS_ERR_INVALID, call + ": null argument");
        const MultiTables admitted(tables, n_tables);
        admit_multi_tables(ctx, call, admitted);
        std::vector<ts::LogupSpec> specs;
        const std::vector<ts::MultiBusTable> mts = multi_table_shapes(admitted, specs);
        TS_REQUIRE(!key || key->k.ctx == &ctx->ctx, ts::TS_ERR_INVALID, call + ": the key was made on another context");
        ts::check_multi_statement(ts::multi_call(0, nullptr), mts, key ? &key->k : nullptr);

        // per table its key matrix (null without preprocessed columns); the aux tables and their builder arguments
        std::vector<const ts_matrix*> pre(n_tables, nullptr), traces(n_tables, nullptr);
        std::vector<const ts_logup_spec*> bus_specs(n_tables, nullptr);
        std::vector<const ts_logup_spec*> a_specs;
        std::vector<const ts_matrix*> a_pre, a_traces;
        std::vector<int> aux_of(n_tables, -1);
        size_t ki = 0;
        for (uint32_t t = 0; t < n_tables; t++) {
            traces[t] = tables[t].trace;
            if (mts[t].air->preprocessed_width) pre[t] = key->values[ki++].get();
            if (!tables[t].logup) continue;
            bus_specs[t] = tables[t].logup;
            aux_of[t] = (int)a_specs.size();
            a_specs.push_back(tables[t].logup);
            a_pre.push_back(pre[t]);
            a_traces.push_back(tables[t].trace);
        }
        auto passed = [&](ts_status st) {  // a call of this library on the same context: its text is the text
            if (st != TS_OK) throw ts::Error(st, std::string(ctx->ctx.last_error));
        };
        const uint32_t n_aux = (uint32_t)a_specs.size();
        std::vector<ts_matrix*> aux(n_aux, nullptr);
        std::vector<uint32_t> exposed(4 * (size_t)n_aux);
        struct FreeAux {
            std::vector<ts_matrix*>& aux;
            ~FreeAux() {
                for (ts_matrix* m : aux) delete m;
            }
        } free_aux{aux};
        if (n_aux)
            passed(ts_logup_aux_build_multi_pre(ctx, n_aux, a_specs.data(), a_pre.data(), a_traces.data(), challenges,
                                                aux.data(), exposed.data()));
        for (uint32_t t = 0; t < n_tables; t++) {
            const int a = aux_of[t];
            int64_t fv = -1;
            passed(ts_check_constraints_pre_aux(ctx, tables[t].air, pre[t], a >= 0 ? aux[a] : nullptr, tables[t].trace,
                                                tables[t].public_values, tables[t].n_public, a >= 0 ? challenges : nullptr,
                                                a >= 0 ? exposed.data() + 4 * (size_t)a : nullptr, &fv));
            if (fv != -1) {
                *bad_table = (int32_t)t;
                *first_violation = fv;
                break;
            }
        }
        if (n_aux) passed(ts_bus_check(ctx, n_tables, bus_specs.data(), pre.data(), traces.data(), report, shares));
    });
}

// ------------------------------------------------------------------ prove_batch_lookup
// ts_prove_batch's lanes (run_batch above) for AIRs with a key, aux columns or both: per item the device work of
// ts_prove_pre_aux, with the key owned by the lane and the aux source by the item -- a ts_logup_spec the lane runs
// itself, or a callback on the lane's thread.  What a lane holds while a proof is in flight: DESIGN.md section 4, "Lookup AIRs in batch lanes".
namespace {
bool reads_table(const std::vector<ts::LogupTerm>& terms) {
    return std::any_of(terms.begin(), terms.end(), [](const ts::LogupTerm& t) { return t.kind == 2; });
}

struct LookupCall : BatchCall<ts_batch_lookup_item> {
    const ts_batch_lane* lanes = nullptr;
    ts::FriConfig fri;
    // what admit() parsed for the item its lane is on, for prove()
    struct Parsed {
        bool has_spec = false;
        ts::LogupSpec spec;
        std::vector<ts::LogupMultSpec> fills;
    };
    mutable std::vector<Parsed> parsed;  // one per lane, touched by that lane's thread only

    const ts_matrix* table(uint32_t l) const { return lanes ? lanes[l].key_values : nullptr; }

    void reset(ts_batch_lookup_item& it) const {
        it.n_exposed = 0;
        it.n_missing = 0;
        it.first_missing = ~0ull;
    }

    void admit(uint32_t l, ts_batch_lookup_item& it, const ts::AirProgram& prog, uint64_t height,
               const ts::DeviceMatrix* trace) const {
        ts_ctx* ctx = ctxs[l];
        const std::string w = what;
        const ts::PcsData* k = preprocessed_key_any(ctx, airs[l], lanes ? lanes[l].key : nullptr, name);
        if (k) ts::check_side_matrix(*k, prog, 0, height << fri.log_blowup);
        const ts_matrix* kv = table(l);
        if (kv)
            TS_REQUIRE(kv->m.buf.p && kv->m.layout == ts::DeviceMatrix::ROW_MAJOR && kv->m.buf.ctx == &ctx->ctx &&
                           kv->m.width == prog.preprocessed_width && kv->m.height == height,
                       ts::TS_ERR_INVALID, w + ": key_values must be on the lane's context, row-major, of the AIR's "
                                               "preprocessed width and the trace's height");
        const uint32_t aw = prog.aux_width;
        if (aw)
            TS_REQUIRE((it.logup != nullptr) != (it.aux_fn != nullptr), ts::TS_ERR_INVALID,
                       w + ": exactly one of logup / aux_fn must be set for an AIR with aux columns");
        else
            TS_REQUIRE(!it.logup && !it.aux_fn, ts::TS_ERR_INVALID,
                       w + ": an aux source was given for an AIR without aux columns");
        Parsed& ps = parsed[l];
        ps = Parsed{};
        if (it.logup) {
            ps.spec = load_logup_spec(it.logup);
            ps.has_spec = true;
            TS_REQUIRE(prog.n_challenges == 2 && prog.n_exposed == 4 && ts::logup_aux_width(ps.spec, 2) == aw,
                       ts::TS_ERR_INVALID, w + ": a logup spec needs an AIR with 2 challenges, 4 exposed words and "
                                               "the spec's aux width");
            for (const ts::LogupInteraction& in : ps.spec.interactions)
                TS_REQUIRE(kv || !(in.multiplicity.kind == 2 || reads_table(in.values)), ts::TS_ERR_INVALID,
                           w + ": the logup spec reads the preprocessed table, the lane has no key_values");
        }
        TS_REQUIRE(it.n_mult <= 8 && (it.n_mult == 0 || it.mult), ts::TS_ERR_INVALID,
                   w + ": at most 8 multiplicity fills, and n_mult of them in mult");
        for (uint32_t q = 0; q < it.n_mult; q++) {
            ps.fills.push_back(load_mult_spec(&it.mult[q]));
            const ts::LogupMultSpec& f = ps.fills.back();
            TS_REQUIRE(kv || !(reads_table(f.table) || reads_table(f.lookups) || reads_table(f.weights)),
                       ts::TS_ERR_INVALID, w + ": a multiplicity fill reads the preprocessed table, the lane has no key_values");
        }
        if (trace && (aw || it.n_mult))
            TS_REQUIRE(trace->layout == ts::DeviceMatrix::ROW_MAJOR, ts::TS_ERR_INVALID,
                       w + ": the device trace must be row-major (the aux source and the fills read its rows)");
        TS_REQUIRE(!it.exposed_out || it.cap_exposed >= prog.n_exposed, ts::TS_ERR_INVALID,
                   w + ": exposed_out is shorter than the AIR's exposed words");
        it.n_exposed = prog.n_exposed;
    }

    std::vector<uint32_t> prove(uint32_t l, ts_batch_lookup_item& it, ts::TwoAdicFriPcs& pcs, const ts::AirProgram& prog,
                                ts::BfChallenger& chal, ts::DeviceMatrix trace, const std::vector<uint32_t>& pis,
                                ItemOutcome& outcome) const {
        ts_ctx* ctx = ctxs[l];
        Parsed& ps = parsed[l];
        const ts::PcsData* key = lanes && lanes[l].key ? lanes[l].key->d.get() : nullptr;
        const ts::DeviceMatrix* tab = table(l) ? &table(l)->m : nullptr;
        ts_status cb_status = TS_OK;
        ts::AuxSource inner;
        if (ps.has_spec) inner = ts::logup_aux_source(ctx->ctx, std::move(ps.spec), tab);
        else if (it.aux_fn) inner = callback_aux_source(ctx, prog, it.aux_fn, it.aux_user, cb_status, name);
        // the exposed words as the source hands them over: the caller's copy, made once the proof stands
        std::vector<uint32_t> exposed;
        ts::AuxSource source;
        if (inner)
            source = [&](const ts::DeviceMatrix& live, const uint32_t* challenges, uint32_t* exposed_out) {
                ts::DeviceMatrix aux = inner(live, challenges, exposed_out);
                exposed.assign(exposed_out, exposed_out + prog.n_exposed);
                return aux;
            };
        ts::LogupMultResult miss{0, ~0ull};
        std::vector<uint32_t> proof;
        try {
            proof = ts::prove_lookup(pcs, prog, chal, std::move(trace), pis, key, source, ps.fills, tab, &miss);
        } catch (const ts::LookupDataError&) {
            it.n_missing = miss.n_missing;
            it.first_missing = miss.first_missing;
            outcome.lane_goes_on = true;
            throw;
        } catch (const AuxCallbackFailed&) {
            outcome.lane_goes_on = true;
            outcome.status = cb_status;
            throw callback_failure(ctx, cb_status, name);
        }
        if (it.exposed_out && !exposed.empty()) memcpy(it.exposed_out, exposed.data(), exposed.size() * 4);
        return proof;
    }
};
}  // namespace

ts_status ts_prove_batch_lookup(ts_ctx* const* ctxs, const ts_air* const* airs, const ts_batch_lane* lanes,
                                uint32_t n_lanes, const ts_fri_config* cfg, ts_batch_lookup_item* items,
                                uint32_t n_items, double gate_ms, uint32_t flags) {
    // whole-call refusals first: nothing is consumed or written before these pass
    LookupCall call;
    if ((!items && n_items) || !check_lanes(ctxs, airs, n_lanes, cfg, call.fri)) return TS_ERR_INVALID;
    for (uint32_t i = 0; i < n_items; i++)
        if (items[i].struct_size != sizeof(ts_batch_lookup_item)) return TS_ERR_INVALID;
    for (uint32_t l = 0; l < n_lanes; l++)
        if (lanes ? lanes[l].struct_size != sizeof(ts_batch_lane) : airs[l]->a.prog().preprocessed_width != 0)
            return TS_ERR_INVALID;
    call.name = "ts_prove_batch_lookup";
    call.what = "prove_batch_lookup";
    call.ctxs = ctxs;
    call.airs = airs;
    call.lanes = lanes;
    call.parsed.resize(n_lanes);
    return run_batch(call, n_lanes, call.fri, items, n_items, gate_ms, flags);
}

}  // extern "C"
