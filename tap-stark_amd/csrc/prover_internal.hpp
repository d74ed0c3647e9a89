// What the three host provers share (prover_common.cpp, and the FRI commit phase in fri_commit.cpp):
// prove (prover.cpp), prove_sharded (sharded.cpp) and prove_tap (tap_prover.cpp) run the same pipeline
// and differ in where the rows live and in the MMCS.
#pragma once
#include <functional>
#include <initializer_list>

#include "host.hpp"
#include "open_plan.hpp"  // alpha_powers_mont, AlphaLedger, opened_from_raw

namespace ts {

struct FriRound {
    const Ef* vec = nullptr;        // committed vector (rows of two): length 2 * 2^log_leaves
    const uint32_t* tree = nullptr;
    unsigned log_leaves = 0;
    uint32_t root[8];
};

// Device-side state of one commit phase.  The transcript lives on the device from begin to finish:
// per round the kernel that makes the root observes it and samples beta (d_betas[r]).
struct FriCommit {
    // The vector the next round commits to (`len` elements; of a sharded round: this rank's slab of it).
    // deferred != nullptr: `cur` is not in memory yet -- it is the fold of the last round's vector (this pointer)
    // with the last round's challenge, and the next launch computes it while hashing.
    DevBuf<Ef> cur;
    const Ef* deferred = nullptr;
    uint64_t len = 0;
    // One round on `cur`: allocates the tree (and `cur`, if deferred), launches and records the round, defers the
    // next vector into the next launch or folds it now, keeps the buffers.  `top` (sharded rounds, with the slab's
    // coordinates as in FriRoundLaunch): the launch builds the sub-tree only, top(sub-root, round) does the rest.
    using TopStep = std::function<void(const uint32_t* d_subroot, size_t round)>;
    void round(Context& ctx, bool defer_next, const TopStep& top = nullptr, uint64_t h_global = 0, uint64_t row0 = 0);

    std::vector<FriRound> rounds;
    std::vector<DevBuf<Ef>> keep_vecs;
    std::vector<DevBuf<uint32_t>> keep_trees;
    // challenger | round roots | final values in ONE block: one D2H brings all three back at the end
    // (three copies were three launches on the stream); the pointers below look into it
    DevBuf<uint32_t> d_block;
    struct { uint32_t* p = nullptr; } d_chal, d_roots;
    struct { Ef* p = nullptr; } d_final;
    DevBuf<Ef> d_betas;
    uint32_t R_total = 0;
    uint64_t final_len = 0;
    // the tail kernel's proof-of-work hint (word FRI_POW_WORD of the challenger's 64-word slot): the
    // witness it found, or FRI_POW_NONE
    uint32_t pow_hint = 0xffffffffu;
    DevChallenger* dch() { return reinterpret_cast<DevChallenger*>(d_chal.p); }
};
constexpr size_t FRI_POW_WORD = 40;

// moves the transcript to the device and sizes the per-round buffers
void fri_commit_begin(Context& ctx, const FriConfig& fri, unsigned log_max_height,
                      const BfChallenger& challenger, FriCommit& st);
// prover.rs:111-127 on a vector every rank holds whole (it becomes st.cur): rounds until `blowup` values are
// left, adding inputs[next_in..] when the folded length reaches theirs (:124-126)
void fri_commit_rounds(Context& ctx, const FriConfig& fri, DevBuf<Ef> folded, uint64_t len,
                       std::vector<DevBuf<Ef>>& inputs, const std::vector<unsigned>& log_lens,
                       size_t next_in, FriCommit& st);
// brings roots, final values and the transcript back; checks prover.rs:129-134; returns final_poly
Ef fri_commit_finish(Context& ctx, const FriConfig& fri, BfChallenger& challenger, FriCommit& st);
// prover.rs:43 challenger.grind(bits): takes the device's hint if one step of the host transcript
// confirms it, grinds on the host otherwise
uint32_t fri_pow_witness(Context& ctx, BfChallenger& challenger, unsigned bits, const FriCommit& st);

// ---- the LDE stage of a commitment (two_adic_pcs.rs:227-241): fills data.ldes / lde_storage /
// log_height and consumes `evals`.  A batch of equal-height matrices gets ONE allocation, matrix after
// matrix (columns_as_one_matrix below then holds).  n_beta > 0: only the cosets beta0 .. beta0 + n_beta - 1
// of every LDE (the slab of a sharded rank; matrices of one height).  allow_pair: exactly two column-major
// matrices of one shape go through ONE set of LDE launches (TS_LDE_PAIR=0 turns that off).
void lde_stage(Context& ctx, const FriConfig& fri, std::vector<DeviceMatrix>& evals,
               const std::vector<uint32_t>& domain_shifts, uint32_t beta0, uint32_t n_beta, bool allow_pair,
               PcsData& data, bool keep_row_major = false);
// (keep_row_major: a row-major input is only read -- it is transposed into a buffer of the stage's own -- and
// is left to the caller instead of being released)

// ---- where the reduced opening is computed on the low coset and extended (open_reduce_slab): whole LDEs without
// a preprocessed round (the caller's test), from REDUCE_LOW_MIN_WIDTH opened columns (trace + chunk columns) up
// -- below it a proof is bound by its launches and the extension's extra ones cost more than the rows save
// (profiles/reduce_low_coset_crossover.txt).  TS_REDUCE_LOW = 0 never / 1 always, read on every call.
constexpr uint32_t REDUCE_LOW_MIN_WIDTH = 72;
bool reduce_low_wanted(uint32_t opened_columns);

// ---- the statement of a proof (uni-stark/src/prover.rs:43-46), checked
struct Statement {
    unsigned log_degree, lqd;
    uint32_t qd;  // quotient chunks
    unsigned log_N;
    uint32_t w;
};
Statement check_statement(const FriConfig& fri, const AirProgram& air, uint32_t trace_width, uint64_t degree,
                          size_t n_public_values);

// ---- host numerics
// the constant table of an AIR's program for one statement (D_CONST reads it): constants and the `n` public
// values `pis`, Montgomery form, at least one word; refuses a public value that is not canonical
std::vector<uint32_t> air_consts_mont(const AirProgram& air, const uint32_t* pis, size_t n);
// ((z/s)^n - 1)/n, the factor in front of the barycentric sum over the coset s H_n (canonical)
Ef bary_scale(Ef point, uint32_t coset_gen, uint64_t n);
// split_domains (prover.rs:80): chunk c of the quotient lives on the coset base_shift * omega_{n qd}^c
std::vector<uint32_t> chunk_domain_shifts(uint32_t base_shift, unsigned log_degree, unsigned lqd);

// ---- the one place that knows the TSPF word order (parsed by verifier.cpp,
// wire.cpp, the Rust binding and the oracle).  Appends to `out`.
constexpr uint32_t TSPF_MAGIC = 0x46505354u;
class ProofWriter {
public:
    struct Path { const uint32_t* digests; size_t depth; };               // one stretch of a Merkle path
    struct Batch { const std::vector<ColMat>* mats; unsigned depth; };    // a committed batch as opened
    // swap_path_bytes: paths arrive as SHA-256 state words and leave as their bytes read little-endian
    explicit ProofWriter(std::vector<uint32_t>& out, bool swap_path_bytes = false)
        : out_(out), swap_(swap_path_bytes) {}
    // words of one answered query (the same for every query of a proof)
    static size_t words_per_query(const std::vector<Batch>& batches, const std::vector<unsigned>& round_depths,
                                  size_t n_pass_through = 0);

    void words(const uint32_t* p, size_t n) { out_.insert(out_.end(), p, p + n); }
    // version 1; 2 with the extra num_queries word; 3 with the extra preprocessed_width word; 4 with the extra
    // aux_width word (the caller appends n_challenges and n_exposed)
    void header(uint32_t version, unsigned log_degree, uint32_t width, uint32_t qd, uint32_t extra);
    // version 6 (prove_multi): [magic, 6, T], then T x [log_degree, width, qd] in table order; version 7
    // (prove_multi_bus): [magic, 7, T], then T x [log_degree, width, qd, aux_width, n_exposed]; version 8
    // (prove_multi_key): the same with preprocessed_width as a sixth word per table
    struct TableShape { unsigned log_degree; uint32_t width, qd, aux_width, n_exposed, preprocessed_width = 0; };
    void header_multi(const std::vector<TableShape>& tables, uint32_t version = 6);
    void commitment(const uint32_t* roots, size_t n_words) { words(roots, n_words); }  // 8, or Q x 8 (taptrees)
    void opened_values(const std::vector<Ef>& values);
    void begin_rounds(uint32_t n_rounds) { out_.push_back(n_rounds); }  // then one commitment() per round
    void begin_queries(uint32_t n_queries) { out_.push_back(n_queries); }
    // per query: the input proof (n BatchOpenings, or n pass-through values), then one opening per round
    void begin_input_proof(uint32_t n) { out_.push_back(n); }
    void pass_through_value(unsigned log_height, const uint32_t value[4]);
    void batch_opening(const std::vector<ColMat>& mats, const uint32_t* row, unsigned depth,
                       std::initializer_list<Path> path);
    void round_opening(const uint32_t values[8], unsigned depth, std::initializer_list<Path> path);
    void finish(Ef final_poly, uint32_t pow_witness);

private:
    void path(std::initializer_list<Path> parts);
    std::vector<uint32_t>& out_;
    bool swap_;
};

// ---- the query-phase gather (bf_answer_query, fri/src/prover.rs:69-90, and open_input, two_adic_pcs.rs:
// 399-414): everything between "the indices are sampled" and "the ProofWriter serialises the answers".
// The caller registers index lists and adds jobs against them; every add returns the slot of its result
// ([query of the list][words of one answer]) in the one output buffer.  run() then sends every row job,
// descriptor and index in ONE upload, launches k_gather_queries once per index list and brings the answers
// back in ONE D2H (it synchronises); data(slot, j) is the answer to query j of the job's list.
// Row = index >> shift in every job.
class QueryGather {
public:
    struct Slot { size_t at = 0, words = 0; };  // word offset in the output buffer, words per query
    struct Opening { Slot vals, path; };
    explicit QueryGather(Context& ctx) : ctx_(ctx) {}
    unsigned add_indices(const std::vector<uint32_t>& indices);  // -> the list's number
    // the opened rows of a committed batch: total_width words per query
    Slot add_rows(unsigned list, const LeafMats& mats, unsigned shift);
    // a Merkle path: 8 * log_leaves words per query
    Slot add_path(unsigned list, const uint32_t* tree, unsigned log_leaves, unsigned shift);
    // a FRI round opening: the row of two values (8 words per query) and its path
    Opening add_round(unsigned list, const Ef* vec, const uint32_t* tree, unsigned log_leaves, unsigned shift);
    // values only: the row of two values (8 words per query)
    Slot add_values(unsigned list, const Ef* vec, unsigned shift);
    void run();
    const uint32_t* data(Slot s, size_t query) const { return out_.data() + s.at + query * s.words; }

private:
    struct List {
        std::vector<uint32_t> indices;
        std::vector<RowGatherJob> rows;
        std::vector<FriGatherDesc> descs;
        uint32_t max_row_width = 0, max_log_leaves = 0;
    };
    Slot take(const List& l, size_t words_per_query);
    Opening add_desc(unsigned list, const Ef* vec, const uint32_t* tree, unsigned log_leaves, unsigned shift);
    Context& ctx_;
    std::vector<List> lists_;
    std::vector<uint32_t> out_;
    size_t words_ = 0;
};

// ---- small host helpers
void h2d(Context& ctx, void* dst, const void* src, size_t bytes);
void d2h_sync(Context& ctx, void* dst, const void* src, size_t bytes);
Ef efc_mul(Ef a, Ef b);
Ef efc_mul_base(Ef a, uint32_t b);
Ef efc_pow(Ef a, uint64_t e);

}  // namespace ts
