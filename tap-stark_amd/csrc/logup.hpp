// LogUp aux columns (logup.hip): the spec as the C ABI hands it over, and the builder.
#pragma once
#include <memory>
#include <vector>

#include "prover_internal.hpp"

namespace ts {

// limits of a spec, enforced with TS_ERR_INVALID: the kernel holds one batch of denominators in registers and
// takes the whole spec as a launch argument
constexpr uint32_t LOGUP_MAX_INTERACTIONS = 16;
constexpr uint32_t LOGUP_MAX_VALUES = 8;

struct LogupTerm {
    uint32_t kind;   // 0: the canonical constant `value`; 1: main column `value`, local row; 2: column `value` of
                     // the preprocessed table, local row (logup_aux_build with takes_table only)
    uint32_t value;
};
struct LogupInteraction {
    LogupTerm multiplicity;
    std::vector<LogupTerm> values;
};
struct LogupSpec {
    std::vector<LogupInteraction> interactions;
};

// 4 * (ceil(K / 2) + 1); throws TS_ERR_INVALID on a spec outside the limits (a term kind above max_kind included)
uint32_t logup_aux_width(const LogupSpec& spec, uint32_t max_kind = 1);
// The n x aux_width row-major aux matrix of `trace` (row-major, this context) for challenges = gamma ++ beta
// (canonical), and the exposed sum S.  Throws TS_ERR_INVARIANT naming the first (row, interaction) whose
// denominator is zero; synchronises the stream once.
// takes_table: terms of kind 2 are allowed and read `table`, the row-major values of the preprocessed columns
// (this context, the trace's height, not consumed; may be null for a spec without such terms).
DeviceMatrix logup_aux_build(Context& ctx, const LogupSpec& spec, const DeviceMatrix& trace,
                             const uint32_t challenges[8], uint32_t exposed[4], const DeviceMatrix* table = nullptr,
                             bool takes_table = false);

// The same for T traces with ONE set of challenges (the LogUp bus of a multi-table proof): aux matrix k is word for
// word logup_aux_build(specs[k], traces[k]) and exposed[4k .. 4k+3] its S.  The specs travel in a job table in
// device memory; three launches over the workgroups of all tables, one upload, one copy back.  Terms of kind 0 and
// 1 only.  Throws what the single call throws, before anything is allocated, and TS_ERR_INVARIANT naming the least
// (table, row, interaction) whose denominator is zero (table k is called table_ids[k] there, if given);
// synchronises the stream once.
// `tables` (logup_aux_build_multi_pre): one entry per spec, the row-major values of that table's preprocessed columns
// or null; terms of kind 2 are then allowed and read it, as logup_aux_build with takes_table does.  A job without a
// table runs the body it runs without `tables`.
constexpr uint32_t LOGUP_MAX_TABLES = 64;
std::vector<DeviceMatrix> logup_aux_build_multi(Context& ctx, const std::vector<const LogupSpec*>& specs,
                                                const std::vector<const DeviceMatrix*>& traces,
                                                const uint32_t challenges[8], uint32_t* exposed,
                                                const uint32_t* table_ids = nullptr,
                                                const std::vector<const DeviceMatrix*>* tables = nullptr);

// ---- several tables in one proof (prove_multi.cpp; TSPF v6, v7 and v8)
struct MultiBusTable {
    const AirProgram* air = nullptr;   // aux columns exactly with n_challenges 2, n_exposed 4
    DeviceMatrix trace;                // consumed; row-major where the AIR has aux columns
    std::vector<uint32_t> public_values;
    const LogupSpec* logup = nullptr;  // null exactly for an AIR without aux columns (a plain table)
};
// One committed batch of preprocessed matrices of mixed heights, on their natural domains; made once, consumed by
// no proof.  `values[i]`: the row-major input of matrix i, kept alive by the commit (no second copy) and owned by
// whoever made the key, where it was made with keep_values; null otherwise.
struct MultiKey {
    std::unique_ptr<PcsData> data;
    std::vector<const DeviceMatrix*> values;
    std::vector<uint64_t> heights;  // natural heights
    std::vector<uint32_t> widths;
    unsigned log_blowup = 0;
    Context* ctx = nullptr;
};
// What a call makes of a round that only some statements have (the key's, the aux matrices'): never there, there in
// every statement, or there where a table has such columns.
enum class MultiRound { NEVER, ALWAYS, AS_TABLES_HAVE };
struct MultiCall {
    const char* name;       // leads every text
    MultiRound key, aux;
    const FriConfig* fri;   // null: the shape rules that need none (widths, public values; every trace row-major)
};
// the calls there are: version 6 prove_multi (tied by nothing: plain tables), 7 prove_multi_bus (a LogUp bus: at least
// one aux table, no key), 8 prove_multi_key (fixed tables on the bus: a key, aux tables or none); any other version
// check_multi, the debug counterpart of the bus proofs (`fri` is not looked at; a key exactly when a table has
// preprocessed columns, made with keep_values)
MultiCall multi_call(uint32_t version, const FriConfig* fri);
// The one statement walk, on shapes alone; nothing is consumed.  Throws what prove() throws for a table alone
// (check_statement); TS_ERR_UNSUPPORTED for columns of a round the call never has; TS_ERR_INVALID for more than 64
// tables or chunks, for a spec that is missing, unwanted or does not fit its AIR, trace and key matrix, for a
// column-major trace under an aux table, for a statement without a round the call always has, for a null key, a key no
// table uses and a key whose count, heights, widths, blowup or kept values do not fit.  The i-th table with
// preprocessed columns, in table order, reads key matrix i; a spec's kind-2 terms read the table's key matrix.
void check_multi_statement(const MultiCall& call, const std::vector<MultiBusTable>& tables, const MultiKey* key);
// The three provers, one body; each checks its statement first.  prove_multi_bus: gamma and beta once for every table,
// one commit of the LogUp matrices.  prove_multi_key: the key's root observed after the shapes, the key matrices as
// the first side matrix of their tables' quotients and as the first opened round; without any aux table the challenge
// phase is skipped whole.  Throw TS_ERR_INVARIANT naming (table, row, interaction) of a zero denominator; the traces
// are consumed by then.
std::vector<uint32_t> prove_multi(TwoAdicFriPcs& pcs, BfChallenger& challenger, std::vector<MultiBusTable>& tables);
std::vector<uint32_t> prove_multi_bus(TwoAdicFriPcs& pcs, BfChallenger& challenger, std::vector<MultiBusTable>& tables);
std::vector<uint32_t> prove_multi_key(TwoAdicFriPcs& pcs, BfChallenger& challenger, std::vector<MultiBusTable>& tables,
                                      const MultiKey& key);
// TS_MULTI_LOGUP_PER_TABLE=1 (read on every call; a test and measurement knob): prove_multi_bus loops
// logup_aux_build per table instead of logup_aux_build_multi.  Same proof.
bool multi_logup_per_table();

// ---- the multiplicity column of one table (logup_mult.hip)
constexpr uint32_t LOGUP_MULT_MAX_LOOKUPS = 16;

struct LogupMultSpec {
    std::vector<LogupTerm> table;     // n_values terms: the table's tuple on row t
    std::vector<LogupTerm> lookups;   // n_lookups * n_values terms: lookup l's tuple on row r
    std::vector<LogupTerm> weights;   // n_lookups terms: lookup l's weight on row r
    uint32_t out_column = 0;          // the main column that receives the result
    uint32_t negate = 0;              // 1: p - sum
};
struct LogupMultResult {
    uint64_t n_missing, first_missing;  // lookups of non-zero weight in no table row; the least r * n_lookups + l (~0: none)
};
// Overwrites trace[t][out_column] (row-major, this context, not consumed) for every t with the field sum of the
// weights of the lookups whose tuple is the table's tuple on row t -- on the lowest row of each class of equal
// table rows, 0 on the others -- or p minus it.  `table`: the row-major values of the preprocessed columns for
// kind-2 terms (the trace's height, this context; may be null without such terms).  Throws TS_ERR_INVALID before
// any device work on a spec outside the limits (out_column among the main columns it reads included);
// synchronises the stream once.
LogupMultResult logup_multiplicities(Context& ctx, const LogupMultSpec& spec, DeviceMatrix& trace,
                                     const DeviceMatrix* table);

// ---- the same with the lookups in OTHER traces: the table side of a LogUp bus (logup_mult.hip)
constexpr uint32_t LOGUP_MULT_MAX_LOOKERS = 16;
struct LogupMultLooker {
    std::vector<LogupTerm> lookups;   // n_lookups * n_values terms over THIS looker's row
    std::vector<LogupTerm> weights;   // n_lookups terms over this looker's row
};
struct LogupMultBusSpec {
    std::vector<LogupTerm> table;     // n_values terms over the TABLE trace's row; kinds 0 and 1 on every side
    std::vector<LogupMultLooker> lookers;
    uint32_t out_column = 0;          // the column of the table trace that receives the result
    uint32_t negate = 0;
};
struct LogupMultBusResult {
    uint64_t n_missing;               // lookups of non-zero weight in no table row, over all lookers
    uint64_t looker, row, lookup;     // the least miss in that lexicographic order (~0 each: none)
};
// logup_multiplicities with the lookups on the rows of `lookers` (row-major, this context, any heights, read only;
// one of them may be the table trace itself): same classes, sums, skipped zero weights and words on every run.  One
// k_mult_insert launch over the table, one k_mult_count launch per looker, one k_mult_write launch, one copy back.
// Throws TS_ERR_INVALID before any device work, as the single-trace call does per matrix; out_column may be read
// by no term over the table trace.
// takes_pre (logup_multiplicities_bus_pre): the TABLE's terms may be of kind 2 and read `table_pre`, the row-major
// values of the table's preprocessed columns (the table trace's height, this context, not consumed; may be null
// without such terms); the lookers keep kinds 0 and 1.
LogupMultBusResult logup_multiplicities_bus(Context& ctx, const LogupMultBusSpec& spec, DeviceMatrix& trace,
                                            const std::vector<const DeviceMatrix*>& lookers,
                                            const DeviceMatrix* table_pre = nullptr, bool takes_pre = false);

// ---- the exact balance of a whole bus, before any challenge (bus_check.hip)
// The refusals logup_aux_build_multi makes with `tables` about one spec, its trace and its preprocessed table (null
// without kind-2 terms), and nothing else: no allocation, no device work.
void logup_check_spec(Context& ctx, const LogupSpec& spec, const DeviceMatrix& trace, const DeviceMatrix* table);
constexpr uint64_t BUS_CHECK_MAX_CONTRIBUTIONS = 1ull << 30;  // sum over the tables of height * interactions
struct BusShare {
    uint64_t count = 0;                        // table k's contributions to the reported tuple
    uint32_t sum = 0;                          // their multiplicity sum mod p
    uint32_t first_row = ~0u, first_interaction = ~0u;  // the least (row, interaction) among them, ~0 without any
};
struct BusReport {
    uint64_t n_contributions = 0;              // (table, row, interaction) whose multiplicity is non-zero mod p
    uint64_t n_tuples = 0;                     // distinct zero-padded tuples among them
    uint64_t n_unbalanced = 0;                 // tuples whose multiplicities do not sum to 0 mod p
    uint32_t first_table = ~0u, first_row = ~0u, first_interaction = ~0u;  // the least contribution to any of those
    uint32_t n_values = 0;                     // of that contribution's interaction
    uint32_t tuple[LOGUP_MAX_VALUES] = {};     // its values, zero-padded
    uint32_t sum = 0;                          // its tuple's multiplicity sum, canonical, non-zero
    std::vector<BusShare> shares;              // one per table
};
// A hash join over the resident traces: for every distinct tuple (the value terms of an interaction, zero-padded to
// eight words and compared as stored) the field sum of the multiplicities over all tables, rows and interactions.
// specs[k] null: table k is not on the bus (its trace is not looked at).  `tables`: per spec the row-major values of
// its preprocessed columns or null, as logup_aux_build_multi takes them.  Reads the traces only; every output is a
// count, a minimum or an integer sum and the same on every run.  Throws TS_ERR_INVALID before any device work (what
// logup_check_spec refuses for any k, a count outside 1 .. 64, no spec at all, more than 2^30 possible contributions);
// synchronises the stream once, twice when the bus is unbalanced.
BusReport bus_check(Context& ctx, const std::vector<const LogupSpec*>& specs,
                    const std::vector<const DeviceMatrix*>& traces, const std::vector<const DeviceMatrix*>& tables);

// ---- a lookup proof inside a batch lane (prover.cpp): no launch of its own
// What a lookup argument says about an item's DATA, raised after the kernels finished normally: a zero denominator
// reported by the builder, a lookup found in no table row.  The context is sound, so a lane goes on after one.
struct LookupDataError : Error {
    using Error::Error;
};
// the text of a miss, as ts_logup_multiplicities reports it
std::string logup_miss_text(const LogupMultResult& r, uint32_t n_lookups);
// The aux source that runs `spec` on the live trace: logup_aux_build with takes_table and `table` (the lane's
// row-major table values; may be null for a spec without kind-2 terms; must outlive the source).  The builder's
// zero-denominator report leaves as a LookupDataError.
AuxSource logup_aux_source(Context& ctx, LogupSpec spec, const DeviceMatrix* table);
// prove_pre_aux of the trace as it stands after `fills`: each is logup_multiplicities on the row-major trace with
// `table`, in order, before the commit.  A fill that misses throws LookupDataError (logup_miss_text) after *miss
// received its counts; *miss is {0, ~0} otherwise.
std::vector<uint32_t> prove_lookup(TwoAdicFriPcs& pcs, const AirProgram& air, BfChallenger& challenger,
                                   DeviceMatrix trace, const std::vector<uint32_t>& public_values, const PcsData* key,
                                   const AuxSource& aux_source, const std::vector<LogupMultSpec>& fills,
                                   const DeviceMatrix* table, LogupMultResult* miss);

}  // namespace ts
