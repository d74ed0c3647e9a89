// LogUp aux columns (logup.hip): the spec as the C ABI hands it over, and the builder.
#pragma once
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
