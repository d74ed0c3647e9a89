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

}  // namespace ts
