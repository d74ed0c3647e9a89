// The spec of ts_matrix_expand_rows: the checks that need no matrix, the plan they leave, the height rule with its two
// refusals, and the plain sequential loop over host rows.  No device code and no context: ts_expand_check and
// ts_expand_rows_host are all of this, and ts_matrix_expand_rows makes the same checks first.
#include "expand.hpp"

#include <string>

#include "context.hpp"

namespace ts {

ExpandPlan expand_check(const uint32_t* spec, size_t n_words) {
    TS_REQUIRE(spec != nullptr, TS_ERR_INVALID, "expand: null spec");
    TS_REQUIRE(n_words >= EXPAND_HEADER, TS_ERR_INVALID, "expand: the spec is shorter than its header");
    TS_REQUIRE(spec[0] == EXPAND_MAGIC, TS_ERR_INVALID, "expand: bad magic (not a TEXP spec)");
    TS_REQUIRE(spec[1] == 1, TS_ERR_INVALID, "expand: unknown spec version " + std::to_string(spec[1]));
    const uint32_t src_width = spec[2], out_width = spec[3];
    TS_REQUIRE(src_width >= 1 && src_width <= EXPAND_MAX_SRC_WIDTH, TS_ERR_INVALID,
               "expand: src_width " + std::to_string(src_width) + " outside [1, 2^16]");
    TS_REQUIRE(out_width >= 1 && out_width <= EXPAND_MAX_WIDTH, TS_ERR_INVALID,
               "expand: out_width " + std::to_string(out_width) + " outside [1, " + std::to_string(EXPAND_MAX_WIDTH) + "]");
    const size_t want = EXPAND_HEADER + 4 * (size_t)out_width;
    TS_REQUIRE(n_words == want, TS_ERR_INVALID,
               "expand: " + std::to_string(n_words) + " words, the header asks for " + std::to_string(want));
    const uint32_t sel_kind = spec[4], sel_value = spec[5], count_kind = spec[6], count_value = spec[7];
    const uint32_t max_count = spec[8];
    TS_REQUIRE(max_count >= 1 && max_count <= EXPAND_MAX_COUNT, TS_ERR_INVALID,
               "expand: max_count " + std::to_string(max_count) + " outside [1, 2^27]");
    TS_REQUIRE(sel_kind <= 1, TS_ERR_INVALID, "expand: selector kind must be 0 (always) or 1 (column)");
    TS_REQUIRE(sel_kind == 1 || sel_value == 1, TS_ERR_INVALID, "expand: a constant selector must be 1");
    TS_REQUIRE(sel_kind == 0 || sel_value < src_width, TS_ERR_INVALID, "expand: the selector column is outside the source");
    TS_REQUIRE(count_kind <= 1, TS_ERR_INVALID, "expand: count kind must be 0 (constant) or 1 (column)");
    TS_REQUIRE(count_kind == 1 || (count_value >= 1 && count_value <= max_count), TS_ERR_INVALID,
               "expand: a constant count must be in [1, max_count]");
    TS_REQUIRE(count_kind == 0 || count_value < src_width, TS_ERR_INVALID, "expand: the count column is outside the source");

    ExpandPlan plan;
    plan.src_width = src_width;
    plan.out_width = out_width;
    plan.sel = sel_kind ? sel_value : EXPAND_NO_COLUMN;
    plan.count_col = count_kind ? count_value : EXPAND_NO_COLUMN;
    plan.count_const = count_kind ? 0 : count_value;
    plan.max_count = max_count;
    const uint32_t* w = spec + EXPAND_HEADER;
    for (uint32_t c = 0; c < out_width; c++, w++) {
        TS_REQUIRE(*w < P, TS_ERR_INVALID, "expand: pad word " + std::to_string(c) + " is not below p");
        plan.pad.push_back(*w);
    }
    for (uint32_t c = 0; c < out_width; c++, w += 3) {
        const uint32_t kind = w[0], value = w[1], step = w[2];
        const std::string term = "expand: term " + std::to_string(c) + ": ";
        TS_REQUIRE(kind <= X_STEPPED, TS_ERR_INVALID, term + "kind must be in [0, 7]");
        TS_REQUIRE(kind != X_CONST || value < P, TS_ERR_INVALID, term + "the constant is not below p");
        TS_REQUIRE((kind != X_COL && kind != X_STEPPED) || value < src_width, TS_ERR_INVALID,
                   term + "the column is outside the source");
        TS_REQUIRE(kind < X_ROW || kind > X_LAST || value == 0, TS_ERR_INVALID,
                   term + "the value word of kinds 2 to 6 must be 0");
        TS_REQUIRE(kind == X_STEPPED || step == 0, TS_ERR_INVALID, term + "the step word must be 0 for every kind but 7");
        TS_REQUIRE(step < P, TS_ERR_INVALID, term + "the step is not below p");
        plan.terms.push_back({kind, value, step});
    }
    return plan;
}

void expand_check_out_height(uint64_t out_height) {
    TS_REQUIRE(out_height <= EXPAND_MAX_HEIGHT && (out_height & (out_height - 1)) == 0, TS_ERR_INVALID,
               "expand: out_height " + std::to_string(out_height) + " is neither 0 nor a power of two in [1, 2^27]");
}

uint64_t expand_height(const ExpandPlan& plan, const ExpandTotals& t, uint64_t out_height) {
    TS_REQUIRE(t.bad_row == ~0ull, TS_ERR_INVARIANT,
               "expand: row " + std::to_string(t.bad_row) + " asks for " + std::to_string(t.bad_count) +
                   " rows, max_count " + std::to_string(plan.max_count));
    const uint64_t limit = out_height ? out_height : EXPAND_MAX_HEIGHT;
    TS_REQUIRE(t.total <= limit, TS_ERR_INVALID,
               "expand: " + std::to_string(t.total) + " rows asked for, out_height " + std::to_string(limit));
    if (out_height) return out_height;
    uint64_t h = 1;
    while (h < t.total) h <<= 1;
    return h;
}

ExpandTotals expand_count_host(const ExpandPlan& plan, const uint32_t* src, uint64_t height) {
    ExpandTotals t;
    for (uint64_t r = 0; r < height; r++) {
        const uint32_t cnt = expand_row_count(src + r * plan.src_width, plan.sel, plan.count_col, plan.count_const);
        t.total += cnt;
        if (cnt > plan.max_count && t.bad_row == ~0ull) {
            t.bad_row = r;
            t.bad_count = cnt;
        }
    }
    return t;
}

void expand_rows_host(const ExpandPlan& plan, const uint32_t* src, uint64_t height, uint64_t out_height, uint32_t* out) {
    const uint32_t W = plan.out_width;
    uint64_t at = 0;
    for (uint64_t r = 0; r < height; r++) {
        const uint32_t* row = src + r * plan.src_width;
        const uint32_t cnt = expand_row_count(row, plan.sel, plan.count_col, plan.count_const);
        for (uint32_t j = 0; j < cnt; j++, at++)
            for (uint32_t c = 0; c < W; c++) out[at * W + c] = expand_term(plan.terms[c], row, r, j, cnt);
    }
    for (; at < out_height; at++)
        for (uint32_t c = 0; c < W; c++) out[at * W + c] = plan.pad[c];
}

}  // namespace ts
