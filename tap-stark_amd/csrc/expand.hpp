// Expanded rows: every row of one resident row-major matrix repeated by a count read from the row itself, each copy
// reshaped to one tuple form, in (row, inner index) order, padded to a power of two (include/tapstark.h "expanded
// rows").  The inverse of the collect: a load-balanced expansion.  expand.cpp holds the checks, the plan, the height
// rule and the plain sequential loop over host rows; expand.hip the three kernels.  How many rows a source row asks
// for, and what a term of an output row is, are written once here, for both.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bb.hpp"

namespace ts {

constexpr uint32_t EXPAND_MAGIC = 0x50584554u;       // "TEXP"
constexpr uint32_t EXPAND_MAX_WIDTH = 64;            // of the output
constexpr uint32_t EXPAND_MAX_SRC_WIDTH = 1u << 16;  // as the collect
constexpr uint64_t EXPAND_MAX_HEIGHT = 1ull << 27;   // of the source and of the output
constexpr uint32_t EXPAND_MAX_COUNT = 1u << 27;      // of max_count
constexpr uint32_t EXPAND_NO_COLUMN = 0xFFFFFFFFu;   // ExpandPlan::sel: every row; ExpandPlan::count_col: the constant
constexpr size_t EXPAND_HEADER = 9;

enum ExpandTerm : uint32_t {
    X_CONST = 0, X_COL = 1, X_ROW = 2, X_INNER = 3, X_REMAINING = 4, X_FIRST = 5, X_LAST = 6, X_STEPPED = 7
};

struct ExpandTermWord {
    uint32_t kind, value, step;
};

// What the checks leave.
struct ExpandPlan {
    uint32_t src_width = 0, out_width = 0;
    uint32_t sel = EXPAND_NO_COLUMN;        // the selector column, or every row
    uint32_t count_col = EXPAND_NO_COLUMN;  // the count column, or the constant
    uint32_t count_const = 0;               // 1 .. max_count, where count_col is EXPAND_NO_COLUMN
    uint32_t max_count = 0;
    std::vector<uint32_t> pad;            // out_width
    std::vector<ExpandTermWord> terms;    // out_width
};

// The rows a source row asks for: 0 where the selector word, reduced mod p, is 0 (the collect's rule: 0, p and 2p do not
// fire, 0xFFFFFFFF does); else the count word reduced mod p (p asks for 0 rows, p + 3 for 3), or the constant.  Below
// p; whether it is over max_count is the caller's question.
TS_HD uint32_t expand_row_count(const uint32_t* row, uint32_t sel, uint32_t count_col, uint32_t count_const) {
    if (sel != EXPAND_NO_COLUMN && row[sel] % P == 0) return 0;
    return count_col == EXPAND_NO_COLUMN ? count_const : row[count_col] % P;
}

// The word of one term on output row (source row r, inner index j of cnt).
TS_HD uint32_t expand_term(const ExpandTermWord& t, const uint32_t* row, uint64_t r, uint32_t j, uint32_t cnt) {
    switch (t.kind) {
        case X_CONST: return t.value;
        case X_COL: return row[t.value];  // as stored
        case X_ROW: return (uint32_t)r;
        case X_INNER: return j;
        case X_REMAINING: return cnt - 1 - j;
        case X_FIRST: return j == 0;
        case X_LAST: return j == cnt - 1;
        default: return (uint32_t)(((uint64_t)(row[t.value] % P) + (uint64_t)j * t.step) % P);  // X_STEPPED
    }
}

// What the rows ask for together, and the least row over max_count.
struct ExpandTotals {
    uint64_t total = 0;      // the sum of all counts, exact
    uint64_t bad_row = ~0ull;  // the least row asking for more than max_count, ~0 when there is none
    uint64_t bad_count = 0;  // its count
};

// Every rule that needs no matrix; throws TS_ERR_INVALID with a text.
ExpandPlan expand_check(const uint32_t* spec, size_t n_words);
// out_height as the caller gave it: 0 or a power of two in [1, 2^27]; throws TS_ERR_INVALID
void expand_check_out_height(uint64_t out_height);
// The height of the result, or the refusal: TS_ERR_INVARIANT "expand: row R asks for C rows, max_count M" first, then
// TS_ERR_INVALID "expand: N rows asked for, out_height H".
uint64_t expand_height(const ExpandPlan& plan, const ExpandTotals& t, uint64_t out_height);
ExpandTotals expand_count_host(const ExpandPlan& plan, const uint32_t* src, uint64_t height);
// out (out_height x out_width, row-major): the plain sequential loop, then the pad rows.
void expand_rows_host(const ExpandPlan& plan, const uint32_t* src, uint64_t height, uint64_t out_height, uint32_t* out);
// A new row-major matrix (expand.hip) from the plan of a checked spec and its source: row-major, on ctx, read only.
// Throws TS_ERR_INVALID before any device work, and one of the two refusals of expand_height after the one host wait.
// Three launches.
struct Context;
struct DeviceMatrix;
DeviceMatrix expand_matrix(Context& ctx, const ExpandPlan& plan, const DeviceMatrix& src, uint64_t out_height,
                           uint64_t* n_live);

}  // namespace ts
