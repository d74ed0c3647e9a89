// The scans of ts_matrix_scan: the checks that need no matrix and the recurrences run row after row over host rows.
// No device code and no context: ts_scan_rows_host is all of this, and scan.hip makes the same checks first.
#include "scan.hpp"

#include <string>

#include "context.hpp"

namespace ts {

ScanPlan scan_check(const ScanSpec& spec, uint32_t src_width) {
    const size_t n = spec.columns.size();
    TS_REQUIRE(n >= 1 && n <= SCAN_MAX_COLUMNS, TS_ERR_INVALID,
               "scan: n_columns " + std::to_string(n) + " outside [1, " + std::to_string(SCAN_MAX_COLUMNS) + "]");
    TS_REQUIRE(src_width >= 1 && src_width <= SCAN_MAX_WIDTH, TS_ERR_INVALID, "scan: src_width outside [1, 2^16]");
    uint32_t widest = src_width, past_dst = 0;
    for (size_t k = 0; k < n; k++) {
        const ScanColumn& c = spec.columns[k];
        const std::string at = "scan: column " + std::to_string(k) + ": ";
        TS_REQUIRE(c.a_kind <= 1 && c.b_kind <= 1, TS_ERR_INVALID, at + "term kind must be 0 (constant) or 1 (column)");
        TS_REQUIRE(c.a_kind == 1 || c.a_value < P, TS_ERR_INVALID, at + "the constant a is not below p");
        TS_REQUIRE(c.b_kind == 1 || c.b_value < P, TS_ERR_INVALID, at + "the constant b is not below p");
        TS_REQUIRE(c.a_kind == 0 || c.a_value < src_width, TS_ERR_INVALID, at + "the column of a is outside the source");
        TS_REQUIRE(c.b_kind == 0 || c.b_value < src_width, TS_ERR_INVALID, at + "the column of b is outside the source");
        TS_REQUIRE(c.init < P, TS_ERR_INVALID, at + "init is not below p");
        TS_REQUIRE(c.reset_column == SCAN_NO_RESET || c.reset_column < src_width, TS_ERR_INVALID,
                   at + "the reset column is outside the source");
        TS_REQUIRE(c.flags <= SCAN_EXCLUSIVE, TS_ERR_INVALID, at + "unknown flag bits");
        TS_REQUIRE(c.dst_column < SCAN_MAX_WIDTH, TS_ERR_INVALID, at + "the matrix would be wider than 2^16 columns");
        if (c.dst_column + 1 > widest) widest = c.dst_column + 1;
        if (c.dst_column + 1 > past_dst) past_dst = c.dst_column + 1;
    }
    ScanPlan plan;
    plan.src_width = src_width;
    plan.out_width = spec.out_width ? spec.out_width : widest;
    TS_REQUIRE(plan.out_width >= past_dst && plan.out_width <= widest, TS_ERR_INVALID,
               "scan: out_width " + std::to_string(spec.out_width) + " outside [" + std::to_string(past_dst) + ", " +
                   std::to_string(widest) + "] (1 + the last dst column, the full width)");
    plan.named.assign((plan.out_width + 31) / 32, 0);
    for (const ScanColumn& c : spec.columns) {
        const uint32_t d = c.dst_column;
        TS_REQUIRE(!((plan.named[d >> 5] >> (d & 31)) & 1), TS_ERR_INVALID,
                   "scan: column " + std::to_string(d) + " is the dst of two scans");
        plan.named[d >> 5] |= 1u << (d & 31);
    }
    for (uint32_t c = src_width; c < plan.out_width; c++)
        TS_REQUIRE((plan.named[c >> 5] >> (c & 31)) & 1, TS_ERR_INVALID,
                   "scan: column " + std::to_string(c) + " is beyond the source and no scan writes it");
    return plan;
}

void scan_rows_host(const ScanSpec& spec, const ScanPlan& plan, const uint32_t* src, uint64_t height, uint32_t* out,
                    uint32_t* finals) {
    const size_t n = spec.columns.size();
    uint64_t y[SCAN_MAX_COLUMNS];
    for (size_t k = 0; k < n; k++) y[k] = spec.columns[k].init;
    for (uint64_t row = 0; row < height; row++) {
        const uint32_t* r = src + row * plan.src_width;
        uint32_t* o = out + row * plan.out_width;
        for (uint32_t c = 0; c < plan.out_width; c++)
            if (!((plan.named[c >> 5] >> (c & 31)) & 1)) o[c] = r[c];
        for (size_t k = 0; k < n; k++) {
            const ScanColumn& c = spec.columns[k];
            const uint64_t a = (c.a_kind ? r[c.a_value] : c.a_value) % P, b = (c.b_kind ? r[c.b_value] : c.b_value) % P;
            if (c.reset_column != SCAN_NO_RESET && r[c.reset_column] % P != 0) y[k] = c.init;
            const uint64_t before = y[k];
            y[k] = (a * before + b) % P;
            o[c.dst_column] = (uint32_t)(c.flags & SCAN_EXCLUSIVE ? before : y[k]);
        }
    }
    if (finals)
        for (size_t k = 0; k < n; k++) finals[k] = (uint32_t)y[k];
}

}  // namespace ts
