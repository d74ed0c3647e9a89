// The spec of ts_matrix_join_rows: the checks that need no matrix but its width, the plan they leave, and the plain
// sequential loop over host rows.  No device code and no context: ts_join_check and ts_join_rows_host are all of this,
// and ts_matrix_join_rows makes the same checks first.
#include "join.hpp"

#include <algorithm>
#include <array>
#include <map>

#include "context.hpp"

namespace ts {

namespace {
void check_term(const std::string& at, const JoinTerm& t, uint32_t width, const char* matrix) {
    TS_REQUIRE(t.kind <= 1, TS_ERR_INVALID, at + "kind must be 0 (constant) or 1 (column)");
    TS_REQUIRE(t.kind != 0 || t.value < P, TS_ERR_INVALID, at + "the constant is not below p");
    TS_REQUIRE(t.kind != 1 || t.value < width, TS_ERR_INVALID, at + "the column is outside the " + matrix);
}
}  // namespace

JoinPlan join_check(const JoinSpecIn& spec, uint32_t src_width, uint32_t table_width) {
    TS_REQUIRE(spec.size_ok, TS_ERR_INVALID, "join: bad struct_size");
    TS_REQUIRE(spec.n_keys >= 1 && spec.n_keys <= JOIN_MAX_KEYS, TS_ERR_INVALID,
               "join: n_keys " + std::to_string(spec.n_keys) + " outside [1, " + std::to_string(JOIN_MAX_KEYS) + "]");
    TS_REQUIRE(spec.n_fetch <= JOIN_MAX_FETCH, TS_ERR_INVALID,
               "join: n_fetch " + std::to_string(spec.n_fetch) + " outside [0, " + std::to_string(JOIN_MAX_FETCH) + "]");
    TS_REQUIRE((spec.flags & ~JOIN_ALL_FLAGS) == 0, TS_ERR_INVALID, "join: unknown flag");
    TS_REQUIRE(spec.n_fetch != 0 || (spec.flags & (JOIN_TABLE_ROW | JOIN_HIT)), TS_ERR_INVALID,
               "join: nothing to write: n_fetch 0 and neither TS_JOIN_TABLE_ROW nor TS_JOIN_HIT");
    TS_REQUIRE(spec.src_keys && spec.table_keys, TS_ERR_INVALID, "join: null key terms");
    TS_REQUIRE(spec.n_fetch == 0 || (spec.table_columns && spec.dst_columns && spec.defaults), TS_ERR_INVALID,
               "join: null fetch arrays");
    TS_REQUIRE(src_width >= 1 && src_width <= JOIN_MAX_WIDTH, TS_ERR_INVALID, "join: the source's width outside [1, 2^16]");
    TS_REQUIRE(table_width >= 1, TS_ERR_INVALID, "join: the table's width is 0");

    JoinPlan plan;
    plan.n_keys = spec.n_keys;
    plan.flags = spec.flags;
    plan.src_width = src_width;
    plan.table_width = table_width;
    plan.table_rows = spec.table_rows;
    for (uint32_t q = 0; q < spec.n_keys; q++) {
        check_term("join: source key " + std::to_string(q) + ": ", spec.src_keys[q], src_width, "source");
        check_term("join: table key " + std::to_string(q) + ": ", spec.table_keys[q], table_width, "table");
        plan.src_keys[q] = spec.src_keys[q];
        plan.table_keys[q] = spec.table_keys[q];
    }
    check_term("join: when: ", spec.when, src_width, "source");
    plan.when = spec.when;

    struct Dst {
        uint32_t col, from, def;
    };
    std::vector<Dst> dst;
    uint32_t base = src_width;
    for (uint32_t f = 0; f < spec.n_fetch; f++) {
        const std::string at = "join: fetch " + std::to_string(f) + ": ";
        TS_REQUIRE(spec.table_columns[f] < table_width, TS_ERR_INVALID, at + "the column is outside the table");
        TS_REQUIRE(spec.dst_columns[f] < JOIN_MAX_WIDTH, TS_ERR_INVALID, at + "the result would be wider than 2^16");
        TS_REQUIRE(spec.defaults[f] < P, TS_ERR_INVALID, at + "the default is not below p");
        dst.push_back({spec.dst_columns[f], spec.table_columns[f], spec.defaults[f]});
        base = std::max(base, spec.dst_columns[f] + 1);
    }
    std::sort(dst.begin(), dst.end(), [](const Dst& a, const Dst& b) { return a.col < b.col; });
    for (size_t f = 1; f < dst.size(); f++)
        TS_REQUIRE(dst[f].col != dst[f - 1].col, TS_ERR_INVALID,
                   "join: dst column " + std::to_string(dst[f].col) + " appears twice");
    // every column behind the source is named: the sorted dst columns at or beyond src_width are src_width, +1, ...
    uint32_t next = src_width;
    for (const Dst& d : dst)
        if (d.col >= src_width) {
            TS_REQUIRE(d.col == next, TS_ERR_INVALID,
                       "join: column " + std::to_string(next) + " of the result is neither the source's nor a dst column");
            next++;
        }
    plan.base_width = base;
    uint32_t width = base;
    if (spec.flags & JOIN_TABLE_ROW) dst.push_back({width++, JOIN_FROM_ROW, 0});
    if (spec.flags & JOIN_HIT) dst.push_back({width++, JOIN_FROM_HIT, 0});
    TS_REQUIRE(width <= JOIN_MAX_WIDTH, TS_ERR_INVALID, "join: the result would be wider than 2^16");
    plan.out_width = width;
    plan.n_dst = (uint32_t)dst.size();
    for (size_t f = 0; f < dst.size(); f++) {
        plan.dst_col[f] = dst[f].col;
        plan.dst_from[f] = dst[f].from;
        plan.dst_default[f] = dst[f].def;
    }
    return plan;
}

uint64_t join_table_rows(const JoinPlan& plan, uint64_t src_height, uint64_t table_height) {
    TS_REQUIRE(src_height >= 1 && src_height <= JOIN_MAX_HEIGHT, TS_ERR_INVALID,
               "join: the height of the source must be in [1, 2^27]");
    TS_REQUIRE(table_height >= 1 && table_height <= JOIN_MAX_HEIGHT, TS_ERR_INVALID,
               "join: the height of the table must be in [1, 2^27]");
    TS_REQUIRE(plan.table_rows <= table_height, TS_ERR_INVALID,
               "join: table_rows " + std::to_string(plan.table_rows) + " above the table's height " +
                   std::to_string(table_height));
    return plan.table_rows ? plan.table_rows : table_height;
}

uint64_t join_match_host(const JoinPlan& plan, const uint32_t* src, uint64_t src_height, const uint32_t* table,
                         uint64_t table_rows, std::vector<uint32_t>& match, uint64_t* first_missing) {
    typedef std::array<uint32_t, JOIN_MAX_KEYS> Tuple;
    auto tuple = [&](const JoinTerm* terms, const uint32_t* row) {
        Tuple t = {};
        for (uint32_t q = 0; q < plan.n_keys; q++) t[q] = terms[q].kind ? row[terms[q].value] : terms[q].value;
        return t;
    };
    std::map<Tuple, uint32_t> lowest;
    for (uint64_t t = 0; t < table_rows; t++)
        lowest.emplace(tuple(plan.table_keys, table + t * plan.table_width), (uint32_t)t);  // (the first one stays)
    match.assign(src_height, JOIN_NO_MATCH);
    uint64_t n_missing = 0;
    *first_missing = ~0ull;
    for (uint64_t r = 0; r < src_height; r++) {
        const uint32_t* row = src + r * plan.src_width;
        if (!join_takes_part(plan.when.kind ? row[plan.when.value] : plan.when.value)) continue;
        const auto it = lowest.find(tuple(plan.src_keys, row));
        if (it != lowest.end()) {
            match[r] = it->second;
        } else if (n_missing++ == 0) {
            *first_missing = r;
        }
    }
    return n_missing;
}

void join_rows_host(const JoinPlan& plan, const uint32_t* src, uint64_t src_height, const uint32_t* table,
                    const std::vector<uint32_t>& match, uint32_t* out) {
    const uint32_t SW = plan.src_width, W = plan.out_width;
    const bool keep = plan.flags & JOIN_KEEP;
    for (uint64_t r = 0; r < src_height; r++) {
        const uint32_t* row = src + r * SW;
        uint32_t* o = out + r * W;
        for (uint32_t c = 0; c < SW; c++) o[c] = row[c];  // (all reads see the source: out is another buffer)
        const uint32_t m = match[r];
        for (uint32_t f = 0; f < plan.n_dst; f++) {
            const uint32_t c = plan.dst_col[f], from = plan.dst_from[f];
            if (m != JOIN_NO_MATCH)
                o[c] = from == JOIN_FROM_ROW ? m : from == JOIN_FROM_HIT ? 1u : table[(uint64_t)m * plan.table_width + from];
            else if (!(keep && c < SW))
                o[c] = plan.dst_default[f];
        }
    }
}

std::string join_miss_text(uint64_t n_missing, uint64_t first_missing) {
    return "join: the key of source row " + std::to_string(first_missing) + " is in no table row (" +
           std::to_string(n_missing) + " such rows)";
}

}  // namespace ts
