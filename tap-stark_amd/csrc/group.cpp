// The TGRP form of the collect's spec: the checks that need no matrix, the plan they leave, the height rule and the
// plain sequential loop over host rows.  No device code and no context: ts_collect_check and ts_collect_rows_host are
// all of this for a TGRP tape, and ts_matrix_collect_rows makes the same checks first.
#include "group.hpp"

#include <array>
#include <string>
#include <unordered_map>

#include "context.hpp"

namespace ts {

GroupPlan group_check(const uint32_t* spec, size_t n_words) {
    TS_REQUIRE(spec != nullptr, TS_ERR_INVALID, "group: null spec");
    TS_REQUIRE(n_words >= GROUP_HEADER, TS_ERR_INVALID, "group: the spec is shorter than its header");
    TS_REQUIRE(spec[0] == GROUP_MAGIC, TS_ERR_INVALID, "group: bad magic (not a TGRP spec)");
    TS_REQUIRE(spec[1] == 1, TS_ERR_INVALID, "group: unknown spec version " + std::to_string(spec[1]));
    const uint32_t src_width = spec[2], out_width = spec[3], n_keys = spec[4];
    TS_REQUIRE(src_width >= 1 && src_width <= GROUP_MAX_SRC_WIDTH, TS_ERR_INVALID,
               "group: src_width " + std::to_string(src_width) + " outside [1, 2^16]");
    TS_REQUIRE(out_width >= 1 && out_width <= GROUP_MAX_WIDTH, TS_ERR_INVALID,
               "group: out_width " + std::to_string(out_width) + " outside [1, " + std::to_string(GROUP_MAX_WIDTH) + "]");
    TS_REQUIRE(n_keys >= 1 && n_keys <= GROUP_MAX_KEYS, TS_ERR_INVALID,
               "group: n_keys " + std::to_string(n_keys) + " outside [1, " + std::to_string(GROUP_MAX_KEYS) + "]");
    const size_t want = GROUP_HEADER + 2 * (size_t)n_keys + 3 * (size_t)out_width;
    TS_REQUIRE(n_words == want, TS_ERR_INVALID,
               "group: " + std::to_string(n_words) + " words, the header asks for " + std::to_string(want));
    const uint32_t sel_kind = spec[5], sel_value = spec[6];
    TS_REQUIRE(sel_kind <= 1, TS_ERR_INVALID, "group: selector kind must be 0 (always) or 1 (column)");
    TS_REQUIRE(sel_kind == 1 || sel_value == 1, TS_ERR_INVALID, "group: a constant selector must be 1");
    TS_REQUIRE(sel_kind == 0 || sel_value < src_width, TS_ERR_INVALID, "group: the selector column is outside the source");

    GroupPlan plan;
    plan.src_width = src_width;
    plan.out_width = out_width;
    plan.n_keys = n_keys;
    plan.sel = sel_kind ? sel_value : COLLECT_ALWAYS;
    const uint32_t* w = spec + GROUP_HEADER;
    for (uint32_t q = 0; q < n_keys; q++, w += 2) {
        const std::string key = "group: key " + std::to_string(q) + ": ";
        TS_REQUIRE(w[0] <= 1, TS_ERR_INVALID, key + "kind must be 0 (constant) or 1 (column)");
        TS_REQUIRE(w[0] == 1 || w[1] < P, TS_ERR_INVALID, key + "the constant is not below p");
        TS_REQUIRE(w[0] == 0 || w[1] < src_width, TS_ERR_INVALID, key + "the column is outside the source");
        plan.keys[q] = {w[0], w[1]};
    }
    for (uint32_t c = 0; c < out_width; c++, w++) {
        TS_REQUIRE(*w < P, TS_ERR_INVALID, "group: pad word " + std::to_string(c) + " is not below p");
        plan.pad.push_back(*w);
    }
    for (uint32_t c = 0; c < out_width; c++, w += 2) {
        const uint32_t kind = w[0], value = w[1];
        const std::string term = "group: term " + std::to_string(c) + ": ";
        TS_REQUIRE(kind <= G_INDEX, TS_ERR_INVALID, term + "kind must be in [0, 9]");
        const bool column = kind == G_FIRST || kind == G_LAST || (kind >= G_SUM && kind <= G_MAX);
        TS_REQUIRE(kind != G_CONST || value < P, TS_ERR_INVALID, term + "the constant is not below p");
        TS_REQUIRE(!column || value < src_width, TS_ERR_INVALID, term + "the column is outside the source");
        TS_REQUIRE(kind == G_CONST || column || value == 0, TS_ERR_INVALID,
                   term + "the value word of kinds 3, 4, 5 and 9 must be 0");
        uint32_t slot = 0;
        if (kind >= G_SUM && kind <= G_MAX) slot = plan.n_aggregates++;
        plan.terms.push_back({kind, value, slot});
    }
    TS_REQUIRE(plan.n_aggregates <= GROUP_MAX_AGGREGATES, TS_ERR_INVALID,
               "group: " + std::to_string(plan.n_aggregates) + " terms of kinds 6 to 8, more than " +
                   std::to_string(GROUP_MAX_AGGREGATES));
    return plan;
}

uint64_t group_height(uint64_t n_groups, uint64_t out_height) {
    TS_REQUIRE(out_height == 0 || n_groups <= out_height, TS_ERR_INVALID,
               "group: " + std::to_string(n_groups) + " groups, out_height " + std::to_string(out_height));
    if (out_height) return out_height;
    uint64_t h = 1;
    while (h < n_groups) h <<= 1;  // n_groups <= the source's height <= 2^27
    return h;
}

namespace {
typedef std::array<uint32_t, GROUP_MAX_KEYS> GroupKey;
struct GroupKeyHash {
    size_t operator()(const GroupKey& k) const {
        uint64_t h = 0x9E3779B97F4A7C15ull;
        for (uint32_t v : k) h = (h ^ v) * 0x100000001B3ull;
        return (size_t)(h ^ (h >> 29));
    }
};
}  // namespace

std::vector<unsigned long long> group_records_host(const GroupPlan& plan, const uint32_t* src, uint64_t height) {
    const size_t stride = GROUP_RECORD_HEAD + plan.n_aggregates;
    std::vector<unsigned long long> records;
    std::unordered_map<GroupKey, size_t, GroupKeyHash> index;  // key tuple, as stored -> its group
    for (uint64_t r = 0; r < height; r++) {
        const uint32_t* row = src + r * plan.src_width;
        if (plan.sel != COLLECT_ALWAYS && !collect_fires(row[plan.sel])) continue;
        GroupKey key = {};
        for (uint32_t q = 0; q < plan.n_keys; q++) key[q] = plan.keys[q].kind ? row[plan.keys[q].value] : plan.keys[q].value;
        const auto found = index.emplace(key, index.size());
        const size_t at = found.first->second * stride;
        if (found.second) {
            records.resize(at + stride);
            records[at + GROUP_FIRST] = r;
            records[at + GROUP_COUNT] = 0;
            for (const GroupTermWord& t : plan.terms)
                if (t.kind >= G_SUM && t.kind <= G_MAX) records[at + GROUP_RECORD_HEAD + t.slot] = group_identity(t.kind);
        }
        unsigned long long* rec = records.data() + at;
        rec[GROUP_LAST] = r;
        rec[GROUP_COUNT]++;
        for (const GroupTermWord& t : plan.terms) {
            if (t.kind < G_SUM || t.kind > G_MAX) continue;
            const unsigned long long v = group_canonical(row[t.value]);
            unsigned long long& a = rec[GROUP_RECORD_HEAD + t.slot];
            a = t.kind == G_SUM ? a + v : t.kind == G_MIN ? (v < a ? v : a) : (v > a ? v : a);
        }
    }
    return records;
}

void group_rows_host(const GroupPlan& plan, const std::vector<unsigned long long>& records, const uint32_t* src,
                     uint64_t height, uint32_t* out) {
    const uint32_t W = plan.out_width;
    const size_t stride = GROUP_RECORD_HEAD + plan.n_aggregates;
    const uint64_t n_groups = records.size() / stride;
    for (uint64_t g = 0; g < n_groups; g++)
        for (uint32_t c = 0; c < W; c++)
            out[g * W + c] = group_term(plan.terms[c], records.data() + g * stride, g, src, plan.src_width);
    for (uint64_t at = n_groups; at < height; at++)
        for (uint32_t c = 0; c < W; c++) out[at * W + c] = plan.pad[c];
}

}  // namespace ts
