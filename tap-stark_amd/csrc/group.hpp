// Grouped rows: one output row per distinct key tuple among the rows of one resident row-major matrix that take part,
// in order of first appearance, each made of words of the group's first and last row, its size, and sums, minima and
// maxima over it, padded to a power of two (include/tapstark.h "grouped rows").  The group form of the collect: the
// same three entry points take its tape, told apart by the magic.  group.cpp holds the checks, the plan and the plain
// sequential loop over host rows; group.hip the kernels.  What a group's record holds and what a term makes of it are
// written once here, for both.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bb.hpp"
#include "collect.hpp"

namespace ts {

constexpr uint32_t GROUP_MAGIC = 0x50524754u;  // "TGRP"
constexpr uint32_t GROUP_MAX_KEYS = 8;
constexpr uint32_t GROUP_MAX_AGGREGATES = 16;
constexpr uint32_t GROUP_MAX_WIDTH = COLLECT_MAX_WIDTH;          // of the output
constexpr uint32_t GROUP_MAX_SRC_WIDTH = COLLECT_MAX_SRC_WIDTH;  // as the collect
constexpr uint64_t GROUP_MAX_HEIGHT = COLLECT_MAX_HEIGHT;        // of the source and of the output
constexpr size_t GROUP_HEADER = 7;

enum GroupTerm : uint32_t {
    G_CONST = 0, G_FIRST = 1, G_LAST = 2, G_FIRST_ROW = 3, G_LAST_ROW = 4, G_COUNT = 5, G_SUM = 6, G_MIN = 7, G_MAX = 8,
    G_INDEX = 9
};

// One output column.  slot: for kinds 6 to 8 the term's place among the spec's aggregates, in column order.
struct GroupTermWord {
    uint32_t kind, value, slot;
};

// What the checks leave.
struct GroupPlan {
    uint32_t src_width = 0, out_width = 0, n_keys = 0, n_aggregates = 0;
    uint32_t sel = COLLECT_ALWAYS;  // the selector column, or every row
    CollectTermWord keys[GROUP_MAX_KEYS] = {};  // kind 0 a constant, kind 1 a column; zero behind n_keys
    std::vector<uint32_t> pad;                  // out_width
    std::vector<GroupTermWord> terms;           // out_width
};

// A group's record is GROUP_RECORD_HEAD + n_aggregates 64-bit words: its least row, its greatest row, its size, then
// one word per aggregate: the exact integer sum of the canonical words (below 2^58 at 2^27 rows), or their least or
// greatest in the low half.
constexpr uint32_t GROUP_FIRST = 0, GROUP_LAST = 1, GROUP_COUNT = 2, GROUP_RECORD_HEAD = 3;

// canonical, whatever word the column held (2^32 < 3 p)
TS_HD uint32_t group_canonical(uint32_t w) {
    w = w >= P ? w - P : w;
    return w >= P ? w - P : w;
}

// What an aggregate's word holds before any row.
TS_HD uint64_t group_identity(uint32_t kind) { return kind == G_MIN ? 0xFFFFFFFFull : 0ull; }

// The word of one term for group `index` with record `rec`; src: the source, row-major, src_width words a row.
TS_HD uint32_t group_term(const GroupTermWord& t, const unsigned long long* rec, uint64_t index, const uint32_t* src,
                          uint32_t src_width) {
    switch (t.kind) {
        case G_CONST: return t.value;
        case G_FIRST: return src[rec[GROUP_FIRST] * src_width + t.value];  // as stored
        case G_LAST: return src[rec[GROUP_LAST] * src_width + t.value];
        case G_FIRST_ROW: return (uint32_t)rec[GROUP_FIRST];
        case G_LAST_ROW: return (uint32_t)rec[GROUP_LAST];
        case G_COUNT: return (uint32_t)rec[GROUP_COUNT];  // <= 2^27
        case G_SUM: return (uint32_t)(rec[GROUP_RECORD_HEAD + t.slot] % P);
        case G_MIN:
        case G_MAX: return (uint32_t)rec[GROUP_RECORD_HEAD + t.slot];
        default: return (uint32_t)index;  // G_INDEX
    }
}

// Every rule that needs no matrix; throws TS_ERR_INVALID with a text.
GroupPlan group_check(const uint32_t* spec, size_t n_words);
// The height of the result for n_groups groups (out_height checked by collect_check_out_height); throws TS_ERR_INVALID
// "group: N groups, out_height H".
uint64_t group_height(uint64_t n_groups, uint64_t out_height);
// The records of the groups over `height` host rows, in order of first appearance: the plain sequential loop.
std::vector<unsigned long long> group_records_host(const GroupPlan& plan, const uint32_t* src, uint64_t height);
// out (height x out_width, row-major) from the records, then the pad rows.
void group_rows_host(const GroupPlan& plan, const std::vector<unsigned long long>& records, const uint32_t* src,
                     uint64_t height, uint32_t* out);
// A new row-major matrix (group.hip) from the plan of a checked spec and its source: row-major, on ctx, read only.
// Throws TS_ERR_INVALID before any device work, and after the one host wait if there are more groups than the height
// takes.
struct Context;
struct DeviceMatrix;
DeviceMatrix group_matrix(Context& ctx, const GroupPlan& plan, const DeviceMatrix& src, uint64_t out_height,
                          uint64_t* n_live);

}  // namespace ts
