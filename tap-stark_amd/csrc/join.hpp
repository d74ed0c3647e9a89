// Joined rows: for every row of a resident row-major source, the table row with the same key tuple, and chosen columns
// of that row written into the source's row (include/tapstark.h "joined rows").  A keyed fetch: the hash table of the
// multiplicity fill, kept for the row it finds.  join.cpp holds the checks, the plan and the plain sequential loop over
// host rows; join.hip the two kernels.  Whether a `when` word takes part is written once here, for both.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "bb.hpp"

namespace ts {

constexpr uint32_t JOIN_MAX_KEYS = 8;  // = LOGUP_MAX_VALUES: the tuple of logup_dev.hpp
constexpr uint32_t JOIN_MAX_FETCH = 32;
constexpr uint32_t JOIN_MAX_DST = JOIN_MAX_FETCH + 2;  // the fetched columns, then TABLE_ROW and HIT
constexpr uint32_t JOIN_MAX_WIDTH = 1u << 16;          // of the result, as derive, scan and the sort
constexpr uint64_t JOIN_MAX_HEIGHT = 1ull << 27;
constexpr uint32_t JOIN_TABLE_ROW = 1, JOIN_HIT = 2, JOIN_KEEP = 4, JOIN_ALL_FLAGS = 7;
constexpr uint32_t JOIN_NO_MATCH = 0xFFFFFFFFu;  // no table row (a table has at most 2^27)
// JoinPlan::dst_from beyond the table's columns: the matched row's index, and the constant 1
constexpr uint32_t JOIN_FROM_ROW = 0xFFFFFFFEu, JOIN_FROM_HIT = 0xFFFFFFFDu;

struct JoinTerm {  // the layout of ts_logup_term
    uint32_t kind, value;
};

// The spec as the caller gave it (ts_join_spec without its struct_size).
struct JoinSpecIn {
    bool size_ok;
    uint32_t n_keys;
    const JoinTerm *src_keys, *table_keys;
    JoinTerm when;
    uint32_t n_fetch;
    const uint32_t *table_columns, *dst_columns, *defaults;
    uint32_t flags;
    uint64_t table_rows;
};

// What the checks leave.  The dst list is sorted by column and holds the flag columns too, so that "is column c
// written, and from where" is one search in one list for the host loop and the kernel alike.
struct JoinPlan {
    uint32_t n_keys = 0, flags = 0, src_width = 0, table_width = 0;
    uint32_t base_width = 0;  // max(src_width, 1 + max dst): where the flag columns start
    uint32_t out_width = 0;
    uint64_t table_rows = 0;  // as given: 0 = all
    JoinTerm src_keys[JOIN_MAX_KEYS] = {}, table_keys[JOIN_MAX_KEYS] = {}, when = {0, 1};
    uint32_t n_dst = 0;
    uint32_t dst_col[JOIN_MAX_DST] = {}, dst_from[JOIN_MAX_DST] = {}, dst_default[JOIN_MAX_DST] = {};
};

// Does a row whose `when` word is this take part?  The selector rule of the collected rows: reduced mod p it must be
// != 0, so 0, p and 2p do not fire, 1 and 0xFFFFFFFF do.
TS_HD bool join_takes_part(uint32_t word) { return word % P != 0; }

// Every rule that needs no matrix but the two widths; throws TS_ERR_INVALID with a text.
JoinPlan join_check(const JoinSpecIn& spec, uint32_t src_width, uint32_t table_width);
// The rows of the table that are entered; throws TS_ERR_INVALID for heights outside [1, 2^27] and for table_rows above
// the table's height.
uint64_t join_table_rows(const JoinPlan& plan, uint64_t src_height, uint64_t table_height);
// match[r]: the lowest of the table rows [0, table_rows) whose tuple equals the tuple of source row r, or JOIN_NO_MATCH
// for a row that takes no part or finds none.  Returns the number of misses; first_missing <- the least row that takes
// part and finds none, or ~0.
uint64_t join_match_host(const JoinPlan& plan, const uint32_t* src, uint64_t src_height, const uint32_t* table,
                         uint64_t table_rows, std::vector<uint32_t>& match, uint64_t* first_missing);
// out (src_height x out_width, row-major) from the matches: the plain sequential loop.
void join_rows_host(const JoinPlan& plan, const uint32_t* src, uint64_t src_height, const uint32_t* table,
                    const std::vector<uint32_t>& match, uint32_t* out);
// The text of the refusal a miss is when the caller takes no count.
std::string join_miss_text(uint64_t n_missing, uint64_t first_missing);

// A new row-major matrix (join.hip) from a checked plan: src and table row-major, on ctx, read only; they may be one
// matrix.  Throws TS_ERR_INVALID before any device work; with fail_on_miss, TS_ERR_INVARIANT after the one host wait.
// Two kernel launches.
struct Context;
struct DeviceMatrix;
DeviceMatrix join_matrix(Context& ctx, const JoinPlan& plan, const DeviceMatrix& src, const DeviceMatrix& table,
                         bool fail_on_miss, uint64_t* n_missing, uint64_t* first_missing);

}  // namespace ts
