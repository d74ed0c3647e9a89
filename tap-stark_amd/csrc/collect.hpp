// Collected rows: the rows of up to four resident row-major matrices that a spec selects, reshaped to one tuple form,
// stacked in (source, row, emitter) order and padded to a power of two (include/tapstark.h "collected rows").  It is a
// stream compaction: the one call whose output has another height than its source.  collect.cpp holds the checks, the
// plan and the plain sequential loop over host rows; collect.hip the three kernels.  Whether a selector word fires is
// written once here, for both.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bb.hpp"

namespace ts {

constexpr uint32_t COLLECT_MAGIC = 0x4C4F4354u;  // "TCOL"
constexpr uint32_t COLLECT_MAX_SOURCES = 4;
constexpr uint32_t COLLECT_MAX_EMITTERS = 16;
constexpr uint32_t COLLECT_MAX_WIDTH = 64;           // of the output
constexpr uint32_t COLLECT_MAX_SRC_WIDTH = 1u << 16;  // as derive, scan and the sort
constexpr uint64_t COLLECT_MAX_HEIGHT = 1ull << 27;   // of a source and of the output
constexpr uint32_t COLLECT_MAX_ENTRIES = 4096;        // fired (row, emitter) pairs of one block: the LDS list of k_collect_write
constexpr uint32_t COLLECT_ALWAYS = 0xFFFFFFFFu;      // CollectPlan::sel: no selector column, the emitter always fires

enum CollectTerm : uint32_t { C_CONST = 0, C_COL = 1, C_ROW = 2 };

struct CollectTermWord {
    uint32_t kind, value;
};

// What the checks leave.  The emitters are grouped by source, in spec order inside a source: the order the rule asks
// for.  terms holds out_width entries per emitter, in that grouped order.
struct CollectPlan {
    uint32_t n_sources = 0, out_width = 0;
    std::vector<uint32_t> src_width;           // n_sources
    std::vector<uint32_t> pad;                 // out_width
    std::vector<uint32_t> sel;                 // per emitter, grouped by source: COLLECT_ALWAYS or its selector column
    std::vector<CollectTermWord> terms;        // sel.size() * out_width
    uint32_t first_emitter[COLLECT_MAX_SOURCES + 1] = {0};  // emitters of source s: [first_emitter[s], first_emitter[s+1])
};

// Does a selector word fire?  Reduced mod p it must be != 0: 0, p and 2p do not fire, 0xFFFFFFFF does (the rule of
// the scan's reset column).
TS_HD bool collect_fires(uint32_t word) { return word % P != 0; }

// Every rule that needs no matrix; throws TS_ERR_INVALID with a text.
CollectPlan collect_check(const uint32_t* spec, size_t n_words);
// out_height as the caller gave it: 0 or a power of two in [1, 2^27]; throws TS_ERR_INVALID
void collect_check_out_height(uint64_t out_height);
// The height of the result for n_live fired triples; throws TS_ERR_INVALID "collect: N rows selected, out_height H"
uint64_t collect_height(uint64_t n_live, uint64_t out_height);
// The number of fired triples over host rows (heights[s] rows of src_width[s] words each).
uint64_t collect_count_host(const CollectPlan& plan, const uint32_t* const* src, const uint64_t* heights);
// out (height x out_width, row-major): the plain sequential loop, then the pad rows.
void collect_rows_host(const CollectPlan& plan, const uint32_t* const* src, const uint64_t* heights, uint64_t height,
                       uint32_t* out);
// A new row-major matrix (collect.hip) from the plan of a checked spec and its plan.n_sources sources, none null:
// row-major, on ctx, read only.  Throws TS_ERR_INVALID before any device work, and after the one host wait if more rows
// fired than the height takes.  Three launches.
struct Context;
struct DeviceMatrix;
DeviceMatrix collect_matrix(Context& ctx, const CollectPlan& plan, const DeviceMatrix* const* sources,
                            uint64_t out_height, uint64_t* n_live);

}  // namespace ts
