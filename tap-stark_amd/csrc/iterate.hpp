// Iterated trace columns: a TITR row program (include/tapstark.h "iterated columns") -- derive's row program plus
// registers carried down each group of rows.  The tape checks and the lowering are derive_lower's (derive.cpp); this
// header has what one instruction of the lowered list does, written once for iterate_rows_host (iterate.cpp, the plain
// loop down host rows) and k_iterate_walk (iterate.hip, one lane per group in HBM).
#pragma once
#include <stdint.h>

#include "collect.hpp"  // collect_fires: the one rule of what a selector or reset word means
#include "derive.hpp"

namespace ts {

// Whether `row` starts a group: row 0 does, and every row whose reset word fires.
TS_HD bool iterate_starts(const uint32_t* src, uint64_t row, uint32_t width, uint32_t reset_column) {
    return row == 0 || (reset_column != ITERATE_NO_RESET && collect_fires(src[row * width + reset_column]));
}

// One instruction of a lowered TITR list on `row`, which is row `step` of its group and its last one or not.
// rd(slot) / wr(slot, value): the slot file (Montgomery values); ld(offset, column): the word COL reads; st(column,
// word): a canonical word of the out row.  Ops 40 to 43 and V_LATCH are here, every other value is derive_value's.
template <class Rd, class Wr, class Ld, class St>
TS_HD void iterate_instruction(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint64_t row, uint64_t height, uint32_t step,
                               bool group_last, Rd&& rd, Wr&& wr, Ld&& ld, St&& st) {
    const uint32_t op = x & 255, dst = (x >> 8) & 255;
    uint32_t v;
    switch (op) {
        case V_STORE: st(w, from_mont(rd(y))); return;
        case V_LATCH: wr(dst, rd(y)); return;
        case V_CARRY: v = rd(y); break;
        case V_STEP: v = to_mont(step); break;  // below 2^27 < p
        case V_IS_GROUP_FIRST: v = step == 0 ? R_MOD_P : 0u; break;
        case V_IS_GROUP_LAST: v = group_last ? R_MOD_P : 0u; break;
        default: v = derive_value(op, y, z, row, height, rd, ld);
    }
    wr(dst, v);
    if (x >> 16) st(w, from_mont(v));
}

// The least start row of a group longer than max_group_rows, ~0 when there is none; its length.
struct IterateLong {
    uint64_t start = ~0ull, rows = 0;
};
IterateLong iterate_find_long(const DeriveProgram& prog, const uint32_t* src, uint64_t height);
// Throws the refusal of an over-long group: TS_ERR_INVARIANT "iterate: the group that starts at row R has N rows,
// max_group_rows is M".  One text for the host loop and the device call.
void iterate_refuse_long(const DeriveProgram& prog, const IterateLong& bad);
void iterate_rows_host(const DeriveProgram& prog, const uint32_t* src, uint64_t height, uint32_t* out);
// A new row-major matrix of src's height (iterate.hip).  `prog` is a lowered TITR program for src's width.  Four
// launches and exactly one host wait, after which an over-long group refuses the call before the walk is launched.
struct Context;
struct DeviceMatrix;
DeviceMatrix iterate_matrix(Context& ctx, const DeriveProgram& prog, const DeviceMatrix& src);

}  // namespace ts
