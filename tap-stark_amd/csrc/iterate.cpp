// The host side of a TITR program (iterate.hpp): the plain loop down the rows through the lowered list, and the search
// for a group longer than max_group_rows.  No device code and no context.
#include "iterate.hpp"

#include <string>

#include "context.hpp"

namespace ts {

IterateLong iterate_find_long(const DeriveProgram& prog, const uint32_t* src, uint64_t height) {
    IterateLong bad;
    uint64_t start = 0;
    for (uint64_t row = 1; row <= height; row++) {
        if (row < height && !iterate_starts(src, row, prog.src_width, prog.reset_column)) continue;
        if (row - start > prog.max_group_rows) {
            bad.start = start;
            bad.rows = row - start;
            return bad;
        }
        start = row;
    }
    return bad;
}

void iterate_refuse_long(const DeriveProgram& prog, const IterateLong& bad) {
    TS_REQUIRE(bad.start == ~0ull, TS_ERR_INVARIANT,
               "iterate: the group that starts at row " + std::to_string(bad.start) + " has " + std::to_string(bad.rows) +
                   " rows, max_group_rows is " + std::to_string(prog.max_group_rows));
}

void iterate_rows_host(const DeriveProgram& prog, const uint32_t* src, uint64_t height, uint32_t* out) {
    iterate_refuse_long(prog, iterate_find_long(prog, src, height));
    std::vector<uint32_t> slots(prog.n_live);
    const uint32_t n_instr = prog.n_instr();
    uint32_t step = 0;
    for (uint64_t row = 0; row < height; row++) {
        if (iterate_starts(src, row, prog.src_width, prog.reset_column)) {
            step = 0;
            for (size_t k = 0; k < prog.inits.size(); k++) slots[k] = prog.inits[k];
        }
        const bool group_last = row + 1 == height || iterate_starts(src, row + 1, prog.src_width, prog.reset_column);
        const uint32_t* rows[3] = {src + row * prog.src_width,
                                   src + (row + 1 == height ? 0 : row + 1) * prog.src_width,
                                   src + (row == 0 ? height - 1 : row - 1) * prog.src_width};
        uint32_t* o = out + row * prog.out_width;
        for (uint32_t c = 0; c < prog.out_width; c++)
            if (!((prog.named[c >> 5] >> (c & 31)) & 1)) o[c] = rows[0][c];
        for (uint32_t pc = 0; pc < n_instr; pc++) {
            const uint32_t* ins = prog.code.data() + 4 * (size_t)pc;
            iterate_instruction(
                ins[0], ins[1], ins[2], ins[3], row, height, step, group_last, [&](uint32_t slot) { return slots[slot]; },
                [&](uint32_t slot, uint32_t v) { slots[slot] = v; },
                [&](uint32_t offset, uint32_t column) { return rows[offset][column]; },
                [&](uint32_t column, uint32_t word) { o[column] = word; });
        }
        step++;
    }
}

}  // namespace ts
