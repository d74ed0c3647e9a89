// Derived trace columns: a row program (a word tape, include/tapstark.h "derived columns") lowered to an instruction
// list over a slot file, and its two evaluators -- k_derive (derive.hip), one lane per row in HBM, and derive_rows_host
// (derive.cpp), the same list over host rows.  Both call derive_value below, so what an instruction MEANS is written
// once.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bb.hpp"

namespace ts {

constexpr uint32_t DERIVE_MAGIC = 0x52454454u;  // "TDER"
constexpr uint32_t DERIVE_MAX_NODES = 4096;
constexpr uint32_t DERIVE_MAX_OUTPUTS = 256;
constexpr uint32_t DERIVE_MAX_LIVE = 48;            // 48 slots x 256 lanes x 4 B = 48 KiB of LDS (quotient.hip plan_reg_file)
constexpr uint32_t DERIVE_MAX_WIDTH = 1u << 16;     // as the sort: height * width stays below 2^43 words
constexpr uint64_t DERIVE_MAX_HEIGHT = 1ull << 27;
// The second program kind of the same entry points (include/tapstark.h "iterated columns"): a row program with
// registers carried down each group of rows.  iterate.hpp has its evaluator, iterate.cpp the host loop, iterate.hip
// the kernels; the checks and the lowering are derive_lower's.
constexpr uint32_t ITERATE_MAGIC = 0x52544954u;  // "TITR"
constexpr uint32_t ITERATE_MAX_CARRIES = 16;
constexpr uint64_t ITERATE_MAX_WORK = 1ull << 20;   // max_group_rows x instructions: what one lane may be asked to run
constexpr uint32_t ITERATE_NO_RESET = 0xFFFFFFFFu;  // reset_column: the whole matrix is one group

// The tape's op numbers; an instruction keeps its node's.  V_STORE exists only in the lowered list: one more
// destination column for the value of the instruction before it.  40 to 43 are ops of a TITR tape alone; V_LATCH exists
// only in its lowered list: carry slot <- the value its node had on this row.
enum DeriveOp : uint32_t {
    V_CONST = 0, V_COL = 1, V_IS_FIRST = 3, V_IS_LAST = 4, V_IS_TRANSITION = 5, V_ADD = 6, V_SUB = 7, V_NEG = 8, V_MUL = 9,
    V_ROW = 32, V_INV = 33, V_IS_ZERO = 34, V_LT = 35, V_BITS = 36, V_AND = 37, V_XOR = 38,
    V_CARRY = 40, V_STEP = 41, V_IS_GROUP_FIRST = 42, V_IS_GROUP_LAST = 43, V_LATCH = 62, V_STORE = 63,
};

// One instruction, four words (one scalar 16-byte load on the device):
//   x = op | slot << 8 | stores << 16   slot: where the value goes (< n_live); stores: 1 = it is also out column w
//   y, z = the operands: slots for the arithmetic ops (z is BITS's shift | nbits << 8); CONST: y = the value in
//          Montgomery form; COL: y = row offset, z = column; V_STORE: y = the slot; CARRY: y = the carry's slot
//          (carry k owns slot k for the whole walk); V_LATCH: slot = the carry's, y = the slot of its node
//   w = the destination column of a store
// Every value in a slot is a field element in Montgomery form; a store writes its canonical word.
// A TITR program: the latches stand at the END of the list, after every CARRY has been read, and each reads the slot
// of a node, never a carry slot (CARRY is an instruction with a slot of its own), so their order does not matter.
struct DeriveProgram {
    uint32_t src_width = 0, out_width = 0;
    uint32_t n_nodes_kept = 0;             // instructions but for V_STORE: the nodes an output reaches
    uint32_t n_live = 0;                   // slots
    std::vector<uint32_t> code;            // 4 words per instruction
    std::vector<uint32_t> named;           // bit c: out column c is written by a store (else copied from src)
    bool iterate = false;                  // a TITR program: the fields below, and n_live counts the carry slots
    uint32_t reset_column = ITERATE_NO_RESET, max_group_rows = 0;
    std::vector<uint32_t> inits;           // per carry, Montgomery form
    uint32_t n_instr() const { return (uint32_t)(code.size() / 4); }
};

// Checks the tape against every rule that needs no matrix and lowers it; throws TS_ERR_INVALID with a text.
DeriveProgram derive_lower(const uint32_t* program, size_t n_words, uint32_t src_width);
// out (height x out_width, row-major) from src (height x src_width) through the lowered list, on the host.  A TITR
// program goes to iterate_rows_host (iterate.cpp), which refuses a group longer than max_group_rows before it writes.
void derive_rows_host(const DeriveProgram& prog, const uint32_t* src, uint64_t height, uint32_t* out);
// A new row-major matrix of src's height and the program's out_width (derive.hip).  `src` is row-major, on ctx, read
// only.  Throws TS_ERR_INVALID before any device work; one upload of the lowered list through the context's page-locked
// arena and one launch, no host wait.  A TITR program goes to iterate_matrix (iterate.hip): four launches, one wait.
struct Context;
struct DeviceMatrix;
DeviceMatrix derive_matrix(Context& ctx, const uint32_t* program, size_t n_words, const DeviceMatrix& src);

// ---- what an instruction means (host and device) ------------------------------------------------------------
// The value of one instruction but V_STORE, on `row` of `height` rows: rd(slot) is an operand's value (Montgomery),
// ld(offset, column) the word COL reads, as stored (any 32-bit word: to_mont reduces it).  One flat switch, so that an
// instruction costs one dispatch.  The integer ops act on the canonical form and go back: that is where the
// conversions are, and nowhere else.  An operand word that names no slot (BITS's z, a unary op's) is never read as one.
template <class Rd, class Ld>
TS_HD uint32_t derive_value(uint32_t op, uint32_t y, uint32_t z, uint64_t row, uint64_t height, Rd&& rd, Ld&& ld) {
    switch (op) {
        case V_CONST: return y;
        case V_COL: return to_mont(ld(y, z));
        case V_IS_FIRST: return row == 0 ? R_MOD_P : 0u;
        case V_IS_LAST: return row + 1 == height ? R_MOD_P : 0u;
        case V_IS_TRANSITION: return row + 1 == height ? 0u : R_MOD_P;
        case V_ROW: return to_mont((uint32_t)row);  // row < 2^27 < p
        case V_ADD: return add(rd(y), rd(z));
        case V_SUB: return sub(rd(y), rd(z));
        case V_NEG: return neg(rd(y));
        case V_MUL: return mont_mul(rd(y), rd(z));
        case V_INV: return mont_inv(rd(y));  // a^(p-2): 0 stays 0
        case V_IS_ZERO: return rd(y) == 0 ? R_MOD_P : 0u;
        case V_LT: return from_mont(rd(y)) < from_mont(rd(z)) ? R_MOD_P : 0u;
        case V_BITS: return to_mont((from_mont(rd(y)) >> (z & 255)) & ((1u << (z >> 8)) - 1));
        case V_AND: return to_mont(from_mont(rd(y)) & from_mont(rd(z)));  // below both operands: canonical already
        default: return to_mont(from_mont(rd(y)) ^ from_mont(rd(z)));     // V_XOR: below 2^31, which to_mont reduces
    }
}

}  // namespace ts
