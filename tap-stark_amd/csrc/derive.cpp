// The row program of ts_matrix_derive: tape checks, lowering to the instruction list of derive.hpp, and that list
// evaluated over host rows.  No device code and no context: ts_derive_check and ts_derive_rows_host are all of this.
// Both program kinds, TDER and TITR, are checked and lowered here; the host loop of a TITR list is iterate.cpp's.
#include "derive.hpp"

#include <string>

#include "context.hpp"
#include "iterate.hpp"

namespace ts {

namespace {

struct Node {
    uint32_t op, a, b;
};

// how many of a, b name nodes
int node_operands(uint32_t op) {
    switch (op) {
        case V_ADD: case V_SUB: case V_MUL: case V_LT: case V_AND: case V_XOR: return 2;
        case V_NEG: case V_INV: case V_IS_ZERO: case V_BITS: return 1;
        default: return 0;
    }
}

}  // namespace

DeriveProgram derive_lower(const uint32_t* program, size_t n_words, uint32_t src_width) {
    TS_REQUIRE(program != nullptr, TS_ERR_INVALID, "derive: null program");
    TS_REQUIRE(n_words >= 5, TS_ERR_INVALID, "derive: the program is shorter than its header");
    const bool iterate = program[0] == ITERATE_MAGIC;
    TS_REQUIRE(iterate || program[0] == DERIVE_MAGIC, TS_ERR_INVALID, "derive: bad magic (not a TDER program)");
    // A TITR tape is a TDER tape with three more header words and the carries behind the outputs; its refusals read
    // "iterate: ..." in the same forms.
    const std::string who = iterate ? "iterate: " : "derive: ";
    const size_t hdr = iterate ? 8 : 5;
    TS_REQUIRE(n_words >= hdr, TS_ERR_INVALID, who + "the program is shorter than its header");
    TS_REQUIRE(program[1] == 1, TS_ERR_INVALID, who + "unknown program version " + std::to_string(program[1]));
    const uint32_t n_nodes = program[3], n_outputs = program[4];
    const uint32_t n_carries = iterate ? program[5] : 0;
    TS_REQUIRE(!iterate || (n_carries >= 1 && n_carries <= ITERATE_MAX_CARRIES), TS_ERR_INVALID,
               who + "n_carries " + std::to_string(n_carries) + " outside [1, " + std::to_string(ITERATE_MAX_CARRIES) + "]");
    TS_REQUIRE(n_nodes >= 1 && n_nodes <= DERIVE_MAX_NODES, TS_ERR_INVALID,
               who + "n_nodes " + std::to_string(n_nodes) + " outside [1, " + std::to_string(DERIVE_MAX_NODES) + "]");
    TS_REQUIRE(n_outputs >= 1 && n_outputs <= DERIVE_MAX_OUTPUTS, TS_ERR_INVALID,
               who + "n_outputs " + std::to_string(n_outputs) + " outside [1, " + std::to_string(DERIVE_MAX_OUTPUTS) + "]");
    const size_t asked = hdr + 3 * (size_t)n_nodes + 2 * (size_t)n_outputs + 2 * (size_t)n_carries;
    TS_REQUIRE(n_words == asked, TS_ERR_INVALID,
               who + std::to_string(n_words) + " words, the header asks for " + std::to_string(asked));
    TS_REQUIRE(program[2] == src_width, TS_ERR_INVALID,
               who + "the program is written for a source of " + std::to_string(program[2]) + " columns, this one has " +
                   std::to_string(src_width));
    TS_REQUIRE(src_width >= 1 && src_width <= DERIVE_MAX_WIDTH, TS_ERR_INVALID, who + "src_width outside [1, 2^16]");
    if (iterate) {
        TS_REQUIRE(program[6] == ITERATE_NO_RESET || program[6] < src_width, TS_ERR_INVALID,
                   who + "reset_column " + std::to_string(program[6]) + " is outside the source");
        TS_REQUIRE(program[7] >= 1, TS_ERR_INVALID, who + "max_group_rows is 0");
    }

    const Node* nodes = reinterpret_cast<const Node*>(program + hdr);
    for (uint32_t i = 0; i < n_nodes; i++) {
        const Node& n = nodes[i];
        const std::string at = who + "node " + std::to_string(i) + ": ";
        switch (iterate || n.op < V_CARRY ? n.op : ~0u) {  // (40 to 43 are unknown to a TDER tape)
            case V_CONST:
                TS_REQUIRE(n.a < P, TS_ERR_INVALID, at + "CONST value is not below p");
                break;
            case V_COL:
                TS_REQUIRE(n.a <= 2, TS_ERR_INVALID, at + "COL row offset above 2");
                TS_REQUIRE(n.b < src_width, TS_ERR_INVALID, at + "COL column outside the source");
                break;
            case V_IS_FIRST: case V_IS_LAST: case V_IS_TRANSITION: case V_ROW:
            case V_STEP: case V_IS_GROUP_FIRST: case V_IS_GROUP_LAST:
                break;
            case V_CARRY:
                TS_REQUIRE(n.a < n_carries, TS_ERR_INVALID, at + "CARRY names no carry");
                break;
            case V_ADD: case V_SUB: case V_MUL: case V_LT: case V_AND: case V_XOR:
                TS_REQUIRE(n.a < i && n.b < i, TS_ERR_INVALID, at + "an operand does not name an earlier node");
                break;
            case V_NEG: case V_INV: case V_IS_ZERO:
                TS_REQUIRE(n.a < i, TS_ERR_INVALID, at + "the operand does not name an earlier node");
                break;
            case V_BITS: {
                TS_REQUIRE(n.a < i, TS_ERR_INVALID, at + "the operand does not name an earlier node");
                const uint32_t shift = n.b & 255, nbits = n.b >> 8;
                TS_REQUIRE(nbits >= 1 && shift + nbits <= 31, TS_ERR_INVALID, at + "BITS needs nbits >= 1 and shift + nbits <= 31");
                break;
            }
            default:
                TS_REQUIRE(false, TS_ERR_INVALID, at + "unknown op " + std::to_string(n.op));
        }
    }

    const uint32_t* outs = program + hdr + 3 * (size_t)n_nodes;
    const uint32_t* carries = outs + 2 * (size_t)n_outputs;  // n_carries x {node, init}
    uint32_t out_width = src_width;
    for (uint32_t k = 0; k < n_outputs; k++) {
        TS_REQUIRE(outs[2 * k] < n_nodes, TS_ERR_INVALID, who + "output " + std::to_string(k) + " names no node");
        TS_REQUIRE(outs[2 * k + 1] < DERIVE_MAX_WIDTH, TS_ERR_INVALID,
                   who + "output " + std::to_string(k) + ": the matrix would be wider than 2^16 columns");
        if (outs[2 * k + 1] + 1 > out_width) out_width = outs[2 * k + 1] + 1;
    }
    DeriveProgram prog;
    prog.src_width = src_width;
    prog.out_width = out_width;
    prog.named.assign((out_width + 31) / 32, 0);
    for (uint32_t k = 0; k < n_outputs; k++) {
        const uint32_t c = outs[2 * k + 1];
        TS_REQUIRE(!((prog.named[c >> 5] >> (c & 31)) & 1), TS_ERR_INVALID,
                   who + "column " + std::to_string(c) + " is named by two outputs");
        prog.named[c >> 5] |= 1u << (c & 31);
    }
    for (uint32_t c = src_width; c < out_width; c++)
        TS_REQUIRE((prog.named[c >> 5] >> (c & 31)) & 1, TS_ERR_INVALID,
                   who + "column " + std::to_string(c) + " is beyond the source and no output names it");
    prog.iterate = iterate;
    for (uint32_t k = 0; k < n_carries; k++) {
        TS_REQUIRE(carries[2 * k] < n_nodes, TS_ERR_INVALID, who + "carry " + std::to_string(k) + " names no node");
        TS_REQUIRE(carries[2 * k + 1] < P, TS_ERR_INVALID, who + "carry " + std::to_string(k) + ": init is not below p");
        prog.inits.push_back(to_mont(carries[2 * k + 1]));
    }
    if (iterate) {
        prog.reset_column = program[6];
        prog.max_group_rows = program[7];
    }

    // the nodes an output or a carry reaches, and where each is last read
    std::vector<char> kept(n_nodes, 0);
    for (uint32_t k = 0; k < n_outputs; k++) kept[outs[2 * k]] = 1;
    for (uint32_t k = 0; k < n_carries; k++) kept[carries[2 * k]] = 1;
    std::vector<uint32_t> last_use(n_nodes);
    for (uint32_t i = n_nodes; i-- > 0;) {
        last_use[i] = i;
        if (!kept[i]) continue;
        const int n_op = node_operands(nodes[i].op);
        if (n_op >= 1) kept[nodes[i].a] = 1;
        if (n_op >= 2) kept[nodes[i].b] = 1;
    }
    for (uint32_t i = 0; i < n_nodes; i++) {
        if (!kept[i]) continue;
        const int n_op = node_operands(nodes[i].op);
        if (n_op >= 1) last_use[nodes[i].a] = i;
        if (n_op >= 2) last_use[nodes[i].b] = i;
    }
    for (uint32_t k = 0; k < n_carries; k++) last_use[carries[2 * k]] = n_nodes;  // read by its latch, behind every node

    // One instruction per kept node, in tape order.  A value holds the lowest free slot from its instruction to its
    // last use; operands that die at an instruction give their slots back BEFORE its destination is chosen.  Carry k
    // owns slot k from the first row of a group to its last, so the temporaries start behind the carries.
    std::vector<uint32_t> slot_of(n_nodes, 0);
    std::vector<char> in_use(n_carries, 1);
    uint32_t held = n_carries;
    prog.n_live = n_carries;
    auto release = [&](uint32_t node) {
        in_use[slot_of[node]] = 0;
        held--;
    };
    for (uint32_t i = 0; i < n_nodes; i++) {
        if (!kept[i]) continue;
        const Node& n = nodes[i];
        const int n_op = node_operands(n.op);
        uint32_t y = n.a, z = n.op == V_COL || n.op == V_BITS ? n.b : 0u;
        if (n.op == V_CONST) y = to_mont(n.a);
        if (n_op >= 1) y = slot_of[n.a];
        if (n_op >= 2) z = slot_of[n.b];
        if (n_op >= 1 && last_use[n.a] == i) release(n.a);
        if (n_op >= 2 && n.b != n.a && last_use[n.b] == i) release(n.b);
        uint32_t s = 0;
        while (s < in_use.size() && in_use[s]) s++;
        if (s == in_use.size()) in_use.push_back(0);
        in_use[s] = 1;
        held++;
        slot_of[i] = s;
        if (held > prog.n_live) prog.n_live = held;
        const size_t at = prog.code.size();
        prog.code.insert(prog.code.end(), {n.op | s << 8, y, z, 0u});
        prog.n_nodes_kept++;
        bool first = true;
        for (uint32_t k = 0; k < n_outputs; k++) {
            if (outs[2 * k] != i) continue;
            if (first) {
                prog.code[at] |= 1u << 16;
                prog.code[at + 3] = outs[2 * k + 1];
            } else {
                prog.code.insert(prog.code.end(), {(uint32_t)V_STORE, s, 0u, outs[2 * k + 1]});
            }
            first = false;
        }
        if (last_use[i] == i) release(i);  // read by nothing later: the stores above were its only use
    }
    for (uint32_t k = 0; k < n_carries; k++)
        prog.code.insert(prog.code.end(), {(uint32_t)V_LATCH | k << 8, slot_of[carries[2 * k]], 0u, 0u});
    TS_REQUIRE(prog.n_live <= DERIVE_MAX_LIVE, TS_ERR_INVALID,
               who + "the program holds " + std::to_string(prog.n_live) + " values at once, the limit is " +
                   std::to_string(DERIVE_MAX_LIVE));
    // What one lane may be asked to run on a machine it shares: a condition, not a measurement.
    TS_REQUIRE(!iterate || (uint64_t)prog.max_group_rows * prog.n_instr() <= ITERATE_MAX_WORK, TS_ERR_INVALID,
               who + "max_group_rows " + std::to_string(prog.max_group_rows) + " x " + std::to_string(prog.n_instr()) +
                   " instructions is above the work limit of " + std::to_string(ITERATE_MAX_WORK));
    return prog;
}

void derive_rows_host(const DeriveProgram& prog, const uint32_t* src, uint64_t height, uint32_t* out) {
    if (prog.iterate) return iterate_rows_host(prog, src, height, out);
    std::vector<uint32_t> slots(prog.n_live ? prog.n_live : 1);
    const uint32_t n_instr = prog.n_instr();
    for (uint64_t row = 0; row < height; row++) {
        const uint32_t* rows[3] = {src + row * prog.src_width,
                                   src + (row + 1 == height ? 0 : row + 1) * prog.src_width,
                                   src + (row == 0 ? height - 1 : row - 1) * prog.src_width};
        uint32_t* o = out + row * prog.out_width;
        for (uint32_t c = 0; c < prog.out_width; c++)
            if (!((prog.named[c >> 5] >> (c & 31)) & 1)) o[c] = rows[0][c];
        for (uint32_t pc = 0; pc < n_instr; pc++) {
            const uint32_t* ins = prog.code.data() + 4 * (size_t)pc;
            const uint32_t op = ins[0] & 255, dst = (ins[0] >> 8) & 255, y = ins[1], z = ins[2];
            if (op == V_STORE) {
                o[ins[3]] = from_mont(slots[y]);
                continue;
            }
            const uint32_t v = derive_value(op, y, z, row, height, [&](uint32_t slot) { return slots[slot]; },
                                            [&](uint32_t offset, uint32_t column) { return rows[offset][column]; });
            slots[dst] = v;
            if (ins[0] >> 16) o[ins[3]] = from_mont(v);
        }
    }
}

}  // namespace ts
