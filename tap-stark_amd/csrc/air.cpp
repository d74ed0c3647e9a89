#include "air.hpp"

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "bb.hpp"
#include "context.hpp"

namespace ts {

AirProgram compile_air(const uint32_t* tape, size_t n_words) {
    TS_REQUIRE(tape && n_words >= 6 && tape[0] == TAPE_MAGIC && tape[1] >= 1 && tape[1] <= 3, TS_ERR_INVALID,
               "air tape: bad header");
    // version 2 (symbolic_builder.rs:68-99 with a preprocessed_width): one more header word, one more leaf;
    // version 3: three more words (aux_width, n_challenges, n_exposed) and three more leaves
    const bool v3 = tape[1] == 3, v2 = tape[1] >= 2;
    AirProgram p;
    p.tape_header = v3 ? 10 : v2 ? 7 : 6;
    TS_REQUIRE(n_words >= p.tape_header, TS_ERR_INVALID, "air tape: bad header");
    p.width = tape[2];
    p.n_public = tape[3];
    const uint32_t n_nodes = tape[4];
    p.n_constraints = tape[5];
    p.preprocessed_width = v2 ? tape[6] : 0;
    if (v3) {
        p.aux_width = tape[7];
        p.n_challenges = tape[8];
        p.n_exposed = tape[9];
        TS_REQUIRE(p.n_challenges <= (1u << 20) && p.n_exposed <= (1u << 20) && p.n_public <= (1u << 28), TS_ERR_INVALID,
                   "air tape: more than 2^20 challenges or exposed words");
    }
    TS_REQUIRE((size_t)p.tape_header + 3 * (size_t)n_nodes + p.n_constraints == n_words, TS_ERR_INVALID,
               "air tape: length does not match header");
    TS_REQUIRE(p.width >= 1, TS_ERR_INVALID, "air tape: zero width");
    const uint32_t* nodes = tape + p.tape_header;
    const uint32_t* cons = nodes + 3 * (size_t)n_nodes;

    // validation + degree_multiple (symbolic_expression.rs:41-61)
    std::vector<uint32_t> deg(n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) {
        uint32_t op = nodes[3 * i], a = nodes[3 * i + 1], b = nodes[3 * i + 2];
        switch (op) {
            case T_CONST:
                TS_REQUIRE(a < P, TS_ERR_INVALID, "air tape: non-canonical constant");
                deg[i] = 0;
                break;
            case T_MAIN:
                TS_REQUIRE(a <= 1 && b < p.width, TS_ERR_INVALID, "air tape: bad main variable");
                deg[i] = 1;
                break;
            case T_PREP:  // degree multiple 1, like MAIN (symbolic_variable.rs:34-39)
                TS_REQUIRE(v2, TS_ERR_INVALID, "air tape: preprocessed variable in a version-1 tape");
                TS_REQUIRE(a <= 1 && b < p.preprocessed_width, TS_ERR_INVALID,
                           "air tape: bad preprocessed variable");
                deg[i] = 1;
                break;
            case T_PUBLIC:
                TS_REQUIRE(a < p.n_public, TS_ERR_INVALID, "air tape: bad public index");
                deg[i] = 0;
                break;
            case T_AUX:  // degree multiple 1, like MAIN
                TS_REQUIRE(v3, TS_ERR_INVALID, "air tape: aux variable in a version-1 or version-2 tape");
                TS_REQUIRE(a <= 1 && b < p.aux_width, TS_ERR_INVALID, "air tape: bad aux variable");
                deg[i] = 1;
                break;
            case T_CHALLENGE:  // degree multiple 0, like a public value
                TS_REQUIRE(v3, TS_ERR_INVALID, "air tape: challenge in a version-1 or version-2 tape");
                TS_REQUIRE(a < 4 * p.n_challenges, TS_ERR_INVALID, "air tape: bad challenge word index");
                deg[i] = 0;
                break;
            case T_EXPOSED:
                TS_REQUIRE(v3, TS_ERR_INVALID, "air tape: exposed value in a version-1 or version-2 tape");
                TS_REQUIRE(a < p.n_exposed, TS_ERR_INVALID, "air tape: bad exposed value index");
                deg[i] = 0;
                break;
            case T_IS_FIRST:
            case T_IS_LAST:
                deg[i] = 1;
                break;
            case T_IS_TRANSITION:
                deg[i] = 0;
                break;
            case T_ADD:
            case T_SUB:
                TS_REQUIRE(a < i && b < i, TS_ERR_INVALID, "air tape: forward reference");
                deg[i] = std::max(deg[a], deg[b]);
                break;
            case T_NEG:
                TS_REQUIRE(a < i, TS_ERR_INVALID, "air tape: forward reference");
                deg[i] = deg[a];
                break;
            case T_MUL:
                TS_REQUIRE(a < i && b < i, TS_ERR_INVALID, "air tape: forward reference");
                deg[i] = deg[a] + deg[b];
                break;
            default:
                throw Error(TS_ERR_INVALID, "air tape: unknown op");
        }
    }
    uint32_t mx = 0;
    for (uint32_t c = 0; c < p.n_constraints; c++) {
        TS_REQUIRE(cons[c] < n_nodes, TS_ERR_INVALID, "air tape: bad constraint id");
        mx = std::max(mx, deg[cons[c]]);
    }
    p.max_degree = mx;
    uint32_t d = std::max(mx, 2u);  // symbolic_builder.rs:24-26
    uint32_t lq = 0;
    while ((1u << lq) < d - 1) lq++;  // log2_ceil(d - 1), :31
    p.log_quotient_degree = lq;
    p.tape.assign(tape, tape + n_words);

    // ---- lowering: liveness + linear-scan register allocation --------------------------------
    // reachable nodes
    std::vector<uint8_t> live(n_nodes, 0);
    for (uint32_t c = 0; c < p.n_constraints; c++) live[cons[c]] = 1;
    for (int64_t i = (int64_t)n_nodes - 1; i >= 0; i--) {
        if (!live[i]) continue;
        uint32_t op = nodes[3 * i], a = nodes[3 * i + 1], b = nodes[3 * i + 2];
        if (op == T_ADD || op == T_SUB || op == T_MUL) live[a] = live[b] = 1;
        if (op == T_NEG) live[a] = 1;
    }
    // Schedule: a node is emitted right before its first use (demand-driven, depth first in
    // constraint order), so leaf loads are not all hoisted to the top and register pressure stays
    // close to the expression depth.  Each constraint is asserted as soon as its root is computed.
    // use counts
    std::vector<uint32_t> uses(n_nodes, 0);
    for (uint32_t i = 0; i < n_nodes; i++) {
        if (!live[i]) continue;
        uint32_t op = nodes[3 * i], a = nodes[3 * i + 1], b = nodes[3 * i + 2];
        if (op == T_ADD || op == T_SUB || op == T_MUL) { uses[a]++; uses[b]++; }
        if (op == T_NEG) uses[a]++;
    }
    for (uint32_t c = 0; c < p.n_constraints; c++) uses[cons[c]]++;

    std::vector<int32_t> reg_of(n_nodes, -1);
    std::vector<uint32_t> free_regs;
    uint32_t next_reg = 0;
    auto alloc_reg = [&]() -> uint32_t {
        if (!free_regs.empty()) {
            uint32_t r = free_regs.back();
            free_regs.pop_back();
            return r;
        }
        return next_reg++;
    };
    auto emit = [&](uint32_t op, uint32_t dst, uint32_t a, uint32_t b) {
        p.code.push_back(op);
        p.code.push_back(dst);
        p.code.push_back(a);
        p.code.push_back(b);
    };
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> const_slot;  // (public index | ~0u, value) -> slot
    auto add_const = [&](uint32_t canonical, uint32_t public_idx) -> uint32_t {
        auto [it, fresh] = const_slot.try_emplace({public_idx, canonical}, (uint32_t)p.const_canonical.size());
        if (fresh) {
            p.const_canonical.push_back(canonical);
            p.const_public_idx.push_back(public_idx);
        }
        return it->second;
    };
    auto release = [&](uint32_t node) {
        if (--uses[node] == 0) {
            free_regs.push_back((uint32_t)reg_of[node]);
            reg_of[node] = -1;
        }
    };

    // iterative post-order evaluation
    std::vector<std::pair<uint32_t, int>> stack;
    auto eval_node = [&](uint32_t root) {
        if (reg_of[root] >= 0) return;
        stack.push_back({root, 0});
        while (!stack.empty()) {
            auto [nd, state] = stack.back();
            uint32_t op = nodes[3 * nd], a = nodes[3 * nd + 1], b = nodes[3 * nd + 2];
            bool binary = (op == T_ADD || op == T_SUB || op == T_MUL);
            if (reg_of[nd] >= 0) { stack.pop_back(); continue; }
            if (state == 0) {
                stack.back().second = 1;
                if ((binary || op == T_NEG) && reg_of[a] < 0) { stack.push_back({a, 0}); continue; }
            }
            if (state <= 1) {
                stack.back().second = 2;
                if (binary && reg_of[b] < 0) { stack.push_back({b, 0}); continue; }
            }
            // operands ready (note: evaluating b cannot have freed a, a still has this pending use)
            uint32_t ra = 0, rb = 0;
            if (binary || op == T_NEG) ra = (uint32_t)reg_of[a];
            if (binary) rb = (uint32_t)reg_of[b];
            // free operands before allocating dst so that dst may reuse an operand register
            if (binary || op == T_NEG) release(a);
            if (binary) release(b);
            uint32_t dst = alloc_reg();
            reg_of[nd] = (int32_t)dst;
            switch (op) {
                case T_CONST: emit(D_CONST, dst, add_const(a, ~0u), 0); break;
                case T_PUBLIC: emit(D_CONST, dst, add_const(0, a), 0); break;
                case T_MAIN: emit(D_LOAD, dst, a, b); break;
                case T_PREP: emit(D_LOAD, dst, a + 2, b); break;
                // version 3: the aux trace takes side matrix 0's load operands (side matrix 1's beside
                // preprocessed columns), challenges and exposed words the public slots after the public values
                case T_AUX: emit(D_LOAD, dst, a + p.aux_load_base(), b); break;
                case T_CHALLENGE: emit(D_CONST, dst, add_const(0, p.n_public + a), 0); break;
                case T_EXPOSED: emit(D_CONST, dst, add_const(0, p.n_public + 4 * p.n_challenges + a), 0); break;
                case T_IS_FIRST: emit(D_SEL, dst, 0, 0); break;
                case T_IS_LAST: emit(D_SEL, dst, 1, 0); break;
                case T_IS_TRANSITION: emit(D_SEL, dst, 2, 0); break;
                case T_ADD: emit(D_ADD, dst, ra, rb); break;
                case T_SUB: emit(D_SUB, dst, ra, rb); break;
                case T_MUL: emit(D_MUL, dst, ra, rb); break;
                case T_NEG: emit(D_NEG, dst, ra, 0); break;
            }
            stack.pop_back();
        }
    };
    for (uint32_t c = 0; c < p.n_constraints; c++) {
        eval_node(cons[c]);
        emit(D_ASSERT, 0, (uint32_t)reg_of[cons[c]], c);
        release(cons[c]);
    }
    p.n_regs = std::max(next_reg, 1u);
    return p;
}

// ---- segment plan ------------------------------------------------------------------------------
namespace {
bool is_leaf(uint32_t op) { return op == D_LOAD || op == D_CONST || op == D_SEL; }
bool is_computed(uint32_t op) { return op == D_ADD || op == D_SUB || op == D_NEG || op == D_MUL; }
}  // namespace

SegmentPlan plan_segments(const AirProgram& p, uint32_t S, uint32_t reg_budget) {
    const uint32_t n = (uint32_t)(p.code.size() / 4);
    TS_REQUIRE(S >= 1 && reg_budget >= 4, TS_ERR_INVALID, "segment plan: bad size or budget");
    TS_REQUIRE(n <= SEG_MAX_INSTR, TS_ERR_INVALID, "segmented AIR: program above 2^20 lowered instructions");
    SegmentPlan plan;
    auto op_of = [&](uint32_t i) { return p.code[4 * i]; };
    // SSA view of the register program: the defining instruction of every operand
    plan.opdef.assign(2 * (size_t)n, ~0u);
    std::vector<uint32_t> cur(p.n_regs, ~0u), last_use(n, 0);
    std::vector<uint8_t> used(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t op = op_of(i), dst = p.code[4 * i + 1], a = p.code[4 * i + 2], b = p.code[4 * i + 3];
        const int nops = (op == D_ADD || op == D_SUB || op == D_MUL) ? 2 : (op == D_NEG || op == D_ASSERT) ? 1 : 0;
        const uint32_t regs[2] = {a, b};
        for (int k = 0; k < nops; k++) {
            const uint32_t v = cur[regs[k]];
            TS_REQUIRE(v != ~0u, TS_ERR_INVARIANT, "segment plan: read of an unwritten register");
            plan.opdef[2 * (size_t)i + k] = v;
            last_use[v] = i;
            used[v] = 1;
        }
        if (op != D_ASSERT) cur[dst] = i;
    }
    // cross[c]: computed values defined before instruction c and used at or after it (a cut before c)
    std::vector<int64_t> cross(n + 2, 0);
    for (uint32_t v = 0; v < n; v++)
        if (is_computed(op_of(v)) && used[v] && last_use[v] > v) {
            cross[v + 1]++;
            cross[last_use[v] + 1]--;
        }
    for (uint32_t c = 1; c <= n; c++) cross[c] += cross[c - 1];

    // values held at once by the kernel of [b, e): a value defined there lives from its definition to its
    // last use there; one from an earlier segment (a slot load or a re-emitted leaf) from its first to its
    // last use there
    std::vector<uint32_t> stamp(n, ~0u), first_in(n, 0), last_in(n, 0);
    std::vector<int32_t> diff(S + 2, 0);
    uint32_t epoch = 0;
    // `outs`: live-outs of [b, e) whose store waits (SegmentPlan::Slot::at) hold their value until then
    auto pressure = [&](uint32_t b, uint32_t e, const std::vector<SegmentPlan::Slot>* outs = nullptr) -> uint32_t {
        epoch++;
        std::vector<uint32_t> touched;
        auto touch = [&](uint32_t v, uint32_t i) {
            if (stamp[v] != epoch) {
                stamp[v] = epoch;
                first_in[v] = v >= b ? v : i;
                touched.push_back(v);
            }
            last_in[v] = i;
        };
        for (uint32_t i = b; i < e; i++) {
            for (int k = 0; k < 2; k++)
                if (plan.opdef[2 * (size_t)i + k] != ~0u) touch(plan.opdef[2 * (size_t)i + k], i);
            if (op_of(i) != D_ASSERT) touch(i, i);
        }
        if (outs)
            for (const auto& o : *outs) last_in[o.def] = std::max(last_in[o.def], o.at);
        std::fill(diff.begin(), diff.begin() + (e - b) + 2, 0);
        for (uint32_t v : touched) {
            diff[first_in[v] - b]++;
            diff[last_in[v] - b + 1]--;
        }
        int32_t run = 0, mx = 0;
        for (uint32_t i = 0; i < e - b; i++) mx = std::max(mx, run += diff[i]);
        return (uint32_t)mx;
    };

    uint32_t b = 0;
    while (b < n) {
        // the longest segment within S and the register budget (pressure grows with the end)
        uint32_t lo = b + 1, hi = std::min(n, b + S);
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (pressure(b, mid) <= reg_budget) lo = mid; else hi = mid - 1;
        }
        uint32_t e = lo;
        if (e < n) {  // cut at the fewest crossing values in the second half of the window (latest on a tie)
            const uint32_t w0 = b + std::max(1u, (e - b) / 2);
            uint32_t best = e;
            for (uint32_t c = e; c >= w0; c--)
                if (cross[c] < cross[best]) best = c;
            e = best;
        }
        SegmentPlan::Segment sg;
        sg.begin = b;
        sg.end = e;
        plan.segs.push_back(std::move(sg));
        b = e;
    }

    // slots: a live-out takes a free slot, else the slot of a value that dies in this segment once that value
    // has been loaded (the store then waits for the load), else a new one.  The width is the most values
    // crossing any one cut: when a new slot is opened, every slot in use holds a value that crosses the next cut.
    std::vector<uint32_t> slot_of(n, ~0u), free_slots;
    for (size_t k = 0; k < plan.segs.size(); k++) {
        SegmentPlan::Segment& sg = plan.segs[k];
        epoch++;
        std::vector<std::pair<uint32_t, uint32_t>> dying;  // (load position, slot)
        for (uint32_t i = sg.begin; i < sg.end; i++)
            for (int q = 0; q < 2; q++) {
                const uint32_t v = plan.opdef[2 * (size_t)i + q];
                if (v == ~0u || v >= sg.begin || !is_computed(op_of(v)) || stamp[v] == epoch) continue;
                stamp[v] = epoch;
                sg.live_in.push_back({v, slot_of[v], i});
                if (last_use[v] < sg.end) dying.push_back({i, slot_of[v]});
            }
        size_t dn = 0;  // dying is in load order already
        for (uint32_t v = sg.begin; v < sg.end; v++) {
            if (!is_computed(op_of(v)) || !used[v] || last_use[v] < sg.end) continue;
            while (dn < dying.size() && dying[dn].first <= v) free_slots.push_back(dying[dn++].second);
            uint32_t slot, at = v;
            if (!free_slots.empty()) {
                slot = free_slots.back();
                free_slots.pop_back();
            } else if (dn < dying.size()) {
                at = dying[dn].first;
                slot = dying[dn++].second;
            } else {
                slot = plan.slab_width++;
            }
            slot_of[v] = slot;
            sg.live_out.push_back({v, slot, at});
        }
        while (dn < dying.size()) free_slots.push_back(dying[dn++].second);
        sg.pressure = pressure(sg.begin, sg.end, &sg.live_out);
    }
    return plan;
}

}  // namespace ts
