// Constraint tape -> device program.
//
// The AIR crosses the C ABI as the serialised symbolic-constraint DAG that the reference obtains
// from `get_symbolic_constraints` (uni-stark/src/symbolic_builder.rs:52-64; node kinds of
// symbolic_expression.rs:12-37).  `compile_air` validates it, applies the reference's degree rules
// (symbolic_expression.rs:41-61,137,182,227; symbolic_builder.rs:15-32) and lowers it to a linear
// register program that the quotient kernel interprets (quotient.hip), one thread per row.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <vector>

namespace ts {

// tape format (include/tapstark.h)
constexpr uint32_t TAPE_MAGIC = 0x54415354u;
enum TapeOp : uint32_t {
    T_CONST = 0, T_MAIN = 1, T_PUBLIC = 2, T_IS_FIRST = 3, T_IS_LAST = 4, T_IS_TRANSITION = 5,
    T_ADD = 6, T_SUB = 7, T_NEG = 8, T_MUL = 9,
    T_PREP = 10,  // version-2 tapes only: a preprocessed column (symbolic_variable.rs:9-15 Entry::Preprocessed)
    // version-3 tapes only (build-defined: the reference has no challenge phase)
    T_AUX = 11,        // a = offset 0|1, b = column of the challenge-phase (aux) trace
    T_CHALLENGE = 12,  // a = word index < 4 * n_challenges
    T_EXPOSED = 13     // a = index < n_exposed
};

// device instruction: 4 x u32 {op, dst, a, b}.  Operands of ADD/SUB/MUL/NEG/ASSERT are register ids.
enum DevOp : uint32_t {
    D_LOAD = 0,     // dst <- to_mont(rows[a][b = column]); a = row offset + 2 * (matrix): 0/1 main local/next,
                    // 2/3 local/next of side matrix 0, 4/5 of side matrix 1 (AirProgram::n_side)
    D_CONST = 1,    // dst <- consts[a]           (Montgomery; constants and public values)
    D_SEL = 2,      // dst <- selector a (0 first, 1 last, 2 transition)
    D_ADD = 3,
    D_SUB = 4,
    D_NEG = 5,
    D_MUL = 6,
    D_ASSERT = 7,   // acc += reg[a] * alpha_pow[b]   (b = constraint index)
};

// The hiprtc-specialised quotient kernels of one AIR (jit.cpp), built whole and then published once
// (AirProgram::jit).  fns.size() == 1 and seg == nullptr: the monolithic k_quotient_jit; otherwise one
// k_quotient_seg<k> per segment of *seg, launched in order over a slab (quotient.hip).
struct SegmentPlan;
struct JitKernelSet {
    std::vector<void*> modules;
    std::vector<void*> fns;
    const SegmentPlan* seg = nullptr;
};
// A pointer that copies by value: readers load it once per launch (acquire); the owner stores it once,
// after the modules are loaded (release).
struct KernelSetRef {
    std::atomic<const JitKernelSet*> p{nullptr};
    KernelSetRef() = default;
    KernelSetRef(const KernelSetRef& o) : p(o.p.load(std::memory_order_acquire)) {}
    KernelSetRef& operator=(const KernelSetRef& o) {
        p.store(o.p.load(std::memory_order_acquire), std::memory_order_release);
        return *this;
    }
    const JitKernelSet* load() const { return p.load(std::memory_order_acquire); }
    void publish(const JitKernelSet* k) { p.store(k, std::memory_order_release); }
};

struct AirProgram {
    uint32_t width = 0;
    uint32_t preprocessed_width = 0;        // version-2 tapes (0: the AIR reads the main trace only)
    // version-3 tapes: the challenge-phase (aux) trace, its challenges (extension elements) and exposed words
    uint32_t aux_width = 0, n_challenges = 0, n_exposed = 0;
    uint32_t n_public = 0;
    // The side matrices: the committed matrices the program reads beside the main trace, in D_LOAD operand order
    // (side matrix i is a = 2 + 2i, 3 + 2i).  Key first, then aux: the preprocessed key if the AIR has one, then
    // the aux trace if it has one.  The same order is the opening order and the order of every list of them
    // (SideLdes, SideRows, LeadingMats).
    uint32_t n_side() const { return (preprocessed_width > 0) + (aux_width > 0); }
    bool side_is_aux(uint32_t i) const { return aux_width > 0 && i + 1 == n_side(); }
    uint32_t side_width(uint32_t i) const { return side_is_aux(i) ? aux_width : i == 0 ? preprocessed_width : 0; }
    // D_LOAD's operand a of the aux trace's local row
    uint32_t aux_load_base() const { return preprocessed_width ? 4 : 2; }
    // The public vector the lowered program indexes: public values ++ challenge words ++ exposed words
    uint32_t n_public_slots() const { return n_public + 4 * n_challenges + n_exposed; }
    uint32_t n_constraints = 0;
    uint32_t max_degree = 0;
    uint32_t log_quotient_degree = 0;
    uint32_t n_regs = 0;
    std::vector<uint32_t> code;             // 4 words per instruction
    std::vector<uint32_t> const_canonical;  // constants (canonical); publics are appended per proof
    std::vector<uint32_t> const_public_idx; // for entries that are public values: index, else ~0u
    std::vector<uint32_t> tape;             // the validated input (kept for the verifier side)
    uint32_t tape_header = 6;               // words before the nodes: 6 (version 1), 7 (version 2), 10 (version 3)
    const uint32_t* tape_nodes() const { return tape.data() + tape_header; }
    const uint32_t* tape_constraints() const { return tape_nodes() + 3 * (size_t)tape[4]; }
    // device copy of `code`, owned by the context that compiled it
    uint32_t* d_code = nullptr;
    // hiprtc-specialised quotient kernel(s) (jit.cpp); null => the interpreter in quotient.hip is used
    KernelSetRef jit;
};

// throws ts::Error(TS_ERR_INVALID) on a malformed tape
AirProgram compile_air(const uint32_t* tape, size_t n_words);

// ---- segmented specialisation (opt-in, ts_air_compile_opts): the lowered program cut into segments of at
// most S instructions, each its own kernel.  A computed value (ADD/SUB/NEG/MUL) defined in one segment and
// used in a later one crosses through a slot of an explicit slab in HBM, [slot][row of the tile]; leaves
// (LOAD/CONST/SEL) are never slotted but re-emitted where they are used.  Values are named by the index of
// the instruction that defines them.  The four EF4 accumulators of the ASSERT sum cross every cut too, as
// 8 words (lo, hi of a0..a3, after lazy_fix) in slab rows [slab_width, slab_width + 8).
constexpr uint32_t SEG_MAX_INSTR = 1u << 20;  // programs above this are refused (TS_ERR_INVALID)
constexpr uint32_t SEG_ACC_SLOTS = 8;
struct SegmentPlan {
    struct Slot {
        uint32_t def;   // defining instruction
        uint32_t slot;
        uint32_t at;    // live-out: stored right after instruction `at` (>= def: after the load of the slot's
                        // previous owner in this segment); live-in: loaded right before instruction `at`
                        // (its first use in the segment)
    };
    struct Segment {
        uint32_t begin = 0, end = 0;  // [begin, end) in lowered instructions
        std::vector<Slot> live_in, live_out;
        uint32_t pressure = 0;        // most values held at once in the segment (the kernel's live set)
    };
    uint32_t slab_width = 0;  // value slots: the most values live across any one cut
    std::vector<Segment> segs;
    // per instruction: the defining instructions of its operands a and b (~0u: not a register operand)
    std::vector<uint32_t> opdef;
};
// `reg_budget`: the most values one segment may hold at once; a segment is shortened below S to respect it
SegmentPlan plan_segments(const AirProgram& p, uint32_t S, uint32_t reg_budget);

}  // namespace ts
