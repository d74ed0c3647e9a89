"""Test-side model of the segmented quotient kernels (``ts_air_segment_plan``, tap-stark_amd/csrc/air.cpp
plan_segments, jit.cpp jit_segment_sources) in numpy.  TEST INFRASTRUCTURE: the lowered program is read in
SSA form (a value is named by the instruction that defines it), cut as the plan says and run segment by
segment with nothing carried between segments but a numpy slab [slot][row]; leaves (LOAD, CONST, SEL) are
re-emitted where a later segment uses them.  Loads and stores follow the generator's order, so a slot that
is reused too early shows up as a wrong value, or as the owner check below."""
import numpy as np

from _air_program import D_ADD, D_ASSERT, D_CONST, D_LOAD, D_MUL, D_NEG, D_SEL, D_SUB, P

LEAVES = (D_LOAD, D_CONST, D_SEL)
COMPUTED = (D_ADD, D_SUB, D_NEG, D_MUL)


def ssa(prog: dict):
    """(opdefs, last_use): per instruction the defining instructions of its register operands, and per value
    its last use (-1: never used)."""
    code = prog["code"].tolist()
    cur = {}
    opdefs, last_use = [], [-1] * len(code)
    for i, (op, dst, a, b) in enumerate(code):
        regs = (a, b) if op in (D_ADD, D_SUB, D_MUL) else (a,) if op in (D_NEG, D_ASSERT) else ()
        ds = tuple(cur[r] for r in regs)
        for v in ds:
            last_use[v] = i
        opdefs.append(ds)
        if op != D_ASSERT:
            cur[dst] = i
    return opdefs, last_use


def max_live_across_cut(prog: dict, cuts) -> int:
    """The most computed values defined before a cut and used at or after it, over the given cuts."""
    code = prog["code"]
    _, last_use = ssa(prog)
    n = len(code)
    cross = np.zeros(n + 2, dtype=np.int64)
    for v in range(n):
        if code[v][0] in COMPUTED and last_use[v] > v:
            cross[v + 1] += 1
            cross[last_use[v] + 1] -= 1
    cross = np.cumsum(cross)
    return max((int(cross[c]) for c in cuts), default=0)


def store_positions(plan: dict, prog: dict):
    """Per segment {def: position after which the generator stores it}: at its definition, or after the
    first use here of the slot's previous owner when that value dies in this segment."""
    opdefs, _ = ssa(prog)
    out = []
    for sg in plan["segments"]:
        first = {}
        for pc in range(sg["begin"], sg["end"]):
            for v in opdefs[pc]:
                first.setdefault(v, pc)
        owner_load = {slot: first[v] for v, slot in sg["live_in"]}
        out.append({v: max(v, owner_load.get(slot, v)) for v, slot in sg["live_out"]})
    return out


def run_segmented(prog: dict, plan: dict, local, nxt, pis, sels, n_constraints: int):
    """(m, n_constraints) constraint values, as _air_program.run_program, through the plan's segments."""
    m = local.shape[0]
    p = np.uint64(P)
    code = prog["code"].tolist()
    opdefs, _ = ssa(prog)
    consts = [int(pis[pi]) if pi != 0xFFFFFFFF else int(v) for v, pi in zip(prog["consts"], prog["const_public"])]
    rows = (local.astype(np.uint64), nxt.astype(np.uint64))
    sels = sels.astype(np.uint64)
    width = plan["slab_width"]
    slab = np.zeros((max(width, 1), m), dtype=np.uint64)
    owner = [-1] * max(width, 1)
    out = np.zeros((m, n_constraints), dtype=np.uint32)
    seen = np.zeros(n_constraints, dtype=bool)
    stores = store_positions(plan, prog)

    def leaf(i):
        op, _, a, b = code[i]
        if op == D_LOAD:
            return rows[a][:, b]
        if op == D_CONST:
            return np.full(m, consts[a], dtype=np.uint64)
        assert op == D_SEL
        return sels[:, a]

    for sg, st in zip(plan["segments"], stores):
        b, e = sg["begin"], sg["end"]
        slot_in = dict(sg["live_in"])
        at = {}
        for v, pos in st.items():
            at.setdefault(pos, []).append(v)
        slot_out = dict(sg["live_out"])
        vals = {}  # this segment's kernel: nothing survives it but the slab
        for pc in range(b, e):
            for v in opdefs[pc]:
                if v >= b or v in vals:
                    continue
                if code[v][0] in LEAVES:
                    vals[v] = leaf(v)
                else:
                    s = slot_in[v]
                    assert owner[s] == v, f"slot {s} holds {owner[s]}, not {v}"
                    vals[v] = slab[s].copy()
            op = code[pc][0]
            ov = [vals[v] for v in opdefs[pc]]
            if op in LEAVES:
                vals[pc] = leaf(pc)
            elif op == D_ADD:
                vals[pc] = (ov[0] + ov[1]) % p
            elif op == D_SUB:
                vals[pc] = (ov[0] + p - ov[1]) % p
            elif op == D_NEG:
                vals[pc] = (p - ov[0]) % p
            elif op == D_MUL:
                vals[pc] = (ov[0] * ov[1]) % p
            else:
                c = code[pc][3]
                assert op == D_ASSERT and not seen[c]
                seen[c] = True
                out[:, c] = ov[0]
            for v in at.get(pc, ()):
                s = slot_out[v]
                slab[s] = vals[v]
                owner[s] = v
    assert seen.all(), "a constraint was never asserted"
    return out
