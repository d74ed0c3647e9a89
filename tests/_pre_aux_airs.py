"""Test-side maps between an AIR with preprocessed AND challenge-phase (aux) columns (tape version 3 with both
widths, include/tapstark.h) and the same constraints over ONE trace of width P + A + W with the public vector
pis ++ challenges ++ exposed, which the frozen oracle and the version-1 product path understand: the quotient
over (P key, A aux, W main) is, row by row, the quotient of the joined AIR over hstack(pre, aux, main).  Also a
local copy of the register interpreter over six row arrays, and the remap of a LogUp spec with table terms onto
hstack(trace, table).  TEST INFRASTRUCTURE."""
import numpy as np

from _air_program import D_ADD, D_ASSERT, D_CONST, D_LOAD, D_MUL, D_NEG, D_SEL, D_SUB
from _aux_airs import split_counts, split_publics  # noqa: F401  (the publics split as for a pure-aux AIR)

P = 0x78000001
TAPE_MAGIC = 0x54415354
OP_MAIN, OP_PUBLIC, OP_PREP, OP_AUX, OP_CHALLENGE, OP_EXPOSED = 1, 2, 10, 11, 12, 13


def _parts(tape):
    tape = np.asarray(tape, dtype=np.uint32)
    hdr = {1: 6, 2: 7, 3: 10}[int(tape[1])]
    n_nodes = int(tape[4])
    nodes = tape[hdr:hdr + 3 * n_nodes].reshape(n_nodes, 3).copy()
    return tape, nodes, tape[hdr + 3 * n_nodes:]


def split_widths(seed: int, w: int, which: int):
    """(p, a) of a width-w random AIR, w >= 3.  which 0: the narrowest (1, 1); 1: main left with one column,
    the rest halved by seed parity; 2: a wide key, p = w - 2 and a = 1 (p above both a and the main width
    when w >= 5)."""
    assert w >= 3
    if which == 0:
        return 1, 1
    if which == 1:
        p = 1 + (seed % (w - 2))
        return p, w - 1 - p
    return w - 2, 1


def split_tape_pre_aux(v1_tape, p: int, a: int) -> np.ndarray:
    """MAIN(off, c < p) -> PREP(off, c); MAIN(off, p <= c < p + a) -> AUX(off, c - p); the rest MAIN(off, c - p -
    a); the public values as _aux_airs.split_tape_aux splits them.  Version-3 header with both widths."""
    tape, nodes, cons = _parts(v1_tape)
    assert int(tape[1]) == 1 and p >= 0 and a >= 0 and p + a < int(tape[2])
    q = int(tape[3])
    keep, nc, ne = split_counts(q)
    main = nodes[:, 0] == OP_MAIN
    prep = main & (nodes[:, 2] < p)
    aux = main & ~prep & (nodes[:, 2] < p + a)
    rest = main & ~prep & ~aux
    nodes[rest, 2] -= p + a
    nodes[aux, 2] -= p
    nodes[aux, 0] = OP_AUX
    nodes[prep, 0] = OP_PREP
    pub = nodes[:, 0] == OP_PUBLIC
    chal = pub & (nodes[:, 1] >= q - 4) if nc else None  # (both masks before either rewrite)
    expo = pub & (nodes[:, 1] == q - 5) if ne else None
    if nc:
        nodes[chal, 1] -= q - 4
        nodes[chal, 0] = OP_CHALLENGE
    if ne:
        nodes[expo, 1] = 0
        nodes[expo, 0] = OP_EXPOSED
    head = [TAPE_MAGIC, 3, int(tape[2]) - p - a, keep, len(nodes), len(cons), p, a, nc, ne]
    return np.concatenate([np.asarray(head, dtype=np.uint32), nodes.reshape(-1), cons]).astype(np.uint32)


def join_tape_pre_aux(v3_tape) -> np.ndarray:
    """The version-1 tape over hstack(pre, aux, main) with the public values pis ++ challenges ++ exposed."""
    tape, nodes, cons = _parts(v3_tape)
    assert int(tape[1]) == 3
    q, p, a, nc, ne = int(tape[3]), int(tape[6]), int(tape[7]), int(tape[8]), int(tape[9])
    nodes[nodes[:, 0] == OP_MAIN, 2] += p + a
    auxm = nodes[:, 0] == OP_AUX
    nodes[auxm, 2] += p
    nodes[auxm, 0] = OP_MAIN
    nodes[nodes[:, 0] == OP_PREP, 0] = OP_MAIN
    chal, expo = nodes[:, 0] == OP_CHALLENGE, nodes[:, 0] == OP_EXPOSED
    nodes[chal, 1] += q
    nodes[expo, 1] += q + 4 * nc
    nodes[chal | expo, 0] = OP_PUBLIC
    head = [TAPE_MAGIC, 1, int(tape[2]) + p + a, q + 4 * nc + ne, len(nodes), len(cons)]
    return np.concatenate([np.asarray(head, dtype=np.uint32), nodes.reshape(-1), cons]).astype(np.uint32)


def run_program6(prog: dict, rows6, pis, sels: np.ndarray, n_constraints: int):
    """_air_program.run_program over SIX row arrays: rows6[a] is what D_LOAD's operand a reads -- (main local,
    main next, key local, key next, aux local, aux next), each (m, its width) canonical.  (m, n_constraints)
    constraint values."""
    m = sels.shape[0]
    p = np.uint64(P)
    consts = [int(pis[pi]) if pi != 0xFFFFFFFF else int(v) for v, pi in zip(prog["consts"], prog["const_public"])]
    regs = np.zeros((prog["n_regs"], m), dtype=np.uint64)
    written = np.zeros(prog["n_regs"], dtype=bool)
    out = np.zeros((m, n_constraints), dtype=np.uint32)
    seen = np.zeros(n_constraints, dtype=bool)
    rows = [np.asarray(r).astype(np.uint64) for r in rows6]
    sels = sels.astype(np.uint64)
    for op, dst, a, b in prog["code"].tolist():
        if op == D_LOAD:
            assert a < 6 and b < rows[a].shape[1], "load outside its matrix"
            v = rows[a][:, b]
        elif op == D_CONST:
            v = np.full(m, consts[a], dtype=np.uint64)
        elif op == D_SEL:
            v = sels[:, a]
        elif op == D_ASSERT:
            assert written[a] and not seen[b]
            seen[b] = True
            out[:, b] = regs[a]
            continue
        else:
            assert written[a] and (op == D_NEG or written[b]), "read of a register never written"
            if op == D_ADD:
                v = (regs[a] + regs[b]) % p
            elif op == D_SUB:
                v = (regs[a] + p - regs[b]) % p
            elif op == D_NEG:
                v = (p - regs[a]) % p
            elif op == D_MUL:
                v = (regs[a] * regs[b]) % p
            else:
                raise AssertionError(f"unknown op {op}")
        regs[dst] = v
        written[dst] = True
    assert seen.all(), "a constraint was never asserted"
    return out


def remap_logup(interactions, W: int):
    """A LogUp spec with table terms (kind 2, column c) as the spec over hstack(trace, table): (1, W + c)."""
    term = lambda t: (1, W + t[1]) if t[0] == 2 else t
    return [(term(m), [term(v) for v in vals]) for m, vals in interactions]
