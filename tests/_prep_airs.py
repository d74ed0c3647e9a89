"""Test-side maps between an AIR with preprocessed columns (tape version 2, include/tapstark.h) and the same
constraints over ONE trace of width P + W, which the frozen oracle and the version-1 product path understand:
the quotient of an AIR with P preprocessed and W main columns is, row by row, the quotient of the joined AIR
over hstack(preprocessed, main).  TEST INFRASTRUCTURE."""
import numpy as np

from _air_program import D_LOAD

TAPE_MAGIC = 0x54415354
OP_MAIN, OP_PREP = 1, 10


def _parts(tape):
    tape = np.asarray(tape, dtype=np.uint32)
    hdr = 7 if int(tape[1]) == 2 else 6
    n_nodes = int(tape[4])
    nodes = tape[hdr:hdr + 3 * n_nodes].reshape(n_nodes, 3).copy()
    return tape, nodes, tape[hdr + 3 * n_nodes:]


def split_tape(v1_tape, P: int) -> np.ndarray:
    """MAIN(off, c < P) -> PREP(off, c), MAIN(off, c >= P) -> MAIN(off, c - P), version-2 header."""
    tape, nodes, cons = _parts(v1_tape)
    assert int(tape[1]) == 1 and 0 <= P < int(tape[2])
    main = nodes[:, 0] == OP_MAIN
    prep = main & (nodes[:, 2] < P)
    nodes[main & ~prep, 2] -= P
    nodes[prep, 0] = OP_PREP
    head = [TAPE_MAGIC, 2, int(tape[2]) - P, int(tape[3]), len(nodes), len(cons), P]
    return np.concatenate([np.asarray(head, dtype=np.uint32), nodes.reshape(-1), cons]).astype(np.uint32)


def join_tape(v2_tape) -> np.ndarray:
    """The inverse: the version-1 tape over hstack(preprocessed, main)."""
    tape, nodes, cons = _parts(v2_tape)
    assert int(tape[1]) == 2
    P = int(tape[6])
    nodes[nodes[:, 0] == OP_MAIN, 2] += P
    nodes[nodes[:, 0] == OP_PREP, 0] = OP_MAIN
    head = [TAPE_MAGIC, 1, int(tape[2]) + P, int(tape[3]), len(nodes), len(cons)]
    return np.concatenate([np.asarray(head, dtype=np.uint32), nodes.reshape(-1), cons]).astype(np.uint32)


def join_program(prog: dict, P: int) -> dict:
    """A lowered version-2 program (LOAD a = offset + 2 * preprocessed) on joined columns, as
    _air_program.run_program runs it: a = 2, 3 -> (a - 2, column); a = 0, 1 -> (a, column + P)."""
    code = prog["code"].copy()
    load = code[:, 0] == D_LOAD
    prep = load & (code[:, 2] >= 2)
    code[load & ~prep, 3] += P
    code[prep, 2] -= 2
    return {**prog, "code": code}


def prep_width(seed: int, w: int) -> int:
    """The split of a width-w random AIR (w >= 2): P from {1, w // 2, w - 1}, chosen by seed."""
    return max(1, (1, w // 2, w - 1)[(seed // 2) % 3])


def next_row_loads(prog: dict):
    """(preprocessed, main) columns the lowered program reads from the next row."""
    code = prog["code"]
    ld = code[code[:, 0] == D_LOAD]
    return set(ld[ld[:, 2] == 3, 3].tolist()), set(ld[ld[:, 2] == 1, 3].tolist())
