"""Test-side maps between an AIR with challenge-phase (aux) columns (tape version 3, include/tapstark.h) and the
same constraints over ONE trace of width A + W with the public vector pis ++ challenges ++ exposed, which the
frozen oracle and the version-1 product path understand; a Python-integer EF4 and a Python-integer LogUp
reference.  TEST INFRASTRUCTURE."""
import numpy as np

from _prep_airs import prep_width

P = 0x78000001
TAPE_MAGIC = 0x54415354
OP_MAIN, OP_PUBLIC, OP_AUX, OP_CHALLENGE, OP_EXPOSED = 1, 2, 11, 12, 13
EF_W = 11


def _parts(tape):
    tape = np.asarray(tape, dtype=np.uint32)
    hdr = {1: 6, 2: 7, 3: 10}[int(tape[1])]
    n_nodes = int(tape[4])
    nodes = tape[hdr:hdr + 3 * n_nodes].reshape(n_nodes, 3).copy()
    return tape, nodes, tape[hdr + 3 * n_nodes:]


def aux_width_of(seed: int, w: int) -> int:
    """The split of a width-w random AIR (w >= 2): A from {1, w // 2, w - 1}, chosen by seed."""
    return prep_width(seed, w)


def split_counts(q: int):
    """(public values kept, challenges, exposed words) of an AIR with q public values."""
    return (q - 5, 1, 1) if q >= 5 else (q - 4, 1, 0) if q >= 4 else (q, 0, 0)


def split_tape_aux(v1_tape, A: int) -> np.ndarray:
    """MAIN(off, c < A) -> AUX(off, c), MAIN(off, c >= A) -> MAIN(off, c - A); with q public values: if q >= 4
    the last four become CHALLENGE 0..3, and if q >= 5 the one before them EXPOSED 0.  Version-3 header."""
    tape, nodes, cons = _parts(v1_tape)
    assert int(tape[1]) == 1 and 0 <= A < int(tape[2])
    q = int(tape[3])
    keep, nc, ne = split_counts(q)
    main = nodes[:, 0] == OP_MAIN
    aux = main & (nodes[:, 2] < A)
    nodes[main & ~aux, 2] -= A
    nodes[aux, 0] = OP_AUX
    pub = nodes[:, 0] == OP_PUBLIC
    chal = pub & (nodes[:, 1] >= q - 4) if nc else None  # (both masks before either rewrite)
    expo = pub & (nodes[:, 1] == q - 5) if ne else None
    if nc:
        nodes[chal, 1] -= q - 4
        nodes[chal, 0] = OP_CHALLENGE
    if ne:
        nodes[expo, 1] = 0
        nodes[expo, 0] = OP_EXPOSED
    head = [TAPE_MAGIC, 3, int(tape[2]) - A, keep, len(nodes), len(cons), 0, A, nc, ne]
    return np.concatenate([np.asarray(head, dtype=np.uint32), nodes.reshape(-1), cons]).astype(np.uint32)


def join_tape_aux(v3_tape) -> np.ndarray:
    """The version-1 tape over hstack(aux, main) with the public values pis ++ challenges ++ exposed."""
    tape, nodes, cons = _parts(v3_tape)
    assert int(tape[1]) == 3 and int(tape[6]) == 0
    q, A, nc, ne = int(tape[3]), int(tape[7]), int(tape[8]), int(tape[9])
    nodes[nodes[:, 0] == OP_MAIN, 2] += A
    nodes[nodes[:, 0] == OP_AUX, 0] = OP_MAIN
    chal, expo = nodes[:, 0] == OP_CHALLENGE, nodes[:, 0] == OP_EXPOSED
    nodes[chal, 1] += q
    nodes[expo, 1] += q + 4 * nc
    nodes[chal | expo, 0] = OP_PUBLIC
    head = [TAPE_MAGIC, 1, int(tape[2]) + A, q + 4 * nc + ne, len(nodes), len(cons)]
    return np.concatenate([np.asarray(head, dtype=np.uint32), nodes.reshape(-1), cons]).astype(np.uint32)


def split_publics(pis):
    """The public values of the unsplit AIR -> (public values, challenge words, exposed words) of the split one;
    their concatenation is the public vector of the joined tape."""
    pis = np.asarray(pis, dtype=np.uint32)
    keep, nc, ne = split_counts(len(pis))
    return pis[:keep].copy(), pis[len(pis) - 4 * nc:].copy(), pis[keep:keep + ne].copy()


def join_program_aux(prog: dict, A: int) -> dict:
    """A lowered version-3 program on joined columns, as _air_program.run_program runs it: LOAD a = 2, 3 ->
    (a - 2, column); a = 0, 1 -> (a, column + A).  The public slots already are those of the joined tape."""
    from _air_program import D_LOAD
    code = prog["code"].copy()
    load = code[:, 0] == D_LOAD
    aux = load & (code[:, 2] >= 2)
    code[load & ~aux, 3] += A
    code[aux, 2] -= 2
    return {**prog, "code": code}


# ---------------------------------------------------------------------------------------------- EF4 on Python integers
def ef(x=0):
    return (int(x) % P, 0, 0, 0)


def ef_add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def ef_sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def ef_mul(a, b):
    out = [0, 0, 0, 0]
    for i in range(4):
        for j in range(4):
            k = i + j
            out[k % 4] += a[i] * b[j] * (EF_W if k >= 4 else 1)
    return tuple(x % P for x in out)


def ef_scale(a, s):
    return tuple(x * int(s) % P for x in a)


def ef_inv(a):
    """Through the tower F < F[y]/(y^2 - 11) < F[x]/(x^2 - y): a = A + x B, a (A - x B) = A^2 - y B^2 = c0 + c1 y."""
    a0, a1, a2, a3 = a
    c0 = (a0 * a0 + EF_W * a2 * a2 - EF_W * 2 * a1 * a3) % P
    c1 = (2 * a0 * a2 - a1 * a1 - EF_W * a3 * a3) % P
    nrm = (c0 * c0 - EF_W * c1 * c1) % P
    if nrm == 0:
        raise ZeroDivisionError("EF4 inverse of zero")
    ninv = pow(nrm, P - 2, P)
    return ef_scale(ef_mul((a0, -a1 % P, a2, -a3 % P), (c0, 0, -c1 % P, 0)), ninv)


# ---------------------------------------------------------------------------------------------- LogUp on Python integers
def logup_reference(interactions, trace, gamma, beta):
    """interactions: [((kind, value), [(kind, value), ...]), ...] with kind 0 constant / 1 main column.
    Returns (aux (n, 4 (G + 1)) uint32, S as four words)."""
    trace = np.asarray(trace)
    n, K = trace.shape[0], len(interactions)
    G = (K + 1) // 2
    gamma, beta = tuple(int(x) for x in gamma), tuple(int(x) for x in beta)
    n_pow = max(len(v) for _, v in interactions)
    bp = [ef(1)]
    for _ in range(1, n_pow):
        bp.append(ef_mul(bp[-1], beta))
    aux = np.zeros((n, 4 * (G + 1)), dtype=np.uint32)
    phi = ef(0)
    rows = trace.tolist()
    term = lambda t, row: t[1] if t[0] == 0 else row[t[1]]
    for r in range(n):
        row = rows[r]
        total = ef(0)
        for g in range(G):
            h = ef(0)
            for i in (2 * g, 2 * g + 1):
                if i >= K:
                    continue
                m, vals = interactions[i]
                d = gamma
                for j, v in enumerate(vals):
                    d = ef_add(d, ef_scale(bp[j], term(v, row)))
                h = ef_add(h, ef_scale(ef_inv(d), term(m, row)))
            aux[r, 4 * g:4 * g + 4] = h
            total = ef_add(total, h)
        aux[r, 4 * G:] = phi
        phi = ef_add(phi, total)
    return aux, np.array(phi, dtype=np.uint32)
