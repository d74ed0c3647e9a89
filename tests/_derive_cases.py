"""Row programs (``ts_matrix_derive``) for tests/test_derive_cpu.py and tests/test_gpu_derive.py: an exact reference
that works from the tape words alone -- it knows nothing of the library's lowering --, the operands, and seeded random
programs."""
import numpy as np

from _field_cases import E, P

MAGIC = 0x52454454
CONST, COL, IS_FIRST, IS_LAST, IS_TRANS, ADD, SUB, NEG, MUL = 0, 1, 3, 4, 5, 6, 7, 8, 9
ROW, INV, IS_ZERO, LT, BITS, AND, XOR = 32, 33, 34, 35, 36, 37, 38
LEAVES = (CONST, COL, IS_FIRST, IS_LAST, IS_TRANS, ROW)
UNARY = (NEG, INV, IS_ZERO, BITS)
BINARY = (ADD, SUB, MUL, LT, AND, XOR)
ALL_OPS = LEAVES + UNARY + BINARY

# stored words: the field's edge set and the words no canonical matrix holds
STORED = list(E) + [P, P + 1, 1 << 31, 0xFFFFFFFF]


def tape(src_width, nodes, outputs):
    w = [MAGIC, 1, src_width, len(nodes), len(outputs)]
    for n in nodes:
        w += list(n)
    for o in outputs:
        w += list(o)
    return np.array(w, dtype=np.uint64).astype(np.uint32)


def parse(program):
    t = [int(x) for x in np.asarray(program).reshape(-1)]
    assert t[0] == MAGIC and t[1] == 1 and len(t) == 5 + 3 * t[3] + 2 * t[4]
    nodes = [tuple(t[5 + 3 * i: 8 + 3 * i]) for i in range(t[3])]
    at = 5 + 3 * t[3]
    outputs = [tuple(t[at + 2 * k: at + 2 * k + 2]) for k in range(t[4])]
    return t[2], nodes, outputs


def _row_int(nodes, rows, r):
    """the node values on row r, in Python integers"""
    h = len(rows)
    v = []
    for op, a, b in nodes:
        if op == CONST:
            x = a
        elif op == COL:
            x = int(rows[(r, (r + 1) % h, (r - 1) % h)[a]][b]) % P
        elif op == IS_FIRST:
            x = int(r == 0)
        elif op == IS_LAST:
            x = int(r == h - 1)
        elif op == IS_TRANS:
            x = int(r != h - 1)
        elif op == ROW:
            x = r
        elif op == ADD:
            x = (v[a] + v[b]) % P
        elif op == SUB:
            x = (v[a] - v[b]) % P
        elif op == NEG:
            x = (-v[a]) % P
        elif op == MUL:
            x = v[a] * v[b] % P
        elif op == INV:
            x = pow(v[a], -1, P) if v[a] else 0
        elif op == IS_ZERO:
            x = int(v[a] == 0)
        elif op == LT:
            x = int(v[a] < v[b])
        elif op == BITS:
            x = (v[a] >> (b & 255)) & ((1 << (b >> 8)) - 1)
        elif op == AND:
            x = (v[a] & v[b]) % P
        elif op == XOR:
            x = (v[a] ^ v[b]) % P
        else:
            raise AssertionError(f"op {op}")
        v.append(x)
    return v


def _cols_u64(nodes, rows):
    """the node values on every row, numpy uint64 (a product of two values below p is below 2^62)"""
    h = rows.shape[0]
    p = np.uint64(P)
    r = np.arange(h, dtype=np.uint64)
    src = (rows.astype(np.uint64) % p, np.roll(rows, -1, axis=0).astype(np.uint64) % p,
           np.roll(rows, 1, axis=0).astype(np.uint64) % p)
    v = []
    for op, a, b in nodes:
        if op == CONST:
            x = np.full(h, a, dtype=np.uint64)
        elif op == COL:
            x = src[a][:, b]
        elif op == IS_FIRST:
            x = (r == 0).astype(np.uint64)
        elif op == IS_LAST:
            x = (r == h - 1).astype(np.uint64)
        elif op == IS_TRANS:
            x = (r != h - 1).astype(np.uint64)
        elif op == ROW:
            x = r.copy()
        elif op == ADD:
            x = (v[a] + v[b]) % p
        elif op == SUB:
            x = (v[a] + p - v[b]) % p
        elif op == NEG:
            x = (p - v[a]) % p
        elif op == MUL:
            x = v[a] * v[b] % p
        elif op == INV:
            x, base, e = np.ones(h, dtype=np.uint64), v[a].copy(), P - 2
            while e:
                if e & 1:
                    x = x * base % p
                base = base * base % p
                e >>= 1
            x[v[a] == 0] = 0
        elif op == IS_ZERO:
            x = (v[a] == 0).astype(np.uint64)
        elif op == LT:
            x = (v[a] < v[b]).astype(np.uint64)
        elif op == BITS:
            x = (v[a] >> np.uint64(b & 255)) & np.uint64((1 << (b >> 8)) - 1)
        elif op == AND:
            x = (v[a] & v[b]) % p
        elif op == XOR:
            x = (v[a] ^ v[b]) % p
        else:
            raise AssertionError(f"op {op}")
        v.append(x)
    return v


def reference(program, rows, force=None):
    """The matrix the program makes of ``rows`` ((h, src_width) uint32, any words): Python integers up to 64 rows,
    numpy uint64 beyond (``force`` = "int" | "u64" picks one)."""
    rows = np.asarray(rows, dtype=np.uint32)
    src_width, nodes, outputs = parse(program)
    assert rows.ndim == 2 and rows.shape[1] == src_width
    h = rows.shape[0]
    out = np.zeros((h, max([src_width] + [d + 1 for _, d in outputs])), dtype=np.uint32)
    out[:, :src_width] = rows
    if force == "int" or (force is None and h <= 64):
        for r in range(h):
            v = _row_int(nodes, rows, r)
            for n, d in outputs:
                out[r, d] = v[n]
    else:
        v = _cols_u64(nodes, rows)
        for n, d in outputs:
            out[:, d] = v[n].astype(np.uint32)
    return out


def planted_pairs(values=None):
    """(len(values)^2, 2): every ordered pair of stored words, one per row"""
    values = STORED if values is None else values
    a = np.array(values, dtype=np.uint64).astype(np.uint32)
    return np.stack([np.repeat(a, len(a)), np.tile(a, len(a))], axis=1)


def op_program(op):
    """width 2 -> 3: column 2 = op over columns 0 and 1 (BITS as the middle 12 bits from bit 7)"""
    nodes = [(COL, 0, 0), (COL, 0, 1)]
    if op in LEAVES:
        nodes.append({CONST: (CONST, P - 1, 0), COL: (COL, 1, 1)}.get(op, (op, 0, 0)))
    elif op in UNARY:
        nodes.append((op, 0, 7 | 12 << 8 if op == BITS else 0))
    else:
        nodes.append((op, 0, 1))
    return tape(2, nodes, [(2, 2)])


def random_program(seed, width):
    """4 to 60 nodes of every op and all three offsets, sub-expressions shared far from where they are defined (an
    operand is as likely an early node as a recent one), 1 to 6 outputs that overwrite and append."""
    rng = np.random.default_rng([seed, width, 0xDE71])
    n = int(rng.integers(4, 61))
    nodes = []
    for i in range(n):
        leaf = i < 2 or rng.random() < 0.3
        op = int(rng.choice(LEAVES if leaf else UNARY + BINARY))

        def pick():
            if rng.random() < 0.5:
                return int(rng.integers(0, i))             # anywhere before: far uses
            return int(rng.integers(max(0, i - 3), i))     # recent
        if op == CONST:
            nodes.append((CONST, int(rng.choice([0, 1, 2, P - 1, int(rng.integers(0, P))])), 0))
        elif op == COL:
            nodes.append((COL, int(rng.integers(0, 3)), int(rng.integers(0, width))))
        elif op in LEAVES:
            nodes.append((op, 0, 0))
        elif op == BITS:
            shift = int(rng.integers(0, 31))
            nodes.append((BITS, pick(), shift | int(rng.integers(1, 32 - shift)) << 8))
        elif op in UNARY:
            nodes.append((op, pick(), 0))
        else:
            nodes.append((op, pick(), pick()))
    n_out = int(rng.integers(1, 7))
    n_over = int(rng.integers(0, min(n_out, width) + 1))
    dsts = [int(c) for c in rng.choice(width, n_over, replace=False)] + list(range(width, width + n_out - n_over))
    outputs = [(int(rng.integers(max(0, n - 8), n)) if k == 0 else int(rng.integers(0, n)), d)
               for k, d in enumerate(dsts)]
    return tape(width, nodes, outputs)


def random_rows(seed, height, width):
    """canonical words, a sprinkling of the stored edge words among them"""
    rng = np.random.default_rng([seed, height, width])
    rows = rng.integers(0, P, (height, width), dtype=np.uint64)
    edge = np.array(STORED, dtype=np.uint64)
    mask = rng.random((height, width)) < 0.15
    rows[mask] = edge[rng.integers(0, len(edge), int(mask.sum()))]
    return rows.astype(np.uint32)


def sum_of_loads_program(k, width=None):
    """k loads, then their sum: holds exactly k values at once"""
    width = k if width is None else width
    nodes = [(COL, 0, c % width) for c in range(k)]
    acc = 0
    for c in range(1, k):
        nodes.append((ADD, acc, c))
        acc = len(nodes) - 1
    return tape(width, nodes, [(acc, width)])
