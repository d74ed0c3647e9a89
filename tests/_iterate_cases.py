"""Row programs with carried state (the iterate form of ``ts_matrix_derive``) for tests/test_iterate_cpu.py and
tests/test_gpu_iterate.py: an exact reference that walks the rows in Python integers straight from the tape words -- it
knows nothing of the library's lowering --, planted inputs, and seeded random programs: derive's random programs plus
carries and the four group ops."""
import numpy as np

import _derive_cases as dc
from _derive_cases import ADD, BINARY, BITS, COL, CONST, LEAVES, MUL, UNARY
from _field_cases import P

MAGIC = 0x52544954
CARRY, STEP, IS_GROUP_FIRST, IS_GROUP_LAST = 40, 41, 42, 43
GROUP_OPS = (CARRY, STEP, IS_GROUP_FIRST, IS_GROUP_LAST)
NO_RESET = 0xFFFFFFFF
MAX_WORK = 1 << 20


def tape(src_width, nodes, outputs, carries, reset_column=NO_RESET, max_group_rows=1 << 12):
    w = [MAGIC, 1, src_width, len(nodes), len(outputs), len(carries), reset_column, max_group_rows]
    for part in (nodes, outputs, carries):
        for x in part:
            w += list(x)
    return np.array(w, dtype=np.uint64).astype(np.uint32)


def parse(program):
    t = [int(x) for x in np.asarray(program).reshape(-1)]
    assert t[0] == MAGIC and t[1] == 1 and len(t) == 8 + 3 * t[3] + 2 * t[4] + 2 * t[5]
    nodes = [tuple(t[8 + 3 * i: 11 + 3 * i]) for i in range(t[3])]
    at = 8 + 3 * t[3]
    outputs = [tuple(t[at + 2 * k: at + 2 * k + 2]) for k in range(t[4])]
    at += 2 * t[4]
    carries = [tuple(t[at + 2 * k: at + 2 * k + 2]) for k in range(t[5])]
    return t[2], nodes, outputs, carries, t[6], t[7]


def group_starts(rows, reset_column):
    """the rows that start a group: row 0, and every row whose reset word is not 0 mod p"""
    h = len(rows)
    if reset_column == NO_RESET:
        return [0]
    return [r for r in range(h) if r == 0 or int(rows[r][reset_column]) % P != 0]


def longest_refusal(rows, reset_column, max_group_rows):
    """the library's text for the least over-long group, or None"""
    s = group_starts(rows, reset_column) + [len(rows)]
    for a, b in zip(s, s[1:]):
        if b - a > max_group_rows:
            return f"iterate: the group that starts at row {a} has {b - a} rows, max_group_rows is {max_group_rows}"
    return None


def _row_local(op, a, b, v, rows, r, h):
    """a TDER op on row r, in Python integers: v holds the node values before it"""
    if op == CONST:
        return a
    if op == COL:
        return rows[(r, (r + 1) % h, (r - 1) % h)[a]][b] % P
    if op == dc.IS_FIRST:
        return int(r == 0)
    if op == dc.IS_LAST:
        return int(r == h - 1)
    if op == dc.IS_TRANS:
        return int(r != h - 1)
    if op == dc.ROW:
        return r
    if op == ADD:
        return (v[a] + v[b]) % P
    if op == dc.SUB:
        return (v[a] - v[b]) % P
    if op == dc.NEG:
        return (-v[a]) % P
    if op == MUL:
        return v[a] * v[b] % P
    if op == dc.INV:
        return pow(v[a], P - 2, P)
    if op == dc.IS_ZERO:
        return int(v[a] == 0)
    if op == dc.LT:
        return int(v[a] < v[b])
    if op == BITS:
        return (v[a] >> (b & 255)) & ((1 << (b >> 8)) - 1)
    if op == dc.AND:
        return (v[a] & v[b]) % P
    if op == dc.XOR:
        return (v[a] ^ v[b]) % P
    raise AssertionError(f"op {op}")


def reference(program, rows):
    """The matrix the program makes of ``rows`` ((h, src_width) uint32, any words): a plain loop down the rows."""
    rows = np.asarray(rows, dtype=np.uint32)
    src_width, nodes, outputs, carries, reset_column, _ = parse(program)
    assert rows.ndim == 2 and rows.shape[1] == src_width
    h = rows.shape[0]
    out = np.zeros((h, max([src_width] + [d + 1 for _, d in outputs])), dtype=np.uint32)
    out[:, :src_width] = rows
    lists = rows.tolist()
    starts = set(group_starts(lists, reset_column))
    state, first = [], 0
    for r in range(h):
        if r in starts:
            state, first = [init for _, init in carries], r
        v = []
        for op, a, b in nodes:
            if op == CARRY:
                x = state[a]
            elif op == STEP:
                x = r - first
            elif op == IS_GROUP_FIRST:
                x = int(r == first)
            elif op == IS_GROUP_LAST:
                x = int(r == h - 1 or r + 1 in starts)
            else:
                x = _row_local(op, a, b, v, lists, r, h)
            v.append(x)
        state = [v[n] for n, _ in carries]
        for n, d in outputs:
            out[r, d] = v[n]
    return out


def with_resets(rows, column, starts, seed=0):
    """``rows`` with ``column`` made a reset column: firing words of every stored kind on ``starts``, words that do not
    fire (0, p, 2p) elsewhere.  Row 0 fires or not, as the seed has it: it starts a group either way."""
    rng = np.random.default_rng([seed, 0x17E7])
    rows = np.array(rows, dtype=np.uint32)
    quiet = np.array([0, P, 2 * P], dtype=np.uint64)
    loud = np.array([1, P + 1, 0xFFFFFFFF, P - 1, 2 * P + 1, 77], dtype=np.uint64)
    h = len(rows)
    rows[:, column] = quiet[rng.integers(0, 3, h)].astype(np.uint32)
    idx = [s for s in starts if s != 0 or rng.random() < 0.5]
    rows[idx, column] = loud[rng.integers(0, len(loud), len(idx))].astype(np.uint32)
    return rows


def starts_of_lengths(lengths):
    s, at = [], 0
    for n in lengths:
        s.append(at)
        at += int(n)
    return s, at


def padded(lengths):
    """the lengths with single-row groups behind them, up to the next power of two rows"""
    total = sum(int(n) for n in lengths)
    return [int(n) for n in lengths] + [1] * ((1 << (total - 1).bit_length()) - total)


def sponge_like(width, reset_column, max_group_rows=1 << 12, word=1, dst=None):
    """one carry: acc = state + word, state = acc^7, written to column dst (default: appended)"""
    dst = width if dst is None else dst
    nodes = [(CARRY, 0, 0), (COL, 0, word % width), (ADD, 0, 1), (MUL, 2, 2), (MUL, 3, 2), (MUL, 3, 3), (MUL, 5, 4)]
    return tape(width, nodes, [(6, dst)], [(6, 5)], reset_column, max_group_rows)


def fibonacci(width, reset_column, max_group_rows=1 << 12):
    """two carries swapped without a temporary: a, b <- b, a + b from (0, 1); a into column width, b behind it"""
    nodes = [(CARRY, 0, 0), (CARRY, 1, 0), (ADD, 0, 1)]
    return tape(width, nodes, [(0, width), (1, width + 1)], [(1, 0), (2, 1)], reset_column, max_group_rows)


def sixteen_carries(width, reset_column, max_group_rows=1 << 12):
    """16 carries rotated by one place, the first one fed by a column: every latch reads another carry's old value"""
    nodes = [(CARRY, k, 0) for k in range(16)] + [(COL, 0, 0), (ADD, 15, 16), (STEP, 0, 0), (ADD, 17, 18)]
    carries = [(19, 1)] + [(k - 1, k + 1) for k in range(1, 16)]
    outputs = [(k, width + k) for k in range(16)]
    return tape(width, nodes, outputs, carries, reset_column, max_group_rows)


def op_program(op):
    """width 3 (reset, x, y) -> 4: column 3 = op over the running sum of x and column y, for derive's ops; the group
    ops themselves for 40 to 43 (CARRY: the running sum before the row)"""
    nodes = [(CARRY, 0, 0), (COL, 0, 1), (ADD, 0, 1), (COL, 0, 2)]
    if op == CARRY:
        out = 0
    elif op in GROUP_OPS:
        nodes.append((op, 0, 0))
        out = 4
    elif op in LEAVES:
        nodes.append({CONST: (CONST, P - 1, 0), COL: (COL, 1, 1)}.get(op, (op, 0, 0)))
        out = 4
    elif op in UNARY:
        nodes.append((op, 2, 7 | 12 << 8 if op == BITS else 0))
        out = 4
    else:
        nodes.append((op, 2, 3))
        out = 4
    return tape(3, nodes, [(out, 3)], [(2, 3)], 0)


ALL_OPS = dc.ALL_OPS + GROUP_OPS


def random_program(seed, width, max_group_rows=1 << 12):
    """derive's random programs (4 to 60 nodes, every op, far and near operands, outputs that overwrite and append)
    with the four group ops among the leaves, 1 to 4 carries whose nodes are anywhere, and a reset column or none."""
    rng = np.random.default_rng([seed, width, 0x17E8])
    n = int(rng.integers(4, 61))
    n_carries = int(rng.integers(1, 5))
    nodes = []
    for i in range(n):
        leaf = i < 2 or rng.random() < 0.35
        op = int(rng.choice(LEAVES + GROUP_OPS + (CARRY,) if leaf else UNARY + BINARY))

        def pick():
            if rng.random() < 0.5:
                return int(rng.integers(0, i))
            return int(rng.integers(max(0, i - 3), i))
        if op == CONST:
            nodes.append((CONST, int(rng.choice([0, 1, 2, P - 1, int(rng.integers(0, P))])), 0))
        elif op == COL:
            nodes.append((COL, int(rng.integers(0, 3)), int(rng.integers(0, width))))
        elif op == CARRY:
            nodes.append((CARRY, int(rng.integers(0, n_carries)), 0))
        elif op in LEAVES or op in GROUP_OPS:
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
    carries = [(int(rng.integers(0, n)), int(rng.choice([0, 1, P - 1, int(rng.integers(0, P))])))
               for _ in range(n_carries)]
    reset = NO_RESET if rng.random() < 0.2 else int(rng.integers(0, width))
    return tape(width, nodes, outputs, carries, reset, max_group_rows)


def random_rows(seed, height, width, reset_column):
    """derive's random rows; the reset column, when there is one, starts a group on about one row in five"""
    rows = dc.random_rows(seed, height, width)
    if reset_column == NO_RESET:
        return rows
    rng = np.random.default_rng([seed, height, 0x17E9])
    return with_resets(rows, reset_column, [r for r in range(height) if rng.random() < 0.2], seed)


def carry_and_loads_program(k):
    """k loads, their sum, and one carry that holds the sum: k temporaries at once beside 1 carry slot"""
    nodes = [(COL, 0, c) for c in range(k)]
    acc = 0
    for c in range(1, k):
        nodes.append((ADD, acc, c))
        acc = len(nodes) - 1
    return tape(k, nodes, [(acc, k)], [(acc, 0)])
