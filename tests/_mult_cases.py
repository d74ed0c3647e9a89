"""The meaning of ts_logup_multiplicities (include/tapstark.h) stated over Python integers, and the inputs the
tests of it share.  `reference` is the yardstick of every comparison in tests/test_logup_mult_cpu.py and
tests/test_gpu_logup_mult.py: nothing there is compared against the code under test.

A term is (kind, value) with kind 0 | "const" a canonical constant, 1 | "col" a main column, 2 | "prep" a column
of the preprocessed matrix, all on the local row."""
import numpy as np

P = 0x78000001
NONE = 2 ** 64 - 1  # first_missing when nothing is missing
KINDS = {"const": 0, "col": 1, "prep": 2}


def _value(term, row, prow):
    kind, v = term
    kind = KINDS.get(kind, kind)
    return int(v) if kind == 0 else int(row[v]) if kind == 1 else int(prow[v])


def reference(trace, table, lookups, weights, out_column, negate=1, preprocessed=None):
    """(the trace after the call, n_missing, first_missing).  Table rows with equal tuples form a class whose
    representative is its lowest row; every lookup of non-zero weight adds its weight to the representative of its
    tuple's class or, if no table row holds the tuple, is a miss; the column ends as the sums mod p (p minus them
    with `negate`) on representatives and 0 elsewhere."""
    rows = np.asarray(trace).tolist()
    prows = np.asarray(preprocessed).tolist() if preprocessed is not None else [None] * len(rows)
    lowest = {}
    for t, (row, prow) in enumerate(zip(rows, prows)):
        lowest.setdefault(tuple(_value(term, row, prow) for term in table), t)
    sums = [0] * len(rows)
    n_missing, first = 0, NONE
    for r, (row, prow) in enumerate(zip(rows, prows)):
        for l, (tup, weight) in enumerate(zip(lookups, weights)):
            w = _value(weight, row, prow) % P
            if w == 0:
                continue
            rep = lowest.get(tuple(_value(term, row, prow) for term in tup))
            if rep is None:
                n_missing += 1
                first = min(first, r * len(lookups) + l)
            else:
                sums[rep] += w
    out = np.array(trace, dtype=np.uint32, copy=True)
    for t, s in enumerate(sums):
        out[t, out_column] = (P - s % P) % P if negate else s % P
    return out, n_missing, first


# ---- inputs
JUNK = 0xFFFFFFF0  # what the out column holds before the call: above p, so a row the call skipped shows


def range_case(n, values=None, seed=1):
    """The range table 0 .. n-1 in main column 1, one lookup of weight 1 of column 0, the result in column 2."""
    if values is None:
        values = np.random.default_rng(seed).integers(0, n, size=n)
    trace = np.empty((n, 3), dtype=np.uint32)
    trace[:, 0] = values
    trace[:, 1] = np.arange(n)
    trace[:, 2] = JUNK
    return trace, None, dict(table=[("col", 1)], lookups=[[("col", 0)]], weights=[("const", 1)], out_column=2, negate=1)


def tuple_case(n, nv, L, seed, in_prep=False, const_at=None, weights="one", negate=1, alphabet=None):
    """A table of `nv`-tuples (main columns, or columns of the preprocessed matrix with `in_prep`) and `L` lookups
    per row, each the tuple of a random table row.  `const_at`: that position is one constant on both sides.  With
    `in_prep` the first term of every lookup reads a preprocessed column too.  `weights`: "one" | "pm1" (constants 1,
    p - 1) | "selector" (a 0/1 column) | "field" (a column of arbitrary field elements that holds 0 and p - 1).
    Small `alphabet`s give tables with equal rows."""
    rng = np.random.default_rng(seed)
    alphabet = alphabet or P
    tab = rng.integers(0, alphabet, size=(n, nv), dtype=np.int64)
    const = 7
    if const_at is not None:
        tab[:, const_at] = const
    pick = rng.integers(0, n, size=(n, L))
    n_main = (0 if in_prep else nv) + L * nv + L + 1
    trace = np.zeros((n, n_main), dtype=np.uint32)
    prep = np.zeros((n, nv + L), dtype=np.uint32) if in_prep else None
    col = 0
    if in_prep:
        prep[:, :nv] = tab
        table = [("prep", q) for q in range(nv)]
    else:
        trace[:, :nv] = tab
        table = [("col", q) for q in range(nv)]
        col = nv
    if const_at is not None:
        table[const_at] = ("const", const)
    lookups, wts = [], []
    for l in range(L):
        looked = tab[pick[:, l]]
        tup = []
        for q in range(nv):
            if q == const_at:
                tup.append(("const", const))
            elif in_prep and q == 0:
                prep[:, nv + l] = looked[:, q]
                tup.append(("prep", nv + l))
            else:
                trace[:, col] = looked[:, q]
                tup.append(("col", col))
            col += 1
        lookups.append(tup)
    for l in range(L):
        if weights == "one":
            wts.append(("const", 1))
        elif weights == "pm1":
            wts.append(("const", P - 1))
        else:
            w = rng.integers(0, 2, size=n) if weights == "selector" else rng.integers(0, P, size=n)
            if weights == "field" and n >= 2:
                w[rng.integers(0, n)] = 0
                w[(int(np.flatnonzero(w == 0)[0]) + 1) % n] = P - 1
            trace[:, col] = w
            wts.append(("col", col))
        col += 1
    trace[:, col] = JUNK
    return trace, prep, dict(table=table, lookups=lookups, weights=wts, out_column=col, negate=negate)


def duplicates_case(n, seed=4):
    """Every table entry occurs four times at scattered rows (n a multiple of 4); one lookup of weight 1."""
    rng = np.random.default_rng(seed)
    trace, prep, spec = range_case(n, values=rng.integers(0, n // 4, size=n))
    trace[:, 1] = rng.permutation(np.repeat(np.arange(n // 4), 4))
    return trace, prep, spec


def all_equal_table_case(n, seed=5):
    """A table whose rows are all equal; half of the lookups hit it, the others have weight 0 and another value."""
    trace = np.empty((n, 4), dtype=np.uint32)
    sel = np.random.default_rng(seed).integers(0, 2, size=n)
    trace[:, 0] = np.where(sel == 1, 9, 3)
    trace[:, 1] = 9
    trace[:, 2] = sel
    trace[:, 3] = JUNK
    return trace, None, dict(table=[("col", 1)], lookups=[[("col", 0)]], weights=[("col", 2)], out_column=3, negate=1)


def one_destination_case(n=1 << 12, L=16):
    """Every lookup the same tuple, every weight p - 1: the sum n L (p - 1) is above 2^32."""
    trace = np.empty((n, 2), dtype=np.uint32)
    trace[:, 0] = np.arange(n)
    trace[:, 1] = JUNK
    return trace, None, dict(table=[("col", 0)], lookups=[[("const", 5)]] * L, weights=[("const", P - 1)] * L,
                             out_column=1, negate=0)
