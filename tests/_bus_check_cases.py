"""The model of ``ts_bus_check`` for tests/test_bus_check_cpu.py and tests/test_gpu_bus_check.py: Python integers and a
dictionary, straight from the definitions in include/tapstark.h, and the small statements both files share.

A table is ``(LogUp or None, trace array or None, preprocessed array or None)``.  ``model(tables)`` returns what
``BusReport.asdict()`` must equal, field by field, shares included."""
import numpy as np

import tapstark_amd as ts

P = 0x78000001
TAG = 7  # the bus tag of the hand-made statements (BUS_TAG of tapstark_amd.airs)


def _term(term, row, pre_row):
    kind, value = term
    if kind == 0:
        return int(value)
    return int(row[value]) if kind == 1 else int(pre_row[value])


def contributions(tables):
    """Every (table, row, interaction, canonical multiplicity != 0, zero-padded tuple), in (table, row, interaction)
    order.  The tuple's words are taken as stored; only the multiplicity is reduced."""
    out = []
    for k, (logup, trace, pre) in enumerate(tables):
        if logup is None:
            continue
        for r in range(trace.shape[0]):
            row, pre_row = trace[r], (pre[r] if pre is not None else None)
            for i, (m, vals) in enumerate(logup.interactions):
                mult = _term(m, row, pre_row) % P
                if mult:
                    tup = tuple(_term(v, row, pre_row) for v in vals)
                    out.append((k, r, i, mult, tup + (0,) * (8 - len(tup)), len(vals)))
    return out


def model(tables):
    cs = contributions(tables)
    classes = {}
    for k, r, i, mult, tup, nv in cs:
        classes.setdefault(tup, []).append((k, r, i, mult, nv))
    bad = {tup: members for tup, members in classes.items() if sum(m[3] for m in members) % P}
    T = len(tables)
    rep = {"n_contributions": len(cs), "n_tuples": len(classes), "n_unbalanced": len(bad), "first": None, "n_values": 0,
           "tuple": [0] * 8, "sum": 0, "shares": [(0, 0, None)] * T}
    if bad:
        # the least contribution over all contributions to unbalanced tuples: each class's list is in order already
        tup, members = min(bad.items(), key=lambda kv: kv[1][0][:3])
        k, r, i, _, nv = members[0]
        rep.update(first=(k, r, i), n_values=nv, tuple=list(tup), sum=sum(m[3] for m in members) % P)
        shares = []
        for t in range(T):
            mine = [m for m in members if m[0] == t]
            shares.append((len(mine), sum(m[3] for m in mine) % P, (mine[0][1], mine[0][2]) if mine else None))
        rep["shares"] = shares
    return rep


def lg(*interactions):
    """A LogUp from ``(multiplicity term, [value terms])`` pairs."""
    return ts.LogUp(list(interactions))


def u32(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32))


def from_cases(tables):
    """The tables of tests/_bus_cases.py or tests/_key_cases.py as model tables."""
    return [(t.logup, t.trace, getattr(t, "key", None) if t.logup is not None else None) for t in tables]


# ---- hand-made statements; columns are named in the comments, every trace is (height, width) uint32
def padding(third):
    """Table 0 sends (TAG, a) on two rows; table 1 receives (TAG, a, third) with the negated count.  third = 0: the
    same tuple, balanced; third = 1: two tuples, both unbalanced."""
    send = u32([[5, 1], [5, 1]])                      # value, multiplicity
    recv = u32([[5, third, P - 2], [3, third, 0]])    # value, third, -count
    return [(lg((("col", 1), [("const", TAG), ("col", 0)])), send, None),
            (lg((("col", 2), [("const", TAG), ("col", 0), ("col", 1)])), recv, None)]


def past_p(rows):
    """`rows` rows of multiplicity p - 1 on one tuple against one row of multiplicity 2^12: balanced exactly at
    rows = 2^12, since 2^12 (p - 1) + 2^12 = 2^12 p.  The integer sum is far past 2^32.  (A resident matrix has a
    power-of-two height: the table is filled up with rows of multiplicity 0, which are no contributions.)"""
    height = 1 << max(rows - 1, 0).bit_length()
    send = u32([[33, P - 1]] * rows + [[33, 0]] * (height - rows))
    recv = u32([[33, 1 << 12]])
    spec = lg((("col", 1), [("const", TAG), ("col", 0)]))
    return [(spec, send, None), (spec, recv, None)]


def two_bad(where):
    """Two unbalanced tuples.  where = "second table": table 0 balances and both live in table 1, the higher row first
    in discovery-friendly order; where = "late interaction": the least contribution is interaction 2 of row 1 of table
    0 while another unbalanced tuple sits in interaction 0 of row 2."""
    spec3 = lg((("col", 3), [("const", TAG), ("col", 0)]), (("col", 4), [("const", TAG), ("col", 1)]),
               (("col", 5), [("const", TAG), ("col", 2)]))
    if where == "second table":
        t0 = u32([[1, 2, 3, 1, 1, 1], [1, 2, 3, P - 1, P - 1, P - 1]])      # cancels inside the table
        t1 = u32([[1, 2, 3, 0, 0, 0], [1, 2, 3, 0, 0, 0], [70, 2, 80, 0, 0, 5], [70, 2, 3, 4, 0, 0]])
        return [(spec3, t0, None), (spec3, t1, None)]
    t0 = u32([[1, 2, 3, 0, 0, 0], [1, 2, 90, 0, 0, 6], [91, 2, 3, 7, 0, 0], [1, 2, 3, 0, 0, 0]])
    t1 = u32([[91, 0, 0, 1, 0, 0]])
    return [(spec3, t0, None), (spec3, t1, None)]


def non_canonical():
    """Multiplicity words 0 and p are no contribution; p + 1 counts as 1 and p + 2 as 2."""
    send = u32([[4, 0], [4, P], [4, P + 1], [4, P + 2], [6, P], [6, 0], [6, P], [6, 0]])
    recv = u32([[4, P - 3]])
    spec = lg((("col", 1), [("const", TAG), ("col", 0)]))
    return [(spec, send, None), (spec, recv, None)]


def cancels_inside():
    """One table whose two interactions send and take the same tuple on different rows."""
    t = u32([[8, 8, 2, 0], [8, 8, 0, P - 2], [9, 9, 1, P - 1], [1, 1, 0, 0]])
    return [(lg((("col", 2), [("col", 0)]), (("col", 3), [("col", 1), ("const", 0)])), t, None)]
