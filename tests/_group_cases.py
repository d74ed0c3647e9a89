"""What the TGRP tape of ts_matrix_collect_rows computes (include/tapstark.h "grouped rows"), in plain Python: a dict
from the key tuple, as stored, to the group's record over Python integers, then one output row per record in order of
first appearance.  And the seeded cases the CPU and the GPU tests share.  Nothing here calls the library."""
import numpy as np

from tapstark_amd.collect import ALWAYS, col, const
from tapstark_amd.group import (COUNT, FIRST_ROW, INDEX, LAST_ROW, GroupSpec, _key, _selector, _term, first, greatest,
                                last, least, total)

P = 0x78000001
EDGE_WORDS = [0, 1, P - 1, P, P + 1, 2 * P, 0xFFFFFFFF]  # as keys seven classes; as selectors 0, p and 2p do not fire


def reference(spec: GroupSpec, src, out_height: int = 0):
    """(matrix, n_groups).  Raises ValueError when there are more groups than out_height takes."""
    src = np.asarray(src, dtype=np.uint32)
    assert src.shape[1] == spec.src_width
    sel_kind, sel_value = _selector(spec.when)
    keys = [_key(k) for k in spec.keys]
    terms = [_term(t) for t in spec.terms]
    aggregates = sorted({t for t in terms if t[0] in (6, 7, 8)})
    groups = {}  # insertion order is first appearance
    for r, row in enumerate(src.tolist()):
        if sel_kind == 1 and row[sel_value] % P == 0:
            continue
        key = tuple(row[v] if k else v for k, v in keys)
        g = groups.get(key)
        if g is None:
            g = groups[key] = {"f": r, "n": 0, "sum": {}, "min": {}, "max": {}}
        g["l"] = r
        g["n"] += 1
        for kind, v in aggregates:  # (a column two terms name is taken once)
            w = row[v] % P
            if kind == 6:
                g["sum"][v] = g["sum"].get(v, 0) + w
            elif kind == 7:
                g["min"][v] = min(g["min"].get(v, w), w)
            else:
                g["max"][v] = max(g["max"].get(v, w), w)
    rows_out = []
    for index, g in enumerate(groups.values()):
        f, l = src[g["f"]].tolist(), src[g["l"]].tolist()
        word = {0: lambda v: v, 1: lambda v: f[v], 2: lambda v: l[v], 3: lambda v: g["f"], 4: lambda v: g["l"],
                5: lambda v: g["n"], 6: lambda v: g["sum"][v] % P, 7: lambda v: g["min"][v], 8: lambda v: g["max"][v],
                9: lambda v: index}
        rows_out.append([word[kind](v) for kind, v in terms])
    n_live = len(rows_out)
    if out_height == 0:
        height = 1
        while height < n_live:
            height *= 2
    else:
        height = out_height
    if n_live > height:
        raise ValueError(f"group: {n_live} groups, out_height {out_height}")
    rows_out += [list(spec.pad)] * (height - n_live)
    return np.array(rows_out, dtype=np.uint32).reshape(height, spec.out_width), n_live


def group_index_of_rows(spec: GroupSpec, src):
    """Per source row the index of its group, -1 for a row that takes no part."""
    src = np.asarray(src, dtype=np.uint32)
    sel_kind, sel_value = _selector(spec.when)
    keys = [_key(k) for k in spec.keys]
    groups, out = {}, []
    for row in src.tolist():
        if sel_kind == 1 and row[sel_value] % P == 0:
            out.append(-1)
            continue
        out.append(groups.setdefault(tuple(row[v] if k else v for k, v in keys), len(groups)))
    return out


def random_rows(seed: int, height: int, width: int, n_values: int = 12) -> np.ndarray:
    """Every column draws from the edge words and a few random ones, so that key tuples repeat, `p + 1` and `1` both
    occur, selectors fire on some rows only and sums wrap; columns from 3 on of wide matrices hold plain random words."""
    rng = np.random.default_rng(seed)
    values = np.array(EDGE_WORDS + [int(v) for v in rng.integers(0, 1 << 32, size=max(1, n_values - len(EDGE_WORDS)))],
                      dtype=np.uint32)
    rows = values[rng.integers(0, len(values), size=(height, width))]
    if width > 4:
        rows[:, 4:] = rng.integers(0, 1 << 32, size=(height, width - 4), dtype=np.uint64).astype(np.uint32)
    return rows


def every_term(width: int, rng) -> list:
    c = lambda: int(rng.integers(0, width))  # noqa: E731
    return [const(int(rng.integers(0, P))), first(c()), last(c()), FIRST_ROW, LAST_ROW, COUNT, total(c()), least(c()),
            greatest(c()), INDEX, P - 1, col(c())]


def random_spec(seed: int, width: int, n_keys: int = 1, when="column") -> GroupSpec:
    """Keys on the first columns (one of them a constant where there are three or more), every term kind once and a
    bare integer and a bare column beside them, a random pad row."""
    rng = np.random.default_rng(7000 + seed)
    keys = [col(int(q % width)) for q in range(n_keys)]
    if n_keys >= 3:
        keys[1] = const(int(rng.integers(0, P)))
    terms = every_term(width, rng)
    sel = ALWAYS if when == "always" else col(int(rng.integers(0, min(width, 4))))
    return GroupSpec(width, len(terms), keys, when=sel, pad=[int(v) for v in rng.integers(0, P, size=len(terms))],
                     terms=terms)


def grid(heights, widths=(1, 5, 17)):
    k = 0
    for h in heights:
        for w in widths:
            for n_keys in (1, 3, 8):
                yield (f"h{h}-w{w}-keys{n_keys}", random_spec(k, w, n_keys, when="always" if k % 4 == 0 else "column"),
                       random_rows(100 + k, h, w, n_values=8 + k % 9))
                k += 1
