"""What ts_matrix_join_rows computes (include/tapstark.h "joined rows"), in plain Python: a dict from the table's key
tuple to the lowest row that carries it, then a loop over the source's rows.  And the seeded cases the CPU and the GPU
tests share.  Nothing here calls the library."""
import numpy as np

from tapstark_amd.join import HIT, KEEP, TABLE_ROW, JoinSpec, col

P = 0x78000001
ODD_WORDS = [0, 1, P, 2 * P, P + 1, 0xFFFFFFFF, P - 1, 5]  # zeros mod p, ones mod p, the largest word


def out_width(spec: JoinSpec, src_width: int) -> int:
    base = max([src_width] + [d + 1 for _, d, _ in spec.fetch])
    return base + bool(spec.flags & TABLE_ROW) + bool(spec.flags & HIT)


def _word(term, row):
    kind, value = term
    return int(row[value]) if kind else value


def reference(spec: JoinSpec, src, table):
    """(the result, n_missing, first_missing or None) for host matrices."""
    src, table = np.asarray(src, dtype=np.uint32), np.asarray(table, dtype=np.uint32)
    n_table = spec.table_rows or table.shape[0]
    lowest = {}
    for t in range(n_table):
        lowest.setdefault(tuple(_word(term, table[t]) for _, term in spec.keys), t)  # matched as stored
    sw = src.shape[1]
    base = max([sw] + [d + 1 for _, d, _ in spec.fetch])
    w = out_width(spec, sw)
    out = np.zeros((src.shape[0], w), dtype=np.uint32)
    out[:, :sw] = src
    n_missing, first = 0, None
    for r in range(src.shape[0]):
        match = None
        if _word(spec.when, src[r]) % P != 0:  # reduced: 0, p and 2p do not fire
            match = lowest.get(tuple(_word(term, src[r]) for term, _ in spec.keys))
            if match is None:
                n_missing += 1
                first = r if first is None else first
        for tc, dc, default in spec.fetch:
            if match is not None:
                out[r, dc] = table[match, tc]
            elif not (spec.flags & KEEP and dc < sw):
                out[r, dc] = default
        at = base
        if spec.flags & TABLE_ROW:
            out[r, at] = 0 if match is None else match
            at += 1
        if spec.flags & HIT:
            out[r, at] = 0 if match is None else 1
    return out, n_missing, first


def case(seed, src_h, table_h, n_keys, n_fetch, flags=0, place="inside", consts=True, pad_row=False, hit=0.7,
         extra=0, entered=None):
    """(spec, src, table): table tuples drawn from few values, the odd words among them, so that classes have several
    rows; source keys copied from table rows with probability ``hit``, random otherwise; a `when` column of odd words.
    ``place``: the dst columns lie "inside" the source beside the keys, are "appended" behind it, or ("overkey") the
    first of them is key column 0.  ``consts``: with two keys or more, key 1 is a constant on the source's side; with
    three or more, key 2 is a constant on the table's side.  ``pad_row``: table_rows = table_h - 1 and the last table
    row carries a tuple of its own that some source rows ask for.  ``extra``: more copied source columns.  ``entered``:
    table_rows, where it is given; the rows behind it hold tuples like the others, which would otherwise match."""
    rng = np.random.default_rng(seed * 7919 + src_h * 31 + table_h * 17 + n_keys * 5 + n_fetch)
    if n_fetch == 0 and not flags & (TABLE_ROW | HIT):
        flags |= HIT
    tw = n_keys + 3
    values = np.array(ODD_WORDS + [7, 1 << 20], dtype=np.uint32)
    table = rng.integers(0, 1 << 32, size=(table_h, tw), dtype=np.uint32)
    few = max(2, int(table_h ** (0.7 / n_keys)) + 1)
    table[:, :n_keys] = values[rng.integers(0, min(few, len(values)), size=(table_h, n_keys))]
    c_src, c_tab = 1 << 20, 7  # the constants: words the key columns draw too
    skeys = [col(q) for q in range(n_keys)]
    tkeys = [col(q) for q in range(n_keys)]
    if consts and n_keys >= 2:
        skeys[1] = c_src
        table[rng.random(table_h) < 0.8, 1] = c_src
    if consts and n_keys >= 3:
        tkeys[2] = c_tab
    n_live = table_h
    if entered is not None:
        pad_row = False
    if pad_row and table_h > 1:
        n_live = table_h - 1
        table[-1, 0] = 0x12345  # in no other row
    inside = n_fetch if place in ("inside", "overkey") else 0
    sw = n_keys + 1 + inside + extra
    src = rng.integers(0, 1 << 32, size=(src_h, sw), dtype=np.uint32)
    pick = rng.integers(0, table_h, size=src_h)
    src[:, :n_keys] = table[pick, :n_keys]
    stray = rng.random(src_h) >= hit
    src[stray, 0] = rng.integers(100, 200, size=int(stray.sum()), dtype=np.uint32)  # in no table row
    if consts and n_keys >= 3:
        src[:, 2] = np.where(rng.random(src_h) < 0.8, c_tab, src[:, 2])
    src[:, n_keys] = values[rng.integers(0, len(ODD_WORDS), size=src_h)]  # the `when` column
    if place == "inside":
        dst = [n_keys + 1 + f for f in range(n_fetch)]
    elif place == "overkey":
        dst = [0] + [n_keys + 1 + f for f in range(1, n_fetch)]
    else:
        dst = [sw + f for f in range(n_fetch)]
    order = rng.permutation(n_fetch)  # the spec's order is not the column order
    fetch = [(int(rng.integers(0, tw)), dst[f], int(rng.integers(0, P))) for f in order]
    spec = JoinSpec(keys=list(zip(skeys, tkeys)), when=col(n_keys), fetch=fetch, flags=flags,
                    table_rows=entered if entered is not None else n_live if pad_row else 0)
    return spec, src, table


PLACES = ["inside", "appended", "overkey"]


def grid(src_heights=(1, 3, 1000), table_heights=(1, 5, 257)):
    """The cases of the grid: every (source height, table height, n_keys, n_fetch); the eight flag combinations, the
    three placements, the constant key terms and the short table cycle through them.  A table height may be a pair
    (height, entered rows): a resident matrix has a power of two of rows, and table_rows says how many are the table."""
    k = 0
    for src_h in src_heights:
        for table_h in table_heights:
            table_h, entered = table_h if isinstance(table_h, tuple) else (table_h, None)
            for n_keys in (1, 3, 8):
                for n_fetch in (0, 1, 32):
                    yield (f"src{src_h}-table{entered or table_h}-keys{n_keys}-fetch{n_fetch}-flags{k % 8}-{PLACES[k % 3]}",
                           case(k, src_h, table_h, n_keys, n_fetch, flags=k % 8, place=PLACES[k % 3],
                                consts=k % 2 == 0, pad_row=k % 5 == 0, entered=entered))
                    k += 1


def chase(seed, n):
    """src is table: column 0 is a row's own key, column 1 the key of another row or of none; the join fetches that
    row's column 2 into column 3."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint32)
    m[:, 0] = rng.permutation(n) + 1000
    m[:, 1] = m[rng.integers(0, n, size=n), 0]
    m[rng.random(n) < 0.2, 1] = 5  # no row's key
    return JoinSpec(keys=[(col(1), col(0))], fetch=[(2, 3, 9)], flags=HIT), m
