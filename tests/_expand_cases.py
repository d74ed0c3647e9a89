"""The exact reference of ts_matrix_expand_rows and ts_expand_rows_host (include/tapstark.h "expanded rows") and the
seeded cases the CPU and GPU tests share: np.repeat plus index ramps, Python integers for the mod-p terms, written from
the header's text and independent of the library."""
import numpy as np

from tapstark_amd.expand import ALWAYS, FIRST, J, LAST, REMAINING, ROW, ExpandSpec, _term, col, const, stepped

P = 0x78000001
QUIET = [0, P, 2 * P]  # selector words that are zeros mod p
LOUD = [1, P + 1, 0xFFFFFFFF]  # selector words that are not
MAX_HEIGHT = 1 << 27


def counts(spec: ExpandSpec, src) -> np.ndarray:
    """What every source row asks for, as int64."""
    src = np.asarray(src, dtype=np.uint32)
    n = len(src)
    takes = src[:, spec.when[1]].astype(np.int64) % P != 0 if spec.when[0] else np.ones(n, dtype=bool)
    cnt = src[:, spec.count[1]].astype(np.int64) % P if spec.count[0] else np.full(n, spec.count[1], dtype=np.int64)
    return np.where(takes, cnt, 0)


def reference(spec: ExpandSpec, src, out_height: int = 0):
    """(matrix, n_live): the (row, inner index) pairs in lexicographic order, then the pad rows.  Raises ValueError
    with the library's text for a row over max_count (the least one) and for a total over the height, in that order."""
    src = np.asarray(src, dtype=np.uint32)
    assert src.ndim == 2 and src.shape[1] == spec.src_width
    cnt = counts(spec, src)
    over = np.flatnonzero(cnt > spec.max_count)
    if len(over):
        raise ValueError(f"expand: row {int(over[0])} asks for {int(cnt[over[0]])} rows, max_count {spec.max_count}")
    n_live = int(sum(int(c) for c in cnt))  # Python integers: exact
    limit = out_height or MAX_HEIGHT
    if n_live > limit:
        raise ValueError(f"expand: {n_live} rows asked for, out_height {limit}")
    height = out_height
    if not height:
        height = 1
        while height < n_live:
            height *= 2
    r = np.repeat(np.arange(len(src), dtype=np.int64), cnt)
    starts = np.cumsum(cnt) - cnt
    j = np.arange(n_live, dtype=np.int64) - np.repeat(starts, cnt)
    c = np.repeat(cnt, cnt)
    out = np.empty((height, spec.out_width), dtype=np.uint32)
    for k, t in enumerate(spec.terms):
        kind, value, step = _term(t)
        if kind == 0:
            column = np.full(n_live, value, dtype=np.int64)
        elif kind == 1:
            column = src[r, value].astype(np.int64)
        elif kind == 2:
            column = r
        elif kind == 3:
            column = j
        elif kind == 4:
            column = c - 1 - j
        elif kind == 5:
            column = (j == 0).astype(np.int64)
        elif kind == 6:
            column = (j == c - 1).astype(np.int64)
        else:
            words = src[r, value].tolist()
            column = np.array([(int(w) % P + int(jj) * step) % P for w, jj in zip(words, j.tolist())], dtype=np.int64)
        out[:n_live, k] = column.astype(np.uint32)
    out[n_live:] = np.array(spec.pad, dtype=np.uint32)
    return out, n_live


def random_rows(seed: int, height: int, width: int, max_count: int = 7, density: float = 0.6) -> np.ndarray:
    """Column 0 holds selector words (a share `density` of them loud, quiet and loud ones drawn from the edge words),
    column 1 -- where the width has one -- count words: 0 .. max_count, a third of them with p added (the reduced value
    decides).  The other columns hold uniform 32-bit words, at and above p too: a copied word is kept as stored."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 1 << 32, size=(height, width), dtype=np.uint64).astype(np.uint32)
    loud = rng.random(height) < density
    pick = rng.integers(0, 3, size=height)
    rows[:, 0] = np.where(loud, np.array(LOUD, dtype=np.uint32)[pick], np.array(QUIET, dtype=np.uint32)[pick])
    if width > 1:
        cnt = rng.integers(0, max_count + 1, size=height, dtype=np.uint64)
        rows[:, 1] = (cnt + np.where(rng.integers(0, 3, size=height) == 0, P, 0)).astype(np.uint32)
    return rows


def random_spec(seed: int, src_width: int, out_width: int, max_count: int = 7, kinds=None) -> ExpandSpec:
    """A seeded spec over rows of random_rows: `when` on column 0 (or every row), the count in column 1 (a constant for
    a source of one column), every term kind -- `kinds` where given -- and a random pad row."""
    rng = np.random.default_rng(7000 + seed)
    when = ALWAYS if rng.integers(0, 4) == 0 else col(0)
    count = col(1) if src_width > 1 else int(rng.integers(1, max_count + 1))
    terms = []
    for c in range(out_width):
        k = int(kinds[c % len(kinds)]) if kinds is not None else int((seed + c) % 8 if c < 8 else rng.integers(0, 8))
        w = int(rng.integers(0, src_width))
        terms.append([const(int(rng.choice([0, 1, P - 1, int(rng.integers(0, P))]))), col(w), ROW, J, REMAINING, FIRST,
                      LAST, stepped(w, int(rng.choice([0, 1, P - 1, int(rng.integers(0, P))])))][k])
    return ExpandSpec(src_width, out_width, count=count, when=when, max_count=max_count,
                      pad=[int(v) for v in rng.integers(0, P, size=out_width)], terms=terms)
