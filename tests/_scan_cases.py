"""The exact reference of ts_matrix_scan and ts_scan_rows_host (include/tapstark.h "scanned columns") and the seeded
cases the CPU and GPU tests share: a sequential loop over the rows in Python integers mod p, written from the header's
text and independent of the library."""
import numpy as np

from tapstark_amd.scan import NO_RESET, ScanSpec, col

P = 0x78000001
EDGE = [0, 1, P - 1, P, P + 1, 1 << 31, 0xFFFFFFFF]  # stored words: canonical, p itself, above p, above 2^31


def reference(spec: ScanSpec, rows, finals: bool = False):
    """out[i][dst] = y[i] (or the state before row i for an exclusive scan), every other kept column as stored."""
    rows = np.asarray(rows, dtype=np.uint32)
    h, w = rows.shape
    width = spec.out_width or max([w] + [c["dst"] + 1 for c in spec.columns])
    out = np.zeros((h, width), dtype=np.uint32)
    keep = min(w, width)
    out[:, :keep] = rows[:, :keep]
    src = rows.tolist()
    last = []
    for c in spec.columns:
        y = c["init"]
        column = []
        for r in src:
            a = (r[c["a"][1]] if c["a"][0] else c["a"][1]) % P
            b = (r[c["b"][1]] if c["b"][0] else c["b"][1]) % P
            if c["reset"] != NO_RESET and r[c["reset"]] % P != 0:
                y = c["init"]
            before = y
            y = (a * y + b) % P
            column.append(before if c["flags"] & 1 else y)
        out[:, c["dst"]] = column
        last.append(y)
    return (out, np.array(last, dtype=np.uint32)) if finals else out


def random_rows(seed: int, height: int, width: int) -> np.ndarray:
    """Uniform words below p with edge words, zeros and ones planted: a zero stops a product, a one in a reset column
    starts a group, and a word at or above p must be reduced where it is read and kept where it is copied."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, P, size=(height, width), dtype=np.uint32)
    kind = rng.integers(0, 8, size=(height, width))
    rows[kind == 0] = 0
    rows[kind == 1] = 1
    edge = np.array(EDGE, dtype=np.uint32)
    pick = kind == 2
    rows[pick] = edge[rng.integers(0, len(edge), size=int(pick.sum()))]
    return rows


def random_spec(seed: int, width: int, n_scans: int | None = None) -> ScanSpec:
    """1 to 8 scans over a source of `width` columns: every term kind and flag, resets or none, dsts that overwrite and
    dsts that are appended (contiguously, as the rules ask), sometimes a truncated result."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 9)) if n_scans is None else n_scans
    inits = [0, 1, P - 1, int(rng.integers(0, P))]
    # distinct dsts: some inside the source, the rest appended right behind it
    inside = [int(c) for c in rng.permutation(width)[:int(rng.integers(0, min(width, n) + 1))]]
    dsts = inside + [width + k for k in range(n - len(inside))]
    rng.shuffle(dsts)
    spec = ScanSpec()
    for k in range(n):
        def term():
            return col(int(rng.integers(0, width))) if rng.integers(0, 3) else int(rng.choice([0, 1, P - 1, int(rng.integers(0, P))]))
        spec.add(dsts[k], a=term(), b=term(), init=inits[int(rng.integers(0, 4))],
                 reset=int(rng.integers(0, width)) if rng.integers(0, 2) else None, exclusive=bool(rng.integers(0, 2)))
    full = max(width, max(dsts) + 1)
    if max(dsts) + 1 < full and rng.integers(0, 2):
        spec.out_width = int(rng.integers(max(dsts) + 1, full + 1))
    return spec
