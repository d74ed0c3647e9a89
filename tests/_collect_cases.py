"""The exact reference of ts_matrix_collect_rows and ts_collect_rows_host (include/tapstark.h "collected rows") and the
seeded cases the CPU and GPU tests share: nested loops over (source, row, emitter) in Python integers, written from
the header's text and independent of the library."""
import numpy as np

from tapstark_amd.collect import ALWAYS, ROW, CollectSpec, col, const

P = 0x78000001
SELECTOR_WORDS = [0, 1, P, P + 1, 2 * P, 0xFFFFFFFF]  # p and 2p are zeros and do not fire; p + 1 and 0xFFFFFFFF fire


def reference(spec: CollectSpec, sources, out_height: int = 0):
    """(matrix, n_live): the fired (source, row, emitter) triples in lexicographic order, then the pad rows.  Raises
    ValueError when more rows fire than out_height takes."""
    rows_out = []
    for s, src in enumerate(sources):
        src = np.asarray(src, dtype=np.uint32)
        assert src.shape[1] == spec.src_widths[s]
        for r, row in enumerate(src.tolist()):
            for source, (sel_kind, sel_value), terms in spec.emitters:
                if source != s:
                    continue
                if sel_kind == 1 and row[sel_value] % P == 0:
                    continue
                rows_out.append([value if kind == 0 else row[value] if kind == 1 else r for kind, value in terms])
    n_live = len(rows_out)
    if out_height == 0:
        height = 1
        while height < n_live:
            height *= 2
    else:
        height = out_height
    if n_live > height:
        raise ValueError(f"collect: {n_live} rows selected, out_height {out_height}")
    rows_out += [list(spec.pad)] * (height - n_live)
    return np.array(rows_out, dtype=np.uint32).reshape(height, spec.out_width), n_live


def random_rows(seed: int, height: int, width: int, density: float = 0.5) -> np.ndarray:
    """Uniform 32-bit words (at and above p too: a copied word is kept as stored); a share `density` of every column's
    words fires when read as a selector, and both the firing and the silent words are drawn from the edge words 0, 1,
    p, p + 1, 0xFFFFFFFF and a random word, so that the mod-p rule decides."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 1 << 32, size=(height, width), dtype=np.uint64).astype(np.uint32)
    fires = rng.random(size=(height, width)) < density
    silent = np.array([0, P, 0, 2 * P], dtype=np.uint32)  # (2p is below 2^32 and a zero too)
    loud = np.array([1, P + 1, 0xFFFFFFFF, 0], dtype=np.uint32)  # the last one is replaced by a random word
    pick = rng.integers(0, 4, size=(height, width))
    word = np.where(fires, loud[pick], silent[pick])
    some = rng.integers(1, P, size=(height, width), dtype=np.uint32)  # canonical and not zero: fires
    word = np.where(fires & (pick == 3), some, word).astype(np.uint32)
    # half of the columns keep plain random words (data); their words fire nearly always
    data = rng.random(size=width) < 0.5
    data[0] = False  # (a selector column for every width)
    return np.where(data[None, :], rows, word).astype(np.uint32)


def selector_columns(rows: np.ndarray) -> list:
    """The columns random_rows filled with selector words (every word of them is an edge word or below p)."""
    edge = np.isin(rows, np.array(SELECTOR_WORDS, dtype=np.uint32)) | (rows < P)
    return [c for c in range(rows.shape[1]) if edge[:, c].all()]


def random_spec(seed: int, src_widths, n_emitters: int, out_width: int, sel_columns=None) -> CollectSpec:
    """`n_emitters` emitters spread over the sources in a seeded order (so the emitters of one source are interleaved
    with the others'), every selector and term kind, a random pad row.  sel_columns[s], where given, lists the columns
    of source s a selector may name."""
    rng = np.random.default_rng(5000 + seed)
    spec = CollectSpec(src_widths, out_width, pad=[int(v) for v in rng.integers(0, P, size=out_width)])
    for e in range(n_emitters):
        s = int(rng.integers(0, len(src_widths)))
        w = src_widths[s]
        cols = list(range(w)) if sel_columns is None else sel_columns[s]
        when = ALWAYS if rng.integers(0, 4) == 0 else col(int(cols[int(rng.integers(0, len(cols)))]))
        terms = []
        for c in range(out_width):
            k = int(rng.integers(0, 4))
            terms.append(ROW if k == 0 else const(int(rng.choice([0, 1, P - 1, int(rng.integers(0, P))]))) if k == 1
                         else col(int(rng.integers(0, w))))
        spec.emit(s, when=when, terms=terms)
    return spec
