"""Cases and the reference of ts_matrix_sort_rows / ts_matrix_gather_rows (tests/test_sort_cpu.py checks the reference
against plain Python ``sorted``; tests/test_gpu_sort.py compares the device with it word for word).

The order is ``np.lexsort`` over the key columns reversed (its LAST key is the primary one), which is stable, over
uint32 words: integers throughout, so the reference is exact for every case.  The two optional columns and the tail
[n_live, height) are numpy too.

Heights: no call makes a matrix whose height is no power of two (ts_matrix_upload and ts_matrix_from_device refuse
it), so a sorted length L that is none is reached as n_live = L inside the next power of two, with tail rows that
would sort first: the sort kernels see exactly L rows either way, the gather sees the tail as well."""
import numpy as np

P = 2013265921  # BabyBear


def pow2_at_least(n: int) -> int:
    h = 1
    while h < n:
        h <<= 1
    return h


def reference(src, keys, group_keys=0, n_live=None, source_row=False, group_start=False):
    """What ts_matrix_sort_rows returns for the host matrix ``src`` (uint32, 2-d)."""
    src = np.ascontiguousarray(src, dtype=np.uint32)
    h = src.shape[0]
    n = h if n_live is None else n_live
    order = np.arange(h, dtype=np.int64)
    if n:
        order[:n] = np.lexsort([src[:n, k] for k in reversed(keys)])
    cols = [src[order]]
    if source_row:
        cols.append(order.astype(np.uint32)[:, None])
    if group_start:
        start = np.zeros(h, dtype=np.uint32)
        if n:
            start[0] = 1
            if group_keys and n > 1:
                lead = src[order[:n]][:, list(keys[:group_keys])]
                start[1:n] = (lead[1:] != lead[:-1]).any(axis=1)
        cols.append(start[:, None])
    return np.concatenate(cols, axis=1)


def python_order(src, keys, n_live):
    """The same order with nothing but ``sorted`` (stable) over tuples of Python ints."""
    rows = [[int(w) for w in r] for r in src]
    return sorted(range(n_live), key=lambda r: tuple(rows[r][k] for k in keys)) + list(range(n_live, len(rows)))


def _rng(seed):
    return np.random.default_rng(seed)


def matrix(key_words, width=3, key_column=None, seed=1):
    """A width-wide matrix of random words whose ``key_column`` (default: the last) holds ``key_words``."""
    key_words = np.asarray(key_words, dtype=np.uint32)
    m = _rng(seed).integers(0, 1 << 32, size=(len(key_words), width), dtype=np.uint64).astype(np.uint32)
    m[:, width - 1 if key_column is None else key_column] = key_words
    return m


EDGE_WORDS = np.array([0, 1, P - 1, P, P + 1, 1 << 31, 0xFFFFFFFF], dtype=np.uint32)


def key_family(name: str, n: int, seed: int = 7) -> np.ndarray:
    """n key words of the named family."""
    r = _rng(seed)
    i = np.arange(n, dtype=np.uint64)
    if name == "all_equal":
        w = np.full(n, 0x12345678, dtype=np.uint64)
    elif name == "sorted":
        w = i * 3
    elif name == "reversed":
        w = (n - 1 - i) * 3
    elif name == "top_byte":      # passes 0 .. 2 are skipped
        w = (r.integers(0, 256, n, dtype=np.uint64) << 24) | 0x00ABCDEF
    elif name == "byte1":         # passes 0, 2, 3 are skipped
        w = (r.integers(0, 256, n, dtype=np.uint64) << 8) | 0x7700_0055
    elif name == "byte0":         # passes 1 .. 3 are skipped
        w = r.integers(0, 256, n, dtype=np.uint64) | 0x7766_5500
    elif name == "edge_words":
        w = EDGE_WORDS[r.integers(0, len(EDGE_WORDS), n)].astype(np.uint64)
    elif name == "wave_one_digit":   # each run of 64 rows on one digit of byte 0, the runs in descending order
        w = (255 - (i // 64) % 256) | (r.integers(0, 4, n, dtype=np.uint64) << 8)
    elif name == "wave_64_digits":   # each run of 64 rows on 64 distinct digits, descending inside the run
        w = (63 - i % 64) * 4 + (i // 64) % 4
    elif name == "digits_0_255":
        w = r.integers(0, 2, n, dtype=np.uint64) * 255
    elif name == "uniform":
        w = r.integers(0, P, n, dtype=np.uint64)
    else:
        raise KeyError(name)
    return w.astype(np.uint32)


KEY_FAMILIES = ("all_equal", "sorted", "reversed", "top_byte", "byte1", "byte0", "edge_words", "wave_one_digit",
                "wave_64_digits", "digits_0_255", "uniform")


def tail_case(key_words, height, width=3, seed=3):
    """(matrix of ``height`` rows, n_live): the live rows carry ``key_words`` in the last column, the tail rows are all
    zero -- they would sort first -- except a row marker in column 0."""
    n = len(key_words)
    m = np.zeros((height, width), dtype=np.uint32)
    m[:n] = matrix(key_words, width, seed=seed)
    if width > 1:
        m[n:, 0] = np.arange(n, height, dtype=np.uint32) + 0x5000_0000
    return m, n


def multi_key_case(n, n_keys, width=6, seed=11):
    """Heavy ties in the leading key (4 values), fewer in each following one; key columns not in column order."""
    r = _rng(seed)
    m = r.integers(0, 1 << 32, size=(n, width), dtype=np.uint64).astype(np.uint32)
    columns = [4, 1, 5, 0][:n_keys]
    spans = [4, 8, 16, 1 << 32][:n_keys]
    for c, s in zip(columns, spans):
        m[:, c] = r.integers(0, s, n, dtype=np.uint64).astype(np.uint32)
    return m, columns
