"""Specs for ``expand_rows`` (``ts_matrix_expand_rows``, include/tapstark.h "expanded rows"): every row of one resident
matrix repeated by a count read from the row itself, each copy reshaped to one tuple form, in (row, inner index) order
and padded to a power of two -- the element table of a block instruction, the rounds of a precompile call.

    spec = ExpandSpec(4, 5, count=col(2), when=col(3), max_count=64)      # `len` in column 2, a selector in column 3
    spec.terms = [col(0), J, LAST, stepped(1, 1), 1]                      # id, j, last flag, base + j, the constant 1
    table, n_live = ts.expand_rows(ctx, spec, calls)

A term is an integer or ``const(v)`` (a constant mod p), ``col(c)`` (column c of the source row, copied as stored),
``ROW`` (the index of the source row), ``J`` (the inner index), ``REMAINING`` (cnt - 1 - j), ``FIRST`` and ``LAST`` (the
flags of the first and last copy) or ``stepped(c, step)`` ((column c mod p + j * step) mod p).  ``count`` is a column
or an integer constant; ``when`` is ``ALWAYS`` or a column.  ``expand_rows_host`` needs no GPU: the library's checks and
its sequential loop over host rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .collect import ALWAYS, col, const  # the same selector and term objects as the collect's

P = 0x78000001
MAGIC = 0x50584554  # "TEXP"
MAX_WIDTH = 64
MAX_HEIGHT = MAX_COUNT = 1 << 27


class stepped:
    """``(column c mod p + j * step) mod p``: the address of element j of a span."""

    def __init__(self, c: int, step: int = 1):
        self.c, self.step = int(c), int(step) % P


class _Named:
    def __init__(self, name: str, kind: int):
        self.name, self.kind = name, kind

    def __repr__(self):
        return self.name


ROW, J, REMAINING, FIRST, LAST = (_Named(n, k) for k, n in enumerate(("ROW", "J", "REMAINING", "FIRST", "LAST"), 2))


def _term(t) -> tuple[int, int, int]:
    if isinstance(t, col):
        return 1, t.c, 0
    if isinstance(t, _Named):
        return t.kind, 0, 0
    if isinstance(t, stepped):
        return 7, t.c, t.step
    if isinstance(t, (tuple, list)):  # raw (kind, value, step), for the tests of the refusals
        return int(t[0]), int(t[1]), int(t[2])
    if type(t).__name__ == "_Row":  # the collect's ROW
        return 2, 0, 0
    return 0, t.v if isinstance(t, const) else int(t) % P, 0


def _pair(s, constant_kind_value) -> tuple[int, int]:
    if isinstance(s, col):
        return 1, s.c
    if isinstance(s, (tuple, list)):  # raw (kind, value)
        return int(s[0]), int(s[1])
    return constant_kind_value(s)


class ExpandSpec:
    """One expansion.  Nothing is checked here: the call that runs the spec is the judge."""

    def __init__(self, src_width: int, out_width: int, count=1, when=ALWAYS, max_count: int = 1, pad=None, terms=None):
        self.src_width, self.out_width = int(src_width), int(out_width)
        self.count = _pair(count, lambda c: (0, int(c)))
        self.when = _pair(when, lambda s: (0, 1))
        self.max_count = int(max_count)
        self.pad = [0] * self.out_width if pad is None else [int(v) for v in pad]
        self.terms = [0] * self.out_width if terms is None else list(terms)

    def words(self) -> np.ndarray:
        words = [MAGIC, 1, self.src_width, self.out_width, *self.when, *self.count, self.max_count, *self.pad]
        for t in self.terms:
            words += _term(t)
        return np.array(words, dtype=np.uint32)


def _tape(spec) -> np.ndarray:
    return spec.words() if isinstance(spec, ExpandSpec) else np.ascontiguousarray(spec, dtype=np.uint32)


def _p(a):
    return a.ctypes.data_as(_lib.u32p)


def expand_check(spec) -> tuple[int, int]:
    """``ts_expand_check``: (src_width, out_width) of a spec every matrix-free rule accepts; raises ``TsError`` with the
    library's text otherwise."""
    t = _tape(spec)
    sw, ow = C.c_uint32(), C.c_uint32()
    l = _lib.lib()
    st = l.ts_expand_check(_p(t), len(t), C.byref(sw), C.byref(ow))
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return int(sw.value), int(ow.value)


def expand_rows_host(spec, src, out_height: int = 0, capacity_rows: int | None = None):
    """``ts_expand_rows_host``: the pair (matrix, n_live) that ``expand_rows`` gives for the same source, computed by the
    library's sequential loop on the host.  ``capacity_rows`` sizes the output buffer (by default: enough for what the
    rows ask for, counted here with the header's rule); raises ``TsError`` with the library's text."""
    t = _tape(spec)
    src = np.ascontiguousarray(src, dtype=np.uint32)
    assert src.ndim == 2
    src_width, out_width = expand_check(t)
    # (the library reads rows of the spec's width: a host array of another width would be read past its end)
    assert src.shape[1] == src_width, "the source's width differs from the spec's"
    if capacity_rows is None:
        takes = (src[:, int(t[5])].astype(np.uint64) % P != 0) if int(t[4]) else np.ones(len(src), dtype=bool)
        cnt = (src[:, int(t[7])].astype(np.uint64) % P) if int(t[6]) else np.full(len(src), int(t[7]), dtype=np.uint64)
        most = max(1, int(cnt[takes].sum()))
        if most > (out_height or MAX_HEIGHT) or (cnt[takes] > int(t[8])).any():
            most = 1  # (the call is refused before it looks at the buffer)
        capacity_rows = max(out_height, 1 << (most - 1).bit_length())
    out = np.zeros((capacity_rows, out_width), dtype=np.uint32)
    used, live = C.c_uint64(), C.c_uint64()
    l = _lib.lib()
    st = l.ts_expand_rows_host(_p(t), len(t), _p(src), src.shape[0], out_height, _p(out), out.size, C.byref(used),
                               C.byref(live))
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return out[:int(used.value)].copy(), int(live.value)
