"""Specs for ``group_rows`` (the TGRP tape of ``ts_matrix_collect_rows``, include/tapstark.h "grouped rows"): one output
row per distinct key tuple among the rows of one resident matrix that take part, in order of first appearance, made of
words of the group's first and last row, its size, and sums, minima and maxima over it -- the table of touched
addresses of a memory trace, with each address's final value and the clock of its last access.

    spec = GroupSpec(src_width=5, out_width=6, keys=[col(0)], when=col(4))
    spec.terms = [first(0), last(1), last(2), COUNT, total(3), INDEX]
    table, n_groups = ts.group_rows(ctx, spec, accesses)

A key term is ``col(c)`` (column c, compared as stored) or ``const(v)``.  An output term is an integer or ``const(v)``,
``first(c)`` / ``last(c)`` (column c of the group's least / greatest row, as stored), ``FIRST_ROW`` / ``LAST_ROW`` (those
rows' indices), ``COUNT``, ``total(c)`` / ``least(c)`` / ``greatest(c)`` (sum, minimum, maximum of column c over the
group, the words reduced mod p) or ``INDEX`` (the group's own output row).  ``col(c)`` as an output term means
``first(c)``.  ``group_rows_host`` needs no GPU: the library's checks and its sequential loop over host rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .collect import ALWAYS, P, _p, _selector, col, const  # noqa: F401  (the collect's selector and key terms)

MAGIC = 0x50524754  # "TGRP"
MAX_KEYS, MAX_AGGREGATES, MAX_WIDTH = 8, 16, 64
K_CONST, K_FIRST, K_LAST, K_FIRST_ROW, K_LAST_ROW, K_COUNT, K_SUM, K_MIN, K_MAX, K_INDEX = range(10)


class _Term:
    def __init__(self, kind: int, value: int = 0, name: str = ""):
        self.kind, self.value, self.name = int(kind), int(value), name

    def __repr__(self):
        return self.name or f"term({self.kind}, {self.value})"


def first(c: int) -> _Term:
    """Column ``c`` of the group's least row, as stored."""
    return _Term(K_FIRST, c, f"first({c})")


def last(c: int) -> _Term:
    """Column ``c`` of the group's greatest row, as stored."""
    return _Term(K_LAST, c, f"last({c})")


def total(c: int) -> _Term:
    """The sum over the group of column ``c``, each word reduced mod p; canonical."""
    return _Term(K_SUM, c, f"total({c})")


def least(c: int) -> _Term:
    """The least word of column ``c`` over the group, each reduced mod p."""
    return _Term(K_MIN, c, f"least({c})")


def greatest(c: int) -> _Term:
    """The greatest word of column ``c`` over the group, each reduced mod p."""
    return _Term(K_MAX, c, f"greatest({c})")


FIRST_ROW = _Term(K_FIRST_ROW, 0, "FIRST_ROW")
LAST_ROW = _Term(K_LAST_ROW, 0, "LAST_ROW")
COUNT = _Term(K_COUNT, 0, "COUNT")
INDEX = _Term(K_INDEX, 0, "INDEX")


def _key(t) -> tuple[int, int]:
    if isinstance(t, col):
        return 1, t.c
    if isinstance(t, (tuple, list)):  # raw (kind, value), for the tests of the refusals
        return int(t[0]), int(t[1])
    return 0, t.v if isinstance(t, const) else int(t) % P


def _term(t) -> tuple[int, int]:
    if isinstance(t, _Term):
        return t.kind, t.value
    if isinstance(t, col):
        return K_FIRST, t.c
    if isinstance(t, (tuple, list)):
        return int(t[0]), int(t[1])
    return K_CONST, t.v if isinstance(t, const) else int(t) % P


class GroupSpec:
    """One group call.  Nothing is checked here: the call that runs the spec is the judge."""

    def __init__(self, src_width: int, out_width: int, keys, when=ALWAYS, pad=None, terms=()):
        self.src_width, self.out_width = int(src_width), int(out_width)
        self.keys = list(keys)
        self.when = when
        self.pad = [0] * self.out_width if pad is None else [int(v) for v in pad]
        self.terms = list(terms)

    def tape(self) -> np.ndarray:
        words = [MAGIC, 1, self.src_width, self.out_width, len(self.keys), *_selector(self.when)]
        for k in self.keys:
            words += _key(k)
        words += self.pad
        for t in self.terms:
            words += _term(t)
        return np.array(words, dtype=np.uint32)


def _tape(spec) -> np.ndarray:
    return spec.tape() if isinstance(spec, GroupSpec) else np.ascontiguousarray(spec, dtype=np.uint32)


def group_check(spec) -> tuple[int, int]:
    """``ts_collect_check`` on a TGRP tape: (1, out_width) of a spec every matrix-free rule accepts; raises ``TsError``
    with the library's text otherwise."""
    t = _tape(spec)
    n, w = C.c_uint32(), C.c_uint32()
    l = _lib.lib()
    st = l.ts_collect_check(_p(t), len(t), C.byref(n), C.byref(w))
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return int(n.value), int(w.value)


def group_rows_host(spec, src, out_height: int = 0, capacity_rows: int | None = None):
    """``ts_collect_rows_host`` on a TGRP tape: the pair (matrix, n_groups) that ``group_rows`` gives for the same
    source, computed by the library's sequential loop on the host.  ``capacity_rows`` sizes the output buffer (by
    default: enough for every row being a group of its own); raises ``TsError`` with the library's text."""
    t = _tape(spec)
    src = np.ascontiguousarray(src, dtype=np.uint32)
    assert src.ndim == 2
    _, out_width = group_check(t)
    # (the library reads rows of the spec's width: a host array of another width would be read past its end)
    assert src.shape[1] == int(t[2]), "the source's width differs from the spec's"
    if capacity_rows is None:
        capacity_rows = max(out_height, 1 << (max(1, src.shape[0]) - 1).bit_length())
    out = np.zeros((capacity_rows, out_width), dtype=np.uint32)
    ptrs = (_lib.u32p * 1)(_p(src))
    heights = (C.c_uint64 * 1)(src.shape[0])
    used, live = C.c_uint64(), C.c_uint64()
    l = _lib.lib()
    st = l.ts_collect_rows_host(_p(t), len(t), ptrs, heights, out_height, _p(out), out.size, C.byref(used), C.byref(live))
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return out[:int(used.value)].copy(), int(live.value)
