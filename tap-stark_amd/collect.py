"""Specs for ``collect_rows`` (``ts_matrix_collect_rows``, include/tapstark.h "collected rows"): the rows that emitters
select from up to four resident matrices, each reshaped to one tuple form, stacked in (source, row, emitter) order and
padded to a power of two -- the access table of a machine trace with several conditional access slots per row.

    spec = CollectSpec([10], out_width=5)                             # one source of 10 columns, pad row all zero
    spec.emit(0, when=col(4), terms=[col(2), col(1), col(3), 0, 1])   # slot a where column 4 is not zero mod p
    spec.emit(0, when=ALWAYS, terms=[col(7), ROW, const(9), 1, 1])    # a second slot on every row
    table, n_live = ts.collect_rows(ctx, spec, [cpu])

A term is an integer or ``const(v)`` (a constant mod p), ``col(c)`` (column c of the emitter's source, copied as stored)
or ``ROW`` (the index of the source row).  ``collect_rows_host`` needs no GPU: the library's checks and its sequential
loop over host rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

P = 0x78000001
MAGIC = 0x4C4F4354  # "TCOL"
MAX_SOURCES, MAX_EMITTERS, MAX_WIDTH = 4, 16, 64
MAX_HEIGHT = 1 << 27


class col:
    """Column ``c`` of the emitter's source: as a selector or as a term."""

    def __init__(self, c: int):
        self.c = int(c)


class const:
    """The constant ``v`` mod p as a term."""

    def __init__(self, v: int):
        self.v = int(v) % P


class _Row:
    def __repr__(self):
        return "ROW"


class _Always:
    def __repr__(self):
        return "ALWAYS"


ROW = _Row()
ALWAYS = _Always()


def _term(t) -> tuple[int, int]:
    if isinstance(t, col):
        return 1, t.c
    if isinstance(t, _Row):
        return 2, 0
    if isinstance(t, (tuple, list)):  # raw (kind, value), for the tests of the refusals
        return int(t[0]), int(t[1])
    return 0, t.v if isinstance(t, const) else int(t) % P


def _selector(s) -> tuple[int, int]:
    if isinstance(s, _Always):
        return 0, 1
    if isinstance(s, col):
        return 1, s.c
    return int(s[0]), int(s[1])  # raw (kind, value)


class CollectSpec:
    """Collects the emitters of one call.  Nothing is checked here: the call that runs the spec is the judge."""

    def __init__(self, src_widths, out_width: int, pad=None):
        self.src_widths = [int(w) for w in src_widths]
        self.out_width = int(out_width)
        self.pad = [0] * self.out_width if pad is None else [int(v) for v in pad]
        self.emitters: list[tuple[int, tuple[int, int], list[tuple[int, int]]]] = []

    def emit(self, source: int, when=ALWAYS, terms=()) -> "CollectSpec":
        """One more emitter: on every row of ``source`` where ``when`` fires, one output row made of ``terms``."""
        self.emitters.append((int(source), _selector(when), [_term(t) for t in terms]))
        return self

    def tape(self) -> np.ndarray:
        words = [MAGIC, 1, len(self.src_widths), len(self.emitters), self.out_width, *self.src_widths, *self.pad]
        for source, (sel_kind, sel_value), terms in self.emitters:
            words += [source, sel_kind, sel_value]
            for kind, value in terms:
                words += [kind, value]
        return np.array(words, dtype=np.uint32)


def _tape(spec) -> np.ndarray:
    return spec.tape() if isinstance(spec, CollectSpec) else np.ascontiguousarray(spec, dtype=np.uint32)


def _p(a):
    return a.ctypes.data_as(_lib.u32p)


def collect_check(spec) -> tuple[int, int]:
    """``ts_collect_check``: (n_sources, out_width) of a spec every matrix-free rule accepts; raises ``TsError`` with
    the library's text otherwise."""
    t = _tape(spec)
    n, w = C.c_uint32(), C.c_uint32()
    l = _lib.lib()
    st = l.ts_collect_check(_p(t), len(t), C.byref(n), C.byref(w))
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return int(n.value), int(w.value)


def collect_rows_host(spec, sources, out_height: int = 0, capacity_rows: int | None = None):
    """``ts_collect_rows_host``: the pair (matrix, n_live) that ``collect_rows`` gives for the same sources, computed by
    the library's sequential loop on the host.  ``capacity_rows`` sizes the output buffer (by default: enough for every
    emitter firing on every row); raises ``TsError`` with the library's text."""
    t = _tape(spec)
    sources = [np.ascontiguousarray(s, dtype=np.uint32) for s in sources]
    assert all(s.ndim == 2 for s in sources)
    n_sources, out_width = collect_check(t)
    assert len(sources) == n_sources, "as many sources as the spec names"
    # (the library reads rows of the spec's widths: a host array of another width would be read past its end)
    assert [s.shape[1] for s in sources] == [int(w) for w in t[5:5 + n_sources]], "source widths differ from the spec's"
    if capacity_rows is None:
        most = max(1, int(t[3]) * sum(s.shape[0] for s in sources))
        capacity_rows = max(out_height, 1 << (most - 1).bit_length())
    out = np.zeros((capacity_rows, out_width), dtype=np.uint32)
    ptrs = (_lib.u32p * n_sources)(*[_p(s) for s in sources])
    heights = (C.c_uint64 * n_sources)(*[s.shape[0] for s in sources])
    used, live = C.c_uint64(), C.c_uint64()
    l = _lib.lib()
    st = l.ts_collect_rows_host(_p(t), len(t), ptrs, heights, out_height, _p(out), out.size, C.byref(used), C.byref(live))
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return out[:int(used.value)].copy(), int(live.value)
