"""Specs for ``DeviceMatrix.join_rows`` (``ts_matrix_join_rows``, include/tapstark.h "joined rows"): for every row of
a resident source the table row with the same key tuple, and chosen columns of that row written into the source's row
-- the instruction a machine row fetched from a program ROM, the flags an opcode decodes to, an S-box entry.

    spec = JoinSpec(keys=[(col(0), col(0))],                  # source column 0 against table column 0
                    when=col(3),                              # on the rows where column 3 is not zero mod p
                    fetch=[(1, 1, 0), (2, 2, 0)])             # table columns 1, 2 -> columns 1, 2; 0 without a match
    filled, n_missing, first_missing = trace.join_rows(rom, spec, allow_missing=True)

A key term is an integer or ``const(v)`` (a constant mod p) or ``col(c)`` (column c of the side's own row, matched as
stored).  ``join_rows_host`` needs no GPU: the library's checks and its sequential loop over host rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .collect import col, const

P = 0x78000001
MAX_KEYS, MAX_FETCH = 8, 32
TABLE_ROW, HIT, KEEP = 1, 2, 4  # TS_JOIN_TABLE_ROW, TS_JOIN_HIT, TS_JOIN_KEEP
ALWAYS = (0, 1)  # the constant 1 as `when`: every row takes part


def _term(t) -> tuple[int, int]:
    if isinstance(t, col):
        return 1, t.c
    if isinstance(t, (tuple, list)):  # raw (kind, value), for the tests of the refusals
        return int(t[0]), int(t[1])
    return 0, t.v if isinstance(t, const) else int(t) % P


class JoinSpec:
    """The spec of one join.  Nothing is checked here: the call that runs the spec is the judge.  ``keys`` pairs a term
    on the source's row with a term on the table's row; ``fetch`` lists (table column, dst column, default)."""

    def __init__(self, keys, when=ALWAYS, fetch=(), flags: int = 0, table_rows: int = 0):
        self.keys = [(_term(s), _term(t)) for s, t in keys]
        self.when = _term(when)
        self.fetch = [(int(t), int(d), int(v)) for t, d, v in fetch]
        self.flags = int(flags)
        self.table_rows = int(table_rows)
        self.struct_size = C.sizeof(_lib.JoinSpecC)

    def c_spec(self):
        """(the ``ts_join_spec``, the arrays it points to): keep the second alive as long as the first is used."""
        n, m = len(self.keys), len(self.fetch)
        src = (_lib.LogupTermC * max(n, 1))(*[_lib.LogupTermC(*s) for s, _ in self.keys])
        tab = (_lib.LogupTermC * max(n, 1))(*[_lib.LogupTermC(*t) for _, t in self.keys])
        cols = [(C.c_uint32 * max(m, 1))(*[f[k] & 0xFFFFFFFF for f in self.fetch]) for k in range(3)]
        spec = _lib.JoinSpecC(self.struct_size, n, src, tab, _lib.LogupTermC(*self.when), m, cols[0], cols[1], cols[2],
                              self.flags, self.table_rows)
        return spec, (src, tab, cols)


def _p(a):
    return a.ctypes.data_as(_lib.u32p)


def join_check(spec: JoinSpec, src_width: int, table_width: int) -> int:
    """``ts_join_check``: the width of the result of a spec every matrix-free rule accepts; raises ``TsError`` with the
    library's text otherwise."""
    s, _keep = spec.c_spec()
    w = C.c_uint32()
    l = _lib.lib()
    st = l.ts_join_check(C.byref(s), src_width, table_width, C.byref(w))
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return int(w.value)


def join_rows_host(spec: JoinSpec, src, table, allow_missing: bool = True, capacity_words: int | None = None):
    """``ts_join_rows_host``: the triple (matrix, n_missing, first_missing) that ``DeviceMatrix.join_rows`` gives for
    the same matrices, computed by the library's sequential loop on the host; ``first_missing`` is None without a miss.
    ``capacity_words`` sizes the output buffer (by default: exactly what the result needs); raises ``TsError``."""
    src = np.ascontiguousarray(src, dtype=np.uint32)
    table = src if table is src else np.ascontiguousarray(table, dtype=np.uint32)
    assert src.ndim == 2 and table.ndim == 2
    width = join_check(spec, src.shape[1], table.shape[1])
    out = np.zeros(src.shape[0] * width if capacity_words is None else capacity_words, dtype=np.uint32)
    s, _keep = spec.c_spec()
    n, first = C.c_uint64(), C.c_uint64()
    l = _lib.lib()
    st = l.ts_join_rows_host(C.byref(s), _p(src), src.shape[0], src.shape[1], _p(table), table.shape[0], table.shape[1],
                             _p(out), out.size, C.byref(n) if allow_missing else None, C.byref(first))
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    first_missing = None if first.value == 0xFFFFFFFFFFFFFFFF else int(first.value)
    return out[:src.shape[0] * width].reshape(src.shape[0], width).copy(), int(n.value), first_missing
