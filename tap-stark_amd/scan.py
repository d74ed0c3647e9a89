"""Scans for ``DeviceMatrix.scan`` (``ts_matrix_scan``, include/tapstark.h "scanned columns"): first-order linear
recurrences ``y[i] = a[i] y[i-1] + b[i]`` over BabyBear down the rows of a resident matrix, optionally started over
where a reset column is not zero -- running sums, counts and products, "carry the last written value".

    spec = running_sum(2, dst=4, reset=3)          # column 4 = the sum of column 2 inside each group that column 3 starts
    spec.add(dst=5, a=col(1), b=1, init=1)         # a second scan in the same call
    wide = matrix.scan(spec)

A term is an integer (a constant mod p) or ``col(c)`` (column c of the source, read as stored and reduced mod p).
``scan_rows_host`` needs no GPU: the library's checks and its sequential loop over host rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

P = 0x78000001
MAX_COLUMNS = 8
NO_RESET = 0xFFFFFFFF
EXCLUSIVE = 1


class col:
    """Column ``c`` of the source as the ``a`` or ``b`` of a scan."""

    def __init__(self, c: int):
        self.c = int(c)


def _term(t) -> tuple[int, int]:
    return (1, t.c) if isinstance(t, col) else (0, int(t) % P)


class ScanSpec:
    """Collects the scans of one call.  Nothing is checked here: the call that runs the spec is the judge.
    ``out_width`` 0 keeps every column; another value keeps columns ``[0, out_width)`` only."""

    def __init__(self, out_width: int = 0):
        self.columns: list[dict] = []
        self.out_width = int(out_width)

    def add(self, dst: int, a=1, b=0, init: int = 0, reset: int | None = None, exclusive: bool = False,
            flags: int | None = None) -> "ScanSpec":
        """One more scan: column ``dst`` of the result holds ``y[i] = a[i] y[i-1] + b[i]``, ``y[-1] = init``; where
        column ``reset`` is not zero the row starts over from ``init``.  ``exclusive``: the state before the row."""
        self.columns.append({"a": _term(a), "b": _term(b), "init": int(init),
                             "reset": NO_RESET if reset is None else int(reset), "dst": int(dst),
                             "flags": (EXCLUSIVE if exclusive else 0) if flags is None else int(flags)})
        return self

    def extend(self, other: "ScanSpec") -> "ScanSpec":
        self.columns += other.columns
        return self

    def c_spec(self) -> "_lib.ScanSpecC":
        s = _lib.ScanSpecC()
        s.struct_size = C.sizeof(_lib.ScanSpecC)
        s.n_columns = len(self.columns)
        s.out_width = self.out_width
        for k, c in enumerate(self.columns[:MAX_COLUMNS]):
            sc = s.columns[k]
            (sc.a.kind, sc.a.value), (sc.b.kind, sc.b.value) = c["a"], c["b"]
            sc.init, sc.reset_column, sc.dst_column, sc.flags = c["init"], c["reset"], c["dst"], c["flags"]
        return s


def running_sum(column: int, reset: int | None = None, dst: int | None = None, init: int = 0,
                exclusive: bool = False) -> ScanSpec:
    """``y[i] = y[i-1] + src[i][column]`` (``dst`` defaults to ``column``: the sum replaces its summand)."""
    return ScanSpec().add(column if dst is None else dst, a=1, b=col(column), init=init, reset=reset, exclusive=exclusive)


def running_product(column: int, reset: int | None = None, dst: int | None = None, init: int = 1,
                    exclusive: bool = False) -> ScanSpec:
    """``y[i] = src[i][column] y[i-1]``, from 1: the running product of a permutation argument."""
    return ScanSpec().add(column if dst is None else dst, a=col(column), b=0, init=init, reset=reset, exclusive=exclusive)


def carry_last(flag_col: int, value_col: int, src_width: int, dst: int | None = None, reset: int | None = None,
               init: int = 0):
    """"Carry the last written value": ``y[i] = value[i]`` where ``flag[i]`` is 1, else ``y[i-1]``.  As a recurrence that
    is ``a = 1 - flag``, ``b = flag * value``, and a scan reads its ``a`` and ``b`` from columns, so two helper columns
    are needed.  Returns ``(program, spec)``: ``program`` is the ``DeriveBuilder`` that appends them to a source of
    ``src_width`` columns (``a`` at ``src_width``, ``b`` at ``src_width + 1``), ``spec`` the scan over the widened matrix,
    which writes ``dst`` (default: ``value_col``) and drops the two helpers again:

        program, spec = carry_last(3, 2, src_width=8, reset=7)
        filled = matrix.derive(program).scan(spec)
    """
    from .derive import DeriveBuilder
    b = DeriveBuilder(src_width)
    flag = b.col(flag_col)
    b.output(1 - flag, src_width)
    b.output(flag * b.col(value_col), src_width + 1)
    dst = value_col if dst is None else dst
    spec = ScanSpec(out_width=max(src_width, dst + 1))
    spec.add(dst, a=col(src_width), b=col(src_width + 1), init=init, reset=reset)
    return b, spec


def _p(a: np.ndarray):
    return a.ctypes.data_as(_lib.u32p)


def out_width(spec: ScanSpec, src_width: int) -> int:
    """The width of the result (the library checks the rules; this only computes)."""
    return spec.out_width or max([src_width] + [c["dst"] + 1 for c in spec.columns])


def scan_rows_host(spec: ScanSpec, rows, finals: bool = False):
    """``ts_scan_rows_host``: what ``DeviceMatrix.upload(rows).scan(spec)`` holds, computed by the library's sequential
    loop on the host; with ``finals`` the pair (matrix, the last value of each scan).  Raises ``TsError`` with the
    library's text."""
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    assert rows.ndim == 2
    h, w = rows.shape
    out = np.zeros((h, min(out_width(spec, w), 1 << 16)), dtype=np.uint32)
    last = np.zeros(MAX_COLUMNS, dtype=np.uint32)
    l = _lib.lib()
    st = l.ts_scan_rows_host(C.byref(spec.c_spec()), _p(rows), h, w, _p(out), out.size, _p(last) if finals else None)
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return (out, last[:len(spec.columns)].copy()) if finals else out
