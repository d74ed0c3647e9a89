"""Row programs for ``DeviceMatrix.derive`` (``ts_matrix_derive``, include/tapstark.h "derived columns"): columns
that are a function of their own row and its two neighbours, evaluated in HBM.

    b = DeriveBuilder(4)
    x = b.col(2)
    b.output(x.bits(0, 16), 4)           # two 16-bit limbs of column 2, appended
    b.output(x.bits(16, 15), 5)
    wide = matrix.derive(b.tape())

``derive_check`` and ``derive_rows_host`` need no GPU: the library's checks and its lowered program over host rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

P = 0x78000001
MAGIC = 0x52454454  # "TDER"
MAX_NODES, MAX_OUTPUTS, MAX_LIVE = 4096, 256, 48

CONST, COL, IS_FIRST_ROW, IS_LAST_ROW, IS_TRANSITION, ADD, SUB, NEG, MUL = 0, 1, 3, 4, 5, 6, 7, 8, 9
ROW, INV, IS_ZERO, LT, BITS, AND, XOR = 32, 33, 34, 35, 36, 37, 38


class DeriveExpr:
    """A node of a ``DeriveBuilder``; integers on the other side of an operator become constants mod p."""

    def __init__(self, builder: "DeriveBuilder", node: int):
        self.b = builder
        self.node = node

    def _bin(self, op, other, swap=False):
        o = self.b._lift(other)
        x, y = (o, self) if swap else (self, o)
        return self.b._node(op, x.node, y.node)

    def __add__(self, o): return self._bin(ADD, o)
    def __radd__(self, o): return self._bin(ADD, o, True)
    def __sub__(self, o): return self._bin(SUB, o)
    def __rsub__(self, o): return self._bin(SUB, o, True)
    def __mul__(self, o): return self._bin(MUL, o)
    def __rmul__(self, o): return self._bin(MUL, o, True)
    def __and__(self, o): return self._bin(AND, o)
    def __rand__(self, o): return self._bin(AND, o, True)
    def __xor__(self, o): return self._bin(XOR, o)
    def __rxor__(self, o): return self._bin(XOR, o, True)
    def __neg__(self): return self.b._node(NEG, self.node, 0)

    def inv(self): return self.b._node(INV, self.node, 0)
    def is_zero(self): return self.b._node(IS_ZERO, self.node, 0)
    def lt(self, o): return self._bin(LT, o)

    def bits(self, shift: int, n: int):
        """``(self >> shift) & (2^n - 1)`` on the canonical integer."""
        return self.b._node(BITS, self.node, int(shift) | int(n) << 8)


class DeriveBuilder:
    """Collects the nodes and outputs of a row program over a source matrix of ``src_width`` columns.  Nothing is
    checked here: ``derive_check`` (or the call that runs the program) is the judge."""

    def __init__(self, src_width: int):
        self.src_width = int(src_width)
        self.nodes: list[tuple[int, int, int]] = []
        self.outputs: list[tuple[int, int]] = []

    def _node(self, op, a, b) -> DeriveExpr:
        self.nodes.append((op, a, b))
        return DeriveExpr(self, len(self.nodes) - 1)

    def _lift(self, v) -> DeriveExpr:
        if isinstance(v, DeriveExpr):
            if v.b is not self:
                raise ValueError("an expression of another DeriveBuilder")
            return v
        return self.constant(int(v) % P)

    def constant(self, v: int) -> DeriveExpr: return self._node(CONST, int(v), 0)
    def col(self, c: int) -> DeriveExpr: return self._node(COL, 0, int(c))
    def next(self, c: int) -> DeriveExpr: return self._node(COL, 1, int(c))
    def prev(self, c: int) -> DeriveExpr: return self._node(COL, 2, int(c))
    def row(self) -> DeriveExpr: return self._node(ROW, 0, 0)
    def is_first_row(self) -> DeriveExpr: return self._node(IS_FIRST_ROW, 0, 0)
    def is_last_row(self) -> DeriveExpr: return self._node(IS_LAST_ROW, 0, 0)
    def is_transition(self) -> DeriveExpr: return self._node(IS_TRANSITION, 0, 0)

    def output(self, expr, dst: int) -> None:
        """Column ``dst`` of the result holds ``expr``."""
        self.outputs.append((self._lift(expr).node, int(dst)))

    def tape(self) -> np.ndarray:
        words = [MAGIC, 1, self.src_width, len(self.nodes), len(self.outputs)]
        for n in self.nodes:
            words += n
        for o in self.outputs:
            words += o
        return np.array(words, dtype=np.uint64).astype(np.uint32)


def _tape(program) -> np.ndarray:
    if isinstance(program, DeriveBuilder):
        program = program.tape()
    return np.ascontiguousarray(program, dtype=np.uint32).reshape(-1)


def _p(a: np.ndarray):
    return a.ctypes.data_as(_lib.u32p)


def derive_check(program, src_width: int) -> dict:
    """``ts_derive_check``: {"out_width", "n_instructions", "n_live"}; raises ``TsError`` with the library's text."""
    t = _tape(program)
    l = _lib.lib()
    w, n, live = C.c_uint32(), C.c_uint32(), C.c_uint32()
    st = l.ts_derive_check(_p(t), len(t), src_width, C.byref(w), C.byref(n), C.byref(live))
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return {"out_width": int(w.value), "n_instructions": int(n.value), "n_live": int(live.value)}


def derive_rows_host(program, rows) -> np.ndarray:
    """``ts_derive_rows_host``: what ``DeviceMatrix.upload(rows).derive(program)`` holds, computed on the host by the
    library's own lowered program."""
    t = _tape(program)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    assert rows.ndim == 2
    h, w = rows.shape
    out_width = derive_check(t, w)["out_width"]
    out = np.zeros((h, out_width), dtype=np.uint32)
    l = _lib.lib()
    st = l.ts_derive_rows_host(_p(t), len(t), _p(rows), h, w, _p(out), out.size)
    if st:
        raise _lib.TsError(st, (l.ts_last_error(None) or b"").decode())
    return out
