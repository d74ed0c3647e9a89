"""Row programs with carried state for ``DeviceMatrix.iterate`` (the iterate form of ``ts_matrix_derive``,
include/tapstark.h "iterated columns"): derive's row program plus up to 16 registers carried down each group of rows.
A group starts at row 0 and at every row whose ``reset_column`` word is not 0 mod p.

    b = IterateBuilder(3, reset_column=0, max_group_rows=64)     # first, word, state
    state = b.carry(IV)                  # the state after the previous row of the group, IV on its first row
    acc = state + b.col(1)
    new = acc * acc * acc
    b.set_carry(state, new)
    b.output(new, 2)
    filled = matrix.iterate(b)

``iterate_check`` and ``iterate_rows_host`` need no GPU: they are ``derive_check`` and ``derive_rows_host``, the same
three entry points told apart by the tape's magic.
"""
from __future__ import annotations

import numpy as np

from .derive import DeriveBuilder, DeriveExpr, P, derive_check, derive_rows_host

MAGIC = 0x52544954  # "TITR"
MAX_CARRIES, MAX_WORK = 16, 1 << 20
NO_RESET = 0xFFFFFFFF
CARRY, STEP, IS_GROUP_FIRST, IS_GROUP_LAST = 40, 41, 42, 43


class IterateBuilder(DeriveBuilder):
    """A ``DeriveBuilder`` whose program is walked down each group of rows with carried registers.  Nothing is checked
    here: ``iterate_check`` (or the call that runs the program) is the judge."""

    def __init__(self, src_width: int, reset_column=None, max_group_rows: int = 1024):
        super().__init__(src_width)
        self.reset_column = NO_RESET if reset_column is None else int(reset_column)
        self.max_group_rows = int(max_group_rows)
        self.carries: list[list[int]] = []  # [node or None, init]

    def carry(self, init: int = 0) -> DeriveExpr:
        """A new carry: the expression reads its value from BEFORE this row -- ``init`` on a group's first row, else
        what ``set_carry`` gave it on the previous row.  Each call to ``carry`` makes one register."""
        self.carries.append([None, int(init) % P])
        e = self._node(CARRY, len(self.carries) - 1, 0)
        e.carry = len(self.carries) - 1
        return e

    def set_carry(self, carry: DeriveExpr, expr) -> None:
        """After a row the carry holds ``expr`` of that row."""
        if getattr(carry, "carry", None) is None or carry.b is not self:
            raise ValueError("not a carry of this IterateBuilder")
        self.carries[carry.carry][0] = self._lift(expr).node

    def step(self) -> DeriveExpr: return self._node(STEP, 0, 0)
    def is_group_first(self) -> DeriveExpr: return self._node(IS_GROUP_FIRST, 0, 0)
    def is_group_last(self) -> DeriveExpr: return self._node(IS_GROUP_LAST, 0, 0)

    def tape(self) -> np.ndarray:
        words = [MAGIC, 1, self.src_width, len(self.nodes), len(self.outputs), len(self.carries), self.reset_column,
                 self.max_group_rows]
        for n in self.nodes:
            words += n
        for o in self.outputs:
            words += o
        for k, (node, init) in enumerate(self.carries):
            if node is None:
                raise ValueError(f"carry {k} was never set")
            words += [node, init]
        return np.array(words, dtype=np.uint64).astype(np.uint32)


def iterate_check(program, src_width: int) -> dict:
    """``ts_derive_check`` of a TITR program: ``n_live`` counts the carry slots, ``n_instructions`` the nodes kept."""
    return derive_check(program, src_width)


def iterate_rows_host(program, rows) -> np.ndarray:
    """``ts_derive_rows_host`` of a TITR program: what ``DeviceMatrix.upload(rows).iterate(program)`` holds."""
    return derive_rows_host(program, rows)
