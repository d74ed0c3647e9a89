"""Symbolic AIR capture -> constraint tape.

Host-side mirror of the reference's symbolic constraint capture, which is how an
``Air::eval`` body (user code) reaches the prover:

* ``SymbolicVariable`` / ``Entry``    -- reference uni-stark/src/symbolic_variable.rs:9-38
* ``SymbolicExpression``              -- reference uni-stark/src/symbolic_expression.rs:12-61
  (degree rules at :41-61, :137 add, :182 sub, :227 mul)
* ``SymbolicAirBuilder``              -- reference uni-stark/src/symbolic_builder.rs:68-148
* ``get_symbolic_constraints`` / ``get_max_constraint_degree`` / ``get_log_quotient_degree``
                                      -- reference uni-stark/src/symbolic_builder.rs:15-64
* ``FilteredAirBuilder`` (``when_first_row`` ...) -- p3-air semantics, SURVEY.md App. A.7

The DAG is serialised into the "tape" the C ABI takes (``include/tapstark.h``, TS_OP_*):
``[magic, version, width, n_public, n_nodes, n_constraints, nodes(op,a,b)..., constraint ids...]``;
an AIR with preprocessed columns (``PairBuilder::preprocessed()``, symbolic_builder.rs:144-148) gives a
version-2 tape: one more header word, ``preprocessed_width``, and the leaf ``OP_PREP(offset, column)``.
An AIR with challenge-phase columns (columns that depend on verifier challenges drawn after the main trace is
committed: LogUp and its relatives; build-defined, the reference has one phase) gives a version-3 tape: a
10-word header ``[..., preprocessed_width, aux_width, n_challenges, n_exposed]`` and the leaves
``OP_AUX(offset, column)``, ``OP_CHALLENGE(word)``, ``OP_EXPOSED(index)``.  ``ExtExpr`` writes extension-valued
constraints as four base constraints; ``LogUp`` emits the LogUp constraints from an interaction spec.
Python is only the capture front-end; the tape is evaluated by HIP kernels.
"""
from __future__ import annotations

import numpy as np

P = 0x78000001  # reference basic/src/field/mod.rs:45

TAPE_MAGIC = 0x54415354
OP_CONST, OP_MAIN, OP_PUBLIC, OP_IS_FIRST, OP_IS_LAST, OP_IS_TRANSITION = 0, 1, 2, 3, 4, 5
OP_ADD, OP_SUB, OP_NEG, OP_MUL = 6, 7, 8, 9
OP_PREP = 10  # version-2 tapes: Entry::Preprocessed { offset }, symbolic_variable.rs:9-15
OP_AUX, OP_CHALLENGE, OP_EXPOSED = 11, 12, 13  # version-3 tapes (include/tapstark.h)
EF_W = 11  # EF4 = F[x] / (x^4 - 11)


class SymbolicExpression:
    """Node of the constraint DAG (hash-consed per builder so shared sub-expressions are
    emitted once, like the reference's ``Rc`` sharing)."""

    __slots__ = ("b", "id", "degree_multiple")

    def __init__(self, b: "SymbolicAirBuilder", node_id: int, degree_multiple: int):
        self.b = b
        self.id = node_id
        self.degree_multiple = degree_multiple

    def _lift(self, other) -> "SymbolicExpression":
        if isinstance(other, SymbolicExpression):
            return other
        return self.b.constant(int(other))

    def __add__(self, o):
        o = self._lift(o)
        return self.b._node(OP_ADD, self.id, o.id, max(self.degree_multiple, o.degree_multiple))

    __radd__ = lambda self, o: self._lift(o).__add__(self)

    def __sub__(self, o):
        o = self._lift(o)
        return self.b._node(OP_SUB, self.id, o.id, max(self.degree_multiple, o.degree_multiple))

    def __rsub__(self, o):
        return self._lift(o).__sub__(self)

    def __neg__(self):
        return self.b._node(OP_NEG, self.id, 0, self.degree_multiple)

    def __mul__(self, o):
        o = self._lift(o)
        return self.b._node(OP_MUL, self.id, o.id, self.degree_multiple + o.degree_multiple)

    __rmul__ = lambda self, o: self._lift(o).__mul__(self)


class _Row:
    def __init__(self, exprs):
        self._e = exprs

    def __getitem__(self, i):
        return self._e[i]

    def __len__(self):
        return len(self._e)

    def __iter__(self):
        return iter(self._e)


class _MainWindow:
    """``builder.main()``: two-row window; ``row_slice(0)`` = local, ``row_slice(1)`` = next."""

    def __init__(self, rows):
        self._rows = rows

    def row_slice(self, offset: int) -> _Row:
        return self._rows[offset]


class FilteredAirBuilder:
    """p3-air ``FilteredAirBuilder`` (App. A.7): ``when(c).assert_zero(x)`` => ``assert_zero(c*x)``."""

    def __init__(self, inner, condition):
        self.inner = inner
        self.condition = condition

    def assert_zero(self, x):
        self.inner.assert_zero(self.condition * x)

    def assert_eq(self, x, y):
        self.assert_zero(self.inner._lift(x) - y)

    def assert_one(self, x):
        self.assert_zero(self.inner._lift(x) - 1)

    def assert_zero_ext(self, x):
        for c in x.c:
            self.assert_zero(c)

    def when(self, c):
        return FilteredAirBuilder(self.inner, self.condition * c)


class ExtExpr:
    """An extension-field expression: four ``SymbolicExpression`` coefficients over x^4 - 11.  ``assert_zero_ext``
    emits FOUR base constraints, so an extension-valued constraint is an ordinary constraint of the tape language
    and nothing downstream learns a new accumulation rule."""

    __slots__ = ("b", "c")

    def __init__(self, b: "SymbolicAirBuilder", coeffs):
        self.b = b
        self.c = [b._lift(x) for x in coeffs]
        assert len(self.c) == 4

    @classmethod
    def from_base(cls, b, x) -> "ExtExpr":
        return cls(b, [x, 0, 0, 0])

    def _lift(self, o) -> "ExtExpr":
        return o if isinstance(o, ExtExpr) else ExtExpr.from_base(self.b, o)

    def __add__(self, o):
        o = self._lift(o)
        return ExtExpr(self.b, [x + y for x, y in zip(self.c, o.c)])

    __radd__ = __add__

    def __sub__(self, o):
        o = self._lift(o)
        return ExtExpr(self.b, [x - y for x, y in zip(self.c, o.c)])

    def __rsub__(self, o):
        return self._lift(o).__sub__(self)

    def __neg__(self):
        return ExtExpr(self.b, [-x for x in self.c])

    def mul_base(self, x) -> "ExtExpr":
        x = self.b._lift(x)
        return ExtExpr(self.b, [c * x for c in self.c])

    def __mul__(self, o):
        if not isinstance(o, ExtExpr):
            return self.mul_base(o)
        out = []
        for k in range(4):
            lo = [self.c[i] * o.c[k - i] for i in range(k + 1)]
            hi = [self.c[i] * o.c[k + 4 - i] for i in range(k + 1, 4)]
            acc = lo[0]
            for t in lo[1:]:
                acc = acc + t
            if hi:
                h = hi[0]
                for t in hi[1:]:
                    h = h + t
                acc = acc + h * EF_W
            out.append(acc)
        return ExtExpr(self.b, out)

    __rmul__ = __mul__


class SymbolicAirBuilder:
    """reference uni-stark/src/symbolic_builder.rs:68-148."""

    def __init__(self, width: int, num_public_values: int, preprocessed_width: int = 0, aux_width: int = 0,
                 n_challenges: int = 0, n_exposed: int = 0):
        self.width = width
        self.num_public_values = num_public_values
        self.preprocessed_width = preprocessed_width
        self.aux_width, self.n_challenges, self.n_exposed = aux_width, n_challenges, n_exposed
        self.nodes: list[tuple[int, int, int]] = []
        self._degs: list[int] = []
        self._cse: dict[tuple[int, int, int], int] = {}
        self.constraints: list[int] = []
        # symbolic_builder.rs:79-99: the preprocessed variables first, then main, then the public values
        # (no nodes at all for width 0: the tape of an AIR without such columns is what it always was)
        self._preprocessed = _MainWindow(
            [
                _Row([self._node(OP_PREP, off, c, 1) for c in range(preprocessed_width)])
                for off in (0, 1)
            ]
        )
        self._main = _MainWindow(
            [
                _Row([self._node(OP_MAIN, off, c, 1) for c in range(width)])
                for off in (0, 1)
            ]
        )
        self._public = [self._node(OP_PUBLIC, i, 0, 0) for i in range(num_public_values)]
        # version 3, after everything a version-1 or version-2 tape holds (no nodes at all for zero counts)
        self._aux = _MainWindow(
            [_Row([self._node(OP_AUX, off, c, 1) for c in range(aux_width)]) for off in (0, 1)]
        )
        self._challenges = [ExtExpr(self, [self._node(OP_CHALLENGE, 4 * k + j, 0, 0) for j in range(4)])
                            for k in range(n_challenges)]
        self._exposed = [self._node(OP_EXPOSED, e, 0, 0) for e in range(n_exposed)]

    # -- DAG -----------------------------------------------------------------
    def _node(self, op, a, b, deg) -> SymbolicExpression:
        key = (op, a, b)
        nid = self._cse.get(key)
        if nid is None:
            nid = len(self.nodes)
            self.nodes.append(key)
            self._degs.append(deg)
            self._cse[key] = nid
        return SymbolicExpression(self, nid, self._degs[nid])

    def _lift(self, x) -> SymbolicExpression:
        return x if isinstance(x, SymbolicExpression) else self.constant(int(x))

    def constant(self, v: int) -> SymbolicExpression:
        return self._node(OP_CONST, v % P, 0, 0)

    # -- AirBuilder surface (symbolic_builder.rs:110-139) -----------------------
    def main(self) -> _MainWindow:
        return self._main

    def preprocessed(self) -> _MainWindow:
        """PairBuilder::preprocessed (symbolic_builder.rs:144-148): two row slices, as ``main()``."""
        return self._preprocessed

    def public_values(self):
        return self._public

    def aux(self) -> _MainWindow:
        """The challenge-phase trace: two row slices, as ``main()``."""
        return self._aux

    def challenges(self):
        """One ``ExtExpr`` per challenge."""
        return self._challenges

    def exposed(self):
        """The exposed base words (wrap four in an ``ExtExpr`` for an extension value)."""
        return self._exposed

    def assert_zero_ext(self, x: "ExtExpr"):
        for c in x.c:
            self.assert_zero(c)

    def is_first_row(self):
        return self._node(OP_IS_FIRST, 0, 0, 1)  # symbolic_expression.rs:45

    def is_last_row(self):
        return self._node(OP_IS_LAST, 0, 0, 1)  # :46

    def is_transition(self):
        return self.is_transition_window(2)

    def is_transition_window(self, size: int):
        if size != 2:
            raise ValueError("uni-stark only supports a window size of 2")  # :131
        return self._node(OP_IS_TRANSITION, 0, 0, 0)  # symbolic_expression.rs:47

    def assert_zero(self, x):
        self.constraints.append(self._lift(x).id)  # symbolic_builder.rs:136-138

    def assert_eq(self, x, y):
        self.assert_zero(self._lift(x) - y)

    def assert_one(self, x):
        self.assert_zero(self._lift(x) - 1)

    def when(self, c):
        return FilteredAirBuilder(self, self._lift(c))

    def when_first_row(self):
        return self.when(self.is_first_row())

    def when_last_row(self):
        return self.when(self.is_last_row())

    def when_transition(self):
        return self.when(self.is_transition())

    # -- serialisation -----------------------------------------------------------
    def max_constraint_degree(self) -> int:
        return max((self._degs[c] for c in self.constraints), default=0)

    def tape(self) -> np.ndarray:
        words = [TAPE_MAGIC, 1, self.width, self.num_public_values, len(self.nodes),
                 len(self.constraints)]
        if self.aux_width or self.n_challenges or self.n_exposed:
            words[1] = 3
            words += [self.preprocessed_width, self.aux_width, self.n_challenges, self.n_exposed]
        elif self.preprocessed_width:
            words[1] = 2
            words.append(self.preprocessed_width)
        for op, a, b in self.nodes:
            words += [op, a, b]
        words += self.constraints
        return np.asarray(words, dtype=np.uint32)


class BaseAir:
    """p3-air ``BaseAir``: subclasses give ``width()`` and ``eval(builder)``."""

    def width(self) -> int:  # pragma: no cover - interface
        raise NotImplementedError

    def eval(self, builder) -> None:  # pragma: no cover - interface
        raise NotImplementedError


def get_symbolic_constraints(air: BaseAir, num_public_values: int, preprocessed_width: int = 0, aux_width: int = 0,
                             n_challenges: int = 0, n_exposed: int = 0) -> SymbolicAirBuilder:
    """reference uni-stark/src/symbolic_builder.rs:52-64 (returns the builder holding them)."""
    b = SymbolicAirBuilder(air.width(), num_public_values, preprocessed_width, aux_width, n_challenges, n_exposed)
    air.eval(b)
    return b


def get_max_constraint_degree(air: BaseAir, num_public_values: int, preprocessed_width: int = 0) -> int:
    return get_symbolic_constraints(air, num_public_values, preprocessed_width).max_constraint_degree()


def log2_ceil(n: int) -> int:
    return max(0, (n - 1).bit_length())


def get_log_quotient_degree(air: BaseAir, num_public_values: int, preprocessed_width: int = 0) -> int:
    """reference uni-stark/src/symbolic_builder.rs:15-32 (which takes the preprocessed width too)."""
    d = max(get_max_constraint_degree(air, num_public_values, preprocessed_width), 2)
    return log2_ceil(d - 1)


def air_tape(air: BaseAir, num_public_values: int, preprocessed_width: int = 0, aux_width: int = 0,
             n_challenges: int = 0, n_exposed: int = 0) -> np.ndarray:
    """Version 1 for preprocessed_width 0, version 2 otherwise; version 3 with aux columns, challenges or
    exposed words."""
    return get_symbolic_constraints(air, num_public_values, preprocessed_width, aux_width, n_challenges,
                                    n_exposed).tape()


def aux_dims(air) -> tuple[int, int, int]:
    """(aux_width, n_challenges, n_exposed) of an AIR class: attributes or methods of those names, 0 if absent."""
    def get(name):
        f = getattr(air, name, 0)
        return int(f() if callable(f) else f)
    return get("aux_width"), get("n_challenges"), get("n_exposed")


# ---------------------------------------------------------------------------------------------- LogUp
class LogUp:
    """LogUp over the main trace (include/tapstark.h, csrc/logup.hip).  ``interactions`` is a list of
    ``(multiplicity, [values...])``; a term is ``("const", canonical value)``, ``("col", main column)`` or
    ``("prep", preprocessed column)`` (a lookup against a fixed table; kind 2), read on the local row.  Two challenges gamma, beta; interaction i has d_i = gamma + sum_j beta^j v_ij and the fraction
    m_i / d_i; group g pairs interactions 2g and 2g+1; aux columns 4g..4g+3 hold the group's sum h_g, the last
    four the exclusive running sum phi, and the four exposed words the total S.

    ``eval(builder)`` emits the matching constraints; ``aux_source`` is the callable for ``prove(..., aux=...)``
    (``ts_logup_aux_build``); ``verify`` raises unless the exposed sum is zero."""

    n_challenges = 2
    n_exposed = 4

    def __init__(self, interactions):
        self.interactions = [(self._term(m), [self._term(v) for v in vals]) for m, vals in interactions]
        self.n_groups = (len(self.interactions) + 1) // 2
        self.aux_width = 4 * (self.n_groups + 1)

    @staticmethod
    def _term(t):
        kind, value = t
        kind = {"const": 0, "col": 1, "prep": 2}.get(kind, kind)
        return int(kind), int(value) % P if kind == 0 else int(value)

    def eval(self, builder) -> None:
        main = builder.main().row_slice(0)
        aux, aux_next = builder.aux().row_slice(0), builder.aux().row_slice(1)
        gamma, beta = builder.challenges()[:2]
        prep = builder.preprocessed().row_slice(0)
        term = lambda t: builder.constant(t[1]) if t[0] == 0 else (prep[t[1]] if t[0] == 2 else main[t[1]])
        n_pow = max(len(vals) for _, vals in self.interactions)
        beta_pow = [ExtExpr.from_base(builder, 1)]
        for _ in range(1, n_pow):
            beta_pow.append(beta_pow[-1] * beta)
        dens, mults = [], []
        for m, vals in self.interactions:
            d = gamma
            for j, v in enumerate(vals):
                d = d + beta_pow[j].mul_base(term(v))
            dens.append(d)
            mults.append(term(m))
        G = self.n_groups
        total = None
        for g in range(G):
            h = ExtExpr(builder, [aux[4 * g + k] for k in range(4)])
            a, b = 2 * g, 2 * g + 1
            if b < len(dens):  # h d_a d_b - m_a d_b - m_b d_a = 0
                builder.assert_zero_ext(h * dens[a] * dens[b] - dens[b].mul_base(mults[a]) - dens[a].mul_base(mults[b]))
            else:              # h d_a - m_a = 0
                builder.assert_zero_ext(h * dens[a] - mults[a])
            total = h if total is None else total + h
        phi = ExtExpr(builder, [aux[4 * G + k] for k in range(4)])
        phi_next = ExtExpr(builder, [aux_next[4 * G + k] for k in range(4)])
        S = ExtExpr(builder, builder.exposed()[:4])
        builder.when_first_row().assert_zero_ext(phi)
        builder.when_transition().assert_zero_ext(phi_next - phi - total)
        builder.when_last_row().assert_zero_ext(phi + total - S)

    def _spec_c(self):
        """The ``ts_logup_spec`` and the ctypes arrays it points into (keep the tuple alive over the call)."""
        from . import _lib
        its = (_lib.LogupInteractionC * len(self.interactions))()
        keep = []
        for i, (m, vals) in enumerate(self.interactions):
            arr = (_lib.LogupTermC * len(vals))(*[_lib.LogupTermC(k, v) for k, v in vals])
            keep.append(arr)
            its[i] = _lib.LogupInteractionC(_lib.LogupTermC(*m), len(vals), arr)
        import ctypes as C
        return _lib.LogupSpecC(C.sizeof(_lib.LogupSpecC), len(self.interactions), its), (its, keep)

    @property
    def reads_preprocessed(self) -> bool:
        return any(t[0] == 2 for m, vals in self.interactions for t in [m, *vals])

    def build(self, trace, challenges, preprocessed=None):
        """``ts_logup_aux_build``: (aux ``DeviceMatrix``, the four exposed words).  ``preprocessed``: the row-major
        ``DeviceMatrix`` of the table's values, for a spec with ``("prep", c)`` terms (``ts_logup_aux_build_pre``;
        not consumed)."""
        import ctypes as C
        from . import _lib
        from .stark import DeviceMatrix
        ctx = trace.ctx
        spec, keep = self._spec_c()
        ch = np.ascontiguousarray(challenges, dtype=np.uint32).reshape(-1)
        if len(ch) != 8:
            raise ValueError("LogUp takes two challenges (eight words)")
        h, exposed = C.c_void_p(), np.zeros(4, dtype=np.uint32)
        if preprocessed is not None:
            ctx.check(ctx._l.ts_logup_aux_build_pre(ctx.h, C.byref(spec), preprocessed.h, trace.h,
                                                    ch.ctypes.data_as(_lib.u32p), C.byref(h),
                                                    exposed.ctypes.data_as(_lib.u32p)))
        else:
            ctx.check(ctx._l.ts_logup_aux_build(ctx.h, C.byref(spec), trace.h, ch.ctypes.data_as(_lib.u32p), C.byref(h),
                                                exposed.ctypes.data_as(_lib.u32p)))
        del keep
        return DeviceMatrix(ctx, h), exposed

    @property
    def aux_source(self):
        return self.build

    def aux_source_with(self, preprocessed):
        """The aux source of a spec with ``("prep", c)`` terms: ``preprocessed`` is the table's row-major
        ``DeviceMatrix`` (``PreprocessedKey.values``)."""
        return lambda trace, challenges: self.build(trace, challenges, preprocessed)

    @staticmethod
    def verify(exposed) -> None:
        """The statement of a LogUp argument: the exposed sum is zero."""
        if any(int(x) != 0 for x in np.asarray(exposed).reshape(-1)):
            raise ValueError("LogUp: the exposed sum is not zero: the interactions do not balance")

    def mult_spec(self, table: int, lookups=None) -> dict:
        """The arguments of ``logup_multiplicities`` for the table-side interaction ``table`` (its multiplicity
        term must be ``("col", c)``: that c receives the result; its values are the table's tuple) and the
        interactions ``lookups`` that look it up (default: every other interaction with the same number of
        values; their multiplicity terms are the weights).  ``negate`` is 1: the filled trace balances the sum."""
        m, tuple_terms = self.interactions[table]
        if m[0] != 1:
            raise ValueError("LogUp.fill_multiplicities: the table interaction's multiplicity must be a main column")
        if lookups is None:
            lookups = [i for i, (_, vals) in enumerate(self.interactions) if i != table and len(vals) == len(tuple_terms)]
        lookups = [int(i) for i in lookups]
        if not lookups or table in lookups:
            raise ValueError("LogUp.fill_multiplicities: needs at least one lookup interaction, none of them the table")
        for i in lookups:
            if len(self.interactions[i][1]) != len(tuple_terms):
                raise ValueError(f"LogUp.fill_multiplicities: interaction {i} has another number of values than the table")
        return {"table": list(tuple_terms), "lookups": [list(self.interactions[i][1]) for i in lookups],
                "weights": [self.interactions[i][0] for i in lookups], "out_column": m[1], "negate": 1}

    def fill_multiplicities(self, trace, table: int, lookups=None, preprocessed=None, allow_missing: bool = False):
        """``ts_logup_multiplicities`` for this helper's interactions (``mult_spec``): fills the table interaction's
        multiplicity column of the resident ``trace`` in place.  Returns ``(n_missing, first_missing)``; raises
        if a lookup of non-zero weight is in no table row, unless ``allow_missing``."""
        return logup_multiplicities(trace, **self.mult_spec(table, lookups), preprocessed=preprocessed,
                                    allow_missing=allow_missing)


def logup_build_multi(logups, traces, challenges, preprocessed=None):
    """``preprocessed`` (``ts_logup_aux_build_multi_pre``): one entry per trace, the row-major ``DeviceMatrix`` of that
    table's preprocessed values (``MultiKey.values(i)``; not consumed) or None; ``("prep", c)`` terms read it.

    ``ts_logup_aux_build_multi``: the aux matrices of ``traces`` (row-major ``DeviceMatrix``, one context, not
    consumed) under ``logups`` (one :class:`LogUp` per trace, terms of kind 0 and 1) for ONE pair of challenges, in
    three launches and one copy back instead of three launches and a host wait per table.  Returns ``(list of
    aux DeviceMatrix, exposed)`` with ``exposed`` of shape (n, 4): per table what ``LogUp.build`` returns."""
    import ctypes as C
    from . import _lib
    from .stark import DeviceMatrix
    n = len(logups)
    if n == 0 or len(traces) != n:
        raise ValueError("logup_build_multi: one trace per LogUp, at least one")
    ctx = traces[0].ctx
    specs = [lg._spec_c() for lg in logups]
    spec_ptrs = (C.POINTER(_lib.LogupSpecC) * n)(*[C.pointer(sp) for sp, _ in specs])
    handles = (C.c_void_p * n)(*[t.h for t in traces])
    ch = np.ascontiguousarray(challenges, dtype=np.uint32).reshape(-1)
    if len(ch) != 8:
        raise ValueError("LogUp takes two challenges (eight words)")
    out = (C.c_void_p * n)()
    exposed = np.zeros((n, 4), dtype=np.uint32)
    if preprocessed is not None:
        if len(preprocessed) != n:
            raise ValueError("logup_build_multi: one preprocessed matrix (or None) per trace")
        pre = (C.c_void_p * n)(*[m.h if m is not None else None for m in preprocessed])
        ctx.check(ctx._l.ts_logup_aux_build_multi_pre(ctx.h, n, spec_ptrs, pre, handles, ch.ctypes.data_as(_lib.u32p),
                                                      out, exposed.ctypes.data_as(_lib.u32p)))
    else:
        ctx.check(ctx._l.ts_logup_aux_build_multi(ctx.h, n, spec_ptrs, handles, ch.ctypes.data_as(_lib.u32p), out,
                                                  exposed.ctypes.data_as(_lib.u32p)))
    del specs
    return [DeviceMatrix(ctx, C.c_void_p(h)) for h in out], exposed


class BusShare:
    """``ts_bus_share``: one table's part of the tuple a :class:`BusReport` names -- the number of its contributions,
    their multiplicity sum mod p and the least ``(row, interaction)`` among them (``first`` is None without any)."""

    __slots__ = ("count", "sum", "first")

    def __init__(self, count: int, sum_: int, first):
        self.count, self.sum, self.first = int(count), int(sum_), first

    def astuple(self):
        return (self.count, self.sum, self.first)

    def __eq__(self, other):
        return self.astuple() == (other.astuple() if isinstance(other, BusShare) else tuple(other))

    def __repr__(self):
        return f"BusShare(count={self.count}, sum={self.sum}, first={self.first})"


class BusReport:
    """``ts_bus_report`` with its shares: ``n_contributions`` (table, row, interaction) triples of non-zero
    multiplicity, ``n_tuples`` distinct zero-padded tuples among them, ``n_unbalanced`` of them whose multiplicities do
    not sum to 0 mod p.  Unbalanced: ``first`` = (table, row, interaction) of the least contribution to any such tuple,
    ``n_values`` and ``tuple`` (eight words) its tuple, ``sum`` that tuple's multiplicity sum; ``shares`` one
    :class:`BusShare` per table.  Balanced: ``first`` is None, the rest zero and every share empty."""

    __slots__ = ("n_contributions", "n_tuples", "n_unbalanced", "first", "n_values", "tuple", "sum", "shares")

    def __init__(self, n_contributions, n_tuples, n_unbalanced, first, n_values, tuple_, sum_, shares):
        self.n_contributions, self.n_tuples, self.n_unbalanced = int(n_contributions), int(n_tuples), int(n_unbalanced)
        self.first, self.n_values, self.tuple, self.sum = first, int(n_values), [int(x) for x in tuple_], int(sum_)
        self.shares = list(shares)

    @property
    def balanced(self) -> bool:
        return self.n_unbalanced == 0

    def asdict(self) -> dict:
        d = {k: getattr(self, k) for k in self.__slots__}
        d["shares"] = [s.astuple() for s in self.shares]
        return d

    def __eq__(self, other):
        return isinstance(other, BusReport) and self.asdict() == other.asdict()

    def __repr__(self):
        return f"BusReport({self.asdict()})"

    @classmethod
    def _from_c(cls, rep, shares, n: int) -> "BusReport":
        none = 0xFFFFFFFF
        first = None if rep.n_unbalanced == 0 else (int(rep.first_table), int(rep.first_row), int(rep.first_interaction))
        sh = [BusShare(s.count, s.sum, None if s.first_row == none and s.first_interaction == none
                       else (int(s.first_row), int(s.first_interaction))) for s in shares[:n]]
        return cls(rep.n_contributions, rep.n_tuples, rep.n_unbalanced, first, rep.n_values, list(rep.tuple), rep.sum, sh)


def bus_check(logups, traces, preprocessed=None) -> BusReport:
    """``ts_bus_check`` (include/tapstark.h, csrc/bus_check.hip): the exact balance of a LogUp bus from the resident
    traces, before any challenge.  ``logups``: one :class:`LogUp` per table, or None for a table that is not on the bus;
    ``traces``: the row-major ``DeviceMatrix`` of every table (not consumed; None is allowed beside a None LogUp);
    ``preprocessed``: per table the matrix its ``("prep", c)`` terms read (``MultiKey.values(i)``) or None.  A tuple is
    an interaction's values zero-padded to eight words; the bus balances iff every tuple's multiplicities sum to 0 mod
    p over all tables, rows and interactions.  Returns a :class:`BusReport`."""
    import ctypes as C
    from . import _lib
    n = len(logups)
    if len(traces) != n or (preprocessed is not None and len(preprocessed) != n):
        raise ValueError("bus_check: one trace (and one preprocessed matrix or None) per LogUp")
    ctx = next((t.ctx for t in traces if t is not None), None)
    if ctx is None:
        raise ValueError("bus_check: no trace")
    specs = [lg._spec_c() if lg is not None else None for lg in logups]
    spec_ptrs = (C.POINTER(_lib.LogupSpecC) * max(n, 1))(*[C.pointer(sp[0]) if sp is not None else None for sp in specs])
    handles = (C.c_void_p * max(n, 1))(*[t.h if t is not None else None for t in traces])
    pre = None
    if preprocessed is not None:
        pre = (C.c_void_p * max(n, 1))(*[m.h if m is not None else None for m in preprocessed])
    rep = _lib.BusReportC(struct_size=C.sizeof(_lib.BusReportC))
    shares = (_lib.BusShareC * max(n, 1))()
    ctx.check(ctx._l.ts_bus_check(ctx.h, n, spec_ptrs, pre, handles, C.byref(rep), shares))
    del specs
    return BusReport._from_c(rep, shares, n)


def mult_bus_spec_c(table, lookers, out_column: int, negate: int = 1):
    """The ``ts_logup_mult_bus_spec`` of the arguments ``logup_multiplicities_bus`` takes, and the ctypes arrays it
    points into (keep the tuple alive while the spec is in use)."""
    import ctypes as C
    from . import _lib
    T = _lib.LogupTermC
    table = [LogUp._term(t) for t in table]
    t_arr = (T * len(table))(*[T(k, v) for k, v in table])
    l_arr = (_lib.LogupBusLookerC * max(len(lookers), 1))()
    keep = [t_arr, l_arr]
    for i, (lookups, weights) in enumerate(lookers):
        lookups = [[LogUp._term(t) for t in tup] for tup in lookups]
        weights = [LogUp._term(t) for t in weights]
        if len(weights) != len(lookups) or any(len(tup) != len(table) for tup in lookups):
            raise ValueError("logup_multiplicities_bus: one weight per lookup and one term per table value in every lookup")
        lk = (T * max(len(lookups) * len(table), 1))(*[T(k, v) for tup in lookups for k, v in tup])
        wt = (T * max(len(weights), 1))(*[T(k, v) for k, v in weights])
        keep += [lk, wt]
        l_arr[i] = _lib.LogupBusLookerC(len(lookups), 0, lk, wt)
    spec = _lib.LogupMultBusSpecC(C.sizeof(_lib.LogupMultBusSpecC), len(table), t_arr, len(lookers), int(out_column),
                                  l_arr, int(negate), 0)
    return spec, keep


def logup_multiplicities_bus(table_trace, table, lookers, out_column: int, negate: int = 1, allow_missing: bool = False,
                             table_preprocessed=None, pre: bool = False):
    """``table_preprocessed`` (or ``pre=True`` with None): ``ts_logup_multiplicities_bus_pre``, whose ``table`` terms
    may be ``("prep", c)``: column c of ``table_preprocessed``, the row-major values of the table's preprocessed
    columns (``MultiKey.values(i)``; the table trace's height, not consumed).

    ``ts_logup_multiplicities_bus`` (include/tapstark.h, csrc/logup_mult.hip): the multiplicity column of a table
    whose lookups are rows of OTHER traces.  ``table``: the table's tuple, terms over ``table_trace``'s row;
    ``lookers``: a list of ``(trace, lookups, weights)`` with ``trace`` a resident row-major ``DeviceMatrix`` of any
    height (not consumed; it may be ``table_trace``), ``lookups`` one tuple of terms per lookup and ``weights`` one
    term per lookup, over that trace's row.  Column ``out_column`` of ``table_trace`` is overwritten in HBM as
    ``logup_multiplicities`` does.  Returns ``(n_missing, (looker, row, lookup) of the least miss or None)``; with
    ``allow_missing`` false a miss raises ``TsError`` (TS_ERR_INVARIANT) instead."""
    import ctypes as C
    spec, keep = mult_bus_spec_c(table, [(lk, w) for _, lk, w in lookers], out_column, negate)
    ctx = table_trace.ctx
    handles = (C.c_void_p * max(len(lookers), 1))(*[m.h for m, _, _ in lookers])
    n_missing, first = C.c_uint64(0), (C.c_uint64 * 3)()
    if table_preprocessed is not None or pre:
        ctx.check(ctx._l.ts_logup_multiplicities_bus_pre(
            ctx.h, C.byref(spec), table_preprocessed.h if table_preprocessed is not None else None, table_trace.h,
            handles, C.byref(n_missing) if allow_missing else None, first))
    else:
        ctx.check(ctx._l.ts_logup_multiplicities_bus(ctx.h, C.byref(spec), table_trace.h, handles,
                                                     C.byref(n_missing) if allow_missing else None, first))
    del keep
    return int(n_missing.value), (tuple(int(x) for x in first) if n_missing.value else None)


def mult_spec_c(table, lookups, weights, out_column: int, negate: int = 1):
    """The ``ts_logup_mult_spec`` of the arguments ``logup_multiplicities`` takes (``LogUp.mult_spec`` makes them),
    and the ctypes arrays it points into (keep the tuple alive while the spec is in use)."""
    import ctypes as C
    from . import _lib
    T = _lib.LogupTermC
    table = [LogUp._term(t) for t in table]
    lookups = [[LogUp._term(t) for t in tup] for tup in lookups]
    weights = [LogUp._term(t) for t in weights]
    if len(weights) != len(lookups) or any(len(tup) != len(table) for tup in lookups):
        raise ValueError("logup_multiplicities: one weight per lookup and one term per table value in every lookup")
    t_arr = (T * len(table))(*[T(k, v) for k, v in table])
    l_arr = (T * (len(lookups) * len(table)))(*[T(k, v) for tup in lookups for k, v in tup])
    w_arr = (T * len(weights))(*[T(k, v) for k, v in weights])
    spec = _lib.LogupMultSpecC(C.sizeof(_lib.LogupMultSpecC), len(table), t_arr, len(lookups), l_arr, w_arr,
                               int(out_column), int(negate))
    return spec, (t_arr, l_arr, w_arr)


def logup_multiplicities(trace, table, lookups, weights, out_column: int, negate: int = 1, preprocessed=None,
                         allow_missing: bool = False):
    """``ts_logup_multiplicities`` (include/tapstark.h, csrc/logup_mult.hip) with the explicit spec: ``table`` is
    the table's tuple (a list of terms, as ``LogUp`` takes them), ``lookups`` one tuple per lookup, ``weights`` one
    term per lookup.  Column ``out_column`` of the resident row-major ``trace`` is overwritten in HBM with, on the
    lowest table row of each tuple, the field sum of the weights of the lookups that equal it (``p`` minus it with
    ``negate``), and 0 on the other rows.  ``preprocessed``: the row-major ``DeviceMatrix`` that ``("prep", c)``
    terms read.  Returns ``(n_missing, first_missing)``: the lookups of non-zero weight found in no table row and the
    least ``row * len(lookups) + lookup`` among them (``2**64 - 1`` when none); with ``allow_missing`` false a miss
    raises ``TsError`` (TS_ERR_INVARIANT) instead."""
    import ctypes as C
    spec, keep = mult_spec_c(table, lookups, weights, out_column, negate)
    ctx = trace.ctx
    n_missing, first = C.c_uint64(0), C.c_uint64(0)
    ctx.check(ctx._l.ts_logup_multiplicities(ctx.h, C.byref(spec), preprocessed.h if preprocessed is not None else None,
                                             trace.h, C.byref(n_missing) if allow_missing else None, C.byref(first)))
    return int(n_missing.value), int(first.value)
