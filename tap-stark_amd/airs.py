"""The AIRs named by BASELINE.json's configs, with their trace generators.

* ``FibonacciAir`` / ``generate_fibonacci_trace`` restate the reference's only live AIR,
  reference uni-stark/tests/fib_air.rs:21-78.
* ``SynthMulAir`` and ``SynthExtAir`` are BUILD-DEFINED synthetic stand-ins (SURVEY.md F5,
  section 8(d)): the reference has no "synthetic random AIR" nor a RISC0-recursion AIR.
  ``SynthMulAir``'s shape follows the commented-out reference uni-stark/tests/mul_air.rs:29-116.
"""
from __future__ import annotations

import numpy as np

from .air import BaseAir, LogUp, P

SPLITMIX_SEED = 0x7A957A12


class FibonacciAir(BaseAir):
    """reference uni-stark/tests/fib_air.rs:21-57. Public values = [a, b, x]."""

    NUM_FIBONACCI_COLS = 2

    def width(self) -> int:
        return self.NUM_FIBONACCI_COLS

    def eval(self, builder) -> None:
        main = builder.main()
        pis = builder.public_values()
        a, b, x = pis[0], pis[1], pis[2]
        local, nxt = main.row_slice(0), main.row_slice(1)
        left, right = 0, 1

        when_first_row = builder.when_first_row()
        when_first_row.assert_eq(local[left], a)
        when_first_row.assert_eq(local[right], b)

        when_transition = builder.when_transition()
        # a' <- b
        when_transition.assert_eq(local[right], nxt[left])
        # b' <- a + b
        when_transition.assert_eq(local[left] + local[right], nxt[right])

        builder.when_last_row().assert_eq(local[right], x)


def generate_fibonacci_trace(a: int, b: int, n: int) -> np.ndarray:
    """reference uni-stark/tests/fib_air.rs:59-78 -> row-major (n, 2) canonical u32."""
    assert n & (n - 1) == 0
    t = np.zeros((n, 2), dtype=np.uint32)
    l, r = a % P, b % P
    for i in range(n):
        t[i, 0], t[i, 1] = l, r
        l, r = r, (l + r) % P
    return t


def fibonacci_public_values(trace: np.ndarray) -> np.ndarray:
    """fib_air.rs:133-139: [0, 1, trace.values[len-1]] for the (0,1) start."""
    return np.array([trace[0, 0], trace[0, 1], trace[-1, 1]], dtype=np.uint32)


def splitmix64_stream(seed: int, count: int) -> np.ndarray:
    """SplitMix64, value = next() mod p."""
    mask = (1 << 64) - 1
    idx = np.arange(1, count + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) + idx * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(mask)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % np.uint64(P)).astype(np.uint32)


class SynthMulAir(BaseAir):
    """Build-defined "SynthMulAir-w": ``reps`` triples (a, b, c) + free columns up to ``w``.

    Per triple (shape from the commented reference mul_air.rs:29-116):
      * ``a*a*b - c = 0``                      (degree 3 => quotient_degree 2)
      * first row:  ``a*a + 1 = b``
      * transition: ``a + reps = a'``
    """

    def __init__(self, width: int = 64):
        self._w = width
        self.reps = width // 3

    def width(self) -> int:
        return self._w

    def eval(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        for i in range(self.reps):
            a, b, c = local[3 * i], local[3 * i + 1], local[3 * i + 2]
            builder.assert_zero(a * a * b - c)
            builder.when_first_row().assert_eq(a * a + 1, b)
            builder.when_transition().assert_eq(a + self.reps, nxt[3 * i])


def generate_synth_mul_trace(n: int, width: int = 64, seed: int = SPLITMIX_SEED) -> np.ndarray:
    """Valid trace for ``SynthMulAir(width)``: a = reps*row + k, b random (row 0: a*a+1),
    c = a*a*b, remaining columns random."""
    reps = width // 3
    free = width - 3 * reps
    rnd = splitmix64_stream(seed, n * (reps + free)).reshape(n, reps + free).astype(np.uint64)
    t = np.zeros((n, width), dtype=np.uint64)
    rows = np.arange(n, dtype=np.uint64)
    p = np.uint64(P)
    for k in range(reps):
        a = (np.uint64(reps) * rows + np.uint64(k)) % p
        b = rnd[:, k].copy()
        b[0] = (a[0] * a[0] + np.uint64(1)) % p
        c = (((a * a) % p) * b) % p
        t[:, 3 * k], t[:, 3 * k + 1], t[:, 3 * k + 2] = a, b, c
    for f in range(free):
        t[:, 3 * reps + f] = rnd[:, reps + f]
    return t.astype(np.uint32)


class HighDegreeAir(BaseAir):
    """Build-defined two-column AIR whose one constraint has degree ``degree``: ``a^(degree-1) * b = 0``
    with b = 0 (so quotient_degree = 2^ceil(log2(degree - 1)): 32 for degree 33) plus the transition
    ``a + 1 = a'``.  Exercises quotient degrees above 16 (``log_quotient_degree <= log_blowup``)."""

    def __init__(self, degree: int = 33):
        self.degree = degree

    def width(self) -> int:
        return 2

    def eval(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        acc = local[0]
        for _ in range(self.degree - 2):
            acc = acc * local[0]
        builder.assert_zero(acc * local[1])
        builder.when_transition().assert_eq(local[0] + 1, nxt[0])


def generate_high_degree_trace(n: int) -> np.ndarray:
    t = np.zeros((n, 2), dtype=np.uint32)
    t[:, 0] = (np.arange(n, dtype=np.uint64) + np.uint64(5)) % np.uint64(P)
    return t


class SynthExtAir(BaseAir):
    """Build-defined "SynthExt-w" stand-in for the RISC0-recursion-style config (SURVEY.md
    section 8(d) config 5): columns are ``groups`` triples of EF4 elements (x, y, z: 12 base
    columns per group) plus base columns; constraints ``x*y - z = 0`` in F[X]/(X^4-11)
    (4 base constraints of degree 2 per group) and a base transition on the last column.
    """

    W = 11

    def __init__(self, width: int = 163):
        self._w = width
        self.groups = (width - 1) // 12

    def width(self) -> int:
        return self._w

    def eval(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        for g in range(self.groups):
            base = 12 * g
            x = [local[base + i] for i in range(4)]
            y = [local[base + 4 + i] for i in range(4)]
            z = [local[base + 8 + i] for i in range(4)]
            for k in range(4):
                acc = None
                for i in range(4):
                    for j in range(4):
                        if (i + j) % 4 != k:
                            continue
                        term = x[i] * y[j]
                        if i + j >= 4:
                            term = term * self.W
                        acc = term if acc is None else acc + term
                builder.assert_zero(acc - z[k])
        last = self._w - 1
        builder.when_transition().assert_eq(local[last] + 1, nxt[last])


def generate_synth_ext_trace(n: int, width: int = 163, seed: int = SPLITMIX_SEED) -> np.ndarray:
    groups = (width - 1) // 12
    p = np.uint64(P)
    rnd = splitmix64_stream(seed, n * width).reshape(n, width).astype(np.uint64)
    t = rnd.copy()
    for g in range(groups):
        base = 12 * g
        x = [t[:, base + i] for i in range(4)]
        y = [t[:, base + 4 + i] for i in range(4)]
        for k in range(4):
            acc = np.zeros(n, dtype=np.uint64)
            for i in range(4):
                for j in range(4):
                    if (i + j) % 4 != k:
                        continue
                    term = (x[i] * y[j]) % p
                    if i + j >= 4:
                        term = (term * np.uint64(SynthExtAir.W)) % p
                    acc = (acc + term) % p
            t[:, base + 8 + k] = acc
    t[:, width - 1] = (np.uint64(7) + np.arange(n, dtype=np.uint64)) % p
    return t.astype(np.uint32)


# ---------------------------------------------------------------------------- random AIRs
# The reference's prove() is generic over `Air` (uni-stark/src/prover.rs:25-39): whatever an
# `Air::eval` body writes against the builder reaches the quotient evaluation through
# get_symbolic_constraints (symbolic_builder.rs:52-64).  RandomAir is a seeded family of such
# bodies for fuzzing the two constraint compilers (csrc/air.cpp, csrc/jit.cpp) and the verifier's
# ---------------------------------------------------------------------------------------------
# SelectorAir: a small hand-written AIR with preprocessed columns (BUILD-DEFINED; the reference's
# AIR language has them -- symbolic_builder.rs:144-148 -- but none of its AIRs uses one).


class SelectorAir(BaseAir):
    """Preprocessed columns (sel, rc, spare), main columns (a, b, c); public values [a_0, c_last].

    * ``sel (a b - c) + (1 - sel)(a + b + rc - c) = 0``: the row multiplies or adds, as the key says (degree 3)
    * transition ``next.a = local.c``
    * transition ``next.b = local.b + next.rc``: reads the preprocessed NEXT row
    * first row ``a = pis[0]``, last row ``c = pis[1]``

    ``spare`` is declared (committed in the key) and never referenced."""

    PREPROCESSED_WIDTH = 3

    def width(self) -> int:
        return 3

    def preprocessed_width(self) -> int:
        return self.PREPROCESSED_WIDTH

    def eval(self, builder) -> None:
        prep, main = builder.preprocessed(), builder.main()
        pis = builder.public_values()
        pl, pn = prep.row_slice(0), prep.row_slice(1)
        local, nxt = main.row_slice(0), main.row_slice(1)
        sel, rc = pl[0], pl[1]
        a, b, c = local[0], local[1], local[2]
        builder.assert_zero(sel * (a * b - c) + (1 - sel) * (a + b + rc - c))
        when_transition = builder.when_transition()
        when_transition.assert_eq(nxt[0], c)
        when_transition.assert_eq(nxt[1], b + pn[1])
        builder.when_first_row().assert_eq(a, pis[0])
        builder.when_last_row().assert_eq(c, pis[1])


def generate_selector_preprocessed(n: int, seed: int = SPLITMIX_SEED) -> np.ndarray:
    """(n, 3) canonical u32: sel in {0, 1}, rc and spare arbitrary field elements."""
    assert n & (n - 1) == 0
    s = splitmix64_stream(seed, 3 * n).reshape(n, 3)
    out = np.empty((n, 3), dtype=np.uint32)
    out[:, 0] = (s[:, 0] >> np.uint64(7)) & np.uint64(1)
    out[:, 1:] = s[:, 1:] % np.uint64(P)
    return out


def generate_selector_trace(preprocessed: np.ndarray, a0: int = 3, b0: int = 5):
    """(trace (n, 3) u32, public values [a_0, c_last]) satisfying SelectorAir over ``preprocessed``."""
    n = preprocessed.shape[0]
    t = np.zeros((n, 3), dtype=np.uint32)
    a, b = a0 % P, b0 % P
    for i in range(n):
        sel, rc = int(preprocessed[i, 0]), int(preprocessed[i, 1])
        c = (a * b) % P if sel else (a + b + rc) % P
        t[i] = (a, b, c)
        a, b = c, (b + int(preprocessed[(i + 1) % n, 1])) % P
    return t, np.array([t[0, 0], t[-1, 2]], dtype=np.uint32)


# tape evaluation against the oracle: shared sub-terms, long live ranges, selectors inside and
# outside products, public values in high-degree terms, edge constants.

class _Rng:
    """SplitMix64 (own implementation, so that a seed means the same AIR on every Python)."""

    M = (1 << 64) - 1

    def __init__(self, seed: int):
        self.s = (seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & self.M

    def next(self) -> int:
        self.s = (self.s + 0x9E3779B97F4A7C15) & self.M
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & self.M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & self.M
        return z ^ (z >> 31)

    def below(self, n: int) -> int:
        return self.next() % n

    def field(self) -> int:
        return self.next() % P


EDGE_CONSTANTS = (0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 11, 31, 1 << 27, P - (1 << 27))


class _NumExpr:
    """Value of an expression on every row of a concrete trace (numpy, canonical u64) together with
    its degree_multiple under the reference's rules (symbolic_expression.rs:41-61,137,182,227): the
    numeric twin of SymbolicExpression, used to fill the defined columns of a valid RandomAir trace."""

    __slots__ = ("b", "v", "degree_multiple")

    def __init__(self, b, v, deg):
        self.b, self.v, self.degree_multiple = b, v, deg

    def _lift(self, o):
        return o if isinstance(o, _NumExpr) else self.b.constant(int(o))

    def __add__(self, o):
        o = self._lift(o)
        return _NumExpr(self.b, (self.v + o.v) % np.uint64(P), max(self.degree_multiple, o.degree_multiple))

    __radd__ = lambda self, o: self._lift(o).__add__(self)

    def __sub__(self, o):
        o = self._lift(o)
        return _NumExpr(self.b, (self.v + np.uint64(P) - o.v) % np.uint64(P),
                        max(self.degree_multiple, o.degree_multiple))

    def __rsub__(self, o):
        return self._lift(o).__sub__(self)

    def __neg__(self):
        return _NumExpr(self.b, (np.uint64(P) - self.v) % np.uint64(P), self.degree_multiple)

    def __mul__(self, o):
        o = self._lift(o)
        return _NumExpr(self.b, (self.v * o.v) % np.uint64(P), self.degree_multiple + o.degree_multiple)

    __rmul__ = lambda self, o: self._lift(o).__mul__(self)


class NumericBuilder:
    """Builder over a concrete trace with the row semantics of check_constraints
    (uni-stark/src/check_constraints.rs:18-38: is_first = (i == 0), is_last = (i == h-1),
    is_transition = (i != h-1), next row wrapping).  `constraints` collects one value vector per
    assert_zero, so a trace can be checked in numpy; RandomAir also writes defined columns through it."""

    def __init__(self, trace: np.ndarray, public_values, define: bool = True, preprocessed=None):
        self.trace = trace  # (n, w) uint64, canonical; with define=True RandomAir fills defined columns in
        self.prep = preprocessed  # (n, P) canonical, or None: what preprocessed() reads
        self.define = define
        self.n = trace.shape[0]
        self.pis = [int(v) for v in public_values]
        self.constraints = []
        rows = np.arange(self.n)
        self._first = (rows == 0).astype(np.uint64)
        self._last = (rows == self.n - 1).astype(np.uint64)

    def _col(self, off, c):
        col = self.trace[:, c]
        return _NumExpr(self, np.roll(col, -1) if off else col.copy(), 1)

    def main(self):
        b = self

        class _W:
            def row_slice(self, off):
                class _R:
                    def __getitem__(self, c):
                        return b._col(off, c)

                    def __len__(self):
                        return b.trace.shape[1]

                return _R()

        return _W()

    def preprocessed(self):
        b = self

        class _W:
            def row_slice(self, off):
                class _R:
                    def __getitem__(self, c):
                        col = b.prep[:, c].astype(np.uint64)
                        return _NumExpr(b, np.roll(col, -1) if off else col, 1)

                    def __len__(self):
                        return b.prep.shape[1]

                return _R()

        return _W()

    def public_values(self):
        return [_NumExpr(self, np.full(self.n, v, dtype=np.uint64), 0) for v in self.pis]

    def constant(self, v):
        return _NumExpr(self, np.full(self.n, v % P, dtype=np.uint64), 0)

    def _lift(self, x):
        return x if isinstance(x, _NumExpr) else self.constant(int(x))

    def is_first_row(self):
        return _NumExpr(self, self._first.copy(), 1)

    def is_last_row(self):
        return _NumExpr(self, self._last.copy(), 1)

    def is_transition(self):
        return _NumExpr(self, np.uint64(1) - self._last, 0)

    def is_transition_window(self, size):
        assert size == 2
        return self.is_transition()

    def assert_zero(self, x):
        self.constraints.append(self._lift(x).v)

    def assert_eq(self, x, y):
        self.assert_zero(self._lift(x) - y)

    def assert_one(self, x):
        self.assert_zero(self._lift(x) - 1)

    def when(self, c):
        from .air import FilteredAirBuilder

        return FilteredAirBuilder(self, self._lift(c))

    def when_first_row(self):
        return self.when(self.is_first_row())

    def when_last_row(self):
        return self.when(self.is_last_row())

    def when_transition(self):
        return self.when(self.is_transition())

    def first_violation(self) -> int:
        """-1, or row * 65536 + constraint index of the first failure (check_constraints order)."""
        if not self.constraints:
            return -1
        bad = np.stack(self.constraints, axis=1) != 0  # (n, K)
        rows = np.flatnonzero(bad.any(axis=1))
        if len(rows) == 0:
            return -1
        r = int(rows[0])
        return r * 65536 + int(np.flatnonzero(bad[r])[0])


class RandomAir(BaseAir):
    """Seeded random AIR: ``n_constraints`` constraints of degree <= ``max_degree`` over ``width``
    columns and ``n_public`` public values.

    ``valid=False``  free-form expression DAGs (any leaf anywhere).  No trace satisfies them; the
                     quotient VALUES on a random trace are still a pure function of (tape, LDE,
                     alpha), which is what the compilers are compared on.
    ``valid=True``   structured: ``n_state`` recurrence columns (first/transition/last constraints,
                     public values = their first and last rows), free random columns, and columns
                     DEFINED as random polynomials of earlier columns (local and next row); further
                     constraints are valid ones times arbitrary expressions and multiples of
                     ``is_last * is_transition`` (= Z_H).  Selectors appear only as factors of a
                     vanishing expression, so ``generate_random_air_trace`` gives a trace the
                     reference verifier accepts.  Needs ``n_public >= 2 * n_state``.
    """

    def __init__(self, seed: int, width: int, n_constraints: int, max_degree: int, n_public: int = 3,
                 valid: bool = False, share_pct: int = 35, max_depth: int = 6):
        assert width >= 1 and n_constraints >= 1 and max_degree >= 1
        if valid:
            max_degree = max(max_degree, 2)  # is_first_row * (column - public value) is already degree 2
        self.seed, self._w, self.n_constraints, self.max_degree = seed, width, n_constraints, max_degree
        self.valid, self.share_pct, self.max_depth = valid, share_pct, max_depth
        if valid:
            r = _Rng(seed ^ 0x5EED)
            self.n_state = min(width, 1 + r.below(3))
            self.n_free = min(width - self.n_state, r.below(1 + max(1, width // 3)))
            n_public = max(n_public, 2 * self.n_state)
        self.n_public = n_public

    def width(self) -> int:
        return self._w

    # -- expression generator ---------------------------------------------------------------------
    def _setup(self, builder):
        self._rng = _Rng(self.seed)
        self._b = builder
        main = builder.main()
        self._local, self._next = main.row_slice(0), main.row_slice(1)
        self._pis = builder.public_values()
        self._pool = [[] for _ in range(self.max_degree + 1)]  # sub-terms by degree, oldest first

    def _constant(self):
        r = self._rng
        v = EDGE_CONSTANTS[r.below(len(EDGE_CONSTANTS))] if r.below(2) else r.field()
        return self._b.constant(v)

    def _leaf(self, d: int, max_col: int, selectors: bool):
        r, k = self._rng, self._rng.below(100)
        if d >= 1 and k < 70:
            if selectors and k < 12:
                return self._b.is_first_row() if k < 6 else self._b.is_last_row()
            c = r.below(max_col)
            return (self._next if r.below(3) == 0 else self._local)[c]
        if selectors is True and k < 78:
            return self._b.is_transition()
        if self._pis and k < 90:
            return self._pis[r.below(len(self._pis))]
        return self._constant()

    def _gen(self, d: int, depth: int, max_col: int, selectors: bool):
        """Expression of degree_multiple <= d over columns < max_col.  selectors: False none, True all,
        "rows" only is_first_row / is_last_row -- is_transition counts as degree 0
        (symbolic_expression.rs:47) although it is x - omega^-1, so a valid AIR may multiply it in only
        fewer than max_degree times or the quotient outgrows its qd * n coefficients."""
        r = self._rng
        k = r.below(100)
        if depth <= 0 or k < 18:
            return self._leaf(d, max_col, selectors)
        if k < 18 + self.share_pct:
            dd = r.below(d + 1)
            for deg in range(dd, -1, -1):
                pool = self._pool[deg]
                if pool:
                    # a third of the picks take one of the oldest entries: long live ranges
                    idx = r.below(min(len(pool), 4)) if r.below(3) == 0 else r.below(len(pool))
                    return pool[idx]
            return self._leaf(d, max_col, selectors)
        if k < 80 and d >= 1:
            d1 = r.below(d + 1)
            e = self._gen(d1, depth - 1, max_col, selectors) * self._gen(d - d1, depth - 1, max_col, selectors)
        elif k < 88:
            e = -self._gen(d, depth - 1, max_col, selectors)
        elif k < 94:
            e = self._gen(d, depth - 1, max_col, selectors) - self._gen(r.below(d + 1), depth - 1, max_col, selectors)
        else:
            e = self._gen(d, depth - 1, max_col, selectors) + self._gen(r.below(d + 1), depth - 1, max_col, selectors)
        if e.degree_multiple <= self.max_degree:
            self._pool[e.degree_multiple].append(e)
        return e

    def _full_degree_product(self, max_col: int):
        """Exactly max_degree main variables multiplied together."""
        r = self._rng
        e = self._local[r.below(max_col)]
        for _ in range(self.max_degree - 1):
            e = e * (self._next if r.below(4) == 0 else self._local)[r.below(max_col)]
        return e

    # -- eval ---------------------------------------------------------------------------------------
    def eval(self, builder) -> None:
        self._setup(builder)
        if self.valid:
            self._eval_valid(builder)
        else:
            self._eval_free(builder)

    def _eval_free(self, b) -> None:
        r, D, w = self._rng, self.max_degree, self._w
        for k in range(self.n_constraints):
            if k == self.n_constraints - 1:  # pins max_constraint_degree to D
                b.assert_zero(self._full_degree_product(w) - self._gen(D, 3, w, True))
                break
            d = 1 + r.below(D)
            form = r.below(8)
            g = lambda dd: self._gen(max(dd, 0), self.max_depth, w, True)
            if form == 0:
                b.when_first_row().assert_eq(g(d - 1), g(d - 1))
            elif form == 1:
                b.when_last_row().assert_zero(g(d - 1))
            elif form == 2:
                b.when_transition().assert_eq(g(d), g(d))
            elif form == 3 and d >= 2:
                b.when_first_row().when(g(1)).assert_zero(g(d - 2))
            elif form == 4:
                b.assert_one(g(d))
            elif form == 5:
                b.when(g(d // 2)).assert_eq(g(d - d // 2), r.field())
            else:
                b.assert_zero(g(d))

    def _state_step(self, c: int, local):
        """next value of state column c as an expression of the local row (degree <= 2)."""
        kind, a, k = self._state_kinds[c]
        if kind == 0 or self.max_degree < 2:
            return local[c] * a + k
        if kind == 1:
            return local[c] * local[c] + k
        return local[c] * local[(c + 1) % self.n_state] + a

    def _eval_valid(self, b) -> None:
        r, D, w, s, f = self._rng, self.max_degree, self._w, self.n_state, self.n_free
        local, nxt, pis = self._local, self._next, self._pis
        self._state_kinds = [(r.below(3), 1 + r.field() % (P - 1), r.field()) for _ in range(s)]
        zeros = []  # (expression vanishing on every row, its degree)
        n_emitted = 0

        def emit(fn):
            nonlocal n_emitted
            fn()
            n_emitted += 1

        for c in range(s):
            emit(lambda: b.when_first_row().assert_eq(local[c], pis[c]))
            step = self._state_step(c, local)
            emit(lambda: b.when_transition().assert_eq(nxt[c], step))
            emit(lambda: b.when_last_row().assert_eq(local[c], pis[s + c]))
            z = b.is_transition() * (nxt[c] - step)
            zeros.append((z, z.degree_multiple))
        for j in range(s + f, w):
            filt = r.below(5)
            budget = D - (1 if filt in (1, 2) else 0)
            if budget < 1:
                filt, budget = 0, D
            e = self._gen(budget, self.max_depth, j, False) if j > 0 else self._constant()
            self._define(b, j, e)
            z = e - local[j]
            if filt == 1:
                emit(lambda: b.when_first_row().assert_zero(z))
            elif filt == 2:
                emit(lambda: b.when_last_row().assert_eq(e, local[j]))
            elif filt == 3:
                emit(lambda: b.when_transition().assert_zero(z))
            if filt != 3 or r.below(2):
                emit(lambda: b.assert_zero(z))
            zeros.append((z, max(z.degree_multiple, 1)))
        zh = b.is_last_row() * b.is_transition()  # = Z_H(x): vanishes on the whole trace domain
        zeros.append((zh, 1))
        if self.max_degree >= 2:
            zeros.append((b.is_first_row() * b.is_last_row(), 2))  # vanishes on H for n >= 2
        pinned = False
        while n_emitted < self.n_constraints or not pinned:
            last = n_emitted >= self.n_constraints - 1
            z, dz = zeros[r.below(len(zeros))]
            if last or not pinned and r.below(8) == 0:
                # a term of full degree that still vanishes: Z_H * (D-1 variables)
                if D >= 2:
                    e = zh
                    for _ in range(D - 1):
                        e = e * (nxt if r.below(4) == 0 else local)[r.below(w)]
                    emit(lambda: b.assert_zero(e + z * self._gen(max(D - dz, 0), 3, w, "rows")
                                               if dz <= D else e))
                else:
                    emit(lambda: b.assert_zero(zh))
                pinned = True
                continue
            if dz > D:
                continue
            g = self._gen(D - dz, self.max_depth, w, "rows")
            emit(lambda: b.assert_zero(z * g if r.below(2) else g * z))

    def _define(self, b, j: int, e) -> None:
        if isinstance(b, NumericBuilder) and b.define:
            b.trace[:, j] = e.v


def generate_random_air_trace(air: RandomAir, n: int, seed: int | None = None):
    """(trace, public_values) satisfying ``air`` (``valid=True``) on n >= 2 rows."""
    assert air.valid and n >= 2 and n & (n - 1) == 0
    r = _Rng((air.seed if seed is None else seed) ^ 0x7ACE)
    w, s, f = air.width(), air.n_state, air.n_free
    t = np.zeros((n, w), dtype=np.uint64)
    if f:
        t[:, s:s + f] = splitmix64_stream(r.next() & 0xFFFFFFFF, n * f).reshape(n, f)
    pis = [r.field() for _ in range(air.n_public)]
    # state recurrences, row by row (Python ints).  _state_kinds is a function of the seed: take it
    # from a dry symbolic run.
    from .air import SymbolicAirBuilder

    air.eval(SymbolicAirBuilder(w, air.n_public))
    kinds = list(air._state_kinds)
    cur = [pis[c] for c in range(s)]
    for i in range(n):
        t[i, :s] = cur
        nx = []
        for c in range(s):
            kind, a, k = kinds[c]
            if kind == 0 or air.max_degree < 2:
                nx.append((cur[c] * a + k) % P)
            elif kind == 1:
                nx.append((cur[c] * cur[c] + k) % P)
            else:
                nx.append((cur[c] * cur[(c + 1) % s] + a) % P)
        cur = nx
    for c in range(s):
        pis[s + c] = int(t[n - 1, c])
    nb = NumericBuilder(t, pis)
    air.eval(nb)  # fills the defined columns in order
    return t.astype(np.uint32), np.asarray(pis, dtype=np.uint32), nb


def random_air_case(seed: int):
    """The fuzz campaign's case table: seed -> (air, log_n).  Degrees 1..9 (quotient degree 1, 2, 4,
    8), widths 1..200, 1..3000 constraints; every third case is a valid-trace AIR."""
    r = _Rng(seed ^ 0xF022)
    D = (1, 2, 2, 3, 3, 3, 4, 5, 5, 6, 7, 8, 9, 9)[r.below(14)]
    size = r.below(100)
    if size < 60:
        width, nc = 1 + r.below(12), 1 + r.below(24)
    elif size < 90:
        width, nc = 1 + r.below(64), 1 + r.below(200)
    elif size < 98:
        width, nc = 1 + r.below(200), 200 + r.below(800)
    else:
        width, nc = 100 + r.below(101), 1000 + r.below(2001)
    valid = seed % 3 == 0
    air = RandomAir(seed, width, nc, D, n_public=r.below(5), valid=valid,
                    share_pct=(10, 35, 60)[r.below(3)], max_depth=3 + r.below(5))
    log_n = 1 + r.below(6) if width * nc < 20000 else 1 + r.below(3)
    return air, log_n


# ---------------------------------------------------------------------------------------------- RangeLookupAir
# An AIR with challenge-phase columns (tape version 3): a LogUp range check, the smallest member of the class
# the wide synthetic AIRs stand in for.


class RangeLookupAir(BaseAir):
    """Main columns (value, table, mult); every ``value`` lies in the table ``0 .. n-1`` (n = 2^k rows).

    * first row ``table = 0``, transition ``next.table = local.table + 1``: the table column is the row index
    * LogUp over two interactions, (+1, value) and (mult, table), where the ``mult`` column holds MINUS the number
      of rows whose value equals the row's table entry (a field element): sum 1/(gamma + value) +
      sum mult/(gamma + table) = 0 exactly when the values are a multiset of table entries with those counts.

    The aux columns, challenges and exposed sum are ``LogUp``'s (air.py); the sum being zero is the caller's to
    check after ``verify`` (``RangeLookupAir.logup.verify``)."""

    logup = LogUp([(("const", 1), [("col", 0)]), (("col", 2), [("col", 1)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return 3

    def eval(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        builder.when_first_row().assert_zero(local[1])
        builder.when_transition().assert_eq(nxt[1], local[1] + 1)
        self.logup.eval(builder)


def generate_range_lookup_trace(n: int, seed: int = SPLITMIX_SEED, outside_row: int | None = None) -> np.ndarray:
    """(n, 3) canonical u32 satisfying RangeLookupAir; ``outside_row``: that row looks up ``n``, a value outside
    the table (the proof still verifies, the exposed sum is then non-zero)."""
    assert n & (n - 1) == 0
    values = (splitmix64_stream(seed, n) % np.uint64(n)).astype(np.int64)
    if outside_row is not None:
        values[outside_row] = n
    counts = np.bincount(values[values < n], minlength=n).astype(np.int64)
    out = np.empty((n, 3), dtype=np.uint32)
    out[:, 0] = values
    out[:, 1] = np.arange(n)
    out[:, 2] = (P - counts) % P
    return out


# ---------------------------------------------------------------------------------------------- TableLookupAir
# The same range check as a real AIR states it: the table is a PREPROCESSED column, committed once in a key the
# verifier holds the root of, so nothing of the statement rests on a column the prover fills in.


class TableLookupAir(BaseAir):
    """Main columns (value, mult), one preprocessed column (table); every ``value`` is an entry of the table.

    LogUp over K = 2 interactions, (+1, value) and (mult, table): ``mult`` holds MINUS the number of rows whose
    value equals the row's table entry.  There are no other constraints: what the table holds is fixed by the
    key (``generate_lookup_table``), not by the AIR.  Proved with ``prove(..., preprocessed=key,
    aux=TableLookupAir.logup.aux_source_with(key.values))``; the sum being zero is the caller's to check."""

    logup = LogUp([(("const", 1), [("col", 0)]), (("col", 1), [("prep", 0)])])
    preprocessed_width = 1
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return 2

    def eval(self, builder) -> None:
        self.logup.eval(builder)


def generate_lookup_table(n: int) -> np.ndarray:
    """(n, 1) canonical u32: the table 0 .. n-1 of TableLookupAir's key."""
    assert n & (n - 1) == 0
    return np.arange(n, dtype=np.uint32).reshape(n, 1)


def generate_table_lookup_trace(n: int, seed: int = SPLITMIX_SEED, outside_row: int | None = None) -> np.ndarray:
    """(n, 2) canonical u32 satisfying TableLookupAir against ``generate_lookup_table(n)``: the value and
    multiplicity columns of ``generate_range_lookup_trace``."""
    t = generate_range_lookup_trace(n, seed, outside_row)
    return np.ascontiguousarray(t[:, [0, 2]])


def fill_range_lookup_multiplicities(trace, allow_missing: bool = False):
    """Fills column 2 of a resident RangeLookupAir trace (values in column 0, the table in column 1) in HBM:
    what ``generate_range_lookup_trace`` computes with ``np.bincount``.  Returns ``(n_missing, first_missing)``."""
    return RangeLookupAir.logup.fill_multiplicities(trace, table=1, allow_missing=allow_missing)


def fill_table_lookup_multiplicities(trace, table_values, allow_missing: bool = False):
    """Fills column 1 of a resident TableLookupAir trace against ``table_values``, the row-major ``DeviceMatrix``
    of the key's table (``PreprocessedKey.values``).  Returns ``(n_missing, first_missing)``."""
    return TableLookupAir.logup.fill_multiplicities(trace, table=1, preprocessed=table_values,
                                                    allow_missing=allow_missing)


# ---------------------------------------------------------------------------------------------- the bus AIRs
# Tables of a multi-table proof tied by a LogUp bus (prove_multi_bus): senders put (BUS_TAG, value) on the bus, a
# range table of another height takes each off as often as it was sent.  The tag is the constant first value that
# tells this bus from any other in the same statement.

BUS_TAG = 7


class BusSendAir(BaseAir):
    """Main columns (value_0, sel_0, ..., value_{k-1}, sel_{k-1}); every ``sel_i`` is boolean and row r sends
    (BUS_TAG, value_i) with multiplicity sel_i.  Constraint degree 3 for every k."""

    n_challenges, n_exposed = LogUp.n_challenges, LogUp.n_exposed

    def __init__(self, k: int = 1):
        self.k = int(k)
        self.logup = LogUp([(("col", 2 * i + 1), [("const", BUS_TAG), ("col", 2 * i)]) for i in range(self.k)])
        self.aux_width = self.logup.aux_width

    def width(self) -> int:
        return 2 * self.k

    def eval(self, builder) -> None:
        local = builder.main().row_slice(0)
        for i in range(self.k):
            builder.assert_zero(local[2 * i + 1] * (local[2 * i + 1] - 1))
        # implied by the line above; it puts BusSendAir(1), whose lone LogUp group is quadratic, at the constraint
        # degree 3 of every other bus AIR, so that all tables of a bus have two quotient chunks
        builder.assert_zero(local[0] * local[1] * (local[1] - 1))
        self.logup.eval(builder)


class BusRangeAir(BaseAir):
    """Main columns (table, mult): first row ``table = 0``, ``next.table = table + 1``; the row receives
    (BUS_TAG, table) with multiplicity ``mult`` = MINUS the number of times the senders sent it."""

    logup = LogUp([(("col", 1), [("const", BUS_TAG), ("col", 0)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return 2

    def eval(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        builder.when_first_row().assert_zero(local[0])
        builder.when_transition().assert_eq(nxt[0], local[0] + 1)
        # implied by the first line; constraint degree 3, as every bus AIR (see BusSendAir)
        builder.when_first_row().assert_zero(local[0] * nxt[0])
        self.logup.eval(builder)


def generate_bus_send_trace(n: int, k: int, table_height: int, seed: int = SPLITMIX_SEED) -> np.ndarray:
    """(n, 2k) canonical u32 satisfying BusSendAir(k): values below ``table_height``, selectors 0 or 1."""
    r = splitmix64_stream(seed, 2 * n * k).reshape(n, 2 * k)
    out = np.empty((n, 2 * k), dtype=np.uint32)
    out[:, 0::2] = (r[:, 0::2] % np.uint64(table_height)).astype(np.uint32)
    out[:, 1::2] = ((r[:, 1::2] >> np.uint64(17)) & np.uint64(1)).astype(np.uint32)
    return out


def generate_bus_range_trace(n: int, sender_traces) -> np.ndarray:
    """(n, 2) canonical u32 satisfying BusRangeAir: the table 0 .. n-1 and MINUS the count of every entry among
    the selected values of ``sender_traces`` (values outside the table are not counted: the bus then does not
    balance)."""
    counts = np.zeros(n, dtype=np.int64)
    for t in sender_traces:
        t = np.asarray(t)
        vals = t[:, 0::2][t[:, 1::2] == 1].astype(np.int64)
        counts += np.bincount(vals[vals < n], minlength=n)
    out = np.empty((n, 2), dtype=np.uint32)
    out[:, 0] = np.arange(n)
    out[:, 1] = (P - counts % P) % P
    return out


def fill_bus_range_multiplicities(range_trace, sender_traces, allow_missing: bool = False):
    """Fills column 1 of a resident BusRangeAir trace in HBM from the resident BusSendAir traces (any heights, any
    k): what ``generate_bus_range_trace`` computes on the host.  Returns what ``logup_multiplicities_bus`` returns."""
    from .air import logup_multiplicities_bus
    lookers = []
    for m in sender_traces:
        k = m.dims()[1] // 2
        lookers.append((m, [[("col", 2 * i)] for i in range(k)], [("col", 2 * i + 1) for i in range(k)]))
    return logup_multiplicities_bus(range_trace, [("col", 0)], lookers, out_column=1, negate=1,
                                    allow_missing=allow_missing)


# ---------------------------------------------------------------------------------------------- fixed tables on the bus
# Tables of a multi-table proof against a commit-once key (prove_multi_key): what a table holds is fixed by the
# key's preprocessed columns, not by a constraint, so it need not be an arithmetic progression.


class BusKeyTableAir(BaseAir):
    """Preprocessed columns v_0 .. v_{n_values-1} (a matrix of the key), one main column ``mult``: the row receives
    (tag, v_0, ..., v_{n_values-1}) with multiplicity ``mult`` = MINUS the number of times the senders sent it.  No
    other constraint: the key fixes the contents.  One LogUp group over one interaction: constraint degree 2, one
    quotient chunk at every blowup (no padding is needed to fit log_blowup 1)."""

    n_challenges, n_exposed = LogUp.n_challenges, LogUp.n_exposed

    def __init__(self, tag: int = BUS_TAG, n_values: int = 1):
        self.tag, self.n_values = int(tag), int(n_values)
        self.preprocessed_width = self.n_values
        self.logup = LogUp([(("col", 0), [("const", self.tag)] + [("prep", j) for j in range(self.n_values)])])
        self.aux_width = self.logup.aux_width

    def width(self) -> int:
        return 1

    def eval(self, builder) -> None:
        self.logup.eval(builder)


class BusTupleSendAir(BaseAir):
    """Main columns (v_{0,0}, ..., v_{0,n_values-1}, sel_0, ..., v_{k-1,*}, sel_{k-1}): every ``sel_i`` is boolean and
    row r sends (tag, v_{i,0}, ..., v_{i,n_values-1}) with multiplicity sel_i.  Constraint degree 2 for k = 1 (one
    quotient chunk) and 3 for k >= 2 (two chunks); both fit log_blowup 1 unpadded."""

    n_challenges, n_exposed = LogUp.n_challenges, LogUp.n_exposed

    def __init__(self, tag: int, k: int = 1, n_values: int = 3):
        self.tag, self.k, self.n_values = int(tag), int(k), int(n_values)
        s = self.n_values + 1
        self.logup = LogUp([(("col", s * i + self.n_values),
                             [("const", self.tag)] + [("col", s * i + j) for j in range(self.n_values)])
                            for i in range(self.k)])
        self.aux_width = self.logup.aux_width

    def width(self) -> int:
        return self.k * (self.n_values + 1)

    def eval(self, builder) -> None:
        local = builder.main().row_slice(0)
        s = self.n_values + 1
        for i in range(self.k):
            sel = local[s * i + self.n_values]
            builder.assert_zero(sel * (sel - 1))
        self.logup.eval(builder)


def generate_range_key(n: int) -> np.ndarray:
    """(n, 1) canonical u32: the key matrix 0 .. n-1 of a ``BusKeyTableAir(tag, 1)``."""
    return generate_lookup_table(n)


def generate_xor_key(bits: int) -> np.ndarray:
    """(4^bits, 3) canonical u32: the rows (a, b, a xor b) over ``bits``-bit operands, row a * 2^bits + b."""
    a, b = np.divmod(np.arange(1 << (2 * bits), dtype=np.uint32), np.uint32(1 << bits))
    return np.ascontiguousarray(np.stack([a, b, a ^ b], axis=1).astype(np.uint32))


def generate_xor_send_trace(n: int, k: int, bits: int, seed: int = SPLITMIX_SEED) -> np.ndarray:
    """(n, 4k) canonical u32 satisfying ``BusTupleSendAir(tag, k, 3)``: tuples (a, b, a xor b) over ``bits``-bit
    operands, selectors 0 or 1."""
    r = splitmix64_stream(seed, 3 * n * k).reshape(n, k, 3).astype(np.uint64)
    out = np.empty((n, k, 4), dtype=np.uint32)
    a, b = r[:, :, 0] % np.uint64(1 << bits), r[:, :, 1] % np.uint64(1 << bits)
    out[:, :, 0], out[:, :, 1], out[:, :, 2] = a, b, a ^ b
    out[:, :, 3] = (r[:, :, 2] >> np.uint64(17)) & np.uint64(1)
    return np.ascontiguousarray(out.reshape(n, 4 * k))


def generate_key_table_trace(key_values: np.ndarray, sender_tuples) -> np.ndarray:
    """(n, 1) canonical u32 satisfying a ``BusKeyTableAir``: MINUS the count of every row of ``key_values`` among
    ``sender_tuples``, an (m, n_values) array of the selected tuples (the first row of a duplicate table entry counts;
    tuples outside the table are not counted: the bus then does not balance)."""
    key_values = np.asarray(key_values)
    n = key_values.shape[0]
    first = {}
    for r in range(n):
        first.setdefault(tuple(int(x) for x in key_values[r]), r)
    counts = np.zeros(n, dtype=np.int64)
    for tup in np.asarray(sender_tuples).reshape(-1, key_values.shape[1]):
        r = first.get(tuple(int(x) for x in tup))
        if r is not None:
            counts[r] += 1
    return ((P - counts % P) % P).astype(np.uint32).reshape(n, 1)


def selected_tuples(trace: np.ndarray, n_values: int) -> np.ndarray:
    """The (m, n_values) tuples a ``BusSendAir`` (n_values = 1) or ``BusTupleSendAir`` trace sends: those whose
    selector is 1."""
    t = np.asarray(trace).reshape(trace.shape[0], -1, n_values + 1)
    return t[:, :, :n_values][t[:, :, n_values] == 1]


def fill_bus_key_multiplicities(table_trace, key_values, sender_traces, n_values: int = 1, allow_missing: bool = False):
    """Fills column 0 of a resident ``BusKeyTableAir`` trace in HBM from the resident sender traces (``BusSendAir`` for
    n_values = 1, ``BusTupleSendAir`` otherwise; any heights, any k) against ``key_values``, the row-major
    ``DeviceMatrix`` of the table's key matrix (``MultiKey.values(i)``): what ``generate_key_table_trace`` computes on
    the host.  Returns what ``logup_multiplicities_bus`` returns."""
    from .air import logup_multiplicities_bus
    s = n_values + 1
    lookers = []
    for m in sender_traces:
        k = m.dims()[1] // s
        lookers.append((m, [[("col", s * i + j) for j in range(n_values)] for i in range(k)],
                        [("col", s * i + n_values) for i in range(k)]))
    return logup_multiplicities_bus(table_trace, [("prep", j) for j in range(n_values)], lookers, out_column=0, negate=1,
                                    allow_missing=allow_missing, table_preprocessed=key_values)


# ---------------------------------------------------------------------------------------------- a memory table on the bus
# Two tables of a multi-table proof that hold the same accesses in two orders: MemoryAccessAir in execution order,
# MemoryTableAir sorted by (addr, clk) -- made in HBM with ``DeviceMatrix.sort_rows`` -- where "a read returns the last
# write" is a constraint between neighbouring rows.  The bus ties the two; a range check of ``gap`` (an existing
# BusRangeAir) is what makes "sorted" a proved statement.

MEM_TAG = 11


class MemoryAccessAir(BaseAir):
    """Main columns (addr, clk, value, is_write, sel): ``sel`` and ``is_write`` boolean, first row ``clk = 0``,
    ``next.clk = clk + 1``; the row sends (MEM_TAG, addr, clk, value, is_write) with multiplicity ``sel``
    (BusTupleSendAir's interaction with the clock pinned).  Constraint degree 3."""

    ADDR, CLK, VALUE, IS_WRITE, SEL = range(5)
    logup = LogUp([(("col", 4), [("const", MEM_TAG), ("col", 0), ("col", 1), ("col", 2), ("col", 3)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return 5

    def eval_main(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        sel, is_write = local[self.SEL], local[self.IS_WRITE]
        builder.assert_zero(sel * (sel - 1))
        builder.assert_zero(is_write * (is_write - 1))
        builder.when_first_row().assert_zero(local[self.CLK])
        builder.when_transition().assert_eq(nxt[self.CLK], local[self.CLK] + 1)
        # implied by the first line; constraint degree 3, as every bus AIR (see BusSendAir)
        builder.assert_zero(local[self.ADDR] * sel * (sel - 1))

    def eval(self, builder) -> None:
        self.eval_main(builder)
        self.logup.eval(builder)


class MemoryTableAir(BaseAir):
    """Main columns (addr, clk, value, is_write, live, recv, gap, start): the accesses sorted by (addr, clk), the live
    rows first.  ``start`` is the group-start column ``sort_rows`` appends (the first access of an address), which is
    why it stands last; ``live``, ``recv`` and ``gap`` are the caller's.  With ``cont = live - start``:

    * ``live``, ``start``, ``is_write`` boolean; ``start (1 - live) = 0``; ``recv + live = 0``; first row ``cont = 0``;
    * dead rows stay dead: ``(1 - live) next.live = 0`` on transitions;
    * on transitions ``next.cont (next.addr - addr) = 0``; a read returns the last value:
      ``next.cont (1 - next.is_write) (next.value - value) = 0``;
    * the first access of an address is a write: ``start (1 - is_write) = 0``;
    * on transitions ``next.start (next.addr - addr - 1 - next.gap) + next.cont (next.clk - clk - 1 - next.gap) = 0``.

    The row receives (MEM_TAG, addr, clk, value, is_write) with multiplicity ``recv`` and sends (BUS_TAG, gap) with
    multiplicity ``live`` to a BusRangeAir: addresses strictly ascend from group to group and clocks inside a group
    because every ``gap`` is in the range table.  Constraint degree 3."""

    ADDR, CLK, VALUE, IS_WRITE, LIVE, RECV, GAP, START = range(8)
    logup = LogUp([(("col", 5), [("const", MEM_TAG), ("col", 0), ("col", 1), ("col", 2), ("col", 3)]),
                   (("col", 4), [("const", BUS_TAG), ("col", 6)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return 8

    def eval_main(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        live, start, is_write = local[self.LIVE], local[self.START], local[self.IS_WRITE]
        cont_next = nxt[self.LIVE] - nxt[self.START]
        for b in (live, start, is_write):
            builder.assert_zero(b * (b - 1))
        builder.assert_zero(start * (1 - live))
        builder.assert_zero(local[self.RECV] + live)
        builder.when_first_row().assert_zero(live - start)
        builder.assert_zero(start * (1 - is_write))
        t = builder.when_transition()
        t.assert_zero((1 - live) * nxt[self.LIVE])
        t.assert_zero(cont_next * (nxt[self.ADDR] - local[self.ADDR]))
        t.assert_zero(cont_next * (1 - nxt[self.IS_WRITE]) * (nxt[self.VALUE] - local[self.VALUE]))
        t.assert_zero(nxt[self.START] * (nxt[self.ADDR] - local[self.ADDR] - 1 - nxt[self.GAP])
                      + cont_next * (nxt[self.CLK] - local[self.CLK] - 1 - nxt[self.GAP]))

    def eval(self, builder) -> None:
        self.eval_main(builder)
        self.logup.eval(builder)


def generate_memory_accesses(n: int, n_addr: int, seed: int = SPLITMIX_SEED, n_selected: int | None = None) -> np.ndarray:
    """(n, 5) canonical u32 satisfying MemoryAccessAir: a simulated memory over ``n_addr`` addresses driven by a
    SplitMix64 stream.  Row r is the access at clock r; a read returns the last value written to its address and the
    first access of every address is a write.  The first ``n_selected`` rows (default: all) have ``sel = 1``; the
    others are padding that is not sent."""
    n_selected = n if n_selected is None else n_selected
    r = splitmix64_stream(seed, 3 * n).reshape(n, 3).astype(np.uint64)
    out = np.zeros((n, 5), dtype=np.uint32)
    out[:, 1] = np.arange(n)
    memory = {}
    for i in range(n):
        addr = int(r[i, 0] % np.uint64(n_addr))
        write = bool((int(r[i, 1]) >> 17) & 1) or addr not in memory
        if write and i < n_selected:
            memory[addr] = int(r[i, 2])
        out[i, 0], out[i, 3] = addr, write
        out[i, 2] = int(r[i, 2]) if write else memory[addr]
        out[i, 4] = i < n_selected
    return out


def memory_table_source(accesses: np.ndarray) -> tuple[np.ndarray, int]:
    """((n, 7) canonical u32, n_live): what ``sort_rows(keys=[0, 1], group_keys=1, n_live=n_live, group_start=True)``
    turns into a MemoryTableAir trace but for ``gap``: columns (addr, clk, value, is_write, live, recv, gap = 0) of the
    accesses, whose selected rows must come first."""
    a = np.asarray(accesses, dtype=np.uint32)
    sel = a[:, 4].astype(np.int64)
    n_live = int(sel.sum())
    if not (sel[:n_live] == 1).all():
        raise ValueError("memory_table_source: the selected accesses must be the first rows")
    out = np.zeros((a.shape[0], 7), dtype=np.uint32)
    out[:, :4] = a[:, :4]
    out[:, 4] = sel
    out[:, 5] = (P - sel) % P
    return out, n_live


def fill_memory_gaps(table: np.ndarray) -> np.ndarray:
    """The downloaded sorted table with ``gap`` filled on the host (``memory_gap_program`` is the same column computed
    in HBM): on live row i >= 1 the address step minus one where a group starts, the clock step minus one inside a
    group, mod p; 0 on row 0 and on dead rows.  A table that is not sorted gets a gap near p, outside any range table."""
    t = np.array(table, dtype=np.uint32)
    A = MemoryTableAir
    cur, prev = t[1:].astype(np.int64), t[:-1].astype(np.int64)
    step = np.where(cur[:, A.START] == 1, cur[:, A.ADDR] - prev[:, A.ADDR], cur[:, A.CLK] - prev[:, A.CLK]) - 1
    t[:, A.GAP] = 0
    t[1:, A.GAP] = np.where(cur[:, A.LIVE] == 1, step % P, 0)
    return t


def memory_table_source_program():
    """``memory_table_source`` as a row program for ``DeviceMatrix.derive``: the (n, 5) accesses become (n, 7) -- columns
    0 to 4 copied (``sel`` is ``live``), 5 = ``recv`` = -live, 6 = ``gap`` = 0.  ``n_live`` stays the caller's to know."""
    from .derive import DeriveBuilder
    b = DeriveBuilder(5)
    b.output(-b.col(4), 5)
    b.output(b.constant(0), 6)
    return b


def memory_gap_program():
    """``fill_memory_gaps`` as a row program over the sorted (n, 8) table: column 6 = ``live (1 - is_first_row)
    (start (addr - prev addr) + (1 - start) (clk - prev clk) - 1)``."""
    from .derive import DeriveBuilder
    A = MemoryTableAir
    b = DeriveBuilder(8)
    start = b.col(A.START)
    step = start * (b.col(A.ADDR) - b.prev(A.ADDR)) + (1 - start) * (b.col(A.CLK) - b.prev(A.CLK)) - 1
    b.output(b.col(A.LIVE) * (1 - b.is_first_row()) * step, A.GAP)
    return b


def memory_table_unfilled_source_program():
    """``memory_table_source_program`` for a table whose read values are still to be found: the same (n, 7) columns, but
    ``value`` = ``is_write * value``, 0 on every read.  After the sort, ``memory_fill_helper_program`` and
    ``memory_fill_scan`` put the read values back in HBM."""
    b = memory_table_source_program()
    b.output(b.col(MemoryAccessAir.IS_WRITE) * b.col(MemoryAccessAir.VALUE), MemoryAccessAir.VALUE)
    return b


def memory_fill_helper_program():
    """The two columns ``memory_fill_scan`` reads, appended to the sorted (n, 8) table: 8 = ``a`` = ``live (1 -
    is_write)``, 9 = ``b`` = ``is_write * value``.  A live read carries the value before it; a write, and every dead row,
    keeps its own."""
    from .derive import DeriveBuilder
    A = MemoryTableAir
    b = DeriveBuilder(8)
    is_write = b.col(A.IS_WRITE)
    b.output(b.col(A.LIVE) * (1 - is_write), 8)
    b.output(is_write * b.col(A.VALUE), 9)
    return b


def memory_fill_scan():
    """The value every read returns -- the last value written to its address -- as one scan over the (n, 10) matrix of
    ``memory_fill_helper_program``: ``value[i] = a[i] value[i-1] + b[i]``, started over from 0 where ``start`` is 1 (the
    first access of an address).  The result is the (n, 8) table again: the helper columns are dropped."""
    from .scan import ScanSpec, col
    A = MemoryTableAir
    return ScanSpec(out_width=8).add(A.VALUE, a=col(8), b=col(9), init=0, reset=A.START)


def generate_memory_table(accesses: np.ndarray) -> np.ndarray:
    """(n, 8) canonical u32 satisfying MemoryTableAir, all on the host (``np.lexsort``): what the device route --
    ``memory_table_source``, ``sort_rows``, ``fill_memory_gaps`` -- gives."""
    src, n_live = memory_table_source(accesses)
    order = np.arange(src.shape[0])
    order[:n_live] = np.lexsort((src[:n_live, 1], src[:n_live, 0]))
    t = np.zeros((src.shape[0], 8), dtype=np.uint32)
    t[:, :7] = src[order]
    t[0, 7] = n_live > 0
    if n_live > 1:
        t[1:n_live, 7] = t[1:n_live, 0] != t[:n_live - 1, 0]
    return fill_memory_gaps(t)


class MemoryCpuAir(BaseAir):
    """A machine's side of the memory bus: one row per step, two access slots per row, each conditional.  Main columns
    (clk, ts_a, addr_a, val_a, sel_a, ts_b, addr_b, val_b, wr_b, sel_b): first row ``clk = 0``, ``next.clk = clk + 1``,
    ``ts_a = 2 clk``, ``ts_b = 2 clk + 1``, ``sel_a``, ``sel_b`` and ``wr_b`` boolean.  Slot a is a read: the row sends
    (MEM_TAG, addr_a, ts_a, val_a, 0) with multiplicity ``sel_a``; slot b a read or a write: (MEM_TAG, addr_b, ts_b,
    val_b, wr_b) with multiplicity ``sel_b``.  The receiving MemoryTableAir trace is made from this one in HBM:
    ``collect_rows`` with ``memory_cpu_collect_spec`` stacks the selected slots as an access table, and from there the
    route of the access table is taken unchanged.  Constraint degree 3."""

    CLK, TS_A, ADDR_A, VAL_A, SEL_A, TS_B, ADDR_B, VAL_B, WR_B, SEL_B = range(10)
    WIDTH = 10
    logup = LogUp([(("col", 4), [("const", MEM_TAG), ("col", 2), ("col", 1), ("col", 3), ("const", 0)]),
                   (("col", 9), [("const", MEM_TAG), ("col", 6), ("col", 5), ("col", 7), ("col", 8)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return self.WIDTH

    def eval_main(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        for c in (self.SEL_A, self.SEL_B, self.WR_B):
            builder.assert_zero(local[c] * (local[c] - 1))
        builder.when_first_row().assert_zero(local[self.CLK])
        builder.when_transition().assert_eq(nxt[self.CLK], local[self.CLK] + 1)
        builder.assert_eq(local[self.TS_A], local[self.CLK] * 2)
        builder.assert_eq(local[self.TS_B], local[self.CLK] * 2 + 1)

    def eval(self, builder) -> None:
        self.eval_main(builder)
        self.logup.eval(builder)


def generate_memory_cpu_trace(n: int, n_addr: int, seed: int = SPLITMIX_SEED) -> np.ndarray:
    """(n, 10) canonical u32 satisfying MemoryCpuAir: a simulated memory over ``n_addr`` addresses driven by a
    SplitMix64 stream.  On row r slot b comes after slot a (``ts_b = ts_a + 1``).  Slot a is a read of an address that
    has been written, selected on some rows only (never before the first write); slot b is a read or a write, selected
    on some rows only, and the first access of every address is a write, as in ``generate_memory_accesses``.  An
    unselected slot holds an address and a value all the same: they are not sent."""
    A = MemoryCpuAir
    r = splitmix64_stream(seed, 6 * n).reshape(n, 6).astype(np.uint64)
    out = np.zeros((n, A.WIDTH), dtype=np.uint32)
    out[:, A.CLK] = np.arange(n)
    out[:, A.TS_A] = 2 * np.arange(n)
    out[:, A.TS_B] = 2 * np.arange(n) + 1
    memory = {}
    for i in range(n):
        addr_a = int(r[i, 0] % np.uint64(n_addr))
        sel_a = bool((int(r[i, 1]) >> 17) & 1) and addr_a in memory
        out[i, A.ADDR_A], out[i, A.SEL_A] = addr_a, sel_a
        out[i, A.VAL_A] = memory[addr_a] if sel_a else int(r[i, 1] % np.uint64(P))
        addr_b = int(r[i, 2] % np.uint64(n_addr))
        sel_b = bool((int(r[i, 3]) >> 17) & 3)  # three rows of four
        write = bool((int(r[i, 4]) >> 17) & 1) or addr_b not in memory
        value = int(r[i, 5] % np.uint64(P)) if write else memory[addr_b]
        if write and sel_b:
            memory[addr_b] = value
        out[i, A.ADDR_B], out[i, A.VAL_B], out[i, A.WR_B], out[i, A.SEL_B] = addr_b, value, write, sel_b
    return out


def memory_cpu_collect_spec():
    """The access table of a MemoryCpuAir trace as a spec for ``collect_rows``: slot a and slot b of every row, where
    selected, in the (addr, clk, value, is_write, sel) shape of MemoryAccessAir with ``clk`` = the slot's timestamp and
    ``sel = 1``; the pad row is all zero, so it is a dead row of the memory table.  ``n_live`` from the call is what the
    sort takes."""
    from .collect import CollectSpec, col
    A = MemoryCpuAir
    spec = CollectSpec([A.WIDTH], 5)
    spec.emit(0, when=col(A.SEL_A), terms=[col(A.ADDR_A), col(A.TS_A), col(A.VAL_A), 0, 1])
    spec.emit(0, when=col(A.SEL_B), terms=[col(A.ADDR_B), col(A.TS_B), col(A.VAL_B), col(A.WR_B), 1])
    return spec


def memory_cpu_table(ctx, cpu_trace, out_height: int = 0):
    """The MemoryTableAir trace of a resident MemoryCpuAir trace, without leaving HBM: collect the selected slots, then
    the route of an access table unchanged -- unfilled source columns, the sort with ``n_live`` from the collect, the
    helper columns, the fill scan, the gaps.  Returns (the collected access matrix, the table, n_live)."""
    from .stark import collect_rows
    T = MemoryTableAir
    d_acc, n_live = collect_rows(ctx, memory_cpu_collect_spec(), [cpu_trace], out_height)
    d_sorted = d_acc.derive(memory_table_unfilled_source_program()).sort_rows([T.ADDR, T.CLK], group_keys=1,
                                                                              n_live=n_live, group_start=True)
    d_table = d_sorted.derive(memory_fill_helper_program()).scan(memory_fill_scan()).derive(memory_gap_program())
    return d_acc, d_table, n_live


def fill_memory_range_multiplicities(range_trace, memory_table, allow_missing: bool = False):
    """Fills column 1 of a resident BusRangeAir trace in HBM from the ``gap`` column of a resident MemoryTableAir trace
    (weight ``live``).  Returns what ``logup_multiplicities_bus`` returns."""
    from .air import logup_multiplicities_bus
    A = MemoryTableAir
    return logup_multiplicities_bus(range_trace, [("col", 0)], [(memory_table, [[("col", A.GAP)]], [("col", A.LIVE)])],
                                    out_column=1, negate=1, allow_missing=allow_missing)


# ---------------------------------------------------------------------------------------------- the final state of memory
# The table a continuation hands to the next segment: one row per touched address with its final value and the clock
# of its last access.  The sorted memory table marks the last access of every address and sends it; a table of its own
# -- ONE group call over the sorted table (``group_rows``, include/tapstark.h "grouped rows") -- receives it.

FIN_TAG = 23


class MemoryTableFinalAir(MemoryTableAir):
    """MemoryTableAir with a column ``last`` behind ``start``: boolean, ``last = live (1 - next.cont)`` on transitions
    (``next.cont = next.live - next.start``: the next row goes on with this address) and ``last = live`` on the last
    row -- 1 exactly on the last access of every address.  Beside MemoryTableAir's two interactions the row sends
    (FIN_TAG, addr, clk, value) with multiplicity ``last``.  Constraint degree 3."""

    LAST = 8
    logup = LogUp(MemoryTableAir.logup.interactions + [(("col", 8), [("const", FIN_TAG), ("col", 0), ("col", 1), ("col", 2)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return 9

    def eval_main(self, builder) -> None:
        super().eval_main(builder)
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        last, live = local[self.LAST], local[self.LIVE]
        builder.assert_zero(last * (last - 1))
        builder.when_transition().assert_zero(last - live * (1 - (nxt[self.LIVE] - nxt[self.START])))
        builder.when_last_row().assert_zero(last - live)


class MemoryFinalAir(BaseAir):
    """Main columns (addr, clk, value, count, live, recv): one row per touched address -- its final value, the clock of
    its last access and the number of its accesses -- the live rows first.  ``live`` boolean, ``recv + live = 0``; the
    row receives (FIN_TAG, addr, clk, value) with multiplicity ``recv``.  That every address appears once follows from
    the bus: MemoryTableFinalAir sends one tuple per address group.  ``count`` is carried, not constrained.  Constraint
    degree 3."""

    ADDR, CLK, VALUE, COUNT, LIVE, RECV = range(6)
    logup = LogUp([(("col", 5), [("const", FIN_TAG), ("col", 0), ("col", 1), ("col", 2)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return 6

    def eval_main(self, builder) -> None:
        local = builder.main().row_slice(0)
        live = local[self.LIVE]
        builder.assert_zero(live * (live - 1))
        builder.assert_zero(local[self.RECV] + live)
        # implied by the first line; constraint degree 3, as every bus AIR (see BusSendAir)
        builder.assert_zero(local[self.ADDR] * live * (live - 1))

    def eval(self, builder) -> None:
        self.eval_main(builder)
        self.logup.eval(builder)


def memory_last_program():
    """``last`` as a row program over the sorted (n, 8) MemoryTableAir trace, appended as column 8: ``live (1 - (1 -
    is_last_row) (next.live - next.start))``, a column of its own row and the row after it."""
    from .derive import DeriveBuilder
    A = MemoryTableAir
    b = DeriveBuilder(8)
    goes_on = (1 - b.is_last_row()) * (b.next(A.LIVE) - b.next(A.START))
    b.output(b.col(A.LIVE) * (1 - goes_on), MemoryTableFinalAir.LAST)
    return b


def memory_final_group_spec():
    """The MemoryFinalAir trace as ONE group call over the sorted (n, 9) table: key ``addr``, the live rows take part;
    per address its own word, the clock and the value of its last access, the number of its accesses, ``live = 1`` and
    ``recv = p - 1``.  The pad row is all zero: a dead row."""
    from .collect import col, const
    from .group import COUNT, GroupSpec, first, last
    A = MemoryTableFinalAir
    return GroupSpec(9, 6, keys=[col(A.ADDR)], when=col(A.LIVE),
                     terms=[first(A.ADDR), last(A.CLK), last(A.VALUE), COUNT, const(1), const(P - 1)])


def generate_memory_table_final(accesses: np.ndarray) -> np.ndarray:
    """(n, 9) canonical u32 satisfying MemoryTableFinalAir, all on the host: ``generate_memory_table`` and ``last``."""
    t = generate_memory_table(accesses)
    A = MemoryTableAir
    goes_on = np.zeros(t.shape[0], dtype=np.int64)
    goes_on[:-1] = t[1:, A.LIVE].astype(np.int64) - t[1:, A.START]
    return np.concatenate([t, (t[:, A.LIVE] * (1 - goes_on)).astype(np.uint32)[:, None]], axis=1)


def generate_memory_final(table_final: np.ndarray, out_height: int = 0) -> np.ndarray:
    """(height, 6) canonical u32 satisfying MemoryFinalAir, on the host, from a MemoryTableFinalAir trace: what the group
    call of ``memory_final_group_spec`` gives."""
    A = MemoryTableFinalAir
    t = np.asarray(table_final, dtype=np.uint32)
    ends = np.flatnonzero(t[:, A.LAST] == 1)
    starts = np.flatnonzero(t[:, A.START] == 1)
    height = out_height or 1 << max(len(ends) - 1, 0).bit_length()
    out = np.zeros((height, 6), dtype=np.uint32)
    out[:len(ends), :3] = t[ends][:, [A.ADDR, A.CLK, A.VALUE]]
    out[:len(ends), 3] = ends - starts + 1
    out[:len(ends), 4] = 1
    out[:len(ends), 5] = P - 1
    return out


def memory_final_tables(ctx, accesses, n_live: int, out_height: int = 0):
    """The MemoryTableFinalAir and MemoryFinalAir traces of a resident (n, 5) access table without leaving HBM: the
    source columns, the sort, the gaps, ``last`` by one derive over the next row, then ONE group call.  ``n_live``: the
    selected accesses, which come first.  Returns (the sorted table, the final table, the number of
    touched addresses)."""
    from .stark import group_rows
    T = MemoryTableAir
    d_sorted = accesses.derive(memory_table_source_program()).sort_rows([T.ADDR, T.CLK], group_keys=1, n_live=n_live,
                                                                      group_start=True)
    d_table = d_sorted.derive(memory_gap_program()).derive(memory_last_program())
    d_final, n_addr = group_rows(ctx, memory_final_group_spec(), d_table, out_height)
    return d_table, d_final, n_addr


# ---------------------------------------------------------------------------------------------- a program ROM on the bus
# A machine trace whose rows fetch instructions from a fixed program: BusTupleSendAir(ROM_TAG, k, 3) senders of
# (pc, opcode, arg) against a BusKeyTableAir(ROM_TAG, 3) whose contents are a matrix of the key.  The producer knows
# ``pc`` and ``sel``; opcode and arg are DEFINED BY THE ROM and are fetched in HBM with ``DeviceMatrix.join_rows``.
ROM_TAG = 13


def generate_rom_key(n: int, seed: int = SPLITMIX_SEED) -> np.ndarray:
    """(n, 3) canonical u32, the key matrix of a ``BusKeyTableAir(ROM_TAG, 3)``: rows (pc, opcode, arg) with distinct,
    sparse ``pc`` values in no order (so a row number is no key), opcode < 64, arg < p."""
    r = splitmix64_stream(seed, 4 * n).reshape(n, 4).astype(np.uint64)
    order = np.argsort(r[:, 0], kind="stable").astype(np.uint64)
    out = np.empty((n, 3), dtype=np.uint32)
    out[:, 0] = np.uint64(16) * order + r[:, 1] % np.uint64(16) + np.uint64(4096)
    out[:, 1] = r[:, 2] % np.uint64(64)
    out[:, 2] = r[:, 3] % np.uint64(P)
    return out


def generate_rom_fetch_trace(n: int, k: int, key: np.ndarray, seed: int = SPLITMIX_SEED, unfilled: bool = False) -> np.ndarray:
    """(n, 4k) canonical u32 satisfying ``BusTupleSendAir(ROM_TAG, k, 3)``: slot i of a row holds (pc, opcode, arg, sel)
    with ``pc`` a ROM row's; a selected slot carries that row's opcode and arg, an unselected one zeros.  ``unfilled``:
    opcode and arg are 0 everywhere -- what a producer has before the fetch; ``rom_join_spec`` fills them."""
    key = np.asarray(key, dtype=np.uint32)
    r = splitmix64_stream(seed, 2 * n * k).reshape(n, k, 2).astype(np.uint64)
    rows = (r[:, :, 0] % np.uint64(key.shape[0])).astype(np.int64)
    sel = ((r[:, :, 1] >> np.uint64(17)) & np.uint64(1)).astype(np.uint32)
    out = np.zeros((n, k, 4), dtype=np.uint32)
    out[:, :, 0] = key[rows, 0]
    out[:, :, 3] = sel
    if not unfilled:
        out[:, :, 1] = key[rows, 1] * sel
        out[:, :, 2] = key[rows, 2] * sel
    return np.ascontiguousarray(out.reshape(n, 4 * k))


def rom_join_spec(k: int):
    """The fetch of an unfilled ``generate_rom_fetch_trace`` as ``k`` specs for ``DeviceMatrix.join_rows``, one per
    slot, to be chained (each keeps what the others wrote: ``KEEP``): slot i's ``pc`` against column 0 of the ROM's key
    matrix (``MultiKey.values``), on the rows its ``sel`` selects; opcode and arg into the slot."""
    from .join import KEEP, JoinSpec, col
    return [JoinSpec(keys=[(col(4 * i), col(0))], when=col(4 * i + 3), fetch=[(1, 4 * i + 1, 0), (2, 4 * i + 2, 0)],
                     flags=KEEP) for i in range(k)]


# ---------------------------------------------------------------------------------------------- spans on the bus
# A block instruction (memcpy or memset of ``len`` words, load or store multiple) is one row of the machine and ``len``
# rows of its chip: a table with a data-dependent number of rows per source row.  The chip's trace is made from the
# machine's in HBM with ``expand_rows``; the bus ties the two and a BusRangeAir takes every address of every span.
SPAN_TAG = 17


class SpanCallAir(BaseAir):
    """The machine's side of the span bus: one row per step.  Main columns (id, base, len, sel): first row ``id = 0``,
    ``next.id = id + 1``, ``sel`` boolean; the row sends (SPAN_TAG, id, base, len) with multiplicity ``sel``.  The
    receiving SpanChipAir trace is made from this one in HBM by ``span_chip_table``.  Constraint degree 3."""

    ID, BASE, LEN, SEL = range(4)
    WIDTH = 4
    logup = LogUp([(("col", 3), [("const", SPAN_TAG), ("col", 0), ("col", 1), ("col", 2)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return self.WIDTH

    def eval_main(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        sel = local[self.SEL]
        builder.assert_zero(sel * (sel - 1))
        builder.when_first_row().assert_zero(local[self.ID])
        builder.when_transition().assert_eq(nxt[self.ID], local[self.ID] + 1)
        # implied by the first line; constraint degree 3, as every bus AIR (see BusSendAir)
        builder.assert_zero(local[self.BASE] * sel * (sel - 1))

    def eval(self, builder) -> None:
        self.eval_main(builder)
        self.logup.eval(builder)


class SpanChipAir(BaseAir):
    """The chip of the span bus: one row per element of every selected span, the live rows first.  Main columns (id,
    base, len, j, first, last, live, addr, recv).  With ``cont' = next.live - next.first``:

    * ``first``, ``last``, ``live`` boolean; ``first (1 - live) = 0``; ``last (1 - live) = 0``; ``recv + first = 0``;
      first row ``live - first = 0``;
    * ``first j = 0``; ``last (len - 1 - j) = 0``; ``addr = base + j``;
    * on transitions: dead rows stay dead, ``(1 - live) next.live = 0``; a continued span keeps its call,
      ``cont' (next.id - id) = 0`` and the same for ``base`` and ``len``, and counts on, ``cont' (next.j - j - 1) = 0``;
      nothing continues a finished span, ``last cont' = 0``; an unfinished one is continued,
      ``live (1 - last) (1 - cont') = 0``;
    * last row ``live (1 - last) = 0``.

    The row receives (SPAN_TAG, id, base, len) with multiplicity ``recv`` -- once per span, on its first element -- and
    sends (BUS_TAG, addr) with multiplicity ``live`` to a BusRangeAir, so every address of every span lies in the range
    table.  Constraint degree 3.  It is a demonstrator of the route -- a chip whose trace ``expand_rows`` makes in HBM
    -- not a vetted chip."""

    ID, BASE, LEN, J, FIRST, LAST, LIVE, ADDR, RECV = range(9)
    WIDTH = 9
    logup = LogUp([(("col", 8), [("const", SPAN_TAG), ("col", 0), ("col", 1), ("col", 2)]),
                   (("col", 6), [("const", BUS_TAG), ("col", 7)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return self.WIDTH

    def eval_main(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        first, last, live, j = local[self.FIRST], local[self.LAST], local[self.LIVE], local[self.J]
        cont_next = nxt[self.LIVE] - nxt[self.FIRST]
        for b in (first, last, live):
            builder.assert_zero(b * (b - 1))
        builder.assert_zero(first * (1 - live))
        builder.assert_zero(last * (1 - live))
        builder.assert_zero(local[self.RECV] + first)
        builder.when_first_row().assert_zero(live - first)
        builder.assert_zero(first * j)
        builder.assert_zero(last * (local[self.LEN] - 1 - j))
        builder.assert_eq(local[self.ADDR], local[self.BASE] + j)
        t = builder.when_transition()
        t.assert_zero((1 - live) * nxt[self.LIVE])
        for c in (self.ID, self.BASE, self.LEN):
            t.assert_zero(cont_next * (nxt[c] - local[c]))
        t.assert_zero(cont_next * (nxt[self.J] - j - 1))
        t.assert_zero(last * cont_next)
        t.assert_zero(live * (1 - last) * (1 - cont_next))
        builder.when_last_row().assert_zero(live * (1 - last))

    def eval(self, builder) -> None:
        self.eval_main(builder)
        self.logup.eval(builder)


def generate_span_call_trace(n: int, max_len: int, table_height: int, seed: int = SPLITMIX_SEED) -> np.ndarray:
    """(n, 4) canonical u32 satisfying SpanCallAir, driven by a SplitMix64 stream: about half of the rows selected; a
    selected row has 1 <= len <= max_len and base + len <= table_height.  An unselected row holds a base and a length
    all the same: they are not sent and its span is not expanded."""
    assert 1 <= max_len <= table_height
    r = splitmix64_stream(seed, 3 * n).reshape(n, 3).astype(np.uint64)
    out = np.zeros((n, 4), dtype=np.uint32)
    out[:, 0] = np.arange(n)
    length = r[:, 0] % np.uint64(max_len) + np.uint64(1)
    out[:, 2] = length
    out[:, 1] = r[:, 1] % (np.uint64(table_height + 1) - length)
    out[:, 3] = (r[:, 2] >> np.uint64(17)) & np.uint64(1)
    return out


def span_expand_spec(max_len: int):
    """The element table of a SpanCallAir trace as a spec for ``expand_rows``, ONE call: a selected row asks for ``len``
    rows (id, base, len, j, first, last, live = 1, addr = base + j); the pad row is all zero, so it is a dead row of the
    chip."""
    from .expand import FIRST, J, LAST, ExpandSpec, col, stepped
    A = SpanCallAir
    return ExpandSpec(A.WIDTH, 8, count=col(A.LEN), when=col(A.SEL), max_count=max_len,
                      terms=[col(A.ID), col(A.BASE), col(A.LEN), J, FIRST, LAST, 1, stepped(A.BASE, 1)])


def span_chip_table(ctx, call_trace, out_height: int = 0, max_len: int = 1 << 27):
    """The SpanChipAir trace of a resident SpanCallAir trace, without leaving HBM: the expansion, then one ``derive``
    that appends ``recv = 0 - first``.  A selected row longer than ``max_len`` is refused and named.  Returns (the
    table, n_live)."""
    from .derive import DeriveBuilder
    from .stark import expand_rows
    d_rows, n_live = expand_rows(ctx, span_expand_spec(max_len), call_trace, out_height)
    b = DeriveBuilder(8)
    b.output(-b.col(SpanChipAir.FIRST), SpanChipAir.RECV)
    return d_rows.derive(b), n_live


def generate_span_chip_trace(call_trace: np.ndarray, out_height: int = 0) -> np.ndarray:
    """``span_chip_table`` on the host with numpy, for the comparison: (height, 9) canonical u32 satisfying
    SpanChipAir, padded with dead rows to ``out_height`` or to the least power of two that holds the elements."""
    A, T = SpanCallAir, SpanChipAir
    calls = np.asarray(call_trace, dtype=np.uint32)
    calls = calls[calls[:, A.SEL] == 1].astype(np.int64)
    cnt = calls[:, A.LEN]
    n_live = int(cnt.sum())
    height = out_height or 1 << max(n_live - 1, 0).bit_length()
    assert n_live <= height
    out = np.zeros((height, T.WIDTH), dtype=np.int64)
    live = out[:n_live]
    live[:, :3] = np.repeat(calls[:, [A.ID, A.BASE, A.LEN]], cnt, axis=0)
    live[:, T.J] = np.arange(n_live) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    live[:, T.FIRST] = live[:, T.J] == 0
    live[:, T.LAST] = live[:, T.J] == live[:, T.LEN] - 1
    live[:, T.LIVE] = 1
    live[:, T.ADDR] = (live[:, T.BASE] + live[:, T.J]) % P
    live[:, T.RECV] = (P - live[:, T.FIRST]) % P
    return out.astype(np.uint32)


def fill_span_range_multiplicities(range_trace, chip_table, allow_missing: bool = False):
    """Fills column 1 of a resident BusRangeAir trace in HBM from the ``addr`` column of a resident SpanChipAir trace
    (weight ``live``).  Returns what ``logup_multiplicities_bus`` returns."""
    from .air import logup_multiplicities_bus
    A = SpanChipAir
    return logup_multiplicities_bus(range_trace, [("col", 0)], [(chip_table, [[("col", A.ADDR)]], [("col", A.LIVE)])],
                                    out_column=1, negate=1, allow_missing=allow_missing)


# ---------------------------------------------------------------------------------------------- a sponge on the bus
# A hash call is one row of the machine and ``len`` rows of its chip, where the state after a row is a NONLINEAR function
# of the state after the row before and the word absorbed: no scan computes it.  The chip's rows are made with
# ``expand_rows``, its ``acc`` and ``state`` columns with ``DeviceMatrix.iterate`` -- one lane per call, walking its rows
# -- and each call's digest comes back into the machine's trace with ``join_rows``.
SPONGE_TAG = 19
SPONGE_IV = 0x5EED


class SpongeCallAir(BaseAir):
    """The machine's side of the sponge bus: one row per step.  Main columns (id, w0, len, sel, digest, recv): first row
    ``id = 0``, ``next.id = id + 1``, ``sel`` boolean, ``recv + sel = 0``; the row receives (SPONGE_TAG, id, digest) with
    multiplicity ``recv``.  A selected call absorbs the ``len`` words w0, w0 + 1, ...; ``sponge_chip_table`` makes the
    chip's trace from this one in HBM and ``sponge_fetch_digests`` fills ``digest`` from it.  Constraint degree 3."""

    ID, W0, LEN, SEL, DIGEST, RECV = range(6)
    WIDTH = 6
    logup = LogUp([(("col", 5), [("const", SPONGE_TAG), ("col", 0), ("col", 4)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return self.WIDTH

    def eval_main(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        sel = local[self.SEL]
        builder.assert_zero(sel * (sel - 1))
        builder.assert_zero(local[self.RECV] + sel)
        builder.when_first_row().assert_zero(local[self.ID])
        builder.when_transition().assert_eq(nxt[self.ID], local[self.ID] + 1)
        # implied by the first line; constraint degree 3, as every bus AIR (see BusSendAir)
        builder.assert_zero(local[self.W0] * sel * (sel - 1))

    def eval(self, builder) -> None:
        self.eval_main(builder)
        self.logup.eval(builder)


class SpongeChipAir(BaseAir):
    """The chip of the sponge bus: one row per absorbed word.  Main columns (first, last, id, word, acc, state):

    * ``first`` and ``last`` boolean; ``state = acc^7`` (BabyBear's S-box: gcd(7, p - 1) = 1);
    * first row ``acc = IV + word``; on transitions ``next.acc = next.first IV + (1 - next.first) state + next.word``,
      a continued call keeps its id, ``(1 - next.first) (next.id - id) = 0``, and nothing continues a finished one,
      ``last (1 - next.first) = 0``.

    On ``last`` the row sends (SPONGE_TAG, id, state).  A pad row is (1, 0, 0, 0, IV, IV^7): a call of its own that sends
    nothing.  Constraint degree 7.  It is a demonstrator of the route -- a chip whose state column ``iterate`` fills in
    HBM -- not a vetted chip."""

    FIRST, LAST, ID, WORD, ACC, STATE = range(6)
    WIDTH = 6
    logup = LogUp([(("col", 1), [("const", SPONGE_TAG), ("col", 2), ("col", 5)])])
    aux_width, n_challenges, n_exposed = logup.aux_width, logup.n_challenges, logup.n_exposed

    def width(self) -> int:
        return self.WIDTH

    def eval_main(self, builder) -> None:
        main = builder.main()
        local, nxt = main.row_slice(0), main.row_slice(1)
        first, last, acc = local[self.FIRST], local[self.LAST], local[self.ACC]
        for b in (first, last):
            builder.assert_zero(b * (b - 1))
        a2 = acc * acc
        a4 = a2 * a2
        builder.assert_eq(local[self.STATE], a4 * a2 * acc)
        builder.when_first_row().assert_eq(acc, local[self.WORD] + SPONGE_IV)
        t = builder.when_transition()
        cont = 1 - nxt[self.FIRST]
        t.assert_eq(nxt[self.ACC], nxt[self.FIRST] * SPONGE_IV + cont * local[self.STATE] + nxt[self.WORD])
        t.assert_zero(cont * (nxt[self.ID] - local[self.ID]))
        t.assert_zero(last * cont)

    def eval(self, builder) -> None:
        self.eval_main(builder)
        self.logup.eval(builder)


def generate_sponge_call_trace(n: int, max_len: int, seed: int = SPLITMIX_SEED, unfilled: bool = False) -> np.ndarray:
    """(n, 6) canonical u32 satisfying SpongeCallAir, driven by a SplitMix64 stream: about half of the rows selected,
    1 <= len <= max_len, w0 < p.  ``unfilled``: ``digest`` is 0 everywhere -- what a producer has before the chip ran."""
    r = splitmix64_stream(seed, 3 * n).reshape(n, 3).astype(np.uint64)
    A = SpongeCallAir
    out = np.zeros((n, A.WIDTH), dtype=np.uint32)
    out[:, A.ID] = np.arange(n)
    out[:, A.W0] = r[:, 0] % np.uint64(P)
    out[:, A.LEN] = r[:, 1] % np.uint64(max_len) + np.uint64(1)
    out[:, A.SEL] = (r[:, 2] >> np.uint64(17)) & np.uint64(1)
    out[:, A.RECV] = (P - out[:, A.SEL].astype(np.int64)) % P
    if not unfilled:
        for row in out:
            if row[A.SEL]:
                state = None
                for j in range(int(row[A.LEN])):
                    acc = ((SPONGE_IV if state is None else state) + int(row[A.W0]) + j) % P
                    state = pow(acc, 7, P)
                row[A.DIGEST] = state
    return out


def sponge_expand_spec(max_len: int):
    """The word table of a SpongeCallAir trace as a spec for ``expand_rows``: a selected call asks for ``len`` rows
    (first, last, id, word = w0 + j, 0, 0); the pad row starts a call of its own."""
    from .expand import FIRST, LAST, ExpandSpec, col, stepped
    A = SpongeCallAir
    return ExpandSpec(A.WIDTH, 6, count=col(A.LEN), when=col(A.SEL), max_count=max_len, pad=[1, 0, 0, 0, 0, 0],
                      terms=[FIRST, LAST, col(A.ID), stepped(A.W0, 1), 0, 0])


def sponge_program(max_group_rows: int = 1 << 10):
    """The TITR program that fills ``acc`` and ``state`` of a SpongeChipAir table with one carry: the state after the
    previous row of the call, the IV on its first row.  A call starts where ``first`` is set."""
    from .iterate import IterateBuilder
    T = SpongeChipAir
    b = IterateBuilder(T.WIDTH, reset_column=T.FIRST, max_group_rows=max_group_rows)
    state = b.carry(SPONGE_IV)
    acc = state + b.col(T.WORD)
    a2 = acc * acc
    a4 = a2 * a2
    new = a4 * a2 * acc
    b.set_carry(state, new)
    b.output(acc, T.ACC)
    b.output(new, T.STATE)
    return b


def sponge_chip_table(ctx, call_trace, out_height: int = 0, max_len: int = 1 << 10):
    """The SpongeChipAir trace of a resident SpongeCallAir trace, without leaving HBM: the expansion, then one
    ``iterate``.  Returns (the table, n_live)."""
    from .stark import expand_rows
    d_rows, n_live = expand_rows(ctx, sponge_expand_spec(max_len), call_trace, out_height)
    return d_rows.iterate(sponge_program(max_len)), n_live


def sponge_fetch_digests(call_trace, chip_table):
    """A resident SpongeCallAir trace with ``digest`` filled from a resident chip table: a selected call fetches the
    ``state`` of the row with its id and ``last`` set (``join_rows``); the others keep their word."""
    from .join import KEEP, JoinSpec, col
    A, T = SpongeCallAir, SpongeChipAir
    spec = JoinSpec(keys=[(col(A.ID), col(T.ID)), (1, col(T.LAST))], when=col(A.SEL), fetch=[(T.STATE, A.DIGEST, 0)],
                    flags=KEEP)
    return call_trace.join_rows(chip_table, spec)[0]


def generate_sponge_chip_trace(call_trace: np.ndarray, out_height: int = 0) -> np.ndarray:
    """``sponge_chip_table`` on the host with a plain loop, for the comparison: (height, 6) canonical u32 satisfying
    SpongeChipAir, padded to ``out_height`` or to the least power of two that holds the words."""
    A, T = SpongeCallAir, SpongeChipAir
    rows = []
    for call in np.asarray(call_trace, dtype=np.uint32).tolist():
        if call[A.SEL] != 1:
            continue
        state = SPONGE_IV
        for j in range(call[A.LEN]):
            word = (call[A.W0] + j) % P
            acc = (state + word) % P
            state = pow(acc, 7, P)
            rows.append([int(j == 0), int(j == call[A.LEN] - 1), call[A.ID], word, acc, state])
    height = out_height or 1 << max(len(rows) - 1, 0).bit_length()
    assert len(rows) <= height
    rows += [[1, 0, 0, 0, SPONGE_IV, pow(SPONGE_IV, 7, P)]] * (height - len(rows))
    return np.array(rows, dtype=np.uint32).reshape(height, T.WIDTH)
