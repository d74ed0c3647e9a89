"""Planted edge operands for the constraint compilers, shared by tests/test_quotient_edges_cpu.py (no GPU) and
tests/test_gpu_quotient_edges.py.

A trace is built so that the rows the quotient kernels evaluate ARE chosen values: V (n x w) is planted on the
coset 31 H_n of the LDE domain, the trace T is its interpolant evaluated on H_n (inverse transform, scaling of
coefficient k by 31^-k, forward transform), and for an AIR of degree <= 2 the quotient domain is exactly that
coset.  The planted `next` of row i is row i + 1.

The column pair (x, y) runs over ALL of E x E (tests/_field_cases.py), as consecutive elements of one cyclic
sequence in which every ordered pair of E occurs once (an Euler circuit of the complete digraph with loops):
x_i = s_i, y_i = s_(i+1).  So x + y, x - y, x y see every pair on a row, and next.x - x sees every pair across
two rows.  Consecutive traces overlap by one row, so no pair is lost at a trace boundary.
"""
import numpy as np

from _field_cases import E, P, R, RINV, R_MOD_P, ef_mul_int
from tapstark_amd.air import BaseAir

N = 1 << 8
LOG_N = 8
LOG_BLOWUP = 2
SHIFT = 31


def euler_sequence(m):
    """Vertex sequence (length m*m + 1) of an Euler circuit of the complete digraph with loops on m vertices."""
    nxt = [0] * m  # next unused out-edge of every vertex: v -> nxt[v]
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < m:
            nxt[v] += 1
            stack.append(nxt[v] - 1)
        else:
            out.append(stack.pop())
    return out[::-1]


def planted_matrices():
    """The V of every trace: (n_traces, N, 2) u32."""
    seq = [E[i] for i in euler_sequence(len(E))]
    assert len(seq) == len(E) ** 2 + 1
    mats, at = [], 0
    while at + 1 < len(seq):
        xs = [seq[(at + i) % (len(seq) - 1)] for i in range(N + 1)]  # cyclic: the tail wraps to the start
        mats.append(np.array([xs[:-1], xs[1:]], dtype=np.uint32).T.copy())
        at += N - 1
    return np.stack(mats)


def trace_of(orc, v):
    """T with interpolant(T)(31 w_n^i) = V[i]: coefficients of V on the coset, unscaled, evaluated on H_n."""
    n = v.shape[0]
    coef = orc.dft_batch(v, inverse=True).astype(object)
    s_inv, sk = pow(SHIFT, -1, P), 1
    for k in range(n):
        coef[k] = [int(c) * sk % P for c in coef[k]]
        sk = sk * s_inv % P
    return orc.dft_batch(coef.astype(np.uint32))


def assert_planted(lde, v):
    """Every row of V occurs among the rows of the LDE (the index map is not assumed)."""
    have = {tuple(r) for r in lde.tolist()}
    missing = [tuple(r) for r in v.tolist() if tuple(r) not in have]
    assert not missing, f"{len(missing)} planted rows are not in the LDE, e.g. {missing[0]}"


# ------------------------------------------------------------------------------------------------ single-op AIRs
class OpAir(BaseAir):
    def __init__(self, name, fn, width=2):
        self.name, self.fn, self._w = name, fn, width

    def width(self):
        return self._w

    def eval(self, builder):
        main = builder.main()
        builder.assert_zero(self.fn(main.row_slice(0), main.row_slice(1)))


CONSTS = (P - 1, (P + 1) // 2, P - R_MOD_P)
# name -> (AIR, the constraint on Python ints: (x, y, next x) -> value)
OP_AIRS = {
    "add": (OpAir("add", lambda l, n: l[0] + l[1]), lambda x, y, nx: (x + y) % P),
    "sub": (OpAir("sub", lambda l, n: l[0] - l[1]), lambda x, y, nx: (x - y) % P),
    "neg": (OpAir("neg", lambda l, n: -l[0]), lambda x, y, nx: (-x) % P),
    "mul": (OpAir("mul", lambda l, n: l[0] * l[1]), lambda x, y, nx: x * y % P),
    "square": (OpAir("square", lambda l, n: l[0] * l[0]), lambda x, y, nx: x * x % P),
    "next_minus": (OpAir("next_minus", lambda l, n: n[0] - l[0]), lambda x, y, nx: (nx - x) % P),
}
for _c in CONSTS:
    OP_AIRS[f"add_const_{_c:#x}"] = (OpAir("add_const", lambda l, n, c=_c: l[0] + c), lambda x, y, nx, c=_c: (x + c) % P)


# ------------------------------------------------------------------------------------------------ accumulator AIR
N_ACC = 66
ACC_VALUE = (P - 1) * RINV % P  # the canonical value whose Montgomery form is p - 1


class AccumulatorAir(BaseAir):
    """66 constraints that all take the value of column 0: x, then (x + k) - k.  On the constant column
    ACC_VALUE every constraint value has the Montgomery form p - 1 on every row of every coset, the largest
    factor the lazy 64-bit accumulators of the specialised kernels can meet."""

    def width(self):
        return 1

    def eval(self, builder):
        x = builder.main().row_slice(0)[0]
        builder.assert_zero(x)
        for k in range(1, N_ACC):
            builder.assert_zero((x + k) - k)


def alpha_powers_mont(alpha, count):
    """AP[b] = alpha^(count-1-b), coefficients in Montgomery form (the table the quotient kernels read)."""
    pw, cur = [], [1, 0, 0, 0]
    for _ in range(count):
        pw.append([c * R % P for c in cur])
        cur = ef_mul_int(cur, alpha)
    return pw[::-1]


def accumulator_model(alpha, cadence, value_mont=P - 1, count=N_ACC):
    """The four 64-bit accumulators of the straight-line kernel (jit.cpp emit_assert and its epilogue) in
    wrapping 64-bit arithmetic: acc_q += value * AP[b][q] per assert, lazy_fix after every `cadence`-th assert,
    one more before lazy_finish.  Returns (largest exact accumulator seen, the four finished words, the four
    true words)."""
    ap = alpha_powers_mont(alpha, count)
    m64 = (1 << 64) - 1

    def fix(a):
        hi = a >> 32
        return (min(hi, (hi - P) & 0xFFFFFFFF) << 32) | (a & 0xFFFFFFFF)

    acc, true, peak = [0] * 4, [0] * 4, 0
    for b in range(count):
        for q in range(4):
            true[q] += value_mont * ap[b][q]
            exact = acc[q] + value_mont * ap[b][q]
            peak = max(peak, exact)
            acc[q] = exact & m64
        if (b + 1) % cadence == 0:
            acc = [fix(a) for a in acc]
    acc = [fix(a) for a in acc]       # epilogue
    out = []
    for a in acc:
        a = fix(a)                    # lazy_finish
        t = a + ((a * 0x77FFFFFF) & 0xFFFFFFFF) * P
        r = (t & m64) >> 32
        out.append(min(r, (r - P) & 0xFFFFFFFF))
    return peak, out, [t * RINV % P for t in true]


ALPHA_SEED = 20261018
# what search_alpha() finds (tests/test_quotient_edges_cpu.py re-runs the search): try number and alpha
ALPHA_TRIES = 16
ALPHA = [1108812760, 2006218080, 1236310194, 1565565997]
# 262 lowered instructions in segments of 50: cuts after 13, 25, 37, 49 and 61 of the 66 asserts
ACC_SEGMENT_INSTR = 50
# the single-operation AIRs lower to 3 or 4 instructions: segments of ONE instruction cut every one of them, and
# the result of the operation itself crosses a cut through the slab (slab width 1)
OP_SEGMENT_INSTR = 1


def search_alpha(max_tries=4096):
    """The first alpha of the seeded stream at which one lazy_fix per THREE asserts computes a wrong quotient
    word (its accumulator passes 2p 2^32, and here even 2^64) while the real cadence of two stays in range."""
    rng = np.random.default_rng(ALPHA_SEED)
    for tries in range(max_tries):
        alpha = [int(x) for x in rng.integers(0, P, 4, dtype=np.uint64)]
        peak3, out3, true = accumulator_model(alpha, 3)
        if peak3 >= 2 * P * R and [o % P for o in out3] != true:
            return tries, alpha
    raise AssertionError("no alpha found")
