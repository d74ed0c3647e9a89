"""The probe catalogue of tests/test_gpu_context_state.py: one function per stage of the C ABI, each
``(ctx, orc, log_n, ...) -> None``.  A probe runs its stage through the public Python wrapper on seeded input on the
context it is given and asserts equality, word for word, with the CPU oracle (``orc`` = oracle.oracle_py).  Nothing is
compared with the library's own output on another context; nothing reads a table size back from the library.

Seeded input is ``rand_mat`` of tests/test_gpu_dft.py (canonical words, some forced to 0 and to p - 1) or the trace
generator of the AIR.  ``refs`` is an optional dict a scenario passes to every probe it runs: the oracle's answer for a
(probe, shape, input) is computed once and shared by the calls that ask for it again, never modified.

Every AIR is compiled with TS_NO_JIT=1 set by the caller (the interpreter path: no wait for a background compile)."""
import contextlib

import numpy as np

import tapstark_amd as ts
from tapstark_amd.airs import (FibonacciAir, SynthMulAir, fibonacci_public_values, generate_fibonacci_trace,
                               generate_synth_mul_trace, splitmix64_stream)

import _multi_cases as mc
from _field_cases import extreme_mat
from test_abi_cpu import _fri_rs_inputs
from test_gpu_dft import bitrev_index, powers, rand_mat, rand_shift, scale_rows

P = 0x78000001
G27 = 0x1A427A41  # generator of the 2^27 subgroup
PROVE_CFG = (2, 3, 4)


@contextlib.contextmanager
def fresh_context():
    """A new ``ts.Context(0)``, closed on the way out whatever happened inside."""
    ctx = ts.Context(0)
    try:
        yield ctx
    finally:
        ctx.close()


def memo(refs, key, make):
    if refs is None:
        return make()
    if key not in refs:
        refs[key] = make()
    return refs[key]


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} for {want.shape}"
    bad = np.flatnonzero((got != want).reshape(-1))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {got.size} words differ, first at flat index {int(bad[0])}: "
                           f"{int(got.reshape(-1)[bad[0]]):#x} for {int(want.reshape(-1)[bad[0]]):#x}")


def matrix(log_n, w, kind="rand"):
    """The input of a transform probe: seeded (``rand``) or one of ``_field_cases.EXTREME_KINDS``."""
    if kind == "rand":
        return rand_mat(7000 + 64 * log_n + w, 1 << log_n, w)
    return extreme_mat(kind, 1 << log_n, w)


# ------------------------------------------------------------------ dft
DFT_CALLS = ("dft", "idft", "coset_dft", "coset_idft")


def dft(ctx, orc, log_n, w=3, kind="rand", first="dft", refs=None):
    """dft_batch, idft_batch, coset_dft_batch and coset_idft_batch (one seeded shift), ``first`` first."""
    n = 1 << log_n
    x = matrix(log_n, w, kind)
    shift = rand_shift(77 + log_n)

    def wants():
        inv = orc.dft_batch(x, inverse=True)
        return {"dft": orc.dft_batch(x), "idft": inv,
                "coset_dft": orc.dft_batch(scale_rows(x, powers(shift, n))),
                "coset_idft": scale_rows(inv, powers(pow(shift, P - 2, P), n))}

    want = memo(refs, ("dft", log_n, w, kind), wants)
    d = ts.Radix2Dft(ctx)
    dm = ts.DeviceMatrix.upload(ctx, x)
    calls = {"dft": lambda: d.dft_batch(dm), "idft": lambda: d.idft_batch(dm),
             "coset_dft": lambda: d.coset_dft_batch(dm, shift), "coset_idft": lambda: d.coset_idft_batch(dm, shift)}
    k = DFT_CALLS.index(first)
    for name in DFT_CALLS[k:] + DFT_CALLS[:k]:
        equal(calls[name]().download(), want[name], f"{name} 2^{log_n} x {w} {kind}")
    equal(dm.download(), x, "the input matrix after the transforms")


# ------------------------------------------------------------------ lde
def lde(ctx, orc, log_n, added_bits=1, shift=31, w=3, kind="rand", refs=None):
    """coset_lde_batch(added_bits, shift): natural rows, then bit-reversed rows."""
    x = matrix(log_n, w, kind)
    want = memo(refs, ("lde", log_n, w, kind, added_bits, shift), lambda: orc.coset_lde_batch(x, added_bits, shift))
    d = ts.Radix2Dft(ctx)
    dm = ts.DeviceMatrix.upload(ctx, x)
    what = f"coset_lde_batch 2^{log_n} x {w} {kind} +{added_bits} shift {shift}"
    got = d.coset_lde_batch(dm, added_bits, shift)
    assert got.dims() == (1 << (log_n + added_bits), w)
    equal(got.download(), want, what)
    del got
    got = d.coset_lde_batch(dm, added_bits, shift, bit_reversed=True).download()
    equal(got, want[bitrev_index(log_n + added_bits)], what + " bit-reversed")
    equal(dm.download(), x, "the input matrix after the LDE")


# ------------------------------------------------------------------ commit
def commit(ctx, orc, log_n, w=3, log_blowup=1, shift=1, kind="rand", refs=None):
    """Pcs::commit of one matrix: the LDE rows, every digest level, the root, one opened row with its path."""
    m = matrix(log_n, w, kind)

    def wants():
        rows = orc.commit_lde(m, shift, log_blowup)
        return rows, orc.OracleMmcs([rows])

    want, om = memo(refs, ("commit", log_n, w, kind, log_blowup, shift), wants)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(log_blowup, 4, 8), ctx)
    root, data = pcs.commit([((log_n, shift), m.copy())])
    what = f"commit 2^{log_n} x {w} {kind} blowup {log_blowup} shift {shift}"
    equal(data.lde(0, w), want, what + ": LDE")
    assert data.log_height == log_n + log_blowup
    for lvl in range(data.log_height + 1):
        equal(data.digests(lvl), om.layer(lvl), what + f": digest level {lvl}")
    equal(root, om.root, what + ": root")
    idx = (5 * 977) % (1 << data.log_height)
    rows, path = data.open_batch(idx, w)
    orows, opath = om.open(idx)
    equal(rows, orows, what + ": opened row")
    equal(path, opath, what + ": path")
    assert om.verify(idx, rows, path, root)


# ------------------------------------------------------------------ AIRs
def statement(qd, log_n):
    """(air, trace, public values, tape) of quotient degree ``qd``: Fibonacci (1) or SynthMulAir(7) (2)."""
    n = 1 << log_n
    if qd == 1:
        air, trace = FibonacciAir(), generate_fibonacci_trace(0, 1, n)
        pis = fibonacci_public_values(trace)
    else:
        air, trace, pis = SynthMulAir(7), generate_synth_mul_trace(n, 7), np.zeros(0, dtype=np.uint32)
    return air, trace, pis, ts.air_tape(air, len(pis))


def quotient(ctx, orc, log_n, qd=1, log_blowup=1, refs=None):
    """quotient_chunks on the interpreter against the oracle's chunks (tests/test_gpu_parity.py
    test_quotient_chunks)."""
    air, trace, pis, tape = statement(qd, log_n)
    cair = ts.CompiledAir(ctx, tape)
    assert not cair.is_jit, "the probes run the interpreter: TS_NO_JIT=1"
    assert 1 << cair.log_quotient_degree == qd
    alpha = splitmix64_stream(5, 4)

    def wants():
        rows = orc.commit_lde(trace, 1, log_blowup)
        return orc.split_quotient(orc.quotient_values(tape, rows, log_n, log_blowup, pis, alpha), log_n,
                                  cair.log_quotient_degree)

    want = memo(refs, ("quotient", log_n, qd, log_blowup), wants)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(log_blowup, 4, 8), ctx)
    _, data = pcs.commit([((log_n, 1), trace.copy())])
    chunks = pcs.quotient_chunks(data, cair, pis, alpha)
    assert len(chunks) == want.shape[0]
    for c, ch in enumerate(chunks):
        equal(ch.download(), want[c], f"quotient 2^{log_n} degree {qd}: chunk {c}")


def commit_pair(ctx, orc, log_n, domain_shifts, log_blowup=1):
    """The two chunks of a quotient of degree 2 (column-major on the device) committed on two domains of the caller's
    choosing: ONE set of LDE launches for both matrices (``coset_lde`` with ``evals2`` / ``shift2``), whose scale
    tables have the keys (log_n, 31 / domain_shifts[0]) and (log_n, 31 / domain_shifts[1]).  The chunk values are only
    this probe's input (``quotient`` checks them); their LDEs, the root and an opened row are the oracle's."""
    air, trace, pis, tape = statement(2, log_n)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(log_blowup, 4, 8), ctx)
    _, data = pcs.commit([((log_n, 1), trace.copy())])
    chunks = pcs.quotient_chunks(data, ts.CompiledAir(ctx, tape), pis, splitmix64_stream(5, 4))
    assert len(chunks) == 2
    values = [c.download() for c in chunks]
    root, qdata = pcs.commit([((log_n, s), c) for s, c in zip(domain_shifts, chunks)])
    want = [orc.commit_lde(v, s, log_blowup) for s, v in zip(domain_shifts, values)]
    om = orc.OracleMmcs(want)
    for i in range(2):
        equal(qdata.lde(i, 4), want[i], f"pair commit 2^{log_n}: LDE of matrix {i}")
    equal(root, om.root, f"pair commit 2^{log_n}: root")
    idx = 3 % (1 << qdata.log_height)
    rows, path = qdata.open_batch(idx, 8)
    orows, opath = om.open(idx)
    equal(rows, orows, "pair commit: opened row")
    equal(path, opath, "pair commit: path")


def prove(ctx, orc, log_n, qds=(1, 2), cfg=PROVE_CFG, refs=None):
    """Whole proofs (Fibonacci and SynthMulAir(7) by default), byte-equal to the oracle's."""
    for qd in qds:
        air, trace, pis, tape = statement(qd, log_n)
        want = memo(refs, ("prove", log_n, qd, cfg), lambda: orc.prove(orc.FriConfig(*cfg), tape, trace, pis))
        config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))
        proof = ts.prove(config, ts.CompiledAir(ctx, tape), ts.BfChallenger(), trace.copy(), pis)
        equal(proof.words, want, f"proof 2^{log_n} quotient degree {qd} FRI {cfg}")


def prove_mul(ctx, orc, log_n, width, cfg, refs=None):
    """One SynthMulAir(width) proof, byte-equal to the oracle's."""
    air, trace, pis = SynthMulAir(width), generate_synth_mul_trace(1 << log_n, width), np.zeros(0, dtype=np.uint32)
    tape = ts.air_tape(air, 0)
    want = memo(refs, ("prove_mul", log_n, width, cfg), lambda: orc.prove(orc.FriConfig(*cfg), tape, trace, pis))
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))
    proof = ts.prove(config, ts.CompiledAir(ctx, tape), ts.BfChallenger(), trace.copy(), pis)
    equal(proof.words, want, f"SynthMulAir({width}) proof 2^{log_n} FRI {cfg}")


# ------------------------------------------------------------------ open
def open_(ctx, orc, log_n, qd=2, w=3, refs=None):
    """open_reduce against the oracle (tests/test_gpu_parity.py check_open_reduce), then the general ``pcs.open`` of
    the same commitments at {zeta, zeta w_n} and {zeta}: its opened values are the oracle's too."""
    b = 2
    lqd = qd.bit_length() - 1
    trace = rand_mat(60 + log_n, 1 << log_n, w)
    chunks = [rand_mat(61 + log_n + c, 1 << log_n, 4) for c in range(qd)]
    g = pow(G27, 1 << (27 - (log_n + lqd)), P) if log_n + lqd else 1
    shifts = [31 * pow(g, c, P) % P for c in range(qd)]
    zeta = np.array([5, 6, 7, 8], dtype=np.uint32)
    ch = ts.BfChallenger()
    alpha = ch.clone().sample()  # what pcs.open samples first

    def wants():
        return orc.open_reduce(orc.commit_lde(trace, 1, b), [orc.commit_lde(m, s, b) for s, m in zip(shifts, chunks)],
                               log_n, b, zeta, alpha)

    want_opened, want_ro = memo(refs, ("open", log_n, qd, w), wants)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(b, 3, 4), ctx)
    _, tdata = pcs.commit([((log_n, 1), trace.copy())])
    _, qdata = pcs.commit([((log_n, s), m.copy()) for s, m in zip(shifts, chunks)])
    opened, ro = pcs.open_reduce(tdata, qdata, w, zeta, alpha)
    equal(opened, want_opened, f"open_reduce 2^{log_n}: opened values")
    equal(ro, want_ro, f"open_reduce 2^{log_n}: reduced openings")
    wn = pow(G27, 1 << (27 - log_n), P)
    zeta_next = (zeta.astype(np.uint64) * np.uint64(wn) % np.uint64(P)).astype(np.uint32)
    values, _ = pcs.open([(tdata, [[zeta, zeta_next]]), (qdata, [[zeta]] * qd)], ch)
    equal(np.concatenate([p for r in values for m in r for p in m]), want_opened, f"pcs.open 2^{log_n}: opened values")


# ------------------------------------------------------------------ FRI
def fold(ctx, orc, log_h, refs=None):
    """ts_fri_fold of 2^(log_h + 1) elements: reads the Montgomery inverse twiddles of order 2^(log_h + 1)."""
    vec = rand_mat(80 + log_h, 2 << log_h, 4)
    beta = rand_mat(81, 1, 4)[0]
    want = memo(refs, ("fold", log_h), lambda: orc.fold_matrix(vec, beta))
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 4, 8), ctx)
    equal(pcs.fold_matrix(vec, beta), want, f"fri_fold 2^{log_h}")


def fri(ctx, orc, log_n, cfg=(1, 5, 4), refs=None):
    """ts_fri_prove alone (tests/test_gpu_parity.py test_fri_prove_alone_matches_oracle) on inputs of degrees
    2^1 .. 2^log_n with gaps: the first commit round folds 2^(log_n + log_blowup) elements."""
    degs = sorted({1, max(1, log_n // 2), log_n})
    ins = _fri_rs_inputs(orc, cfg[0], degs)
    want = memo(refs, ("fri", log_n, cfg), lambda: orc.fri_prove(orc.FriConfig(*cfg), ins, orc.OracleChallenger()))
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx)
    equal(pcs.fri_prove(ins, ts.BfChallenger()), want, f"fri_prove degrees {degs} FRI {cfg}")


# ------------------------------------------------------------------ evaluations on a domain
def domain(ctx, orc, log_n, w=3, refs=None):
    """get_evaluations_on_domain of a committed matrix: the trace's own domain 31 H_n against the oracle's coset
    transform, every smaller size against the oracle's commit LDE."""
    m = rand_mat(41 + log_n, 1 << log_n, w)

    def wants():
        return orc.commit_lde(m, 1, 1), orc.coset_lde_batch(m, 0, 31)

    rows, on_trace_domain = memo(refs, ("domain", log_n, w), wants)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 1, 0), ctx)
    _, data = pcs.commit([((log_n, 1), m.copy())])
    equal(pcs.get_evaluations_on_domain(data, 0, log_n).download(), on_trace_domain, f"evaluations on 31 H_2^{log_n}")
    for log_size in sorted({0, log_n // 2, log_n + 1}):
        got = pcs.get_evaluations_on_domain(data, 0, log_size)
        equal(got.download(), rows[: 1 << log_size][bitrev_index(log_size)], f"evaluations, 2^{log_size} rows")


# ------------------------------------------------------------------ several tables in one proof
def multi(ctx, orc=None, log_n=None, refs=None):
    """The smallest multi-table case of tests/_multi_cases.py (case b at log_blowup 1: heights 2^3 and 2^6) against
    its golden words (the oracle has no multi-table prover)."""
    _, _, _, want = mc.load_golden()
    tables = mc.case("b", 1)
    proof = mc.prove(mc.config(ctx, 1), mc.compiled(ctx, tables), tables)
    equal(proof.words, want, "multi-table proof, case b")


PROBES = {"dft": dft, "lde": lde, "commit": commit, "quotient": quotient, "open": open_, "fold": fold, "fri": fri,
          "domain": domain, "multi": multi, "prove": prove}
