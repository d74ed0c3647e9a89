"""Nothing reads HBM that was not written: every stage on a clean context and on two contexts whose device blocks
are filled with a test pattern before they are handed out (TS_POOL_POISON, csrc/context.cpp; tests/_poison.py).

The other GPU tests compare device words with the oracle, which catches a kernel that computes the wrong thing.
A kernel or driver that leaves something unwritten, or reads past what it wrote, passes them whenever the block
it then reads already holds the right words -- and the pool hands a freed block back as it was, to a suite that
proves the same shapes over and over in one context, often once per setting of a knob on the same input.  Here
each case runs on a clean context, on one filled with 0x00000001 and on one filled with 0xFFFFFFFF, twice each
with a call of another shape in between; all six results are the same words, they are the oracle's where the
stage has an oracle, and ts_ctx_stat 9 shows that the two filled contexts did fill blocks and the clean one none.

The shapes are the smallest at which each path still takes its own branches (the first three-pass LDE height
2^13, the wide and narrow barycentric paths, a row_dot_acc tail below eight columns, every level of the LogUp
prefix sum, ...).  Knobs the library reads on every call are set inside a case; those it reads once per process
(TS_LEAF_TREE, TS_LDE_PAIR, TS_FRI_ROUND_LOG) are set for a child process that runs the same cases on three
contexts of its own and reports a digest of each result (test_once_per_process_knobs)."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tapstark_amd as ts  # noqa: E402
from tapstark_amd import taptree as tt  # noqa: E402
from tapstark_amd.air import LogUp, aux_dims  # noqa: E402
from tapstark_amd.airs import (FibonacciAir, HighDegreeAir, RangeLookupAir, SelectorAir, SynthExtAir,  # noqa: E402
                               SynthMulAir, TableLookupAir, fibonacci_public_values, generate_fibonacci_trace,
                               generate_high_degree_trace, generate_lookup_table, generate_range_lookup_trace,
                               generate_selector_preprocessed, generate_selector_trace, generate_synth_ext_trace,
                               generate_synth_mul_trace, generate_table_lookup_trace, splitmix64_stream)
from tapstark_amd.comm import LocalCommGroup  # noqa: E402

import _poison  # noqa: E402
from _aux_airs import logup_reference  # noqa: E402
from _poison import P, digest, flat, make_contexts, rand_mat, same_everywhere  # noqa: E402
from _pre_aux_airs import remap_logup  # noqa: E402

pytestmark = pytest.mark.gpu
G27 = 0x1A427A41
NO_PIS = np.zeros(0, dtype=np.uint32)
CASES = {}  # name -> (run(target, env) -> result, oracle(orc) -> the same result from the oracle | None)


def case(name, oracle=None):
    def add(run):
        assert name not in CASES, name
        CASES[name] = (run, oracle)
        return run
    return add


def names(prefix):
    return [n for n in CASES if n.startswith(prefix)]


# ------------------------------------------------------------------ contexts
@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """One TS_JIT_CACHE_DIR for the module: a specialised kernel is compiled for the first context that needs
    it and loaded by the others (and by the child process)."""
    d = tmp_path_factory.mktemp("jit_cache")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TS_JIT_CACHE_DIR", str(d))
        yield str(d)


@pytest.fixture(scope="module")
def trio(jit_cache):
    from tapstark_amd.build import build

    build()
    return make_contexts()


@pytest.fixture(scope="module")
def groups(trio):
    """Eight contexts per word: the lanes of ts_prove_batch and the ranks of ts_prove_sharded."""
    return make_contexts(8)


_oracle_results = {}
_digests = {}  # name -> digest of the case's result in this process (test_once_per_process_knobs)


def run_case(targets, orc, env, name):
    run, oracle = CASES[name]
    if oracle is not None and name not in _oracle_results:
        _oracle_results[name] = flat(oracle(orc))  # once, shared, never modified
    result = same_everywhere(targets, lambda t: run(t, env), want=_oracle_results.get(name), what=name)
    _digests[name] = digest(result)


def test_the_knob_is_read_by_the_constructor_and_checked(trio, monkeypatch):
    """A context made with the knob unset stays clean whatever the variable says later; a value that is no
    32-bit word is refused with a text; every accepted spelling is the same word."""
    from tapstark_amd._lib import TsError, lib

    clean, one, ones = trio
    monkeypatch.setenv(_poison.KNOB, "0xFFFFFFFF")
    before = [c.stat(_poison.STAT_FILLS) for c in trio]
    for c in trio:
        ts.DeviceMatrix.upload(c, rand_mat(1, 8, 3)).download()
    after = [c.stat(_poison.STAT_FILLS) for c in trio]
    assert after[0] == before[0] == 0 and after[1] > before[1] and after[2] > before[2]
    for bad in ("poison", "0x", "12monkeys", "0x100000000", "-1", "4294967296", " "):
        monkeypatch.setenv(_poison.KNOB, bad)
        with pytest.raises(TsError) as e:
            ts.Context(0)
        assert e.value.code == 1, bad
        assert "TS_POOL_POISON" in (lib().ts_last_error(None) or b"").decode(), bad
    for ok in ("1", "0x1", "01", "4294967295", "0"):
        monkeypatch.setenv(_poison.KNOB, ok)
        c = ts.Context(0)
        ts.DeviceMatrix.upload(c, rand_mat(1, 8, 3))
        assert c.stat(_poison.STAT_FILLS) == 1, ok  # one block: the matrix
    monkeypatch.setenv(_poison.KNOB, "")
    c = ts.Context(0)
    ts.DeviceMatrix.upload(c, rand_mat(1, 8, 3))
    assert c.stat(_poison.STAT_FILLS) == 0


# ------------------------------------------------------------------ commit: LDE and Merkle
def _commit_result(root, data):
    return [root] + [data.lde(i) for i in range(data.n_mats)] + [data.digests(l) for l in range(data.log_height + 1)]


def _commit_oracle(orc, ldes):
    om = orc.OracleMmcs(ldes)
    height = max(l.shape[0] for l in ldes)
    return [om.root] + list(ldes) + [om.layer(l) for l in range(height.bit_length())]


def _add_commit(log_n, w, b, shift):
    x = rand_mat(17 + log_n, 1 << log_n, w)

    @case(f"commit-2p{log_n}x{w}-b{b}-s{shift}", lambda orc: _commit_oracle(orc, [orc.commit_lde(x, shift, b)]))
    def run(ctx, env):
        return _commit_result(*ts.TwoAdicFriPcs(ts.FriConfig(b, 2, 0), ctx).commit([((log_n, shift), x.copy())]))


# (13, 3, 2): the first three-pass height; shift 1 and the generator
for _shape in [(0, 1, 1), (3, 2, 2), (5, 7, 1), (10, 64, 2), (12, 5, 2), (13, 3, 2)]:
    for _shift in (1, 31):
        _add_commit(*_shape, _shift)


def _chunk_shifts(log_n, qd):
    lqd = qd.bit_length() - 1
    g = pow(G27, 1 << (27 - (log_n + lqd)), P) if log_n + lqd else 1
    return [31 * pow(g, c, P) % P for c in range(qd)]


_BATCH4 = [rand_mat(40 + i, 1 << 7, 4) for i in range(4)]


@case("commit-batch-of-four", lambda orc: _commit_oracle(
    orc, [orc.commit_lde(m, s, 2) for s, m in zip(_chunk_shifts(7, 4), _BATCH4)]))
def _(ctx, env):
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(2, 2, 0), ctx)
    return _commit_result(*pcs.commit([((7, s), m.copy()) for s, m in zip(_chunk_shifts(7, 4), _BATCH4)]))


_MIXED_SHAPES = [(9, 3), (6, 5), (9, 2), (3, 70), (6, 1), (0, 2)]
_MIXED = [rand_mat(70 + i, 1 << lg, w) for i, (lg, w) in enumerate(_MIXED_SHAPES)]


@case("commit-mixed-heights", lambda orc: _commit_oracle(orc, [orc.commit_lde(m, 1, 1) for m in _MIXED]))
def _(ctx, env):
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 0), ctx)
    return _commit_result(*pcs.commit([((lg, 1), m.copy()) for (lg, _), m in zip(_MIXED_SHAPES, _MIXED)]))


# rows wider than one hash chunk: the third shape of test_gpu_mmcs.py::test_commit_rows_wider_than_one_chunk
_WIDE = [splitmix64_stream(700 + i, (1 << lh) * w).reshape(1 << lh, w)
         for i, (lh, w) in enumerate([(4, 1030), (3, 700), (4, 2)])]


def _wide_oracle(orc):
    om = orc.OracleMmcs(_WIDE)
    return [om.root] + [om.layer(l) for l in range(5)] + [list(om.open(i)) for i in (0, 5, 15)]


@case("commit-rows-wider-than-a-chunk", _wide_oracle)
def _(ctx, env):
    root, data = ts.Blake3Mmcs(ctx).commit([m.copy() for m in _WIDE])
    return [root] + [data.digests(l) for l in range(5)] + [list(data.open_batch(i)) for i in (0, 5, 15)]


@pytest.mark.parametrize("name", names("commit-"))
def test_commit(trio, orc, monkeypatch, name):
    run_case(trio, orc, monkeypatch, name)


# ------------------------------------------------------------------ the block of an LDE that is its own input
def _bitrev(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2) if bits else 0


def _own_shift(log_n, b, beta):
    """the shift for which block beta of the LDE is the input: w_N^(-bitrev_b(beta))"""
    w = pow(G27, 1 << (27 - (log_n + b)), P)
    return pow(w, (P - 1 - _bitrev(beta, b)) % (P - 1), P)


_OWN = [(b, beta) for b in (1, 2, 3) for beta in range(1 << b)]


def _add_own_lde(log_n, w):
    x = rand_mat(100 + log_n, 1 << log_n, w)

    def oracle(orc):
        return [orc.coset_lde_batch(x, b, _own_shift(log_n, b, beta)) for b, beta in _OWN for _ in "10"] + [x]

    @case(f"own-lde-2p{log_n}x{w}", oracle)
    def run(ctx, env):
        dft, dx, out = ts.Radix2Dft(ctx), ts.DeviceMatrix.upload(ctx, x), []
        for b, beta in _OWN:
            for knob in "10":  # the copy first: what it leaves alone was not computed just before
                env.setenv("TS_LDE_OWN_COSET", knob)
                out.append(dft.coset_lde_batch(dx, b, _own_shift(log_n, b, beta)).download())
        env.delenv("TS_LDE_OWN_COSET")
        return out + [dx.download()]  # and the input is left as it was


_add_own_lde(10, 3)
_add_own_lde(13, 3)


def _chunk_air(name, n):
    if name == "mul5":  # degree 3: two chunks, the pair launch
        return SynthMulAir(5), generate_synth_mul_trace(n, 5)
    return HighDegreeAir(5), generate_high_degree_trace(n)  # degree 5: four chunks


_airs = {}  # (context, key) -> CompiledAir: an AIR is compiled once per context


def _compiled(ctx, key, make):
    if (id(ctx), key) not in _airs:
        _airs[(id(ctx), key)] = make()
    return _airs[(id(ctx), key)]


def _add_chunk_commit(name, log_n):
    air, trace = _chunk_air(name, 1 << log_n)
    tape = ts.air_tape(air, 0)
    alpha = rand_mat(5, 1, 4)[0]

    def oracle(orc):
        lqd = orc.log_quotient_degree(tape)
        chunks = orc.split_quotient(orc.quotient_values(tape, orc.commit_lde(trace, 1, 2), log_n, 2, NO_PIS, alpha),
                                    log_n, lqd)
        ldes = [orc.commit_lde(c, s, 2) for c, s in zip(chunks, _chunk_shifts(log_n, 1 << lqd))]
        return [[list(chunks)] + _commit_oracle(orc, ldes) for _ in "10"]

    @case(f"chunk-commit-{name}-2p{log_n}", oracle)
    def run(ctx, env):
        cair = _compiled(ctx, name, lambda: ts.CompiledAir(ctx, tape))
        qd = 1 << cair.log_quotient_degree
        pcs = ts.TwoAdicFriPcs(ts.FriConfig(2, 2, 0), ctx)
        _, tdata = pcs.commit([((log_n, 1), trace.copy())])
        out = []
        for knob in "10":
            env.setenv("TS_LDE_OWN_COSET", knob)
            chunks = pcs.quotient_chunks(tdata, cair, NO_PIS, alpha)
            vals = [c.download() for c in chunks]
            out.append([vals] + _commit_result(*pcs.commit(
                [((log_n, s), c) for s, c in zip(_chunk_shifts(log_n, qd), chunks)])))
        env.delenv("TS_LDE_OWN_COSET")
        return out


for _name in ("mul5", "deg5"):
    for _log_n in (10, 13):
        _add_chunk_commit(_name, _log_n)


@pytest.mark.parametrize("name", names("own-lde-") + names("chunk-commit-"))
def test_own_coset_lde(trio, orc, monkeypatch, name):
    run_case(trio, orc, monkeypatch, name)


# ------------------------------------------------------------------ quotient
QUOTIENT_AIRS = {
    # name: (air, trace of n rows, public values of a trace, segment size that cuts its program in four or five)
    "fib": (FibonacciAir(), lambda n: generate_fibonacci_trace(0, 1, n), fibonacci_public_values, 8),
    "mul7": (SynthMulAir(7), lambda n: generate_synth_mul_trace(n, 7), lambda t: NO_PIS, 8),
    "ext25": (SynthExtAir(25), lambda n: generate_synth_ext_trace(n, 25), lambda t: NO_PIS, 32),
}
QUOTIENT_PATHS = ("jit", "interp", "interp-global", "segmented")


def _quotient_air(ctx, env, name, tape, path, segment_instr):
    def make():
        with env.context() as m:
            if path.startswith("interp"):
                m.setenv("TS_NO_JIT", "1")
            cair = ts.CompiledAir(ctx, tape, segment_instr=segment_instr) if path == "segmented" else \
                ts.CompiledAir(ctx, tape)
        if path == "segmented":
            assert len(cair.segment_plan()["segments"]) > 1
            state, _ = cair.jit_wait()
            assert state == 3, f"segmented specialisation failed (state {state})"
        assert cair.is_jit == (not path.startswith("interp")), path
        return cair
    return _compiled(ctx, (name, path), make)


def _add_quotient(name, log_n, path):
    air, make_trace, pis_of, seg = QUOTIENT_AIRS[name]
    trace = make_trace(1 << log_n)
    pis = pis_of(trace)
    tape = ts.air_tape(air, len(pis))
    alpha = rand_mat(5, 1, 4)[0]

    def oracle(orc):
        key = ("quotient", name, log_n)
        if key not in _oracle_results:  # one oracle run for the four paths
            q = orc.quotient_values(tape, orc.commit_lde(trace, 1, 2), log_n, 2, pis, alpha)
            _oracle_results[key] = list(orc.split_quotient(q, log_n, orc.log_quotient_degree(tape)))
        return _oracle_results[key]

    @case(f"quotient-{name}-2p{log_n}-{path}", oracle)
    def run(ctx, env):
        cair = _quotient_air(ctx, env, name, tape, path, seg)
        pcs = ts.TwoAdicFriPcs(ts.FriConfig(2, 2, 0), ctx)
        _, data = pcs.commit([((log_n, 1), trace.copy())])
        with env.context() as m:
            if path == "interp-global":  # the register file on the global slab (read at every launch)
                m.setenv("TS_INTERP_GLOBAL_REGS", "1")
            return [c.download() for c in pcs.quotient_chunks(data, cair, pis, alpha)]


for _name in QUOTIENT_AIRS:
    for _log_n in (3, 8, 13):
        for _path in QUOTIENT_PATHS:
            _add_quotient(_name, _log_n, _path)


@pytest.mark.parametrize("name", names("quotient-"))
def test_quotient(trio, orc, monkeypatch, name):
    run_case(trio, orc, monkeypatch, name)


# ------------------------------------------------------------------ open and reduce
def _add_open_reduce(log_n, w, qd):
    trace = rand_mat(60, 1 << log_n, w)
    chunks = [rand_mat(61 + c, 1 << log_n, 4) for c in range(qd)]
    shifts = _chunk_shifts(log_n, qd)
    zeta, alpha = rand_mat(70, 1, 4)[0], rand_mat(71, 1, 4)[0]

    def oracle(orc):
        want = orc.open_reduce(orc.commit_lde(trace, 1, 2), [orc.commit_lde(m, s, 2) for s, m in zip(shifts, chunks)],
                               log_n, 2, zeta, alpha)
        return [list(want), list(want)]

    @case(f"open-reduce-2p{log_n}x{w}-qd{qd}", oracle)
    def run(ctx, env):
        pcs = ts.TwoAdicFriPcs(ts.FriConfig(2, 2, 0), ctx)
        _, tdata = pcs.commit([((log_n, 1), trace.copy())])
        _, qdata = pcs.commit([((log_n, s), m.copy()) for s, m in zip(shifts, chunks)])
        out = []
        for knob in "10":  # the low coset extended by the LDE first, then the one-pass kernel over every row
            env.setenv("TS_REDUCE_LOW", knob)
            out.append(list(pcs.open_reduce(tdata, qdata, w, zeta, alpha)))
        env.delenv("TS_REDUCE_LOW")
        return out


# (10, 64): the wide barycentric path; (10, 69): wide with a row_dot_acc tail of five columns; the others narrow
for _shape in [(3, 2, 1), (6, 5, 2), (10, 64, 2), (10, 69, 2), (13, 9, 4)]:
    _add_open_reduce(*_shape)


def _add_pcs_open(name, log_blowup, shape, multi):
    """fri/tests/pcs.rs: every round committed, observed, zeta sampled, everything opened -- at zeta, or with
    `multi` at the 1, 2 or 3 points zeta 7^j of matrix k (j < 1 + k % 3)."""
    cfg = (log_blowup, 3, 8)
    seed, evals = 1000, []
    for logs in shape:
        evs = []
        for lg in logs:
            seed += 1
            evs.append(rand_mat(seed, 1 << lg, 1 + seed % 5))
        evals.append(evs)

    def oracle(orc):
        roots, zeta, opened, proof = orc.pcs_commit_open(orc.FriConfig(*cfg), shape, evals, multi=multi)
        return [roots, zeta, opened, proof]

    @case(f"pcs-open-{name}", oracle)
    def run(ctx, env):
        pcs = ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx)
        ch = ts.BfChallenger()
        datas = [pcs.commit([((lg, 1), e.copy()) for lg, e in zip(logs, evs)])[1] for logs, evs in zip(shape, evals)]
        for d in datas:
            ch.observe_commitment(d.root)
        zeta = ch.sample()
        rounds, k = [], 0
        for d in datas:
            pts = []
            for _ in range(d.n_mats):
                pts.append([(zeta.astype(np.uint64) * pow(7, j, P) % P).astype(np.uint32)
                            for j in range(1 + k % 3 if multi else 1)])
                k += 1
            rounds.append((d, pts))
        opened, proof = pcs.open(rounds, ch)
        return [np.stack([d.root for d in datas]), zeta, np.concatenate([p for r in opened for m in r for p in m]),
                proof]


_add_pcs_open("one-point-small", 1, [[4, 2], [4, 2]], False)
_add_pcs_open("one-point-beyond-the-tail", 2, [[12, 9, 12], [11, 5]], False)
_add_pcs_open("several-points-rounds", 1, [[6, 3], [4, 4, 2]], True)
_add_pcs_open("several-points-tall", 1, [[11, 8, 11, 2]], True)


@case("pcs-open-two-points")
def _(ctx, env):
    """The shape of a proof through the general open: the trace at {zeta, zeta w}, two chunks at {zeta}; its
    opened values are those of the fused path (test_gpu_parity.py::test_pcs_open_two_points_matches_prove_shape)."""
    log_n, w = 8, 6
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 4), ctx)
    _, td = pcs.commit([((log_n, 1), rand_mat(5, 1 << log_n, w))])
    _, qd = pcs.commit([((log_n, s), rand_mat(6 + c, 1 << log_n, 4)) for c, s in enumerate(_chunk_shifts(log_n, 2))])
    zeta = np.array([5, 6, 7, 8], dtype=np.uint32)
    zeta_next = (zeta.astype(np.uint64) * pow(G27, 1 << (27 - log_n), P) % P).astype(np.uint32)
    ch = ts.BfChallenger()
    alpha = ch.clone().sample()
    opened, proof = pcs.open([(td, [[zeta, zeta_next]]), (qd, [[zeta]] * 2)], ch)
    got = np.concatenate([p for r in opened for m in r for p in m])
    fused, _ = pcs.open_reduce(td, qd, w, zeta, alpha)
    assert (got == fused).all()
    return [got, proof]


@pytest.mark.parametrize("name", names("open-reduce-") + names("pcs-open-"))
def test_open_and_reduce(trio, orc, monkeypatch, name):
    run_case(trio, orc, monkeypatch, name)


# ------------------------------------------------------------------ FRI
def _add_fold(log_h):
    vec, beta = rand_mat(80 + log_h, 2 << log_h, 4), rand_mat(81, 1, 4)[0]

    @case(f"fri-fold-2p{log_h}", lambda orc: orc.fold_matrix(vec, beta))
    def run(ctx, env):
        return ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 0), ctx).fold_matrix(vec, beta)


for _log_h in (0, 1, 4, 11):
    _add_fold(_log_h)

_fri_inputs = {}


def _fri_rs_inputs(log_blowup, degs):
    """fri/tests/fri.rs:68-97 (tests/test_abi_cpu.py): the oracle's LDE of one random polynomial per degree"""
    if (log_blowup, tuple(degs)) not in _fri_inputs:
        from oracle import oracle_py
        from test_abi_cpu import _fri_rs_inputs as make

        oracle_py.build()
        _fri_inputs[(log_blowup, tuple(degs))] = make(oracle_py, log_blowup, degs)
    return _fri_inputs[(log_blowup, tuple(degs))]


def _add_fri_prove(name, cfg, degs):
    def oracle(orc):
        return orc.fri_prove(orc.FriConfig(*cfg), _fri_rs_inputs(cfg[0], degs), orc.OracleChallenger(0, True))

    @case(f"fri-prove-{name}-pow{cfg[2]}", oracle)
    def run(ctx, env):
        return ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx).fri_prove(_fri_rs_inputs(cfg[0], degs), ts.BfChallenger(0, True))


# every height from 2^2 to 2^10: inside the one-workgroup tail; 2^5 .. 2^14 with gaps: round launches, a fold
# deferred into the next launch, an input joining, the hand-over to the tail
for _bits in (0, 8):
    _add_fri_prove("tail", (1, 5, _bits), list(range(1, 10)))
    _add_fri_prove("rounds", (2, 4, _bits), [3, 9, 11, 12])


@pytest.mark.parametrize("name", names("fri-"))
def test_fri(trio, orc, monkeypatch, name):
    run_case(trio, orc, monkeypatch, name)


# ------------------------------------------------------------------ LogUp
# the specs, inputs and challenge seeds of tests/test_gpu_aux.py and tests/test_gpu_pre_aux.py
LOGUP_SPECS = {
    1: [(("const", P - 1), [("col", 0), ("const", 5), ("col", 1)])],
    2: [(("const", 1), [("col", 0)]), (("col", 3), [("col", 1)])],
    3: [(("col", 3), [("col", 0), ("col", 1), ("const", 7)]), (("const", 1), [("col", 2)]),
        (("const", P - 1), [("col", 1)])],
}
LOGUP_PRE_SPECS = {
    1: [(("prep", 1), [("col", 0), ("const", 5), ("prep", 0)])],
    2: [(("prep", 1), [("col", 0)]), (("col", 3), [("prep", 0)])],
    3: [(("col", 3), [("col", 0), ("prep", 1), ("const", 7)]), (("prep", 0), [("col", 2)]),
        (("const", P - 1), [("prep", 0), ("col", 1)])],
}


def _stream(seed, shape):
    return (splitmix64_stream(seed, int(np.prod(shape))) % np.uint64(P)).reshape(shape).astype(np.uint32)


def _add_logup(n, seed, block_rows=None):
    trace = _stream(3 + n, (n, 4))
    trace[0, :] = (0, 1, P - 1, 0)
    table = _stream(3 + n + 77, (n, 2))
    table[0, :] = (P - 1, 0)
    ch = {K: _stream(seed + K, 8) for K in (1, 2, 3)}

    def oracle(orc):
        out = []
        for K in (1, 2, 3):
            out.append(list(logup_reference(LogUp(LOGUP_SPECS[K]).interactions, trace, ch[K][:4], ch[K][4:])))
            joined = LogUp(remap_logup(LogUp(LOGUP_PRE_SPECS[K]).interactions, 4))
            out.append(list(logup_reference(joined.interactions, np.hstack([trace, table]), ch[K][:4], ch[K][4:])))
        return out

    @case(f"logup-n{n}" + (f"-block{block_rows}" if block_rows else ""), oracle)
    def run(ctx, env):
        out = []
        with env.context() as m:
            if block_rows:
                m.setenv("TS_LOGUP_BLOCK_ROWS", str(block_rows))
            trace_m, table_m = ts.DeviceMatrix.upload(ctx, trace), ts.DeviceMatrix.upload(ctx, table)
            for K in (1, 2, 3):
                aux, S = LogUp(LOGUP_SPECS[K]).build(trace_m, ch[K])
                out.append([aux.download(), S])
                aux, S = LogUp(LOGUP_PRE_SPECS[K]).build(trace_m, ch[K], preprocessed=table_m)
                out.append([aux.download(), S])
        return out


# n = 2 .. 2^8 inside one wave, 2^9 and 2^10 across the waves of a workgroup, 2^11 across workgroups
for _log_n in range(1, 12):
    _add_logup(1 << _log_n, 100 + _log_n)
# 1024 totals (eight passes of the totals scan), a short last workgroup, one wave per workgroup
for _rows in (1, 3, 64):
    _add_logup(1 << 10, 200 + _rows, _rows)


@pytest.mark.parametrize("name", names("logup-"))
def test_logup(trio, orc, monkeypatch, name):
    run_case(trio, orc, monkeypatch, name)


# ------------------------------------------------------------------ transforms and ingest
def _dft_oracle(orc):
    from test_gpu_dft import oracle_bit_reverse_rows, powers, scale_rows

    x, n = _DFT_X, _DFT_X.shape[0]
    inv = orc.dft_batch(x, inverse=True)
    return [orc.dft_batch(x), inv, orc.dft_batch(scale_rows(x, powers(31, n))),
            scale_rows(inv, powers(pow(31, P - 2, P), n)), oracle_bit_reverse_rows(orc, x), x]


# 2^7 x 65: full row tiles with one full and one partial column tile
# (tests/test_gpu_dft.py::test_partial_tile_transposes_match_oracle)
_DFT_X = rand_mat(9000 + 64 * 7 + 65, 1 << 7, 65)


@case("transform-dft-2p7x65", _dft_oracle)
def _(ctx, env):
    dft, dm = ts.Radix2Dft(ctx), ts.DeviceMatrix.upload(ctx, _DFT_X)
    return [dft.dft_batch(dm).download(), dft.idft_batch(dm).download(), dft.coset_dft_batch(dm, 31).download(),
            dft.coset_idft_batch(dm, 31).download(), dm.bit_reverse_rows().download(), dm.download()]


def _ingest_cases():
    """(format, packed bytes, height, width, expected words): u8, u16, u32, Montgomery and mixed columns, rows
    with and without slack and planar columns, at 2 and 4096 rows of 3 and 163 columns -- row sizes that are no
    multiple of 4 or 16, so that no tile of the ingest kernel ends where a row or the buffer does."""
    from test_gpu_ingest import column_words, expected, kinds_for, make_format

    rng = np.random.default_rng(20261019)
    out = []
    for kind_name in ("u8", "u16", "u32", "monty32", "monty31", "alternating"):
        for layout_name in ("rows", "rows_stride", "planar"):
            for height, width in ((2, 3), (4096, 3), (64, 163)):
                kinds = kinds_for(kind_name, width)
                fmt = make_format(kinds, layout_name, width)
                words = column_words(rng, kinds, height, width)
                out.append((fmt, fmt.pack(words), height, width, expected(words, kinds)))
    return out


_INGEST = []


def _ingest():
    if not _INGEST:
        _INGEST.extend(_ingest_cases())
    return _INGEST


@case("transform-ingest-packed", lambda orc: [c[4] for c in _ingest()])
def _(ctx, env):
    return [ts.DeviceMatrix.upload_packed(ctx, buf, fmt, h, w).download() for fmt, buf, h, w, _ in _ingest()]


@pytest.mark.parametrize("name", names("transform-"))
def test_transforms_and_ingest(trio, orc, monkeypatch, name):
    run_case(trio, orc, monkeypatch, name)


# ------------------------------------------------------------------ whole proofs
LOG_N = 10
CFG = (2, 6, 8)


def _proof_case(name):
    n = 1 << LOG_N
    if name == "fib":
        trace = generate_fibonacci_trace(0, 1, n)
        return FibonacciAir(), trace, fibonacci_public_values(trace)
    if name == "mul64":
        return SynthMulAir(64), generate_synth_mul_trace(n), NO_PIS
    return SynthExtAir(25), generate_synth_ext_trace(n, 25), NO_PIS


def _config(ctx, cfg=CFG):
    return ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))


def _add_prove(name):
    air, trace, pis = _proof_case(name)
    tape = ts.air_tape(air, len(pis))

    @case(f"prove-{name}", lambda orc: orc.prove(orc.FriConfig(*CFG), tape, trace, pis))
    def run(ctx, env):
        cair = _compiled(ctx, ("prove", name), lambda: ts.CompiledAir(ctx, tape))
        return ts.prove(_config(ctx), cair, ts.BfChallenger(), trace.copy(), pis).words


for _name in ("fib", "mul64", "ext25"):
    _add_prove(_name)


@case("prove-pre")
def _(ctx, env):
    config = _config(ctx)
    prep = generate_selector_preprocessed(1 << LOG_N)
    key = ts.PreprocessedKey(config, prep)
    cair = _compiled(ctx, "selector", lambda: ts.CompiledAir(ctx, ts.air_tape(SelectorAir(), 2, 3)))
    trace, pis = generate_selector_trace(prep)
    proof = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), pis, preprocessed=key)
    ts.verify(config, cair, ts.BfChallenger(), proof, pis, preprocessed_root=key.root)
    return [key.root, proof.words]


@case("prove-aux")
def _(ctx, env):
    air, config = RangeLookupAir(), _config(ctx)
    cair = _compiled(ctx, "range-lookup", lambda: ts.CompiledAir(ctx, ts.air_tape(air, 0, 0, *aux_dims(air))))
    proof = ts.prove(config, cair, ts.BfChallenger(), generate_range_lookup_trace(1 << LOG_N), [],
                     aux=air.logup.aux_source)
    assert not ts.verify(config, cair, ts.BfChallenger(), proof, []).any()
    return proof.words


@case("prove-pre-aux")
def _(ctx, env):
    air, config = TableLookupAir(), _config(ctx)
    cair = _compiled(ctx, "table-lookup", lambda: ts.CompiledAir(ctx, ts.air_tape(air, 0, 1, *aux_dims(air))))
    key = ts.PreprocessedKey(config, generate_lookup_table(1 << LOG_N), keep_values=True)
    proof = ts.prove(config, cair, ts.BfChallenger(), generate_table_lookup_trace(1 << LOG_N), [], preprocessed=key,
                     aux=air.logup.aux_source_with(key.values))
    assert not ts.verify(config, cair, ts.BfChallenger(), proof, [], preprocessed_root=key.root).any()
    return [key.root, proof.words]


TAP_CFG = (2, 2, 8)
_tap = {}


def _tap_case():
    if not _tap:
        trace = generate_fibonacci_trace(0, 1, 1 << LOG_N)
        lock = lambda ci, q, s, u: tt.winternitz_lock_script(bytes([ci, q, s & 0xFF, s >> 8]), u)  # noqa: E731
        _tap.update(trace=trace, pis=fibonacci_public_values(trace),
                    locks=tt.make_lock_table(TAP_CFG[1], 2, 1, LOG_N, lock))
    return _tap["trace"], _tap["pis"], _tap["locks"]


def _tap_oracle(orc):
    trace, pis, locks = _tap_case()
    return orc.prove_tap(orc.FriConfig(*TAP_CFG), ts.air_tape(FibonacciAir(), 3), trace, pis, locks)


@case("prove-tap", _tap_oracle)
def _(ctx, env):
    trace, pis, locks = _tap_case()
    cair = _compiled(ctx, "fib3", lambda: ts.CompiledAir(ctx, ts.air_tape(FibonacciAir(), 3)))
    return tt.prove_tap(_config(ctx, TAP_CFG), cair, ts.BfChallenger(), trace.copy(), pis, locks)


@pytest.mark.parametrize("name", names("prove-"))
def test_whole_proofs(trio, orc, monkeypatch, name):
    run_case(trio, orc, monkeypatch, name)


def test_prove_batch_over_four_lanes(groups, orc):
    """Eight Fibonacci statements over four lanes, every lane's context under the same knob: each proof is
    the oracle's."""
    traces = [generate_fibonacci_trace(a, a + 1, 1 << LOG_N) for a in range(8)]
    pis = [fibonacci_public_values(t) for t in traces]
    tape = ts.air_tape(FibonacciAir(), 3)
    want = [orc.prove(orc.FriConfig(*CFG), tape, t, p) for t, p in zip(traces, pis)]

    def run(ctxs):
        lanes = [(_config(c), _compiled(c, "fib3", lambda: ts.CompiledAir(c, tape))) for c in ctxs[:4]]
        res = ts.prove_batch(lanes, [t.copy() for t in traces], [i % 4 for i in range(8)], public_values=pis)
        return [p.words for p in res.proofs]

    same_everywhere(groups, run, want=want, what="prove_batch")


def _sharded(ctxs, G, cfg, air, trace, pis):
    """One proof over G ranks: G threads of this process, rank r on ctxs[r], the in-process communicator."""
    n = trace.shape[0]
    group = LocalCommGroup(G)
    proofs, errors = [None] * G, [None] * G

    def rank_main(r):
        try:
            c = ctxs[r]
            cair = _compiled(c, ("sharded", air.width()), lambda: ts.CompiledAir(c, ts.air_tape(air, len(pis))))
            rows = np.ascontiguousarray(trace[r * n // G:(r + 1) * n // G])
            proofs[r] = ts.prove_sharded(_config(c, cfg), cair, ts.BfChallenger(), rows, pis, group.comm(r), 4).words
        except BaseException as e:  # noqa: BLE001
            errors[r] = e

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank is stuck in a collective"
    for r in range(G):
        assert errors[r] is None, f"rank {r}: {errors[r]!r}"
    return proofs


# a rank owns whole cosets: two ranks at log_blowup 2 (two cosets each), eight at log_blowup 3 (one each)
@pytest.mark.parametrize("G,cfg", [(2, (2, 6, 8)), (8, (3, 6, 8))], ids=["2-ranks", "8-ranks"])
def test_prove_sharded(groups, orc, G, cfg):
    air, trace, pis = SynthMulAir(64), generate_synth_mul_trace(1 << LOG_N), NO_PIS
    want = orc.prove(orc.FriConfig(*cfg), ts.air_tape(air, 0), trace, pis)
    same_everywhere(groups, lambda ctxs: _sharded(ctxs, G, cfg, air, trace, pis), want=[want] * G,
                    what=f"prove_sharded over {G} ranks")


# ------------------------------------------------------------------ knobs read once per process
PROCESS_KNOBS = {"TS_LEAF_TREE": "0", "TS_LDE_PAIR": "0", "TS_FRI_ROUND_LOG": "0"}
# every Merkle tree of 2^8 leaves and more, the chunk pair, every FRI commit round, and a proof through all three
PROCESS_CASES = [n for n in names("commit-") if "2p0" not in n and "2p3" not in n and "2p5" not in n] + \
    names("chunk-commit-mul5") + names("fri-prove-") + ["prove-mul64"]


def test_once_per_process_knobs(trio, orc, monkeypatch, jit_cache):
    """TS_LEAF_TREE=0 (a leaf launch, level launches, a tree launch), TS_LDE_PAIR=0 (a set of LDE launches per
    quotient chunk) and TS_FRI_ROUND_LOG=0 (every FRI round through the leaf-tree path) in a child process: there
    too the three contexts agree on every case, and with what this process -- and the oracle -- computed."""
    for n in PROCESS_CASES:
        if n not in _digests:  # (run on its own: the tests above have not left their results)
            run_case(trio, orc, monkeypatch, n)
    here = {n: _digests[n] for n in PROCESS_CASES}
    env = dict(os.environ, **PROCESS_KNOBS)
    env.pop(_poison.KNOB, None)
    r = subprocess.run([sys.executable, _poison.__file__] + PROCESS_CASES, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("POISON ")][-1]
    there = json.loads(line[7:])
    assert sorted(there) == sorted(here)
    differ = [n for n in here if there[n] != here[n]]
    assert not differ, f"with {PROCESS_KNOBS} these cases differ from the default launches: {differ}"
