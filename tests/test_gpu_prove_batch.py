"""ts_prove_batch on the GPU: many distinct statements in one call (reference uni-stark/src/prover.rs:25-39,
one call each), every proof returned.  Each item's proof is ts_prove's and the oracle's; host traces (pageable
or pinned), pre-observed challengers, lanes with different AIRs, per-item failures and the start gate are
covered, and config 3 at full size is checked through the returned Blake3 digests.  At most 4 contexts."""
import os
import sys

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.airs import (FibonacciAir, SynthMulAir, fibonacci_public_values, generate_fibonacci_trace,
                               generate_synth_mul_trace)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _digests import hexd, load_large  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = (2, 28, 8)  # uni-stark/tests/fib_air.rs:119-129
TS_ERR_INVALID, TS_ERR_BUFFER = 1, 6
# 12 statements: different starts (a, b), 2^10 .. 2^12 rows
STMTS = [(i + 1, 2 * i + 3, 1 << (10 + i % 3)) for i in range(12)]


class Env:
    def __init__(self):
        from tapstark_amd.build import build

        build()
        self.ctxs = [ts.default_context()] + [ts.Context(0) for _ in range(3)]
        self.fib_tape = ts.air_tape(FibonacciAir(), 3)
        self.mul_tape = ts.air_tape(SynthMulAir(7), 0)
        self.fib = [self.lane(c, self.fib_tape) for c in self.ctxs]
        self.mul = [self.lane(c, self.mul_tape) for c in self.ctxs]

    @staticmethod
    def lane(ctx, tape, cfg=CFG):
        return ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx)), ts.CompiledAir(ctx, tape)


@pytest.fixture(scope="module")
def env():
    return Env()


def host_trace(i):
    a, b, n = STMTS[i]
    return generate_fibonacci_trace(a, b, n)


def pis_of(i):
    return fibonacci_public_values(host_trace(i))


@pytest.fixture(scope="module")
def fib_want(env, orc):
    return [orc.prove(orc.FriConfig(*CFG), env.fib_tape, host_trace(i), pis_of(i)) for i in range(len(STMTS))]


def device_trace(env, lane, i):
    a, b, n = STMTS[i]
    return ts.DeviceMatrix.fibonacci(env.ctxs[lane], a, b, n)


def same(proof, want):
    return proof is not None and len(proof.words) == len(want) and bool((proof.words == want).all())


def test_distinct_statements_are_prove_and_oracle(env, fib_want):
    n = len(STMTS)
    lane_of = [i % 3 for i in range(n)]
    res = ts.prove_batch(env.fib[:3], [device_trace(env, lane_of[i], i) for i in range(n)], lane_of,
                         public_values=[pis_of(i) for i in range(n)])
    assert res.rc == 0 and (res.status == 0).all()
    assert (res.wall_ms > 0).all() and res.digests is None
    for i in range(n):
        assert same(res.proofs[i], fib_want[i]), f"item {i} differs from the oracle"
        conf, air = env.fib[lane_of[i]]
        direct = ts.prove(conf, air, ts.BfChallenger(), device_trace(env, lane_of[i], i), pis_of(i))
        assert same(res.proofs[i], direct.words), f"item {i} differs from ts_prove"
        conf0 = env.fib[0][0]
        ts.verify(conf0, FibonacciAir(), ts.BfChallenger(), res.proofs[i], pis_of(i))
        with pytest.raises(ts.VerificationError) as e:
            ts.verify(conf0, FibonacciAir(), ts.BfChallenger(), res.proofs[i], pis_of((i + 1) % n))
        assert e.value.code == 7  # OodEvaluationMismatch


def test_host_traces_pageable_and_pinned(env, fib_want):
    n = len(STMTS)
    lane_of = [(i + 1) % 3 for i in range(n)]
    pinned = []
    for i in range(n):
        t = host_trace(i)
        p = ts.PinnedHostMatrix(*t.shape)
        p.array[:] = t
        pinned.append(p)
    for traces in ([host_trace(i) for i in range(n)], pinned):
        res = ts.prove_batch(env.fib[:3], traces, lane_of, public_values=[pis_of(i) for i in range(n)])
        for i in range(n):
            assert same(res.proofs[i], fib_want[i]), f"item {i} ({type(traces[i]).__name__})"


def test_challengers_are_cloned_and_final_states_returned(env, fib_want):
    ch_a = ts.BfChallenger()
    ch_a.observe(7)
    ch_a.observe(11)
    ch_b = ts.BfChallenger()
    ch_b.observe_commitment(np.arange(1, 9, dtype=np.uint32))
    ch_b.observe(3)
    chals = [ch_a, ch_b, ch_a, None]  # ch_a serves two items on two lanes
    before = [ch_a.state(), ch_b.state()]
    lane_of = [0, 1, 2, 0]
    res = ts.prove_batch(env.fib[:3], [device_trace(env, lane_of[i], i) for i in range(4)], lane_of,
                         public_values=[pis_of(i) for i in range(4)], challengers=chals)
    assert (res.status == 0).all()
    assert (ch_a.state() == before[0]).all() and (ch_b.state() == before[1]).all(), "a caller's challenger changed"
    for i in range(4):
        clone = (chals[i] or ts.BfChallenger()).clone()
        conf, air = env.fib[lane_of[i]]
        direct = ts.prove(conf, air, clone, device_trace(env, lane_of[i], i), pis_of(i))
        assert same(res.proofs[i], direct.words), f"item {i} differs from ts_prove on a clone"
        assert (res.final_states[i] == clone.state()).all(), f"item {i}: final challenger state"
        ts.verify(conf, FibonacciAir(), (chals[i] or ts.BfChallenger()).clone(), res.proofs[i], pis_of(i))
    assert not same(res.proofs[0], fib_want[0]), "the pre-observed challenger was not used"
    assert same(res.proofs[3], fib_want[3])


def test_config3_full_size_digests(env, orc):
    want = load_large("config3")
    cfg = (want["log_blowup"], want["num_queries"], want["proof_of_work_bits"])
    tape = ts.air_tape(SynthMulAir(64), 0)
    lanes = [Env.lane(c, tape, cfg) for c in env.ctxs]
    n = 1 << want["log_n"]
    lane_of = [i % 4 for i in range(8)]
    mats = [ts.DeviceMatrix.synth_mul(env.ctxs[lane_of[i]], n, 64) for i in range(8)]
    res = ts.prove_batch(lanes, mats, lane_of, public_values=[], gate_ms=1.0, digests=True)
    assert (res.status == 0).all()
    for i in range(8):
        assert res.n_words[i] == want["proof_words"]
        assert hexd(res.digests[i]) == want["proof_blake3"], f"proof {i}: digest differs from the fixture"
        assert orc.blake3(res.proofs[i].words.tobytes()).hex() == want["proof_blake3"], f"proof {i}: words"


def test_lanes_with_different_airs(env, orc, fib_want):
    mul = [generate_synth_mul_trace(1 << 10, 7, seed=77 + i) for i in range(2)]
    lanes = [env.fib[0], env.mul[1]]
    traces = [device_trace(env, 0, 0), mul[0], host_trace(1), ts.DeviceMatrix.upload(env.ctxs[1], mul[1])]
    lane_of = [0, 1, 0, 1]
    pis = [pis_of(0), [], pis_of(1), []]
    res = ts.prove_batch(lanes, traces, lane_of, public_values=pis)
    assert (res.status == 0).all()
    assert same(res.proofs[0], fib_want[0]) and same(res.proofs[2], fib_want[1])
    ocfg = orc.FriConfig(*CFG)
    for i, t in ((1, mul[0]), (3, mul[1])):
        assert same(res.proofs[i], orc.prove(ocfg, env.mul_tape, t, [])), f"SynthMul-7 item {i}"


def test_failures_stay_with_their_item(env, fib_want):
    lane_of = [0, 1, 2, 0]
    pis = [pis_of(i) for i in range(4)]
    # a buffer that is too small: that item alone, with the size it needs
    res = ts.prove_batch(env.fib[:3], [device_trace(env, lane_of[i], i) for i in range(4)], lane_of,
                         public_values=pis, check=False, _cap_words=[None, None, 100, None])
    assert res.rc == TS_ERR_BUFFER
    assert list(res.status) == [0, 0, TS_ERR_BUFFER, 0]
    assert res.n_words[2] == len(fib_want[2]) and res.proofs[2] is None
    for i in (0, 1, 3):
        assert same(res.proofs[i], fib_want[i])

    # a wrong width, an already-consumed trace, a lane that does not exist
    spent = device_trace(env, 2, 2)
    conf, air = env.fib[2]
    ts.prove(conf, air, ts.BfChallenger(), spent, pis[2])
    traces = [device_trace(env, 0, 0), np.zeros((1024, 3), dtype=np.uint32), spent, device_trace(env, 0, 3),
              host_trace(1)]
    res = ts.prove_batch(env.fib[:3], traces, lane_of + [7], public_values=pis + [pis[1]], check=False)
    assert res.rc == TS_ERR_INVALID
    assert list(res.status) == [0, TS_ERR_INVALID, TS_ERR_INVALID, 0, TS_ERR_INVALID]
    assert "width" in res.errors[1] and "consumed" in res.errors[2]
    assert same(res.proofs[0], fib_want[0]) and same(res.proofs[3], fib_want[3])
    with pytest.raises(_lib.TsError) as e:  # check=True: the first failed item, after every item ran
        ts.prove_batch(env.fib[:1], [np.zeros((1024, 3), dtype=np.uint32)], [0], public_values=pis[0])
    assert e.value.code == TS_ERR_INVALID

    # another struct layout refuses the whole call and consumes nothing
    mats = [device_trace(env, i, i) for i in range(3)]
    with pytest.raises(_lib.TsError) as e:
        ts.prove_batch(env.fib[:3], mats, [0, 1, 2], public_values=pis[:3], _struct_size=8)
    assert e.value.code == TS_ERR_INVALID
    for i in range(3):
        conf, air = env.fib[i]
        assert same(ts.prove(conf, air, ts.BfChallenger(), mats[i], pis[i]), fib_want[i])


def test_gate_spaces_the_starts(env):
    n, gate = 9, 2.0
    lane_of = [i % 3 for i in range(n)]
    idx = [3 * (i % 4) for i in range(n)]  # 2^10-row statements
    res = ts.prove_batch(env.fib[:3], [device_trace(env, lane_of[i], idx[i]) for i in range(n)], lane_of,
                         public_values=[pis_of(j) for j in idx], gate_ms=gate)
    assert (res.status == 0).all() and (res.wall_ms > 0).all()
    s = np.sort(res.start_ms)
    # the start stamp is taken inside the gate's critical section: the spacing holds by construction
    assert (np.diff(s) >= gate - 1e-3).all(), np.diff(s)


def test_cpp_batch_example(env, tmp_path):
    import subprocess

    from test_abi_cpu import _build_example
    exe = _build_example(tmp_path, "prove_batch")
    r = subprocess.run([exe, "16", "12"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "16 accepted" in r.stdout and "16 refused" in r.stdout
