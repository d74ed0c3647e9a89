"""Segmented quotient kernels (ts_air_compile_opts) on the GPU: the chunks of ts_quotient_chunks equal the
interpreter's and the oracle's word for word (and the monolithic kernel's where it compiles), whole proofs
equal the default path's through ts_prove, ts_prove_sharded (row ranges, local quotient) and ts_prove_batch
(two lanes sharing one AIR while its kernel set is published), a program above TS_JIT_MAX_INSTR is compiled
in the background and adopted, freeing an AIR kills its compiler children, and TS_JIT_CACHE_DIR keeps every
module.  The reference's counterpart is the monomorphised `Air::eval` inside quotient_values
(uni-stark/src/prover.rs:170-181).  TS_AIR_FUZZ=<n> widens the seed campaign."""
import glob
import os
import threading
import time

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd.airs import (RandomAir, SynthExtAir, SynthMulAir, generate_random_air_trace,
                               generate_synth_ext_trace, generate_synth_mul_trace, random_air_case,
                               splitmix64_stream)

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get("TS_AIR_FUZZ", "50"))
N_CHUNKS = 5
COMPILE_BUDGET_S = 120.0


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def _wait(cair, budget=COMPILE_BUDGET_S):
    """jit_wait on a thread: a compilation past the budget fails the test instead of hanging it."""
    res = []
    t = threading.Thread(target=lambda: res.append(cair.jit_wait()), daemon=True)
    t.start()
    t.join(budget)
    assert res, f"the background compilation did not finish within {budget} s"
    return res[0]


def _segmented(ctx, tape, S, jobs=None):
    cair = ts.CompiledAir(ctx, tape, segment_instr=S, jit_jobs=jobs)
    state, secs = _wait(cair)
    assert state == 3 and cair.is_jit, f"segmented compilation failed (state {state})"
    assert len(cair.segment_plan()["segments"]) > 1
    return cair


def _interp(ctx, tape, monkeypatch):
    with monkeypatch.context() as m:
        m.setenv("TS_NO_JIT", "1")
        cair = ts.CompiledAir(ctx, tape)
    assert not cair.is_jit
    return cair


def _chunks(pcs, data, cair, pis, alpha):
    return np.stack([c.download() for c in pcs.quotient_chunks(data, cair, pis, alpha)])


def _parity(ctx, orc, monkeypatch, tape, trace, pis, S, seed, mono=True):
    log_n = int(np.log2(trace.shape[0]))
    lqd = orc.log_quotient_degree(tape)
    b = max(lqd, 1)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(b, 3, 2), ctx)
    _, data = pcs.commit([((log_n, 1), trace.copy())])
    alpha = splitmix64_stream(seed + 9, 4)
    want = orc.split_quotient(orc.quotient_values(tape, orc.commit_lde(trace, 1, b), log_n, b, pis, alpha), log_n, lqd)
    seg = _segmented(ctx, tape, S)
    got = _chunks(pcs, data, seg, pis, alpha)
    assert (got == _chunks(pcs, data, _interp(ctx, tape, monkeypatch), pis, alpha)).all(), f"{seed}: vs interpreter"
    assert (got == want).all(), f"{seed}: vs oracle"
    if mono:
        plain = ts.CompiledAir(ctx, tape)
        if plain.is_jit or _wait(plain)[0] == 3:
            assert (got == _chunks(pcs, data, plain, pis, alpha)).all(), f"{seed}: vs monolithic kernel"


@pytest.mark.parametrize("S", [16, 64])
@pytest.mark.parametrize("which", ["SynthMulAir-64", "SynthExt-163"])
def test_synth_airs(ctx, orc, monkeypatch, which, S):
    n = 1 << 8
    if which == "SynthMulAir-64":
        tape, trace = ts.air_tape(SynthMulAir(64), 0), generate_synth_mul_trace(n)
    else:
        tape, trace = ts.air_tape(SynthExtAir(163), 0), generate_synth_ext_trace(n)
    _parity(ctx, orc, monkeypatch, tape, trace, np.zeros(0, dtype=np.uint32), S, 1)


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_random_airs(ctx, orc, monkeypatch, chunk):
    per = (N_SEEDS + N_CHUNKS - 1) // N_CHUNKS
    for seed in range(chunk * per, min((chunk + 1) * per, N_SEEDS)):
        air, log_n = random_air_case(seed)
        tape = ts.air_tape(air, air.n_public)
        if len(ts.CompiledAir(None, tape).program()["code"]) <= 64:
            continue  # the monolithic route
        n = 1 << max(log_n, 3)
        if air.valid:
            trace, pis, _ = generate_random_air_trace(air, n)
        else:
            trace = splitmix64_stream(seed + 1, n * air.width()).reshape(n, air.width())
            pis = splitmix64_stream(seed + 2, max(air.n_public, 1))[:air.n_public]
        _parity(ctx, orc, monkeypatch, tape, trace, pis, 64, seed, mono=False)


CFG3 = (2, 28, 8)


def test_whole_proofs(ctx, monkeypatch):
    """SynthMulAir-64 at 2^12 rows with S = 32: ts_prove, and a 2-rank ts_prove_sharded with the local
    quotient (row ranges and coset shifts), give the default path's proof words; ts_verify accepts."""
    from tapstark_amd.comm import LocalCommGroup

    tape = ts.air_tape(SynthMulAir(64), 0)
    n = 1 << 12
    trace = generate_synth_mul_trace(n)
    pis = np.zeros(0, dtype=np.uint32)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG3), ctx))
    want = ts.prove(config, ts.CompiledAir(ctx, tape), ts.BfChallenger(), trace.copy(), pis).words
    seg = _segmented(ctx, tape, 32)
    got = ts.prove(config, seg, ts.BfChallenger(), trace.copy(), pis).words
    assert len(got) == len(want) and (got == want).all()
    ts.verify(config, SynthMulAir(64), ts.BfChallenger(), got, pis)

    G = 2
    ctxs = [ts.Context(0) for _ in range(G)]
    airs = [_segmented(c, tape, 32) for c in ctxs]
    for localq in (False, True):
        group = LocalCommGroup(G)
        out = [None] * G

        def rank(r):
            conf = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG3), ctxs[r]))
            rows = np.ascontiguousarray(trace[r * n // G:(r + 1) * n // G])
            out[r] = ts.prove_sharded(conf, airs[r], ts.BfChallenger(), rows, pis, group.comm(r), min_local_log=2,
                                      local_quotient=localq).words

        threads = [threading.Thread(target=rank, args=(r,)) for r in range(G)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(300)
        for r in range(G):
            assert out[r] is not None and (out[r] == want).all(), f"rank {r} localq={localq}"


def test_past_the_budget(ctx, orc, monkeypatch):
    """37k lowered instructions, above TS_JIT_MAX_INSTR (the monolithic kernel is never compiled): compiled in
    the background by J children while the interpreter proves, then adopted; same proof either way."""
    air = RandomAir(4242, 200, 6000, 5, n_public=4, share_pct=20, max_depth=7)
    tape = ts.air_tape(air, 4)
    log_n, b = 6, 2
    n = 1 << log_n
    trace = splitmix64_stream(99, n * 200).reshape(n, 200)
    pis = splitmix64_stream(98, 4)
    monkeypatch.delenv("TS_JIT_CACHE_DIR", raising=False)  # a cache of an earlier run would skip the children
    t0 = time.time()
    cair = ts.CompiledAir(ctx, tape, segment_instr=1024)
    assert time.time() - t0 < 10 and not cair.is_jit
    assert len(cair.program()["code"]) > 32768
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(b, 3, 2), ctx))
    interp = _interp(ctx, tape, monkeypatch)
    want = ts.prove(config, interp, ts.BfChallenger(), trace.copy(), pis).words
    state, secs = _wait(cair)
    assert state == 3 and secs > 0 and cair.is_jit
    got = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), pis).words
    assert len(got) == len(want) and (got == want).all()


def _jitc_children():
    me, out = os.getpid(), []
    for stat in glob.glob("/proc/[0-9]*/stat"):
        try:
            with open(stat) as f:
                s = f.read()
        except OSError:
            continue
        comm = s[s.index("(") + 1:s.rindex(")")]
        ppid = int(s[s.rindex(")") + 2:].split()[1])
        if ppid == me and comm.startswith("ts_jitc"):
            out.append(int(stat.split("/")[2]))
    return out


def test_free_kills_children(ctx, monkeypatch):
    monkeypatch.delenv("TS_JIT_CACHE_DIR", raising=False)
    air = RandomAir(4242, 200, 1000, 5, n_public=4, share_pct=35, max_depth=7)
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 4), segment_instr=256, jit_jobs=4)
    assert not cair.is_jit and len(_jitc_children()) == 4
    del cair
    assert _jitc_children() == []


def test_batch_lanes_share_one_air(ctx, monkeypatch):
    """Two ts_prove_batch lanes prove with one segmented AIR while its compilation finishes and the kernel set
    is published: every proof is the interpreter's."""
    tape = ts.air_tape(SynthExtAir(163), 0)
    n = 1 << 10
    traces = [generate_synth_ext_trace(n, seed=100 + i) for i in range(12)]
    ref_conf = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG3), ctx))
    interp = _interp(ctx, tape, monkeypatch)
    want = [ts.prove(ref_conf, interp, ts.BfChallenger(), t.copy(), np.zeros(0, dtype=np.uint32)).words for t in traces]
    ctxs = [ts.Context(0) for _ in range(2)]
    monkeypatch.delenv("TS_JIT_CACHE_DIR", raising=False)
    shared = ts.CompiledAir(ctxs[0], tape, segment_instr=16, jit_jobs=2)
    lanes = [(ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG3), c)), shared) for c in ctxs]
    deadline, after = time.time() + COMPILE_BUDGET_S, 0
    while after < 2:  # rounds while the children compile, the one that adopts the set, and one more
        res = ts.prove_batch(lanes, [t.copy() for t in traces], [i % 2 for i in range(12)], public_values=[])
        assert (res.status == 0).all()
        for i in range(12):
            assert (res.proofs[i].words == want[i]).all(), f"item {i}"
        after += shared.is_jit
        assert time.time() < deadline, "the background compilation did not finish within the budget"
    assert _wait(shared)[0] == 3


def test_module_cache(ctx, monkeypatch, tmp_path):
    """TS_JIT_CACHE_DIR: each of the J modules under its own key; a second compile loads them all without
    starting a child and computes the same chunks."""
    monkeypatch.setenv("TS_JIT_CACHE_DIR", str(tmp_path))
    tape = ts.air_tape(SynthExtAir(163), 0)
    first = _segmented(ctx, tape, 64, jobs=3)
    assert len(glob.glob(str(tmp_path / "q_*.co"))) == 3
    t0 = time.time()
    again = ts.CompiledAir(ctx, tape, segment_instr=64, jit_jobs=3)
    assert again.is_jit and time.time() - t0 < 1.0 and _jitc_children() == []
    assert again.jit_wait()[0] == 3
    n = 1 << 8
    trace = generate_synth_ext_trace(n)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), ctx)
    _, data = pcs.commit([((8, 1), trace.copy())])
    alpha = splitmix64_stream(3, 4)
    assert (_chunks(pcs, data, first, np.zeros(0, dtype=np.uint32), alpha) == _chunks(pcs, data, again, np.zeros(0, dtype=np.uint32), alpha)).all()
