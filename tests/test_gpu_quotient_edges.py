"""Planted edge operands through all three constraint compilers (tests/_edge_airs.py): single-operation AIRs
whose operands run over E x E on the very rows the quotient kernels evaluate -- through the hiprtc-specialised
kernel (jit.cpp and its own copy of the field helpers), the interpreter (TS_NO_JIT=1) and the segmented kernels
(segments of one instruction, so that the result of the operation crosses a cut through the slab) -- and one
accumulator AIR that drives the lazy 64-bit sums of the specialised kernels to the edge of their range,
monolithic and cut into segments.  Every quotient chunk equals orc.quotient_values / split_quotient bit for
bit; tests/test_quotient_edges_cpu.py checks the oracle's constraint values on the same rows against Python
integers."""
import numpy as np
import pytest

import _edge_airs as ea
import tapstark_amd as ts
from _field_cases import P

pytestmark = pytest.mark.gpu
ZERO_PIS = np.zeros(0, dtype=np.uint32)


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(scope="module")
def pcs(ctx):
    return ts.TwoAdicFriPcs(ts.FriConfig(ea.LOG_BLOWUP, 4, 8), ctx)


@pytest.fixture(scope="module")
def planted(pcs, orc):
    """[(committed trace, oracle LDE)] of every planted matrix: computed once, left unchanged."""
    out = []
    for v in ea.planted_matrices():
        trace = ea.trace_of(orc, v)
        lde = orc.commit_lde(trace, 1, ea.LOG_BLOWUP)
        ea.assert_planted(lde, v)
        out.append((pcs.commit([((ea.LOG_N, 1), trace.copy())])[1], lde))
    return out


@pytest.fixture(scope="module")
def wanted(orc, planted):
    """The oracle's chunks per AIR, shared by the three compilers."""
    cache = {}

    def get(name, tape, alpha):
        if name not in cache:
            lqd = orc.log_quotient_degree(tape)
            cache[name] = [orc.split_quotient(orc.quotient_values(tape, lde, ea.LOG_N, ea.LOG_BLOWUP, ZERO_PIS, alpha),
                                              ea.LOG_N, lqd) for _, lde in planted]
        return cache[name]

    return get


def compiled(ctx, tape, how, monkeypatch, segment_instr=ea.OP_SEGMENT_INSTR):
    if how == "interp":
        with monkeypatch.context() as m:
            m.setenv("TS_NO_JIT", "1")
            cair = ts.CompiledAir(ctx, tape)
        assert not cair.is_jit
        return cair
    cair = ts.CompiledAir(ctx, tape) if how == "jit" else ts.CompiledAir(ctx, tape, segment_instr=segment_instr)
    if not cair.is_jit:
        assert cair.jit_wait()[0] == 3, "the specialised kernel did not load"
    assert cair.is_jit
    if how == "segmented":  # a program of at most segment_instr instructions would take the monolithic route
        assert len(cair.segment_plan()["segments"]) > 1, "the AIR was not cut into segments"
    return cair


def chunks_of(pcs, data, cair, alpha):
    return np.stack([c.download() for c in pcs.quotient_chunks(data, cair, ZERO_PIS, alpha)])


@pytest.mark.parametrize("how", ["jit", "interp", "segmented"])
@pytest.mark.parametrize("name", list(ea.OP_AIRS))
def test_single_op_air_on_planted_edges(ctx, pcs, planted, wanted, monkeypatch, name, how):
    tape = ts.air_tape(ea.OP_AIRS[name][0], 0)
    alpha = np.full(4, P - 1, dtype=np.uint32)
    cair = compiled(ctx, tape, how, monkeypatch)
    assert cair.log_quotient_degree == 0, "the quotient domain must be the planted coset"
    if how == "segmented":
        assert cair.segment_plan()["slab_width"] >= 1, "the operation's result must cross a cut through the slab"
    want = wanted(name, tape, alpha)
    for t, (data, _) in enumerate(planted):
        got = chunks_of(pcs, data, cair, alpha)
        assert got.shape == want[t].shape and (got == want[t]).all(), \
            f"{name} via {how}, planted trace {t}: {int((got != want[t]).sum())} words differ"


@pytest.mark.parametrize("how", ["jit", "interp", "segmented"])
def test_accumulator_air_at_the_edge_of_the_lazy_range(ctx, pcs, orc, monkeypatch, how):
    """66 constraint values of Montgomery form p - 1 against the alpha of the seeded search (ea.ALPHA, found and
    checked on the CPU): one lazy_fix per two asserts stays below 2p 2^32, one per three would not, and would
    write a different word.  `segmented` cuts the sum five times (after an odd number of asserts too) and
    carries the eight accumulator words through the slab."""
    tape = ts.air_tape(ea.AccumulatorAir(), 0)
    alpha = np.array(ea.ALPHA, dtype=np.uint32)
    trace = np.full((ea.N, 1), ea.ACC_VALUE, dtype=np.uint32)
    lde = orc.commit_lde(trace, 1, ea.LOG_BLOWUP)
    assert (lde == ea.ACC_VALUE).all()
    cair = compiled(ctx, tape, how, monkeypatch, segment_instr=ea.ACC_SEGMENT_INSTR)
    if how == "segmented":
        assert len(cair.segment_plan()["segments"]) == 6
    want = orc.split_quotient(orc.quotient_values(tape, lde, ea.LOG_N, ea.LOG_BLOWUP, ZERO_PIS, alpha), ea.LOG_N,
                              cair.log_quotient_degree)
    _, data = pcs.commit([((ea.LOG_N, 1), trace.copy())])
    got = chunks_of(pcs, data, cair, alpha)
    assert got.shape == want.shape and (got == want).all(), f"{int((got != want).sum())} words differ"
