"""The interpreter kernels (quotient.hip k_quotient / k_check_constraints, one shared program body) where a
persistent grid makes MORE THAN ONE TRIP over the row tiles and where the last tile has INACTIVE LANES: the
fuzz (test_gpu_air_fuzz.py) never caps the register-file slab, so every workgroup there sees one tile.

The AIR has 144 live registers (above the 48 that go to LDS), so the register file is a global slab of
144 x 64 words per workgroup; TS_INTERP_SLAB_MB=1 caps the grid at 2^18 / (144 x 64) = 28 workgroups of 64 rows:
* quotient_chunks, trace height 2^12: a domain of 2^14 rows = 256 tiles, 10 trips
* check_constraints, 2^13 rows = 128 tiles, 5 trips (31 workgroups for the valid AIR's 132 registers)
* quotient_chunks, trace height 2^3: 32 rows, half a wavefront
Everything is compared with the CPU oracle word for word."""
import pytest

import tapstark_amd as ts
from tapstark_amd.airs import RandomAir, generate_random_air_trace, splitmix64_stream

pytestmark = pytest.mark.gpu

W, N_PUBLIC = 200, 4


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def _air(valid: bool):
    air = RandomAir(4242, W, 300, 5, n_public=N_PUBLIC, valid=valid, share_pct=35, max_depth=6)
    return air, ts.air_tape(air, N_PUBLIC)


def _interpreter(ctx, tape, monkeypatch, slab_mb="1", lds=False):
    """The AIR on the interpreter; the knobs are read at every launch, so they stay set for the test."""
    monkeypatch.setenv("TS_NO_JIT", "1")
    monkeypatch.setenv("TS_INTERP_SLAB_MB", slab_mb)
    if lds:  # 144 registers x 64 lanes in LDS: the <64, false> instantiations
        monkeypatch.setenv("TS_INTERP_LDS_MAX_REGS", "1000000")
    cair = ts.CompiledAir(ctx, tape)
    assert not cair.is_jit and cair.program()["n_regs"] > 64
    return cair


def _quotient_case(ctx, orc, cair, tape, log_n):
    n = 1 << log_n
    trace = splitmix64_stream(7 + log_n, n * W).reshape(n, W)
    pis = splitmix64_stream(8, N_PUBLIC)
    alpha = splitmix64_stream(9, 4)
    lqd = orc.log_quotient_degree(tape)
    assert lqd == 2
    want = orc.split_quotient(orc.quotient_values(tape, orc.commit_lde(trace, 1, lqd), log_n, lqd, pis, alpha),
                              log_n, lqd)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(lqd, 3, 2), ctx)
    _, data = pcs.commit([((log_n, 1), trace.copy())])
    chunks = pcs.quotient_chunks(data, cair, pis, alpha)
    assert len(chunks) == want.shape[0] == 4
    for c, ch in enumerate(chunks):
        got = ch.download()
        assert (got == want[c]).all(), f"log_n {log_n}: chunk {c}: {int((got != want[c]).sum())} words differ"


def test_quotient_many_trips(ctx, orc, monkeypatch):
    _, tape = _air(False)
    _quotient_case(ctx, orc, _interpreter(ctx, tape, monkeypatch), tape, 12)


@pytest.mark.parametrize("lds", [False, True])
def test_quotient_inactive_lanes(ctx, orc, monkeypatch, lds):
    _, tape = _air(False)
    _quotient_case(ctx, orc, _interpreter(ctx, tape, monkeypatch, lds=lds), tape, 3)


def test_check_constraints_many_trips(ctx, orc, monkeypatch):
    n = 1 << 13
    # no trace satisfies the free-form AIR: every row reports, the smallest report wins across the trips
    _, tape = _air(False)
    cair = _interpreter(ctx, tape, monkeypatch)
    trace = splitmix64_stream(11, n * W).reshape(n, W)
    pis = splitmix64_stream(8, N_PUBLIC)
    bad = trace.copy()
    bad[n - 1, 5] ^= 1
    for t in (trace, bad):
        assert ts.check_constraints(cair, t, pis, ctx) == orc.check_constraints(tape, t, pis)
    # a trace that satisfies the structured AIR, then one cell of the LAST row changed: the reports (the
    # transition into that row is the first) come from the last tile, which a workgroup reaches on its last trip
    air, tape = _air(True)
    cair = _interpreter(ctx, tape, monkeypatch)
    trace, pis, _ = generate_random_air_trace(air, n)
    assert ts.check_constraints(cair, trace, pis, ctx) == orc.check_constraints(tape, trace, pis) == -1
    bad = trace.copy()
    bad[n - 1, 0] ^= 1
    want = orc.check_constraints(tape, bad, pis)
    assert (want >> 16) // 64 == n // 64 - 1
    assert ts.check_constraints(cair, bad, pis, ctx) == want


def test_check_constraints_inactive_lanes(ctx, orc, monkeypatch):
    """8 rows in a workgroup of 64, register file in the slab and in LDS."""
    air, tape = _air(True)
    trace, pis, _ = generate_random_air_trace(air, 8)
    bad = trace.copy()
    bad[7, 0] ^= 1
    for lds in (False, True):
        cair = _interpreter(ctx, tape, monkeypatch, lds=lds)
        assert ts.check_constraints(cair, trace, pis, ctx) == orc.check_constraints(tape, trace, pis) == -1
        assert ts.check_constraints(cair, bad, pis, ctx) == orc.check_constraints(tape, bad, pis) != -1
