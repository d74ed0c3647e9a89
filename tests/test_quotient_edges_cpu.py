"""CPU twin of tests/test_gpu_quotient_edges.py: the planted traces really put E x E on the rows the quotient
kernels evaluate, the oracle's constraint values on those rows equal plain Python integers (so the oracle is
not the only witness of its own edge cases), and the recorded alpha of the accumulator AIR is what the seeded
search finds and does what the GPU test relies on."""
import numpy as np
import pytest

import _edge_airs as ea
import tapstark_amd as ts
from _field_cases import E, P, R


@pytest.fixture(scope="module")
def planted():
    return ea.planted_matrices()


def test_planted_pairs_cover_e_times_e(planted):
    want = {(a, b) for a in E for b in E}
    rows = {tuple(r) for v in planted for r in v.tolist()}
    assert rows == want, "the (x, y) rows are not E x E"
    across = {(int(v[i, 0]), int(v[i + 1, 0])) for v in planted for i in range(ea.N - 1)}
    assert across == want, "the (x, next x) pairs are not E x E"
    # the pairs uniform data reaches with probability 2^-31 each
    assert sum((a, P - a) in want for a in E) >= 64 and {(a, a) for a in E} <= want and (0, 0) in want


@pytest.mark.parametrize("t", [0, 77, -1])
def test_planted_rows_are_rows_of_the_lde(orc, planted, t):
    v = planted[t]
    lde = orc.commit_lde(ea.trace_of(orc, v), 1, ea.LOG_BLOWUP)
    ea.assert_planted(lde, v)


@pytest.mark.parametrize("name", list(ea.OP_AIRS))
def test_oracle_constraint_values_on_planted_rows(orc, planted, name):
    air, fn = ea.OP_AIRS[name]
    tape = ts.air_tape(air, 0)
    local = np.ascontiguousarray(planted.reshape(-1, 2))
    nxt = np.ascontiguousarray(np.roll(planted, -1, axis=1).reshape(-1, 2))
    sels = np.ones((len(local), 3), dtype=np.uint32)
    got = orc.constraint_values(tape, local, nxt, np.zeros(0, dtype=np.uint32), sels)[:, 0].tolist()
    want = [fn(x, y, nx) for (x, y), (nx, _) in zip(local.tolist(), nxt.tolist())]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{name}: {len(bad)} rows; first: in {local[bad[0]]} next {nxt[bad[0]]} got {got[bad[0]]}"


def test_accumulator_air_values_and_recorded_alpha(orc):
    tape = ts.air_tape(ea.AccumulatorAir(), 0)
    row = np.array([[ea.ACC_VALUE]], dtype=np.uint32)
    got = orc.constraint_values(tape, row, row, np.zeros(0, dtype=np.uint32), np.ones((1, 3), dtype=np.uint32))
    assert got.shape == (1, ea.N_ACC) and (got == ea.ACC_VALUE).all() and ea.ACC_VALUE * R % P == P - 1
    tries, alpha = ea.search_alpha()
    assert (tries, alpha) == (ea.ALPHA_TRIES, ea.ALPHA), "the recorded alpha is not what the seeded search finds"
    peak2, out2, true = ea.accumulator_model(alpha, 2)
    assert peak2 < 2 * P * R and out2 == true, "the real cadence (one lazy_fix per two asserts) must stay in range"
    peak3, out3, _ = ea.accumulator_model(alpha, 3)
    assert peak3 >= 2 * P * R, "a cadence of three must pass 2p 2^32 at least once"
    assert [o % P for o in out3] != true, "and must then compute a different quotient word"


def test_accumulator_program_is_cut_inside_the_sum():
    cair = ts.CompiledAir(None, ts.air_tape(ea.AccumulatorAir(), 0), segment_instr=ea.ACC_SEGMENT_INSTR)
    code = cair.program()["code"]
    asserts = [i for i, ins in enumerate(code) if ins[0] == 7]  # D_ASSERT
    assert len(asserts) == ea.N_ACC
    segs = cair.segment_plan()["segments"]
    cuts = [s["end"] for s in segs[:-1]]
    assert cuts and all(asserts[0] < c <= asserts[-1] for c in cuts), "every cut must fall inside the accumulation"
    # an odd number of asserts before a cut: the closing lazy_fix of a segment is not at the cadence of two
    assert any(sum(a < c for a in asserts) % 2 == 1 for c in cuts)
