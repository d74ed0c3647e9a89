"""AIRs with challenge-phase (aux) columns on the GPU: the LogUp builder against Python integers, the quotient
kernels and check_constraints over (aux, main), whole TSPF v4 proofs, the rejections, the refusals and the
callback.  The reference has one trace phase, so exactness comes from the equalities test_gpu_preprocessed.py
uses for a key:

* the quotient of an AIR with A aux and W main columns is, row by row, the quotient of the joined AIR over
  hstack(aux, main) with the public vector pis ++ challenges ++ exposed, which the oracle and the existing
  ts_quotient_chunks compute;
* a whole proof is the composition of oracle-tested ABI stages -- ts_pcs_commit, ts_pcs_open, the host
  challenger -- around that quotient;
* the LogUp constraints determine the aux matrix from trace and challenges (no denominator is zero), and a
  Python-integer EF4 computes it.

The CPU half is tests/test_air_aux_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib, taptree as tt
from tapstark_amd.air import LogUp, SymbolicAirBuilder, aux_dims
from tapstark_amd.airs import (RangeLookupAir, generate_random_air_trace, generate_range_lookup_trace,
                               random_air_case, splitmix64_stream)
from tapstark_amd.comm import LocalCommGroup
from _aux_airs import aux_width_of, join_tape_aux, logup_reference, split_publics, split_tape_aux

pytestmark = pytest.mark.gpu
P = 0x78000001
G27 = 0x1A427A41
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_UNSUPPORTED, TS_ERR_INVARIANT = 1, 4, 5
SEEDS = [s for s in range(36) if random_air_case(s)[0].width() >= 2]
VALID_SEEDS = [s for s in SEEDS if s % 3 == 0]
SEGMENT_SEEDS = [0, 6, 9, 12, 21, 27]
TALL_SEED = next(s for s in VALID_SEEDS if random_air_case(s)[0].valid)  # checked again at n = 2^10
WAIT_JIT_INSTR = 3000  # larger programs stay on the interpreter in the specialised pass, as in test_gpu_air_fuzz.py


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def _challenges(seed, n=2):
    return (splitmix64_stream(seed, 4 * n) % np.uint64(P)).astype(np.uint32)


# ------------------------------------------------------------------ 1. ts_logup_aux_build
# main columns (a, b, c, m): K = 1 with a tuple of three values, one of them a constant, and the multiplicity
# p - 1; K = 2 with a multiplicity column; K = 3 (an odd last group) with all three kinds of multiplicity
SPECS = {
    1: [(("const", P - 1), [("col", 0), ("const", 5), ("col", 1)])],
    2: [(("const", 1), [("col", 0)]), (("col", 3), [("col", 1)])],
    3: [(("col", 3), [("col", 0), ("col", 1), ("const", 7)]), (("const", 1), [("col", 2)]),
        (("const", P - 1), [("col", 1)])],
}


def _logup_trace(n, seed=3):
    t = (splitmix64_stream(seed + n, 4 * n) % np.uint64(P)).reshape(n, 4).astype(np.uint32)
    t[0, :] = (0, 1, P - 1, 0)  # edge values in the first row
    return t


def _build_and_compare(ctx, n, K, seed):
    lu = LogUp(SPECS[K])
    trace = _logup_trace(n)
    ch = _challenges(seed + K)
    want_aux, want_S = logup_reference(lu.interactions, trace, ch[:4], ch[4:])
    aux, S = lu.build(ts.DeviceMatrix.upload(ctx, trace), ch)
    got = aux.download()
    assert got.shape == want_aux.shape == (n, lu.aux_width)
    assert (got == want_aux).all(), f"n={n} K={K}: {int((got != want_aux).sum())} aux words differ, first row " \
                                    f"{int(np.flatnonzero((got != want_aux).any(axis=1))[0])}"
    assert (S == want_S).all(), f"n={n} K={K}: S differs"


@pytest.mark.parametrize("log_n", range(1, 14))
def test_logup_build_vs_python_integers(ctx, log_n):
    """Default block size: a workgroup owns 1024 rows, four consecutive rows per thread, so a wave covers 256.
    n <= 2^8 stays inside one wave; n = 2^9, 2^10 crosses waves inside one workgroup (the LDS leg of the scan);
    n >= 2^11 crosses workgroups (2 .. 8 totals, one pass of the totals scan).  The pass boundary of the totals
    scan (128 totals) is crossed by test_logup_build_small_blocks."""
    for K in (1, 2, 3):
        _build_and_compare(ctx, 1 << log_n, K, 100 + log_n)


@pytest.mark.parametrize("block_rows", [1, 3, 64, 300])
def test_logup_build_small_blocks(ctx, monkeypatch, block_rows):
    """TS_LOGUP_BLOCK_ROWS at n = 2^8: 1 row per workgroup gives 256 totals, two passes of the 128-wide totals
    scan; 3 gives 86 workgroups with a short last one; 64 one wave per workgroup; 300 two rows per thread and a
    workgroup that ends past the last row."""
    monkeypatch.setenv("TS_LOGUP_BLOCK_ROWS", str(block_rows))
    for K in (1, 2, 3):
        _build_and_compare(ctx, 1 << 8, K, 200 + block_rows)


def test_logup_block_rows_knob_is_checked(ctx, monkeypatch):
    lu = LogUp(SPECS[2])
    m = ts.DeviceMatrix.upload(ctx, _logup_trace(8))
    for bad in ("0", "1025", "-4"):
        monkeypatch.setenv("TS_LOGUP_BLOCK_ROWS", bad)
        with pytest.raises(_lib.TsError) as e:
            lu.build(m, _challenges(1))
        assert e.value.code == TS_ERR_INVALID
    monkeypatch.delenv("TS_LOGUP_BLOCK_ROWS")
    bad_col = LogUp([(("const", 1), [("col", 4)])])  # a column outside the trace
    with pytest.raises(_lib.TsError) as e:
        bad_col.build(m, _challenges(1))
    assert e.value.code == TS_ERR_INVALID
    assert m.dims() == (8, 4)  # the trace is never consumed


def test_logup_two_million_rows(ctx):
    """2^21 rows, no Python reference: the constraints hold on the device (they determine the aux matrix), and a
    true permutation of the table sums to zero.  2048 workgroup totals: 16 passes of the totals scan."""
    n = 1 << 21
    air = RangeLookupAir()
    trace = np.empty((n, 3), dtype=np.uint32)
    trace[:, 1] = np.arange(n)
    trace[:, 0] = np.random.default_rng(5).permutation(n)
    trace[:, 2] = P - 1  # every table entry is looked up once
    ch = _challenges(21)
    m = ts.DeviceMatrix.upload(ctx, trace)
    aux, S = air.logup.build(m, ch)
    assert not S.any()
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0, 0, *aux_dims(air)))
    assert ts.check_constraints(cair, m, [], ctx, aux=aux, challenges=ch, exposed=S) == -1


def test_logup_zero_denominator(ctx):
    """gamma = -v planted for the value of row 37: TS_ERR_INVARIANT naming that row and interaction, no output."""
    n = 128
    trace = _logup_trace(n)
    trace[:, 0] = 1000 + 3 * np.arange(n)  # distinct values: row 37 is the first and only zero
    ch = _challenges(4)
    ch[:4] = (P - int(trace[37, 0]), 0, 0, 0)
    m = ts.DeviceMatrix.upload(ctx, trace)
    with pytest.raises(_lib.TsError) as e:
        LogUp(SPECS[2]).build(m, ch)
    assert e.value.code == TS_ERR_INVARIANT and "row 37, interaction 0" in str(e.value), str(e.value)
    assert m.dims() == (n, 4)


# ------------------------------------------------------------------ 2. quotient over (aux, main)
class Case:
    """A random AIR split into A aux and W main columns (and its last public values into a challenge and an
    exposed word), with its inputs and the oracle's quotient of the joined AIR (computed once, never modified)."""

    def __init__(self, orc, seed):
        self.seed = seed
        air, self.log_n = random_air_case(seed)
        self.air, self.valid = air, air.valid
        n, w = 1 << self.log_n, air.width()
        self.A = aux_width_of(seed, w)
        self.v1 = ts.air_tape(air, air.n_public)
        self.v3 = split_tape_aux(self.v1, self.A)
        self.joined_tape = join_tape_aux(self.v3)
        if air.valid:
            joined, pis, _ = generate_random_air_trace(air, n)
        else:
            joined = splitmix64_stream(seed + 1, n * w).reshape(n, w).astype(np.uint32)
            pis = (splitmix64_stream(seed + 2, max(air.n_public, 1)) % np.uint64(P))[:air.n_public].astype(np.uint32)
        self.joined = np.ascontiguousarray(joined, dtype=np.uint32)
        self.aux = np.ascontiguousarray(self.joined[:, :self.A])
        self.main = np.ascontiguousarray(self.joined[:, self.A:])
        self.pis, self.ch, self.ex = split_publics(pis)
        self.joined_pis = np.concatenate([self.pis, self.ch, self.ex]).astype(np.uint32)
        self.lqd = orc.log_quotient_degree(self.joined_tape)
        self.b = max(self.lqd, 1)
        self.alpha = splitmix64_stream(seed + 3, 4).astype(np.uint32)
        lde = orc.commit_lde(self.joined, 1, self.b)
        self.want = orc.split_quotient(
            orc.quotient_values(self.joined_tape, lde, self.log_n, self.b, self.joined_pis, self.alpha), self.log_n,
            self.lqd)
        self.want.setflags(write=False)


@pytest.fixture(scope="module")
def cases(orc):
    return {s: Case(orc, s) for s in SEEDS}


def _compile(ctx, tape, monkeypatch, jit: bool, **kw):
    with monkeypatch.context() as m:
        if not jit:
            m.setenv("TS_NO_JIT", "1")
        m.setenv("TS_JIT_MAX_INSTR", str(WAIT_JIT_INSTR))
        return ts.CompiledAir(ctx, tape, **kw)


def _commit(pcs, log_n, m):
    return pcs.commit([((log_n, 1), m.copy())])


def _chunks_aux(ctx, case, cair):
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(case.b, 3, 2), ctx)
    _, aux_data = _commit(pcs, case.log_n, case.aux)
    _, data = _commit(pcs, case.log_n, case.main)
    return [ch.download() for ch in pcs.quotient_chunks(data, cair, case.pis, case.alpha, aux=aux_data,
                                                        challenges=case.ch, exposed=case.ex)]


def _same(got, want, what):
    assert len(got) == want.shape[0], what
    for c, g in enumerate(got):
        assert (g == want[c]).all(), f"{what}: chunk {c}: {int((g != want[c]).sum())} words differ"


def test_case_set_has_the_edges(cases):
    assert len(cases) >= 33
    assert sum(len(c.ch) > 0 for c in cases.values()) >= 12 and sum(len(c.ex) > 0 for c in cases.values()) >= 2
    assert any(c.A == 1 and c.main.shape[1] == 1 for c in cases.values())
    assert any(c.A > c.main.shape[1] for c in cases.values())
    assert any(c.lqd == 0 for c in cases.values()) and any(c.lqd == 3 for c in cases.values())


@pytest.mark.parametrize("chunk", range(12))
@pytest.mark.parametrize("jit", [False, True], ids=["interp", "jit"])
def test_quotient_over_aux_and_main(ctx, cases, monkeypatch, jit, chunk):
    """== the oracle's quotient of the joined AIR, and == ts_quotient_chunks of the joined tape on the unsplit
    trace, through the interpreter and through the specialised kernel."""
    n_jit, seeds = 0, SEEDS[chunk::12]
    for seed in seeds:
        case = cases[seed]
        cair = _compile(ctx, case.v3, monkeypatch, jit)
        assert cair.aux_width == case.A and cair.log_quotient_degree == case.lqd
        if jit and not cair.is_jit:
            state, _ = cair.jit_wait()
            assert state == (3 if len(cair.program()["code"]) <= WAIT_JIT_INSTR else 0), seed
        assert cair.is_jit == (jit and len(cair.program()["code"]) <= WAIT_JIT_INSTR), seed
        n_jit += int(cair.is_jit)
        got = _chunks_aux(ctx, case, cair)
        _same(got, case.want, f"seed {seed} vs oracle")
        v1 = _compile(ctx, case.joined_tape, monkeypatch, False)
        pcs = ts.TwoAdicFriPcs(ts.FriConfig(case.b, 3, 2), ctx)
        _, data = _commit(pcs, case.log_n, case.joined)
        ref = [ch.download() for ch in pcs.quotient_chunks(data, v1, case.joined_pis, case.alpha)]
        for c, (g, r) in enumerate(zip(got, ref)):
            assert (g == r).all(), f"seed {seed} vs ts_quotient_chunks: chunk {c}"
    assert n_jit >= (len(seeds) - 1 if jit else 0)


@pytest.mark.parametrize("seed", SEGMENT_SEEDS)
def test_quotient_segmented(ctx, cases, monkeypatch, seed):
    case = cases[seed]
    cair = _compile(ctx, case.v3, monkeypatch, True, segment_instr=16)
    assert len(cair.segment_plan()["segments"]) > 1
    state, _ = cair.jit_wait()
    assert state == 3 and cair.is_jit, f"segmented specialisation failed (state {state})"
    _same(_chunks_aux(ctx, case, cair), case.want, f"seed {seed} segmented")


# ------------------------------------------------------------------ 3. check_constraints
def test_check_constraints_over_aux_and_main(ctx, orc, cases, monkeypatch, global_slab=False):
    n_bad = 0
    for seed in SEEDS:
        case = cases[seed]
        cair = _compile(ctx, case.v3, monkeypatch, False)
        if global_slab:  # read at every launch: the register file goes to the global slab from here on
            monkeypatch.setenv("TS_INTERP_LDS_MAX_REGS", "1")
            assert cair.program()["n_regs"] > 1
        n = 1 << case.log_n
        check = lambda aux, main: ts.check_constraints(cair, main, case.pis, ctx, aux=aux, challenges=case.ch,
                                                       exposed=case.ex)
        want = orc.check_constraints(case.joined_tape, case.joined, case.joined_pis)
        assert check(case.aux, case.main) == want, seed
        assert want == -1 or not case.valid, seed
        n_bad += want >= 0
        bad_main = case.main.copy()
        bad_main[(seed * 7) % n, seed % bad_main.shape[1]] ^= 1
        assert check(case.aux, bad_main) == \
            orc.check_constraints(case.joined_tape, np.hstack([case.aux, bad_main]), case.joined_pis), seed
        bad_aux = case.aux.copy()
        bad_aux[(seed * 5) % n, seed % case.A] ^= 1
        assert check(bad_aux, case.main) == \
            orc.check_constraints(case.joined_tape, np.hstack([bad_aux, case.main]), case.joined_pis), seed
    assert n_bad >= 10 and len(VALID_SEEDS) >= 10


def test_check_constraints_over_aux_and_main_global_slab(ctx, orc, cases, monkeypatch):
    """The same through k_check_constraints_pre<64, true> (the aux trace is the one side matrix): one 64-lane tile
    mostly inactive (n = 2) and exactly full (n = 2^6) among the seeded cases, then n = 2^10, sixteen tiles, which
    they do not reach: a valid trace, and a cell changed in the last tile but one."""
    assert {1, 6} <= {cases[s].log_n for s in SEEDS}
    test_check_constraints_over_aux_and_main(ctx, orc, cases, monkeypatch, global_slab=True)
    case = cases[TALL_SEED]
    n, r = 1 << 10, (1 << 10) - 70
    joined, all_pis, _ = generate_random_air_trace(case.air, n)
    joined = np.ascontiguousarray(joined, dtype=np.uint32)
    pis, ch, ex = split_publics(all_pis)
    joined_pis = np.concatenate([pis, ch, ex]).astype(np.uint32)
    cair = _compile(ctx, case.v3, monkeypatch, False)
    check = lambda m: ts.check_constraints(cair, np.ascontiguousarray(m[:, case.A:]), pis, ctx,
                                           aux=np.ascontiguousarray(m[:, :case.A]), challenges=ch, exposed=ex)
    assert check(joined) == -1 == orc.check_constraints(case.joined_tape, joined, joined_pis)
    late = []
    for col in (0, joined.shape[1] - 1):  # an aux cell, a main cell
        bad = joined.copy()
        bad[r, col] ^= 1
        late.append(orc.check_constraints(case.joined_tape, bad, joined_pis))
        assert check(bad) == late[-1], col
    assert max(late) >> 16 >= r - 1


# ------------------------------------------------------------------ 4. whole proofs
def _mul_base(z, k):
    return np.array([int(x) * k % P for x in z], dtype=np.uint32)


def _staged_proof(pcs, cair, trace, pis, aux_source, chal):
    """The proof of ts_prove_aux built from public stage calls; `chal` ends in the prover's final state."""
    ctx = pcs.ctx
    n = trace.shape[0]
    log_n, lqd = n.bit_length() - 1, cair.log_quotient_degree
    root_t, data_t = pcs.commit([((log_n, 1), trace.copy())])
    chal.observe_commitment(root_t)
    ch = np.concatenate([chal.sample() for _ in range(cair.n_challenges)] + [np.zeros(0, dtype=np.uint32)])
    ch = ch.astype(np.uint32)
    aux, exposed = aux_source(ts.DeviceMatrix.upload(ctx, trace), ch)
    if isinstance(aux, ts.DeviceMatrix):
        aux = aux.download()
    exposed = np.asarray(exposed, dtype=np.uint32)
    root_a, data_a = pcs.commit([((log_n, 1), aux.copy())])
    chal.observe_commitment(root_a)
    for e in exposed:
        chal.observe(int(e))
    alpha = chal.sample()
    chunks = pcs.quotient_chunks(data_t, cair, pis, alpha, aux=data_a, challenges=ch, exposed=exposed)
    g = pow(G27, 1 << (27 - (log_n + lqd)), P) if log_n + lqd else 1
    root_q, data_q = pcs.commit([((log_n, 31 * pow(g, c, P) % P), c_m) for c, c_m in enumerate(chunks)])
    chal.observe_commitment(root_q)
    zeta = chal.sample()
    zeta_next = _mul_base(zeta, pow(G27, 1 << (27 - log_n), P))
    opened, fri = pcs.open([(data_a, [[zeta, zeta_next]]), (data_t, [[zeta, zeta_next]]),
                            (data_q, [[zeta]] * len(chunks))], chal)
    flat = np.concatenate([v for rnd in opened for m in rnd for v in m])
    return root_t, root_a, exposed, root_q, flat, fri, ch


def _check_whole_proof(ctx, cair, trace, pis, aux_source, cfg):
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))
    staged_chal, chal = ts.BfChallenger(), ts.BfChallenger()
    root_t, root_a, exposed, root_q, opened, fri, ch = _staged_proof(config.pcs, cair, trace, pis, aux_source,
                                                                     staged_chal)
    proof = ts.prove(config, cair, chal, trace.copy(), pis, aux=aux_source)
    aw, w, qd, ne = cair.aux_width, trace.shape[1], 1 << cair.log_quotient_degree, cair.n_exposed
    n_open = 4 * (2 * aw + 2 * w + 4 * qd)
    words = proof.words
    assert list(words[:8]) == [0x46505354, 4, trace.shape[0].bit_length() - 1, w, qd, aw, cair.n_challenges, ne]
    assert (words[8:16] == root_t).all() and (words[16:24] == root_a).all()
    assert (words[24:24 + ne] == exposed).all()
    o = 24 + ne
    assert (words[o:o + 8] == root_q).all()
    o += 8
    assert (words[o:o + n_open].reshape(-1, 4) == opened).all(), "opened values differ"
    assert len(words) - o - n_open == len(fri) and (words[o + n_open:] == fri).all(), "FriProof words differ"
    assert (chal.state() == staged_chal.state()).all(), "final challenger state differs"
    assert (proof.aux_commit == root_a).all() and (proof.exposed == exposed).all()
    assert (proof.aux_local == opened[:aw]).all() and (proof.aux_next == opened[aw:2 * aw]).all()
    assert (proof.trace_local == opened[2 * aw:2 * aw + w]).all()
    assert all(len(q.input_proof) == 3 for q in proof.query_proofs)
    return config, proof, exposed, ch


@pytest.mark.parametrize("log_n,b", [(1, 1), (1, 2), (6, 1), (6, 2), (12, 1), (12, 2)])
def test_range_lookup_whole_proof(ctx, log_n, b):
    air = RangeLookupAir()
    trace = generate_range_lookup_trace(1 << log_n)
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0, 0, *aux_dims(air)))
    config, proof, exposed, _ = _check_whole_proof(ctx, cair, trace, [], air.logup.aux_source, (b, 3, 2))
    got = ts.verify(config, cair, ts.BfChallenger(), proof, [])
    assert (got == exposed).all() and not got.any()
    air.logup.verify(got)
    assert not ts.verify(config, air, ts.BfChallenger(), proof, []).any()  # host-only AIR from the class


@pytest.mark.parametrize("seed", [3, 6, 12])
def test_split_random_air_whole_proof(ctx, cases, monkeypatch, seed):
    """A fixed-answer callback: the aux half of the joined trace and its exposed word, whatever the challenge.
    (The traces were made for fixed public values, so a proof whose AIR reads the sampled challenge need not
    verify; without a challenge it does.)"""
    case = cases[seed]
    assert case.valid
    cair = _compile(ctx, case.v3, monkeypatch, True)
    source = lambda trace, challenges: (case.aux.copy(), case.ex.copy())
    config, proof, exposed, _ = _check_whole_proof(ctx, cair, case.main, case.pis, source, (case.b, 3, 2))
    if cair.n_challenges == 0:
        got = ts.verify(config, ts.CompiledAir(None, case.v3), ts.BfChallenger(), proof, case.pis)
        assert (got == case.ex).all()


def test_split_set_for_whole_proofs(cases):
    assert len(cases[6].ch) and len(cases[6].ex) and len(cases[12].ex) and not len(cases[3].ch)


@pytest.fixture(scope="module")
def lookup_proof(ctx):
    air, n = RangeLookupAir(), 64
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), ctx))
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0, 0, *aux_dims(air)))
    trace = generate_range_lookup_trace(n)
    proof = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], aux=air.logup.aux_source)
    assert not ts.verify(config, cair, ts.BfChallenger(), proof, []).any()
    return config, cair, air, trace, proof.words.copy()


def _rejected(config, cair, words):
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(config, cair, ts.BfChallenger(), words, [])
    assert e.value.code != 0


def test_rejections(ctx, lookup_proof):
    config, cair, air, trace, words = lookup_proof
    # words: 8 header, 8 trace root, 8 aux root, 4 exposed, 8 quotient root, then aux_local (8 x 4) ...
    for k in (16 + 3, 24 + 1, 36 + 4 * 2 + 1, 36 + 4 * 8 + 4 * 7):  # aux root, exposed word, aux_local, aux_next
        bad = words.copy()
        bad[k] = (int(bad[k]) + 1) % P if k >= 24 else bad[k] ^ 1
        _rejected(config, cair, bad)
    # one cell of the challenge-dependent trace changed before it is committed: proved all the same, rejected
    def flipped(tr, challenges):
        aux, S = air.logup.build(tr, challenges)
        a = aux.download()
        a[17, 2] = (int(a[17, 2]) + 1) % P
        return a, S
    proof = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], aux=flipped)
    assert proof.words[1] == 4
    _rejected(config, cair, proof.words)
    # a lookup of a value outside the table: the proof verifies, the statement about the sum does not hold
    outside = generate_range_lookup_trace(64, outside_row=9)
    proof = ts.prove(config, cair, ts.BfChallenger(), outside, [], aux=air.logup.aux_source)
    S = ts.verify(config, cair, ts.BfChallenger(), proof, [])
    assert S.any()
    with pytest.raises(ValueError):
        air.logup.verify(S)


def test_prove_aux_without_aux_columns_is_prove(ctx):
    """aux_width 0: ts_prove_aux with a null aux_fn is ts_prove but for the header, and ts_verify_aux accepts it."""
    from tapstark_amd.airs import SynthMulAir, generate_synth_mul_trace
    trace = generate_synth_mul_trace(32, 6)
    cair = ts.CompiledAir(ctx, ts.air_tape(SynthMulAir(6), 0))
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(1, 3, 2), ctx))
    v1 = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), []).words
    l, cfg = _lib.lib(), config.pcs.fri._c()
    out, n_words = np.zeros(len(v1) + 64, dtype=np.uint32), C.c_size_t()
    chal, m = ts.BfChallenger(), ts.DeviceMatrix.upload(ctx, trace)
    ctx.check(l.ts_prove_aux(ctx.h, C.byref(cfg), cair.h, chal.h, m.h, None, 0, _lib.AUX_FN(), None,
                             out.ctypes.data_as(_lib.u32p), len(out), C.byref(n_words)))
    v4 = out[:n_words.value]
    assert list(v4[:8]) == [v1[0], 4, v1[2], v1[3], v1[4], 0, 0, 0] and (v4[8:] == v1[5:]).all()
    got = ts.verify(config, cair, ts.BfChallenger(), v4, [])
    assert got is not None and len(got) == 0
    # an aux_fn for such an AIR is refused before the trace is taken
    m = ts.DeviceMatrix.upload(ctx, trace)
    with pytest.raises(_lib.TsError) as e:
        ts.prove(config, cair, ts.BfChallenger(), m, [], aux=lambda t, c: (np.zeros((32, 4), dtype=np.uint32), []))
    assert e.value.code == TS_ERR_INVALID and m.dims() == (32, 6)


# ------------------------------------------------------------------ 5. refusals and the callback
def _raises(code, f, needle=None):
    with pytest.raises(_lib.TsError) as e:
        f()
    assert e.value.code == code, (e.value.code, str(e.value))
    assert str(e.value), "no text in ts_last_error"
    if needle:
        assert needle in str(e.value), str(e.value)


def _prove_ok(config, cair, air, trace):
    proof = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], aux=air.logup.aux_source)
    assert not ts.verify(config, cair, ts.BfChallenger(), proof, []).any()


def test_calls_without_an_aux_source_refuse_the_air(ctx, lookup_proof):
    config, cair, air, trace, words = lookup_proof
    pcs = config.pcs
    _, data = _commit(pcs, 6, trace)
    alpha = splitmix64_stream(1, 4).astype(np.uint32)
    host_config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), None, host_only=True))
    locks = tt.make_lock_table(3, 3, 2, 6, lambda ci, q, s, u: tt.winternitz_lock_script(bytes([ci, q, s % 251]), u))
    group = LocalCommGroup(1)
    up = lambda: ts.DeviceMatrix.upload(ctx, trace)
    l, cfg = _lib.lib(), pcs.fri._c()
    out, n_words = np.zeros(16, dtype=np.uint32), C.c_size_t()

    def prove_pre():
        m, chal = up(), ts.BfChallenger()
        ctx.check(l.ts_prove_pre(ctx.h, C.byref(cfg), cair.h, chal.h, None, m.h, None, 0,
                                 out.ctypes.data_as(_lib.u32p), len(out), C.byref(n_words)))

    calls = {
        "ts_prove": lambda: ts.prove(config, cair, ts.BfChallenger(), up(), []),
        "ts_prove_pre": prove_pre,
        "ts_quotient_chunks": lambda: pcs.quotient_chunks(data, cair, [], alpha),
        "ts_quotient_chunks_pre": lambda: pcs.quotient_chunks(data, cair, [], alpha, preprocessed=data),
        "ts_check_constraints": lambda: ts.check_constraints(cair, trace, [], ctx),
        "ts_check_constraints_pre": lambda: ts.check_constraints(cair, trace, [], ctx, preprocessed=trace),
        "ts_prove_stream": lambda: ts.prove_stream([(config, cair)], [up()], [0], []),
        "ts_prove_batch": lambda: ts.prove_batch([(config, cair)], [up()], [0], []),
        "ts_prove_sharded": lambda: ts.prove_sharded(config, cair, ts.BfChallenger(), up(), [], group.comm(0)),
        "ts_prove_tap": lambda: tt.prove_tap(config, cair, ts.BfChallenger(), up(), [], locks),
        "ts_prove_tap_sharded": lambda: tt.prove_tap(config, cair, ts.BfChallenger(), up(), [], locks,
                                                     comm=group.comm(0)),
    }
    for name, f in calls.items():
        _raises(TS_ERR_UNSUPPORTED, f, "ts_prove_aux")
    _prove_ok(config, cair, air, trace)
    res = ts.prove_batch([(config, cair)], [up(), up()], [0, 0], [], check=False)
    assert list(res.status) == [TS_ERR_UNSUPPORTED] * 2 and all("ts_prove_aux" in e for e in res.errors)
    # the host-only ones
    v, vchal = C.c_int(-1), ts.BfChallenger()
    rc = l.ts_verify(C.byref(cfg), cair.h, vchal.h, words.ctypes.data_as(_lib.u32p), len(words), None, 0,
                     C.byref(v))
    assert rc == TS_ERR_UNSUPPORTED and "ts_prove_aux" in (l.ts_last_error(None) or b"").decode()
    with pytest.raises(_lib.TsError) as e:
        ts.verify(host_config, cair, ts.BfChallenger(), words, [], preprocessed_root=np.zeros(8, dtype=np.uint32))
    assert e.value.code == TS_ERR_UNSUPPORTED
    with pytest.raises(_lib.TsError) as e:
        tt.verify_tap(host_config, cair, ts.BfChallenger(), words, [], locks)
    assert e.value.code == TS_ERR_UNSUPPORTED
    with pytest.raises(_lib.TsError) as e:
        ts.Proof(words).to_postcard()
    assert e.value.code == TS_ERR_UNSUPPORTED
    _prove_ok(config, cair, air, trace)


def test_preprocessed_with_aux_is_refused_by_the_proving_calls(ctx):
    b = SymbolicAirBuilder(1, 0, preprocessed_width=1, aux_width=4)
    b.assert_zero(b.preprocessed().row_slice(0)[0] * b.aux().row_slice(0)[0] - b.main().row_slice(0)[0])
    cair = ts.CompiledAir(ctx, b.tape())
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(1, 3, 2), ctx))
    pcs = config.pcs
    main, aux = np.ones((8, 1), dtype=np.uint32), np.ones((8, 4), dtype=np.uint32)
    _, data = _commit(pcs, 3, main)
    _, aux_data = _commit(pcs, 3, aux)
    alpha = splitmix64_stream(1, 4).astype(np.uint32)
    m = ts.DeviceMatrix.upload(ctx, main)
    _raises(TS_ERR_UNSUPPORTED, lambda: ts.prove(config, cair, ts.BfChallenger(), m, [], aux=lambda t, c: (aux, [])))
    assert m.dims() == (8, 1)  # refused before the trace is taken
    _raises(TS_ERR_UNSUPPORTED, lambda: pcs.quotient_chunks(data, cair, [], alpha, aux=aux_data))
    _raises(TS_ERR_UNSUPPORTED, lambda: ts.check_constraints(cair, main, [], ctx, aux=aux))
    _raises(TS_ERR_UNSUPPORTED, lambda: ts.prove(config, cair, ts.BfChallenger(), m, []))
    _raises(TS_ERR_UNSUPPORTED, lambda: ts.prove(config, cair, ts.BfChallenger(), m, [], preprocessed=aux_data_key(aux_data)))


class aux_data_key:  # what prove() takes as a key: .data
    def __init__(self, data):
        self.data = data


def test_callback_statuses(ctx, lookup_proof):
    config, cair, air, trace, _ = lookup_proof
    l, cfg = _lib.lib(), config.pcs.fri._c()
    out, n_words = np.zeros(1 << 16, dtype=np.uint32), C.c_size_t()

    def raw(fn):
        m, chal = ts.DeviceMatrix.upload(ctx, trace), ts.BfChallenger()  # (the challenger outlives the call)
        rc = l.ts_prove_aux(ctx.h, C.byref(cfg), cair.h, chal.h, m.h, None, 0, fn, None,
                            out.ctypes.data_as(_lib.u32p), len(out), C.byref(n_words))
        return rc, (l.ts_last_error(ctx.h) or b"").decode(), m

    # a status of the callback's own is propagated, and the text names the callback
    rc, msg, _ = raw(_lib.AUX_FN(lambda user, c, t, ch, n, aux_out, exposed_out: 7))
    assert rc == 7 and "aux callback" in msg and "7" in msg
    # a null aux_fn for an AIR with aux columns: refused before the trace is taken
    rc, msg, m = raw(_lib.AUX_FN())
    assert rc == TS_ERR_INVALID and "aux_fn" in msg and m.dims() == trace.shape
    # a wrong-shape aux: TS_ERR_INVALID, the trace consumed as ts_prove consumes it on that status
    for what, bad in (("width", np.zeros((64, 4), dtype=np.uint32)), ("height", np.zeros((32, 8), dtype=np.uint32))):
        m = ts.DeviceMatrix.upload(ctx, trace)
        _raises(TS_ERR_INVALID, lambda: ts.prove(config, cair, ts.BfChallenger(), m, [],
                                                 aux=lambda t, c: (bad, np.zeros(4, dtype=np.uint32))), "aux matrix")
        _raises(TS_ERR_INVALID, lambda: ts.prove(config, cair, ts.BfChallenger(), m, [], aux=air.logup.aux_source),
                "consumed")
    # made on another context
    other = ts.Context(ctx.device)
    foreign = lambda t, c: (ts.DeviceMatrix.upload(other, np.zeros((64, 8), dtype=np.uint32)), np.zeros(4, dtype=np.uint32))
    _raises(TS_ERR_INVALID, lambda: ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], aux=foreign), "context")
    # the wrong number of exposed words, and an exception of the callback's own: re-raised
    with pytest.raises(ValueError):
        ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], aux=lambda t, c: (np.zeros((64, 8), dtype=np.uint32), [1]))

    class Boom(Exception):
        pass

    def boom(t, c):
        assert t.dims() == trace.shape and len(c) == 8
        raise Boom("from the aux source")

    with pytest.raises(Boom):
        ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], aux=boom)
    # a zero denominator inside ts_logup_aux_build comes back as the library's own error
    _prove_ok(config, cair, air, trace)


# ------------------------------------------------------------------ 6. the C++ example
def test_cpp_lookup_example(ctx, tmp_path):
    """examples/lookup_air.cpp: RangeLookupAir captured with tapstark_air.hpp (the words of the Python tape),
    proved with ts_prove_aux through a C callback that calls ts_logup_aux_build, verified, sum checked zero."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_abi_cpu import _build_example
    exe = _build_example(tmp_path, "lookup_air")
    tape = subprocess.run([exe, "--tape"], capture_output=True, text=True, timeout=60)
    assert tape.returncode == 0, tape.stderr
    got = np.array([int(x) for x in tape.stdout.split()], dtype=np.uint32)
    air = RangeLookupAir()
    want = ts.air_tape(air, 0, 0, *aux_dims(air))
    assert len(got) == len(want) and (got == want).all()
    r = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify -> 0" in r.stdout and "sum is zero" in r.stdout
