"""AIRs with preprocessed AND challenge-phase (aux) columns on the GPU: the quotient kernels and check_constraints
over (key, aux, main), the LogUp builder with table terms, whole TSPF v5 proofs, the rejections, the degenerate
forms, the callback, and the paths that must not move.  The oracle has one matrix, so exactness comes from the
equalities test_gpu_preprocessed.py and test_gpu_aux.py rest on:

* the quotient over (P key, A aux, W main) is, row by row, the quotient of the joined AIR over hstack(pre, aux,
  main) with the public vector pis ++ challenges ++ exposed, which the oracle and ts_quotient_chunks compute;
* a whole v5 proof is the composition of oracle-tested ABI stages -- ts_pcs_commit of key, trace, aux and chunks,
  the host challenger, ts_pcs_open with four rounds -- around that quotient;
* the aux matrix of a LogUp spec with table terms is the matrix ts_logup_aux_build gives for the spec remapped
  onto hstack(trace, table), and the one a Python-integer EF4 computes.

The CPU half is tests/test_air_pre_aux_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.air import LogUp, SymbolicAirBuilder, aux_dims
from tapstark_amd.airs import (RangeLookupAir, SelectorAir, SynthMulAir, TableLookupAir, generate_lookup_table,
                               generate_random_air_trace, generate_range_lookup_trace, generate_selector_preprocessed,
                               generate_selector_trace, generate_synth_mul_trace, generate_table_lookup_trace,
                               random_air_case, splitmix64_stream)
from _aux_airs import logup_reference, split_publics
from _pre_aux_airs import join_tape_pre_aux, remap_logup, split_tape_pre_aux, split_widths

pytestmark = pytest.mark.gpu
P = 0x78000001
G27 = 0x1A427A41
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_UNSUPPORTED, TS_ERR_INVARIANT = 1, 4, 5
# test_gpu_aux.py's segment-seed subset, restricted to AIRs wide enough for a three-way split
SEGMENT_SEEDS = [s for s in (0, 6, 9, 12, 21, 27) if random_air_case(s)[0].width() >= 3]
WAIT_JIT_INSTR = 3000
HEIGHTS = (1, 2, 3, 6, 10)  # log2: n = 2, 4, 8, 2^6, 2^10


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def _rand(seed, shape):
    return (splitmix64_stream(seed, int(np.prod(shape))) % np.uint64(P)).reshape(shape).astype(np.uint32)


# ------------------------------------------------------------------ the hand-made AIR
class WrapAir:
    """w = 2 main, pw = 1 + k preprocessed, aw = 2 aux columns, one public value, one challenge, one exposed word.

    c0 (every row, the wrap-around row included): next.main[0] = sum_{j >= 1} next.prep[j] + next.aux[1] -- the NEXT
       row of all three matrices;
    c1 (transition): next.main[1] = main[1]^(d - 2) prep[0] aux[0] + challenge word 0 + public value 0, degree d;
    c2 (first row): main[1] = exposed word 0.
    d = 2, 3, 5 gives log_quotient_degree 0, 1, 2."""

    def __init__(self, d: int, k: int = 1):
        self.d, self.k = d, k
        self.w, self.pw, self.aw = 2, 1 + k, 2

    def tape(self):
        b = SymbolicAirBuilder(self.w, 1, preprocessed_width=self.pw, aux_width=self.aw, n_challenges=1, n_exposed=1)
        main, nxt = b.main().row_slice(0), b.main().row_slice(1)
        prep, prep_n = b.preprocessed().row_slice(0), b.preprocessed().row_slice(1)
        aux, aux_n = b.aux().row_slice(0), b.aux().row_slice(1)
        s = aux_n[1]
        for j in range(1, self.pw):
            s = s + prep_n[j]
        b.assert_zero(nxt[0] - s)
        prod = prep[0] * aux[0]
        for _ in range(self.d - 2):
            prod = prod * main[1]
        b.when_transition().assert_zero(nxt[1] - prod - b.challenges()[0].c[0] - b.public_values()[0])
        b.when_first_row().assert_zero(main[1] - b.exposed()[0])
        return b.tape()

    def matrices(self, n: int, seed: int, ch):
        """(prep, aux, main, pis, exposed) satisfying the AIR for the challenge words `ch`."""
        prep, aux = _rand(seed, (n, self.pw)), _rand(seed + 1, (n, self.aw))
        pis, ex = _rand(seed + 2, (1,)), _rand(seed + 3, (1,))
        main = np.zeros((n, 2), dtype=np.uint64)
        main[:, 0] = (prep[:, 1:].astype(np.uint64).sum(axis=1) + aux[:, 1]) % P
        cur = int(ex[0])
        for i in range(n):
            main[i, 1] = cur
            cur = (pow(cur, self.d - 2, P) * int(prep[i, 0]) * int(aux[i, 0]) + int(ch[0]) + int(pis[0])) % P
        return prep, aux, main.astype(np.uint32), pis, ex


class Case:
    """One AIR with both kinds of column at one height and blowup: its matrices, the joined trace and public
    vector, and the oracle's quotient of the joined AIR (computed once, never modified)."""

    def __init__(self, orc, tape, prep, aux, main, pis, ch, ex, log_n, b, seed):
        self.tape, self.prep, self.aux, self.main = tape, prep, aux, main
        self.pis, self.ch, self.ex, self.log_n, self.b = pis, ch, ex, log_n, b
        self.joined_tape = join_tape_pre_aux(tape)
        self.joined = np.ascontiguousarray(np.hstack([prep, aux, main]), dtype=np.uint32)
        self.joined_pis = np.concatenate([pis, ch, ex]).astype(np.uint32)
        self.lqd = orc.log_quotient_degree(self.joined_tape)
        assert self.lqd <= b
        self.alpha = splitmix64_stream(seed + 3, 4).astype(np.uint32)
        lde = orc.commit_lde(self.joined, 1, b)
        self.want = orc.split_quotient(
            orc.quotient_values(self.joined_tape, lde, log_n, b, self.joined_pis, self.alpha), log_n, self.lqd)
        self.want.setflags(write=False)


def _wrap_case(orc, d, log_n, b, k=1):
    air = WrapAir(d, k)
    ch = _rand(900 + d + log_n, (4,))
    prep, aux, main, pis, ex = air.matrices(1 << log_n, 40 * d + log_n, ch)
    return Case(orc, air.tape(), prep, aux, main, pis, ch, ex, log_n, b, 7 * d + log_n + b)


def _split_case(orc, seed, which):
    air, log_n = random_air_case(seed)
    n, w = 1 << log_n, air.width()
    p, a = split_widths(seed, w, which)
    v1 = ts.air_tape(air, air.n_public)
    if air.valid:
        joined, pis, _ = generate_random_air_trace(air, n)
    else:
        joined = splitmix64_stream(seed + 1, n * w).reshape(n, w).astype(np.uint32)
        pis = (splitmix64_stream(seed + 2, max(air.n_public, 1)) % np.uint64(P))[:air.n_public].astype(np.uint32)
    joined = np.ascontiguousarray(joined, dtype=np.uint32)
    pis, ch, ex = split_publics(pis)
    tape = split_tape_pre_aux(v1, p, a)
    lqd = orc.log_quotient_degree(join_tape_pre_aux(tape))
    c = Case(orc, tape, np.ascontiguousarray(joined[:, :p]), np.ascontiguousarray(joined[:, p:p + a]),
             np.ascontiguousarray(joined[:, p + a:]), pis, ch, ex, log_n, max(lqd, 1), seed)
    c.valid = air.valid
    return c


@pytest.fixture(scope="module")
def wrap_cases(orc):
    """d -> [(log_n, b)]: every height at both blowups the degree allows."""
    return {d: [_wrap_case(orc, d, log_n, b) for log_n in HEIGHTS for b in (1, 2) if b >= lqd]
            for d, lqd in ((2, 0), (3, 1), (5, 2))}


@pytest.fixture(scope="module")
def split_cases(orc):
    return {(s, which): _split_case(orc, s, which) for s in SEGMENT_SEEDS for which in (0, 1, 2)}


def _compile(ctx, tape, monkeypatch, jit: bool, **kw):
    with monkeypatch.context() as m:
        if not jit:
            m.setenv("TS_NO_JIT", "1")
        m.setenv("TS_JIT_MAX_INSTR", str(WAIT_JIT_INSTR))
        return ts.CompiledAir(ctx, tape, **kw)


def _commit(pcs, log_n, m):
    return pcs.commit([((log_n, 1), m.copy())])


def _chunks(ctx, case, cair):
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(case.b, 3, 2), ctx)
    _, key = _commit(pcs, case.log_n, case.prep)
    _, aux_data = _commit(pcs, case.log_n, case.aux)
    _, data = _commit(pcs, case.log_n, case.main)
    return [ch.download() for ch in pcs.quotient_chunks(data, cair, case.pis, case.alpha, preprocessed=key,
                                                        aux=aux_data, challenges=case.ch, exposed=case.ex)]


def _same(got, want, what):
    assert len(got) == want.shape[0], what
    for c, g in enumerate(got):
        assert (g == want[c]).all(), f"{what}: chunk {c}: {int((g != want[c]).sum())} words differ"


def _joined_chunks(ctx, case, monkeypatch):
    """ts_quotient_chunks of the joined version-1 tape on the unsplit trace."""
    v1 = _compile(ctx, case.joined_tape, monkeypatch, False)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(case.b, 3, 2), ctx)
    _, data = _commit(pcs, case.log_n, case.joined)
    return [ch.download() for ch in pcs.quotient_chunks(data, v1, case.joined_pis, case.alpha)]


PATHS = ["jit", "interp_lds", "interp_global", "segmented"]


def _compile_path(ctx, tape, monkeypatch, path):
    """The AIR compiled so that `path` runs, selected as test_gpu_aux.py selects: TS_NO_JIT for the interpreter
    (TS_INTERP_LDS_MAX_REGS, read at every launch, sends its register file to the global slab), segment_instr small
    enough to cut for the segmented kernels."""
    if path == "segmented":
        cair = _compile(ctx, tape, monkeypatch, True, segment_instr=8)
        assert len(cair.segment_plan()["segments"]) > 1
        state, _ = cair.jit_wait()
        assert state == 3 and cair.is_jit, f"segmented specialisation failed (state {state})"
        return cair
    cair = _compile(ctx, tape, monkeypatch, path == "jit")
    if path == "jit" and not cair.is_jit:
        assert cair.jit_wait()[0] == 3
    assert cair.is_jit == (path == "jit")
    if path == "interp_global":
        monkeypatch.setenv("TS_INTERP_LDS_MAX_REGS", "1")
        assert cair.program()["n_regs"] > 1
    return cair


# ------------------------------------------------------------------ 1. quotient over (key, aux, main)
def test_case_set_has_the_edges(wrap_cases, split_cases):
    assert sorted({c.lqd for cs in wrap_cases.values() for c in cs}) == [0, 1, 2]
    assert {(c.log_n, c.b) for c in wrap_cases[3]} == {(l, b) for l in HEIGHTS for b in (1, 2)}
    # 2^10 rows: more than one 256-thread tile per chunk
    assert all(any(c.log_n == 10 for c in cs) for cs in wrap_cases.values())
    narrow = [c for (s, which), c in split_cases.items() if which == 0]
    assert all(c.prep.shape[1] == 1 and c.aux.shape[1] == 1 for c in narrow)
    assert all(c.main.shape[1] == 1 for (s, which), c in split_cases.items() if which == 1)
    assert any(c.prep.shape[1] > max(c.aux.shape[1], c.main.shape[1]) for c in split_cases.values())
    # the next row of all three matrices is read
    code = ts.CompiledAir(None, WrapAir(3).tape()).program()["code"]
    assert {1, 3, 5} <= set(code[code[:, 0] == 0][:, 2].tolist())


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("d", [2, 3, 5])
def test_quotient_wrap_air(ctx, wrap_cases, monkeypatch, d, path):
    """== the oracle's quotient of the joined AIR and == ts_quotient_chunks of the joined tape, at n = 2, 4, 8, 2^6
    and 2^10 and both blowups, through each of the four kernel paths."""
    cair = _compile_path(ctx, WrapAir(d).tape(), monkeypatch, path)
    assert (cair.preprocessed_width, cair.aux_width, cair.width) == (2, 2, 2)
    for case in wrap_cases[d]:
        assert cair.log_quotient_degree == case.lqd
        got = _chunks(ctx, case, cair)
        _same(got, case.want, f"d {d} n 2^{case.log_n} b {case.b} {path} vs oracle")
        if case.log_n in (1, 10):
            for c, (g, r) in enumerate(zip(got, _joined_chunks(ctx, case, monkeypatch))):
                assert (g == r).all(), f"d {d} n 2^{case.log_n} b {case.b} vs ts_quotient_chunks: chunk {c}"


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("seed", SEGMENT_SEEDS)
def test_quotient_random_splits(ctx, split_cases, monkeypatch, seed, path):
    """The seeded random AIRs split three ways: (1, 1, rest), main left with one column, and a wide key."""
    for which in (0, 1, 2):
        case = split_cases[(seed, which)]
        if path == "segmented" and len(ts.CompiledAir(None, case.tape).program()["code"]) <= 8:
            continue
        cair = _compile_path(ctx, case.tape, monkeypatch, path)
        got = _chunks(ctx, case, cair)
        _same(got, case.want, f"seed {seed} split {which} {path} vs oracle")
        for c, (g, r) in enumerate(zip(got, _joined_chunks(ctx, case, monkeypatch))):
            assert (g == r).all(), f"seed {seed} split {which} vs ts_quotient_chunks: chunk {c}"
        monkeypatch.delenv("TS_INTERP_LDS_MAX_REGS", raising=False)


def test_quotient_argument_refusals(ctx, wrap_cases, monkeypatch):
    case = wrap_cases[3][0]
    cair = _compile(ctx, case.tape, monkeypatch, False)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(case.b, 3, 2), ctx)
    _, key = _commit(pcs, case.log_n, case.prep)
    _, aux_data = _commit(pcs, case.log_n, case.aux)
    _, data = _commit(pcs, case.log_n, case.main)
    q = lambda k, a: pcs.quotient_chunks(data, cair, case.pis, case.alpha, preprocessed=k, aux=a, challenges=case.ch,
                                         exposed=case.ex)
    _, wide = _commit(pcs, case.log_n, np.hstack([case.aux, case.aux]))
    _raises(TS_ERR_INVALID, lambda: q(key, wide), "aux")
    _raises(TS_ERR_INVALID, lambda: q(wide, aux_data), "key")
    _, tall = _commit(pcs, case.log_n + 1, np.vstack([case.aux, case.aux]))
    _raises(TS_ERR_INVALID, lambda: q(key, tall))
    other = ts.Context(ctx.device)
    opcs = ts.TwoAdicFriPcs(ts.FriConfig(case.b, 3, 2), other)
    _, foreign = _commit(opcs, case.log_n, case.aux)
    _raises(TS_ERR_INVALID, lambda: q(key, foreign), "context")
    _same([c.download() for c in q(key, aux_data)], case.want, "after the refusals")


# ------------------------------------------------------------------ 2. check_constraints
def _global_slab(monkeypatch, cair):
    """The interpreter's register file goes to the global slab from here on, as _compile_path("interp_global") sends
    it: k_check_pre_aux<64, true> runs instead of the LDS forms."""
    monkeypatch.setenv("TS_INTERP_LDS_MAX_REGS", "1")
    assert cair.program()["n_regs"] > 1


def test_check_constraints_wrap_air(ctx, orc, wrap_cases, monkeypatch, global_slab=False):
    """-1 on valid traces; one changed cell in each of the three matrices in turn is reported with the row and
    constraint the oracle's check of the joined AIR reports.  A cell of row 0 read only through `next` shows at the
    wrap-around row n - 1, constraint 0."""
    for d in (2, 3, 5):
        cair = _compile(ctx, WrapAir(d).tape(), monkeypatch, False)
        if global_slab:
            _global_slab(monkeypatch, cair)
        for case in wrap_cases[d]:
            if case.b != max(case.lqd, 1):
                continue
            n = 1 << case.log_n
            check = lambda prep, aux, main: ts.check_constraints(cair, main, case.pis, ctx, preprocessed=prep, aux=aux,
                                                                 challenges=case.ch, exposed=case.ex)
            want = lambda prep, aux, main: orc.check_constraints(case.joined_tape, np.hstack([prep, aux, main]),
                                                                 case.joined_pis)
            assert check(case.prep, case.aux, case.main) == -1 == want(case.prep, case.aux, case.main), (d, n)
            # row 0, a column only c0 reads (through `next`): the violation is at the wrap-around row
            for which, col in ((0, 1), (1, 1), (2, 0)):
                mats = [case.prep.copy(), case.aux.copy(), case.main.copy()]
                mats[which][0, col] = (int(mats[which][0, col]) + 1) % P
                assert check(*mats) == (n - 1) * 65536 + 0 == want(*mats), (d, n, which)
            # a cell of the transition constraint, mid-trace (n = 2 has no row that is neither first nor last)
            r = n // 2
            for which, col in ((0, 0), (1, 0), (2, 1)) if n >= 4 else ():
                mats = [case.prep.copy(), case.aux.copy(), case.main.copy()]
                mats[which][r, col] = (int(mats[which][r, col]) + 1) % P
                got = check(*mats)
                assert got == want(*mats) and got >= 0, (d, n, which)


def test_check_constraints_wrap_air_global_slab(ctx, orc, wrap_cases, monkeypatch):
    """The same through k_check_pre_aux<64, true>.  n = 2: the wrap-around row beside 62 inactive lanes of the one
    64-lane tile; n = 2^6: exactly one full tile; n = 2^10: a grid-stride walk over several."""
    assert {1, 6, 10} <= {c.log_n for c in wrap_cases[3]}
    test_check_constraints_wrap_air(ctx, orc, wrap_cases, monkeypatch, global_slab=True)


def test_check_constraints_random_splits(ctx, orc, split_cases, monkeypatch, global_slab=False):
    n_valid = 0
    for (seed, which), case in split_cases.items():
        cair = _compile(ctx, case.tape, monkeypatch, False)
        if global_slab:
            _global_slab(monkeypatch, cair)
        n = 1 << case.log_n
        check = lambda prep, aux, main: ts.check_constraints(cair, main, case.pis, ctx, preprocessed=prep, aux=aux,
                                                             challenges=case.ch, exposed=case.ex)
        want = orc.check_constraints(case.joined_tape, case.joined, case.joined_pis)
        assert check(case.prep, case.aux, case.main) == want, (seed, which)
        assert want == -1 or not case.valid
        n_valid += want == -1
        for k, m in enumerate((case.prep, case.aux, case.main)):
            mats = [case.prep.copy(), case.aux.copy(), case.main.copy()]
            mats[k][(seed * 7 + k) % n, seed % m.shape[1]] ^= 1
            assert check(*mats) == orc.check_constraints(case.joined_tape, np.hstack(mats), case.joined_pis), \
                (seed, which, k)
    assert n_valid >= 6


def test_check_constraints_random_splits_global_slab(ctx, orc, split_cases, monkeypatch):
    test_check_constraints_random_splits(ctx, orc, split_cases, monkeypatch, global_slab=True)


# ------------------------------------------------------------------ 3. ts_logup_aux_build_pre
# main columns (a, b, c, m), table columns (t, u).  Each K has a table term as a value and one as a multiplicity.
SPECS = {
    1: [(("prep", 1), [("col", 0), ("const", 5), ("prep", 0)])],
    2: [(("prep", 1), [("col", 0)]), (("col", 3), [("prep", 0)])],
    3: [(("col", 3), [("col", 0), ("prep", 1), ("const", 7)]), (("prep", 0), [("col", 2)]),
        (("const", P - 1), [("prep", 0), ("col", 1)])],
}


def _logup_inputs(n, seed=3):
    t = _rand(seed + n, (n, 4))
    t[0, :] = (0, 1, P - 1, 0)  # edge values in the first row
    table = _rand(seed + n + 77, (n, 2))
    table[0, :] = (P - 1, 0)
    return t, table


def _challenges(seed, n=2):
    return (splitmix64_stream(seed, 4 * n) % np.uint64(P)).astype(np.uint32)


def _build_and_compare(ctx, n, K, seed):
    """(seeds for which logup_reference meets no zero denominator: it raises ZeroDivisionError if it does, and
    the combinations used below were run through it on the CPU when this file was written)"""
    lu = LogUp(SPECS[K])
    trace, table = _logup_inputs(n)
    ch = _challenges(seed + K)
    remapped = LogUp(remap_logup(lu.interactions, trace.shape[1]))
    joined = np.hstack([trace, table])
    want_aux, want_S = logup_reference(remapped.interactions, joined, ch[:4], ch[4:])
    table_m, trace_m = ts.DeviceMatrix.upload(ctx, table), ts.DeviceMatrix.upload(ctx, trace)
    aux, S = lu.build(trace_m, ch, preprocessed=table_m)
    got = aux.download()
    assert got.shape == want_aux.shape == (n, lu.aux_width)
    assert (got == want_aux).all(), f"n={n} K={K}: {int((got != want_aux).sum())} aux words differ, first row " \
                                    f"{int(np.flatnonzero((got != want_aux).any(axis=1))[0])}"
    assert (S == want_S).all(), f"n={n} K={K}: S differs"
    # word for word the matrix of the remapped spec on hstack(trace, table)
    aux_r, S_r = remapped.build(ts.DeviceMatrix.upload(ctx, joined), ch)
    assert (aux_r.download() == got).all() and (S_r == S).all(), f"n={n} K={K}: differs from the remapped build"
    assert table_m.dims() == table.shape and trace_m.dims() == trace.shape  # neither is consumed


@pytest.mark.parametrize("log_n", range(1, 12))
def test_logup_build_pre_vs_remapped_and_python_integers(ctx, log_n):
    """Default block size, n = 2^1 .. 2^11: inside one wave, across waves of one workgroup (2^9, 2^10), across
    workgroups (2^11), as test_gpu_aux.py's test of ts_logup_aux_build."""
    for K in (1, 2, 3):
        _build_and_compare(ctx, 1 << log_n, K, 100 + log_n)


@pytest.mark.parametrize("block_rows", [1, 3, 64, 300])
def test_logup_build_pre_small_blocks(ctx, monkeypatch, block_rows):
    monkeypatch.setenv("TS_LOGUP_BLOCK_ROWS", str(block_rows))
    for K in (1, 2, 3):
        _build_and_compare(ctx, 1 << 8, K, 200 + block_rows)


def test_logup_zero_denominator_through_a_table_value(ctx):
    n = 128
    trace, table = _logup_inputs(n)
    table[:, 0] = 1000 + 3 * np.arange(n)  # distinct: row 37 is the first and only zero
    ch = _challenges(4)
    ch[:4] = (P - int(table[37, 0]), 0, 0, 0)
    m, tm = ts.DeviceMatrix.upload(ctx, trace), ts.DeviceMatrix.upload(ctx, table)
    lu = LogUp([(("const", 1), [("col", 0)]), (("col", 3), [("prep", 0)])])
    with pytest.raises(_lib.TsError) as e:
        lu.build(m, ch, preprocessed=tm)
    assert e.value.code == TS_ERR_INVARIANT and "row 37, interaction 1" in str(e.value), str(e.value)
    assert m.dims() == (n, 4) and tm.dims() == (n, 2)


def test_logup_table_term_refusals(ctx):
    n = 8
    trace, table = _logup_inputs(n)
    m, tm = ts.DeviceMatrix.upload(ctx, trace), ts.DeviceMatrix.upload(ctx, table)
    ch = _challenges(1)
    lu = LogUp(SPECS[2])
    _raises(TS_ERR_INVALID, lambda: lu.build(m, ch))  # kind 2 through ts_logup_aux_build
    short = ts.DeviceMatrix.upload(ctx, table[:4].copy())
    _raises(TS_ERR_INVALID, lambda: lu.build(m, ch, preprocessed=short), "height")
    _raises(TS_ERR_INVALID, lambda: LogUp([(("const", 1), [("prep", 2)])]).build(m, ch, preprocessed=tm), "column")
    other = ts.Context(ctx.device)
    foreign = ts.DeviceMatrix.upload(other, table)
    _raises(TS_ERR_INVALID, lambda: lu.build(m, ch, preprocessed=foreign), "context")
    # a table term without a table, through the new call
    l, spec_keep = _lib.lib(), lu._spec_c()
    h, ex = C.c_void_p(), np.zeros(4, dtype=np.uint32)
    rc = l.ts_logup_aux_build_pre(ctx.h, C.byref(spec_keep[0]), None, m.h, ch.ctypes.data_as(_lib.u32p), C.byref(h),
                                  ex.ctypes.data_as(_lib.u32p))
    assert rc == TS_ERR_INVALID and not h.value
    assert m.dims() == (n, 4) and tm.dims() == (n, 2) and short.dims() == (4, 2)  # nothing is consumed
    lu.build(m, ch, preprocessed=tm)


# ------------------------------------------------------------------ 4. whole proofs
def _raises(code, f, needle=None):
    with pytest.raises(_lib.TsError) as e:
        f()
    assert e.value.code == code, (e.value.code, str(e.value))
    assert str(e.value), "no text in ts_last_error"
    if needle:
        assert needle in str(e.value), str(e.value)


def _mul_base(z, k):
    return np.array([int(x) * k % P for x in z], dtype=np.uint32)


def _staged_proof(pcs, cair, key, trace, pis, aux_source, chal):
    """The proof of ts_prove_pre_aux built from public stage calls; `chal` ends in the prover's final state."""
    ctx = pcs.ctx
    n = trace.shape[0]
    log_n, lqd = n.bit_length() - 1, cair.log_quotient_degree
    chal.observe_commitment(key.root)
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
    chunks = pcs.quotient_chunks(data_t, cair, pis, alpha, preprocessed=key, aux=data_a, challenges=ch, exposed=exposed)
    g = pow(G27, 1 << (27 - (log_n + lqd)), P) if log_n + lqd else 1
    root_q, data_q = pcs.commit([((log_n, 31 * pow(g, c, P) % P), c_m) for c, c_m in enumerate(chunks)])
    chal.observe_commitment(root_q)
    zeta = chal.sample()
    zeta_next = _mul_base(zeta, pow(G27, 1 << (27 - log_n), P))
    opened, fri = pcs.open([(key.data, [[zeta, zeta_next]]), (data_a, [[zeta, zeta_next]]),
                            (data_t, [[zeta, zeta_next]]), (data_q, [[zeta]] * len(chunks))], chal)
    flat = np.concatenate([v for rnd in opened for m in rnd for v in m])
    return root_t, root_a, exposed, root_q, flat, fri, ch


def _check_whole_proof(ctx, cair, prep, trace, pis, aux_source_of, cfg):
    """`aux_source_of(key)` gives the aux source.  Returns (config, key, proof, exposed)."""
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))
    key = ts.PreprocessedKey(config, prep, keep_values=True)
    source = aux_source_of(key)
    staged_chal, chal = ts.BfChallenger(), ts.BfChallenger()
    root_t, root_a, exposed, root_q, opened, fri, ch = _staged_proof(config.pcs, cair, key, trace, pis, source,
                                                                     staged_chal)
    proof = ts.prove(config, cair, chal, trace.copy(), pis, preprocessed=key, aux=source)
    pw, aw, w, qd, ne = cair.preprocessed_width, cair.aux_width, trace.shape[1], 1 << cair.log_quotient_degree, \
        cair.n_exposed
    n_open = 4 * (2 * pw + 2 * aw + 2 * w + 4 * qd)
    words = proof.words
    assert list(words[:9]) == [0x46505354, 5, trace.shape[0].bit_length() - 1, w, qd, aw, cair.n_challenges, ne, pw]
    assert (words[9:17] == root_t).all() and (words[17:25] == root_a).all()
    assert (words[25:25 + ne] == exposed).all()
    o = 25 + ne
    assert (words[o:o + 8] == root_q).all()
    o += 8
    assert (words[o:o + n_open].reshape(-1, 4) == opened).all(), "opened values differ"
    assert len(words) - o - n_open == len(fri) and (words[o + n_open:] == fri).all(), "FriProof words differ"
    assert (chal.state() == staged_chal.state()).all(), "final challenger state differs"
    assert (proof.aux_commit == root_a).all() and (proof.exposed == exposed).all()
    assert (proof.preprocessed_local == opened[:pw]).all() and (proof.preprocessed_next == opened[pw:2 * pw]).all()
    assert (proof.aux_local == opened[2 * pw:2 * pw + aw]).all()
    assert (proof.aux_next == opened[2 * pw + aw:2 * pw + 2 * aw]).all()
    assert (proof.trace_local == opened[2 * pw + 2 * aw:2 * pw + 2 * aw + w]).all()
    assert all(len(q.input_proof) == 4 for q in proof.query_proofs)
    return config, key, proof, exposed


@pytest.mark.parametrize("log_n,b", [(3, 1), (3, 2), (10, 1), (10, 2)])
def test_table_lookup_whole_proof(ctx, log_n, b):
    """TableLookupAir (pw 1, aw 8, w 2): the words of ts_prove_pre_aux are the stage composition's; the proof
    verifies against the key's root and the exposed sum is zero."""
    air, n = TableLookupAir(), 1 << log_n
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0, 1, *aux_dims(air)))
    config, key, proof, exposed = _check_whole_proof(
        ctx, cair, generate_lookup_table(n), generate_table_lookup_trace(n), [],
        lambda key: air.logup.aux_source_with(key.values), (b, 3, 2))
    got = ts.verify(config, cair, ts.BfChallenger(), proof, [], preprocessed_root=key.root)
    assert (got == exposed).all() and not got.any()
    air.logup.verify(got)
    assert not ts.verify(config, air, ts.BfChallenger(), proof, [], preprocessed_root=key.root).any()  # host-only AIR


@pytest.mark.parametrize("log_n,b", [(3, 1), (3, 2), (10, 1), (10, 2)])
def test_wide_key_whole_proof(ctx, log_n, b):
    """WrapAir with pw = 7 above both w = 2 and aw = 2: the alpha-power table's maximum is the key's width.  The
    trace is committed before the challenge is drawn and was made for challenge word 0 = 0, so this proof need not
    verify: its words are compared with the stage composition's (test_wide_key_proof_verifies has one that does)."""
    air, n = WrapAir(3, 6), 1 << log_n
    cair = ts.CompiledAir(ctx, air.tape())
    assert (cair.preprocessed_width, cair.aux_width, cair.width) == (7, 2, 2)
    prep, aux, main, pis, ex = air.matrices(n, 11 + log_n, np.zeros(4, dtype=np.uint32))
    source_of = lambda key: (lambda trace, challenges: (aux.copy(), ex.copy()))
    _check_whole_proof(ctx, cair, prep, main, pis, source_of, (b, 3, 2))


def test_wide_key_proof_verifies(ctx):
    """The same widths with constraints that hold whatever the challenge is: accepted, exposed word returned."""
    n, pw = 64, 7
    bld = SymbolicAirBuilder(2, 0, preprocessed_width=pw, aux_width=2, n_challenges=1, n_exposed=1)
    nxt, prep_n, aux_n = bld.main().row_slice(1), bld.preprocessed().row_slice(1), bld.aux().row_slice(1)
    s = aux_n[1]
    for j in range(pw):
        s = s + prep_n[j]
    bld.assert_zero(nxt[0] - s)
    bld.when_first_row().assert_zero(bld.main().row_slice(0)[1] - bld.exposed()[0])
    bld.when_transition().assert_zero(nxt[1] - bld.main().row_slice(0)[1] * bld.preprocessed().row_slice(0)[0]
                                      * bld.aux().row_slice(0)[0])
    cair = ts.CompiledAir(ctx, bld.tape())
    prep, aux, ex = _rand(1, (n, pw)), _rand(2, (n, 2)), _rand(3, (1,))
    main = np.zeros((n, 2), dtype=np.uint64)
    main[:, 0] = (prep.astype(np.uint64).sum(axis=1) + aux[:, 1]) % P
    cur = int(ex[0])
    for i in range(n):
        main[i, 1] = cur
        cur = cur * int(prep[i, 0]) * int(aux[i, 0]) % P
    main = main.astype(np.uint32)
    source_of = lambda key: (lambda trace, challenges: (aux.copy(), ex.copy()))
    config, key, proof, exposed = _check_whole_proof(ctx, cair, prep, main, [], source_of, (1, 3, 2))
    got = ts.verify(config, cair, ts.BfChallenger(), proof, [], preprocessed_root=key.root)
    assert (got == ex).all()


@pytest.fixture(scope="module")
def lookup_proof(ctx):
    air, n = TableLookupAir(), 64
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), ctx))
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0, 1, *aux_dims(air)))
    key = ts.PreprocessedKey(config, generate_lookup_table(n), keep_values=True)
    trace = generate_table_lookup_trace(n)
    source = air.logup.aux_source_with(key.values)
    proof = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], preprocessed=key, aux=source)
    assert not ts.verify(config, cair, ts.BfChallenger(), proof, [], preprocessed_root=key.root).any()
    return config, cair, air, key, trace, source, proof.words.copy()


def _rejected(config, cair, words, root):
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(config, cair, ts.BfChallenger(), words, [], preprocessed_root=root)
    assert e.value.code != 0


def _merkle_path_words(words, start):
    """Word offsets of the first digest of each BatchOpening's Merkle path in query 0 of the FriProof at `start`."""
    o = start
    R = int(words[o])
    o += 1 + 8 * R
    o += 1  # Q
    nb = int(words[o])
    o += 1
    out = []
    for _ in range(nb):
        nm = int(words[o])
        o += 1
        for _ in range(nm):
            o += 1 + int(words[o])
        plen = int(words[o])
        o += 1
        out.append(o)
        o += 8 * plen
    return out


def test_rejections(ctx, lookup_proof):
    config, cair, air, key, trace, source, words = lookup_proof
    pw, aw, w, qd, ne = 1, 8, 2, 2, 4
    o = 9 + 8 + 8 + ne + 8  # header, trace root, aux root, exposed, quotient root
    regions = [o, o + 4 * pw, o + 8 * pw, o + 8 * pw + 4 * aw, o + 8 * pw + 8 * aw, o + 8 * pw + 8 * aw + 4 * w,
               o + 8 * pw + 8 * aw + 8 * w]
    for k in regions:  # preprocessed_local, _next, aux_local, _next, trace_local, _next, chunks
        bad = words.copy()
        bad[k + 1] = (int(bad[k + 1]) + 1) % P
        _rejected(config, cair, bad, key.root)
    paths = _merkle_path_words(words, regions[-1] + 16 * qd)
    assert len(paths) == 4
    for k in paths:  # the key's, the aux trace's, the trace's and the chunks' Merkle path of query 0
        bad = words.copy()
        bad[k + 3] ^= 1
        _rejected(config, cair, bad, key.root)
    for k in (17 + 3, 25 + 1):  # the aux root, an exposed word
        bad = words.copy()
        bad[k] = (int(bad[k]) + 1) % P if k >= 25 else bad[k] ^ 1
        _rejected(config, cair, bad, key.root)
    # another key's root
    other_table = generate_lookup_table(64)
    other_table[5, 0] = 99
    other = ts.PreprocessedKey(config, other_table)
    assert not (other.root == key.root).all()
    _rejected(config, cair, words, other.root)


def test_value_outside_the_table(ctx, lookup_proof):
    """A lookup of a value the key's table does not hold: the proof verifies, the exposed sum is not zero; with the
    sum forced to zero the proof is rejected."""
    config, cair, air, key, trace, source, words = lookup_proof
    outside = generate_table_lookup_trace(64, outside_row=9)
    proof = ts.prove(config, cair, ts.BfChallenger(), outside.copy(), [], preprocessed=key, aux=source)
    S = ts.verify(config, cair, ts.BfChallenger(), proof, [], preprocessed_root=key.root)
    assert S.any()
    with pytest.raises(ValueError):
        air.logup.verify(S)

    def forced(tr, challenges):
        aux, _ = air.logup.build(tr, challenges, preprocessed=key.values)
        return aux, np.zeros(4, dtype=np.uint32)

    proof = ts.prove(config, cair, ts.BfChallenger(), outside.copy(), [], preprocessed=key, aux=forced)
    assert proof.words[1] == 5
    _rejected(config, cair, proof.words, key.root)


def test_one_key_serves_two_proofs(ctx, lookup_proof):
    config, cair, air, key, trace, source, words = lookup_proof
    top = [key.data.digests(l).copy() for l in (key.data.log_height, 0)]
    values = key.values.download().copy()
    proofs = []
    for seed in (5, 6):
        t = generate_table_lookup_trace(64, seed=seed)
        proof = ts.prove(config, cair, ts.BfChallenger(), t, [], preprocessed=key, aux=source)
        assert not ts.verify(config, cair, ts.BfChallenger(), proof, [], preprocessed_root=key.root).any()
        proofs.append(proof.words)
    assert not (len(proofs[0]) == len(proofs[1]) and (proofs[0] == proofs[1]).all())
    for l, want in zip((key.data.log_height, 0), top):
        assert (key.data.digests(l) == want).all()
    assert (key.values.download() == values).all()
    # and the first proof again: the words of the fixture's
    again = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], preprocessed=key, aux=source)
    assert len(again.words) == len(words) and (again.words == words).all()


# ------------------------------------------------------------------ 5. the degenerate forms
def _raw_prove_pre_aux(ctx, cfg, cair, key_h, trace, pis, fn, cap=1 << 18):
    l = _lib.lib()
    out, n_words = np.zeros(cap, dtype=np.uint32), C.c_size_t()
    chal, m = ts.BfChallenger(), ts.DeviceMatrix.upload(ctx, trace)
    p = np.ascontiguousarray(pis, dtype=np.uint32)
    rc = l.ts_prove_pre_aux(ctx.h, C.byref(cfg), cair.h, chal.h, key_h, m.h, p.ctypes.data_as(_lib.u32p) if len(p) else None,
                            len(p), fn, None, out.ctypes.data_as(_lib.u32p), len(out), C.byref(n_words))
    return rc, out[:n_words.value].copy(), (l.ts_last_error(ctx.h) or b"").decode(), m


def test_without_preprocessed_columns_is_prove_aux(ctx):
    """pw = 0: the key and the root must be NULL and the words are ts_prove_aux's apart from the header."""
    air, n = RangeLookupAir(), 64
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), ctx))
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0, 0, *aux_dims(air)))
    trace = generate_range_lookup_trace(n)
    v4 = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], aux=air.logup.aux_source).words
    failure: list = []
    from tapstark_amd.stark import _aux_callback
    cb = _aux_callback(ctx, cair, air.logup.aux_source, failure)
    rc, v5, msg, _ = _raw_prove_pre_aux(ctx, config.pcs.fri._c(), cair, None, trace, [], cb)
    assert rc == 0 and not failure, msg
    assert list(v5[:9]) == [v4[0], 5, *v4[2:8], 0] and (v5[9:] == v4[8:]).all()
    l, cfg = _lib.lib(), config.pcs.fri._c()
    verdict, ex, vchal = C.c_int(-1), np.ones(4, dtype=np.uint32), ts.BfChallenger()
    assert l.ts_verify_pre_aux(C.byref(cfg), cair.h, vchal.h, None, v5.ctypes.data_as(_lib.u32p), len(v5), None, 0,
                               ex.ctypes.data_as(_lib.u32p), 4, C.byref(verdict)) == 0
    assert verdict.value == 0 and not ex.any()
    # a key for such an AIR is refused before the trace is taken
    key = ts.PreprocessedKey(config, generate_lookup_table(n))
    rc, _, msg, m = _raw_prove_pre_aux(ctx, cfg, cair, key.data.h, trace, [], cb)
    assert rc == TS_ERR_INVALID and "key" in msg and m.dims() == trace.shape


def test_without_aux_columns_is_prove_pre(ctx):
    """aw = 0: aux_fn must be NULL and the words are ts_prove_pre's apart from the header."""
    air, n = SelectorAir(), 64
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), ctx))
    prep = generate_selector_preprocessed(n)
    trace, pis = generate_selector_trace(prep)
    key = ts.PreprocessedKey(config, prep)
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 2, 3))
    v3 = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), pis, preprocessed=key).words
    cfg = config.pcs.fri._c()
    rc, v5, msg, _ = _raw_prove_pre_aux(ctx, cfg, cair, key.data.h, trace, pis, _lib.AUX_FN())
    assert rc == 0, msg
    assert list(v5[:9]) == [v3[0], 5, v3[2], v3[3], v3[4], 0, 0, 0, v3[5]] and (v5[9:] == v3[6:]).all()
    got = ts.verify(config, cair, ts.BfChallenger(), v5, pis, preprocessed_root=key.root)
    assert got is not None and len(got) == 0
    # an aux_fn for such an AIR, and a null key: refused before the trace is taken
    cb = _lib.AUX_FN(lambda user, c, t, ch, k, aux_out, exposed_out: 0)
    rc, _, msg, m = _raw_prove_pre_aux(ctx, cfg, cair, key.data.h, trace, pis, cb)
    assert rc == TS_ERR_INVALID and "aux_fn" in msg and m.dims() == trace.shape
    rc, _, msg, m = _raw_prove_pre_aux(ctx, cfg, cair, None, trace, pis, _lib.AUX_FN())
    assert rc == TS_ERR_INVALID and "key" in msg and m.dims() == trace.shape


# ------------------------------------------------------------------ 6. the callback and the key argument
def test_callback_statuses_and_key_refusals(ctx, lookup_proof):
    config, cair, air, key, trace, source, words = lookup_proof
    cfg = config.pcs.fri._c()
    # a status of the callback's own is propagated, and the text names the callback
    rc, _, msg, _ = _raw_prove_pre_aux(ctx, cfg, cair, key.data.h, trace, [],
                                       _lib.AUX_FN(lambda user, c, t, ch, k, aux_out, exposed_out: 7))
    assert rc == 7 and "aux callback" in msg and "7" in msg
    # a null aux_fn, a null key: refused before the trace is taken
    rc, _, msg, m = _raw_prove_pre_aux(ctx, cfg, cair, key.data.h, trace, [], _lib.AUX_FN())
    assert rc == TS_ERR_INVALID and "aux_fn" in msg and m.dims() == trace.shape
    # a key of another width, height, context: refused with the trace not consumed
    wide = ts.PreprocessedKey(config, np.hstack([generate_lookup_table(64)] * 2))
    tall = ts.PreprocessedKey(config, generate_lookup_table(128))
    other = ts.Context(ctx.device)
    foreign = ts.PreprocessedKey(ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), other)),
                                 generate_lookup_table(64))
    for what, k in (("width", wide), ("height", tall), ("context", foreign)):
        m = ts.DeviceMatrix.upload(ctx, trace)
        _raises(TS_ERR_INVALID, lambda: ts.prove(config, cair, ts.BfChallenger(), m, [], preprocessed=k, aux=source),
                what)
        assert m.dims() == trace.shape, what
    # an aux matrix of another shape, or made on another context
    for bad in (np.zeros((64, 4), dtype=np.uint32), np.zeros((32, 8), dtype=np.uint32)):
        _raises(TS_ERR_INVALID, lambda: ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], preprocessed=key,
                                                 aux=lambda t, c: (bad, np.zeros(4, dtype=np.uint32))), "aux matrix")
    from_other = lambda t, c: (ts.DeviceMatrix.upload(other, np.zeros((64, 8), dtype=np.uint32)),
                               np.zeros(4, dtype=np.uint32))
    _raises(TS_ERR_INVALID, lambda: ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], preprocessed=key,
                                             aux=from_other), "context")
    again = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], preprocessed=key, aux=source)
    assert (again.words == words).all()


# ------------------------------------------------------------------ 7. the paths that must not move
def test_other_proofs_are_unchanged_by_a_pre_aux_proof(ctx, lookup_proof):
    """On one context: a ts_prove, a ts_prove_pre and a ts_prove_aux proof made after a ts_prove_pre_aux proof
    equal the same proofs made before it."""
    config, cair, air, key, trace, source, words = lookup_proof
    mul_trace = generate_synth_mul_trace(64, 6)
    mul = ts.CompiledAir(ctx, ts.air_tape(SynthMulAir(6), 0))
    sel_prep = generate_selector_preprocessed(64)
    sel_trace, sel_pis = generate_selector_trace(sel_prep)
    sel_key = ts.PreprocessedKey(config, sel_prep)
    sel = ts.CompiledAir(ctx, ts.air_tape(SelectorAir(), 2, 3))
    rng_air = RangeLookupAir()
    rng = ts.CompiledAir(ctx, ts.air_tape(rng_air, 0, 0, *aux_dims(rng_air)))
    rng_trace = generate_range_lookup_trace(64)

    def three():
        return [ts.prove(config, mul, ts.BfChallenger(), mul_trace.copy(), []).words,
                ts.prove(config, sel, ts.BfChallenger(), sel_trace.copy(), sel_pis, preprocessed=sel_key).words,
                ts.prove(config, rng, ts.BfChallenger(), rng_trace.copy(), [], aux=rng_air.logup.aux_source).words]

    before = three()
    mid = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), [], preprocessed=key, aux=source)
    assert (mid.words == words).all()
    after = three()
    assert [int(w[1]) for w in before] == [1, 3, 4]
    for b, a in zip(before, after):
        assert len(a) == len(b) and (a == b).all()


# ------------------------------------------------------------------ 8. the C++ example
def test_cpp_table_lookup_example(ctx, tmp_path):
    """examples/table_lookup_air.cpp: the key committed once, two proofs with ts_prove_pre_aux through a C callback
    that calls ts_logup_aux_build_pre, each verified against the root with the exposed sum zero."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "table_lookup_air")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "table_lookup_air.cpp"), "-L", libdir, "-ltapstark_hip",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("verify -> 0") == 2 and r.stdout.count("sum is zero") == 2 and "TSPF v5" in r.stdout
