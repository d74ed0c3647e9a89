"""ts_prove_multi on the GPU: several plain AIR tables of mixed heights in one TSPF v6 proof.

The oracle proves one table, so exactness comes from composition, as in test_gpu_pre_aux.py: a multi proof is,
word for word, the Python staging of tests/_multi_cases.py -- the host challenger around ts_pcs_commit (mixed
heights), ts_quotient_chunks of every trace committed ALONE, one ts_pcs_commit of all chunks and ts_pcs_open over
the two rounds -- all of them calls that tests/test_oracle.py and tests/test_gpu_pcs*.py pin to the oracle.  The
per-class opening kernels (csrc/open_multi.hip) are pinned to the generic opening by the same equality and by
TS_MULTI_OPEN_GENERIC=1.  The CPU half is tests/test_multi_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.airs import (SelectorAir, SynthMulAir, RangeLookupAir, generate_selector_preprocessed,
                               generate_selector_trace, generate_synth_mul_trace)
from tapstark_amd.air import aux_dims
import _multi_cases as mc
import _poison

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_UNSUPPORTED, TS_ERR_INVARIANT, TS_ERR_BUFFER = 1, 4, 5, 6
KNOB = "TS_MULTI_OPEN_GENERIC"


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(scope="module")
def accepted_b(ctx):
    """One accepted proof of case b at log_blowup 2: (config, tables, host-only AIRs, words)."""
    tables = mc.case("b", 2)
    cfg = mc.config(ctx, 2)
    proof = mc.prove(cfg, mc.compiled(ctx, tables), tables)
    hairs = [ts.CompiledAir(None, t.tape) for t in tables]
    ts.verify_multi(cfg, hairs, ts.BfChallenger(), proof, [t.pis for t in tables])
    proof.words.setflags(write=False)
    return cfg, tables, hairs, proof.words


def _verdict(cfg, airs, words, pis):
    try:
        ts.verify_multi(cfg, airs, ts.BfChallenger(), words, pis)
    except ts.VerificationError as e:
        return e.code
    return 0


def test_case_set_has_the_edges():
    qds = {1 << t.lqd for name in mc.CASE_NAMES for t in mc.case(name, 2)}
    assert {1, 2, 4} <= qds
    assert sorted(1 << t.lqd for t in mc.case("d_equal", 2)) == [1, 2, 4]
    assert sorted(1 << t.lqd for t in mc.case("d_mixed", 2)) == [1, 2, 4]
    assert [t.log_n for t in mc.case("d_mixed", 2)] == [4, 6, 8] and {t.log_n for t in mc.case("d_equal", 2)} == {6}
    assert [t.trace.shape for t in mc.case("a", 2)] == [(32, 2), (32, 72)]
    assert [t.log_n for t in mc.case("b", 2)] == [3, 6, 3]
    assert [(t.log_n, t.trace.shape[1]) for t in mc.case("c", 2)][0] == (16, 8)
    assert [t.log_n for t in mc.case("c", 2)] == [16, 10, 10, 4]
    assert len(mc.case("e", 2)) == 64 and all(t.log_n == 3 for t in mc.case("e", 2))
    # blowup 1 drops exactly the degree-4 AIRs
    assert all(t.lqd <= 1 for name in mc.CASE_NAMES for t in mc.case(name, 1))
    assert len(mc.case("d_equal", 1)) == 2 and len(mc.case("c", 1)) == 3


# ------------------------------------------------------------------ 1. staged composition
@pytest.mark.parametrize("log_blowup", [1, 2])
@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_multi_proof_is_the_staged_composition(ctx, name, log_blowup):
    tables = mc.case(name, log_blowup)
    cfg = mc.config(ctx, log_blowup)
    cairs = mc.compiled(ctx, tables)
    staged_chal, chal = ts.BfChallenger(), ts.BfChallenger()
    root_t, root_q, opened, fri = mc.staged_proof(cfg.pcs, cairs, tables, staged_chal)
    proof = mc.prove(cfg, cairs, tables, chal)
    words, reg = proof.words, mc.regions(tables)
    assert list(words[:reg["tables"][1]]) == mc.header_words(tables)
    assert (words[slice(*reg["trace_root"])] == root_t).all(), "trace root differs"
    assert (words[slice(*reg["quotient_root"])] == root_q).all(), "quotient root differs"
    o = reg["fri"][0]
    assert (words[reg["quotient_root"][1]:o].reshape(-1, 4) == opened).all(), "opened values differ"
    assert len(words) - o == len(fri) and (words[o:] == fri).all(), "FriProof words differ"
    assert (chal.state() == staged_chal.state()).all(), "final challenger state differs"
    # the parsed form
    assert (proof.trace_commit == root_t).all() and (proof.quotient_commit == root_q).all()
    assert [(t.log_degree, t.width, t.qd) for t in proof.tables] == \
        [(t.log_n, t.trace.shape[1], 1 << t.lqd) for t in tables]
    k = 0
    for pt in proof.tables:
        assert (pt.trace_local == opened[k:k + pt.width]).all() and \
            (pt.trace_next == opened[k + pt.width:k + 2 * pt.width]).all()
        k += 2 * pt.width
    for pt in proof.tables:
        assert (pt.quotient_chunks.reshape(-1, 4) == opened[k:k + 4 * pt.qd]).all()
        k += 4 * pt.qd
    assert len(proof.query_proofs) == mc.FRI_QUERIES and (proof.fri_words == fri).all()
    ts.verify_multi(cfg, [ts.CompiledAir(None, t.tape) for t in tables], ts.BfChallenger(), proof,
                    [t.pis for t in tables])


def test_golden_fixture_is_what_the_prover_writes(ctx):
    doc, tapes, pis, want = mc.load_golden()
    tables = mc.case("b", 1)
    assert all((t.tape == tape).all() for t, tape in zip(tables, tapes))
    got = mc.prove(mc.config(ctx, 1), mc.compiled(ctx, tables), tables).words
    assert len(got) == len(want) and (got == want).all()


# ------------------------------------------------------------------ 2. degenerate form
@pytest.mark.parametrize("name", ["t1_fib", "t1_mul"])
def test_one_table_is_ts_prove_behind_the_shape_words(ctx, name):
    (t,) = mc.case(name, 2)
    cfg = mc.config(ctx, 2)
    cair = mc.compiled(ctx, [t])[0]
    c1, c6 = ts.BfChallenger(), ts.BfChallenger()
    c1.observe(1)
    c1.observe(t.log_n)
    single = ts.prove(cfg, cair, c1, t.trace.copy(), t.pis).words
    multi = mc.prove(cfg, [cair], [t], c6).words
    assert list(single[:5]) == [0x46505354, 1, t.log_n, t.trace.shape[1], 1 << t.lqd]
    assert list(multi[:6]) == [0x46505354, 6, 1, t.log_n, t.trace.shape[1], 1 << t.lqd]
    assert len(multi) - 6 == len(single) - 5 and (multi[6:] == single[5:]).all()
    assert (c1.state() == c6.state()).all()


# ------------------------------------------------------------------ 3. both opening paths
def _launches(ctx, cfg, cairs, tables):
    ctx.take_kernel_timings()
    ctx.set_kernel_timing(True)
    try:
        words = mc.prove(cfg, cairs, tables).words
        return words, {k: v[0] for k, v in ctx.take_kernel_timings().items()}
    finally:
        ctx.set_kernel_timing(False)


@pytest.mark.parametrize("name", ["b", "c", "d_equal", "d_mixed"])
def test_class_path_and_generic_path_write_the_same_proof(ctx, monkeypatch, name):
    tables = mc.case(name, 2)
    cfg = mc.config(ctx, 2)
    cairs = mc.compiled(ctx, tables)
    monkeypatch.delenv(KNOB, raising=False)
    words, by_class = _launches(ctx, cfg, cairs, tables)
    monkeypatch.setenv(KNOB, "1")
    generic, by_matrix = _launches(ctx, cfg, cairs, tables)
    assert len(words) == len(generic) and (words == generic).all()
    n_classes = len({t.log_n for t in tables})
    generic_reduces = sum(v for k, v in by_matrix.items() if k.startswith("k_reduce<"))
    assert by_class.get("k_reduce_class", 0) == n_classes and by_class.get("k_bary_finish_jobs", 0) == 1
    assert not any(k.startswith("k_reduce<") for k in by_class)
    assert "k_reduce_class" not in by_matrix and "k_bary_finish_jobs" not in by_matrix
    # the generic path: one k_reduce launch per matrix (its one or two points together)
    assert generic_reduces == len(tables) + sum(1 << t.lqd for t in tables)
    if name == "c":
        assert n_classes == 3


# ------------------------------------------------------------------ 4. unwritten memory
@pytest.fixture(scope="module")
def poison_contexts(ctx):
    return _poison.make_contexts()


@pytest.mark.parametrize("name", ["b", "d_equal", "d_mixed"])
def test_nothing_reads_unwritten_memory(poison_contexts, name):
    tables = mc.case(name, 2)

    def run(c):
        return mc.prove(mc.config(c, 2), mc.compiled(c, tables), tables).words

    _poison.same_everywhere(poison_contexts, run, what=f"prove_multi case {name}")
    assert all(c.stat(_poison.STAT_FILLS) > 0 for c in poison_contexts[1:])
    assert poison_contexts[0].stat(_poison.STAT_FILLS) == 0


# ------------------------------------------------------------------ 5. rejections
def test_one_flipped_word_per_region_is_rejected(accepted_b):
    cfg, tables, hairs, words = accepted_b
    pis = [t.pis for t in tables]
    reg = mc.regions(tables)
    fri0 = reg["fri"][0]
    R = int(words[fri0])
    assert R == 6 and int(words[fri0 + 1 + 8 * R]) == mc.FRI_QUERIES
    n = len(words)
    # region -> (word index, the verdicts that region owns)
    flips = {
        "table width": (reg["tables"][0] + 3 * 1 + 1, {1}),
        "table qd": (reg["tables"][0] + 3 * 2 + 2, {1}),
        "table log_degree": (reg["tables"][0], {7, 1, 9}),         # another transcript and another domain
        "trace root": (reg["trace_root"][0] + 3, {7, 4}),           # another alpha and zeta
        "quotient root": (reg["quotient_root"][0] + 5, {7, 4}),     # another zeta
        "short table's trace value": (reg["trace_values"][2][0] + 1, {7, 9}),
        "chunk value": (reg["chunk_values"][1][0] + 6, {7, 9}),
        "FRI round root": (fri0 + 1 + 8 * 2, {3, 5, 8}),            # another transcript from that round on
        "final polynomial": (n - 5, {6, 9}),
        "PoW witness": (n - 1, {3, 4, 8}),                          # a lucky witness still moves every query index
    }
    for what, (at, owned) in flips.items():
        bad = words.copy()
        bad[at] ^= 1
        v = _verdict(cfg, hairs, bad, pis)
        assert v != 0 and v in owned, f"{what}: verdict {v}"
    assert _verdict(cfg, hairs, words, pis) == 0


def test_swapped_public_values_and_table_order_are_rejected(accepted_b):
    cfg, tables, hairs, words = accepted_b
    pis = [t.pis for t in tables]
    assert not (pis[0] == pis[2]).all()
    assert _verdict(cfg, hairs, words, [pis[2], pis[1], pis[0]]) == 7
    assert _verdict(cfg, hairs[::-1], words, pis[::-1]) != 0                            # same shapes, other statement
    assert _verdict(cfg, [hairs[1], hairs[0], hairs[2]], words, [pis[1], pis[0], pis[2]]) == 1  # other widths
    assert _verdict(cfg, hairs[:2], words, pis[:2]) == 1


def test_single_table_verifiers_answer_a_v6_proof_with_9(accepted_b):
    cfg, tables, hairs, words = accepted_b
    l = _lib.lib()
    fri = cfg.pcs.fri._c()
    air, pis = hairs[0], tables[0].pis
    w = np.ascontiguousarray(words)
    wp, pp = w.ctypes.data_as(_lib.u32p), pis.ctypes.data_as(_lib.u32p)
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(cfg, air, ts.BfChallenger(), w, pis)
    assert e.value.code == 9
    chals = [ts.BfChallenger() for _ in range(4)]  # kept alive across the calls
    v = C.c_int(-1)
    l.ts_verify_pre(C.byref(fri), air.h, chals[0].h, None, wp, len(w), pp, len(pis), C.byref(v))
    assert v.value == 9
    v = C.c_int(-1)
    l.ts_verify_aux(C.byref(fri), air.h, chals[1].h, wp, len(w), pp, len(pis), None, 0, C.byref(v))
    assert v.value == 9
    v = C.c_int(-1)
    l.ts_verify_pre_aux(C.byref(fri), air.h, chals[2].h, None, wp, len(w), pp, len(pis), None, 0, C.byref(v))
    assert v.value == 9
    v = C.c_int(-1)
    scripts, offsets = b"\0", (C.c_uint64 * 1)(0)  # an empty lock table
    rc = l.ts_verify_tap(C.byref(fri), air.h, chals[3].h, wp, len(w), pp, len(pis), scripts, offsets, 0,
                         C.byref(v))
    assert rc == 0 and v.value == 9
    with pytest.raises(_lib.TsError) as e:
        ts.Proof(w).to_postcard()
    assert e.value.code == TS_ERR_UNSUPPORTED


# ------------------------------------------------------------------ 6. refusals
def _call(ctx, cfg, entries, cap=1 << 16, chal=None, struct_size=None):
    """ts_prove_multi on (CompiledAir, DeviceMatrix, pis) entries: (status, text, words or needed size)."""
    T = len(entries)
    tabs = (_lib.MultiTableC * max(T, 1))()
    keep = []
    for k, (a, m, p) in enumerate(entries):
        p = np.asarray(p, dtype=np.uint32)
        keep.append(p)
        tabs[k].struct_size = C.sizeof(_lib.MultiTableC) if struct_size is None else struct_size
        tabs[k].n_public = len(p)
        tabs[k].air = a.h if a is not None else None
        tabs[k].trace = m.h if m is not None else None
        tabs[k].public_values = p.ctypes.data_as(_lib.u32p) if len(p) else None
    out = np.zeros(max(cap, 1), dtype=np.uint32)
    n = C.c_size_t()
    fri = cfg.pcs.fri._c()
    chal = chal or ts.BfChallenger()
    rc = ctx._l.ts_prove_multi(ctx.h, C.byref(fri), chal.h, tabs, T, out.ctypes.data_as(_lib.u32p), cap, C.byref(n))
    text = (ctx._l.ts_last_error(ctx.h) or b"").decode()
    return rc, text, (out[:n.value].copy() if rc == 0 else n.value)


def test_refusals_consume_nothing(ctx):
    cfg1, cfg2 = mc.config(ctx, 1), mc.config(ctx, 2)
    fib, mul, fib2 = mc.case("b", 2)
    cf, cm = ts.CompiledAir(ctx, fib.tape), ts.CompiledAir(ctx, mul.tape)
    high = mc.high(4)
    ch = ts.CompiledAir(ctx, high.tape)
    mats = {}

    def up(t, key=None):
        m = ts.DeviceMatrix.upload(ctx, t.trace.copy())
        mats[key or len(mats)] = (m, t.trace)
        return m

    f, m, h = up(fib), up(mul), up(high)
    other = ts.Context(0)
    f_other = ts.DeviceMatrix.upload(other, fib.trace.copy())
    cf_other = ts.CompiledAir(other, fib.tape)
    cf_host = ts.CompiledAir(None, fib.tape)
    # a version-2 tape with one preprocessed column, a version-3 tape with aux columns
    sel = ts.CompiledAir(ctx, ts.air_tape(SelectorAir(), 2, 3))
    sel_trace, sel_pis = generate_selector_trace(generate_selector_preprocessed(8))
    assert sel.preprocessed_width >= 1
    pre1 = ts.CompiledAir(ctx, ts.air_tape(_OnePrepAir(), 0, 1))
    assert pre1.preprocessed_width == 1
    rng_air = RangeLookupAir()
    rng = ts.CompiledAir(ctx, ts.air_tape(rng_air, 0, 0, *aux_dims(rng_air)))
    assert rng.aux_width > 0
    s = ts.DeviceMatrix.upload(ctx, sel_trace.copy())
    p1 = ts.DeviceMatrix.upload(ctx, np.ones((8, 1), dtype=np.uint32))
    r = ts.DeviceMatrix.upload(ctx, np.zeros((8, rng.width), dtype=np.uint32))
    fibs65 = [ts.DeviceMatrix.upload(ctx, fib.trace.copy()) for _ in range(65)]
    mul8 = mc.mul(3, 6)
    cm8 = ts.CompiledAir(ctx, mul8.tape)
    muls = [ts.DeviceMatrix.upload(ctx, mul8.trace.copy()) for _ in range(32)]

    cases = [
        ("no tables", cfg2, [], {}, TS_ERR_INVALID),
        ("65 tables", cfg2, [(cf, x, fib.pis) for x in fibs65], {}, TS_ERR_INVALID),
        ("65 chunks", cfg2, [(cm8, x, []) for x in muls] + [(cf, f, fib.pis)], {}, TS_ERR_INVALID),
        ("struct_size", cfg2, [(cf, f, fib.pis)], {"struct_size": 24}, TS_ERR_INVALID),
        ("null air", cfg2, [(cf, f, fib.pis), (None, m, [])], {}, TS_ERR_INVALID),
        ("null trace", cfg2, [(cf, f, fib.pis), (cm, None, [])], {}, TS_ERR_INVALID),
        ("trace of another context", cfg2, [(cf, f_other, fib.pis)], {}, TS_ERR_INVALID),
        ("air of another context", cfg2, [(cf_other, f, fib.pis)], {}, TS_ERR_INVALID),
        ("host-only air", cfg2, [(cf_host, f, fib.pis)], {}, TS_ERR_INVALID),
        ("width", cfg2, [(cf, f, fib.pis), (cf, m, fib.pis)], {}, TS_ERR_INVALID),
        ("n_public", cfg2, [(cf, f, fib.pis[:2]), (cm, m, [])], {}, TS_ERR_INVALID),
        ("one handle twice", cfg2, [(cf, f, fib.pis), (cm, m, []), (cf, f, fib2.pis)], {}, TS_ERR_INVALID),
        ("preprocessed columns", cfg2, [(cf, f, fib.pis), (sel, s, sel_pis)], {}, TS_ERR_UNSUPPORTED),
        ("preprocessed width 1", cfg2, [(cf, f, fib.pis), (pre1, p1, [])], {}, TS_ERR_UNSUPPORTED),
        ("aux columns", cfg2, [(rng, r, []), (cf, f, fib.pis)], {}, TS_ERR_UNSUPPORTED),
        ("lqd above the blowup", cfg1, [(cf, f, fib.pis), (ch, h, [])], {}, TS_ERR_INVARIANT),
    ]
    for what, cfg, entries, kw, want in cases:
        rc, text, _ = _call(ctx, cfg, entries, **kw)
        assert rc == want, f"{what}: status {rc} ({text})"
        assert text, f"{what}: no text"
    # every handle is still usable: download and compare, then prove with them
    for key, (mat, values) in mats.items():
        assert (mat.download() == values).all(), key
    assert (f_other.download() == fib.trace).all() and (s.download() == sel_trace).all()
    assert all((x.download() == fib.trace).all() for x in fibs65[::16])
    assert all((x.download() == mul8.trace).all() for x in muls[::8])
    l = ctx._l
    assert l.ts_prove_multi(None, None, None, None, 0, None, 0, None) == TS_ERR_INVALID
    rc, text, _ = _call(ctx, cfg2, [(cf, f, fib.pis), (cm, m, [])])
    assert rc == 0, text


class _OnePrepAir(ts.BaseAir):
    """One main column equal to one preprocessed column: the smallest version-2 tape."""

    def width(self):
        return 1

    def preprocessed_width(self):
        return 1

    def eval(self, builder):
        builder.assert_zero(builder.main().row_slice(0)[0] - builder.preprocessed().row_slice(0)[0])


def test_short_buffer_reports_the_size(ctx):
    cfg = mc.config(ctx, 2)
    fib, mul, _ = mc.case("b", 2)
    cf, cm = ts.CompiledAir(ctx, fib.tape), ts.CompiledAir(ctx, mul.tape)

    def entries():
        return [(cf, ts.DeviceMatrix.upload(ctx, fib.trace.copy()), fib.pis),
                (cm, ts.DeviceMatrix.upload(ctx, mul.trace.copy()), [])]

    rc, text, need = _call(ctx, cfg, entries(), cap=100)
    assert rc == TS_ERR_BUFFER and need > 100 and text
    rc, text, words = _call(ctx, cfg, entries(), cap=need)
    assert rc == 0 and len(words) == need
    assert need == ts.stark._multi_capacity([(8, 2, 0), (64, 6, 1)], cfg.pcs.fri)
    ts.verify_multi(cfg, [ts.CompiledAir(None, fib.tape), ts.CompiledAir(None, mul.tape)], ts.BfChallenger(), words,
                    [fib.pis, []])


def test_a_violated_constraint_gets_the_single_table_status(ctx):
    cfg = mc.config(ctx, 2)
    fib, mul, _ = mc.case("b", 2)
    cf, cm = ts.CompiledAir(ctx, fib.tape), ts.CompiledAir(ctx, mul.tape)
    bad = mul.trace.copy()
    bad[5, 2] ^= 1
    def status(fn):
        try:
            return 0, fn()
        except _lib.TsError as e:
            return e.code, None

    # (a release build of the reference proves such a trace without complaint, and so may ts_prove: the proof is
    # then one no verifier accepts)
    alone, single = status(lambda: ts.prove(cfg, cm, ts.BfChallenger(), bad.copy(), []))
    multi, proof = status(lambda: ts.prove_multi(cfg, [cf, cm], ts.BfChallenger(), [fib.trace.copy(), bad.copy()],
                                                 [fib.pis, []]))
    assert multi == alone
    if multi == 0:
        hairs = [ts.CompiledAir(None, fib.tape), ts.CompiledAir(None, mul.tape)]
        assert _verdict(cfg, hairs, proof.words, [fib.pis, []]) != 0
        with pytest.raises(ts.VerificationError):
            ts.verify(cfg, hairs[1], ts.BfChallenger(), single, [])


# ------------------------------------------------------------------ 7. nothing else moves
def test_other_proofs_are_unchanged_by_a_multi_proof(ctx, accepted_b):
    _, tables, _, words = accepted_b
    cfg = mc.config(ctx, 2)
    mul_trace = generate_synth_mul_trace(64, 6)
    mul = ts.CompiledAir(ctx, ts.air_tape(SynthMulAir(6), 0))
    sel_prep = generate_selector_preprocessed(64)
    sel_trace, sel_pis = generate_selector_trace(sel_prep)
    sel_key = ts.PreprocessedKey(cfg, sel_prep)
    sel = ts.CompiledAir(ctx, ts.air_tape(SelectorAir(), 2, 3))

    def three():
        batch = ts.prove_batch([(cfg, mul)], [mul_trace.copy()], [0])
        return [ts.prove(cfg, mul, ts.BfChallenger(), mul_trace.copy(), []).words,
                ts.prove(cfg, sel, ts.BfChallenger(), sel_trace.copy(), sel_pis, preprocessed=sel_key).words,
                np.asarray(batch.proofs[0].words)]

    before = three()
    mid = mc.prove(cfg, mc.compiled(ctx, tables), tables).words
    assert (mid == words).all()
    after = three()
    assert [int(w[1]) for w in before] == [1, 3, 1]
    for b, a in zip(before, after):
        assert len(a) == len(b) and (a == b).all()


# ------------------------------------------------------------------ 8. the C++ example
def test_cpp_multi_table_example(ctx, tmp_path):
    """examples/multi_table.cpp: a 2^10-row and a 2^6-row Fibonacci table in one proof, verified, then rejected
    with one public value flipped."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "multi_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "multi_table.cpp"), "-L", libdir, "-ltapstark_hip",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TSPF v6" in r.stdout and "verify -> 0" in r.stdout and "flipped public value -> 7" in r.stdout
