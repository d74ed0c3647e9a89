"""ts_prove_multi_bus on the GPU: tables of mixed heights tied by a LogUp bus in one TSPF v7 proof, and
ts_logup_aux_build_multi, the builder of every table's LogUp columns in three launches.

Exactness comes from composition, as in test_gpu_multi.py and test_gpu_aux.py: a bus proof is, word for word, the
Python staging of tests/_bus_cases.py -- the host challenger around ts_pcs_commit, the SINGLE-table
ts_logup_aux_build per table, ts_quotient_chunks_aux of every trace and aux matrix committed ALONE, and ts_pcs_open
over the three rounds.  The job-table builder is pinned to the single-table one by that equality, by
TS_MULTI_LOGUP_PER_TABLE=1 and, directly, by the Python-integer reference of tests/_aux_airs.py.  The CPU half is
tests/test_multi_bus_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.air import LogUp, logup_build_multi
from tapstark_amd.airs import (BusSendAir, SelectorAir, generate_selector_preprocessed, generate_selector_trace,
                               splitmix64_stream)
import _bus_cases as bc
import _multi_cases as mc
import _poison
from _aux_airs import logup_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x78000001
TS_ERR_INVALID, TS_ERR_UNSUPPORTED, TS_ERR_INVARIANT, TS_ERR_BUFFER = 1, 4, 5, 6
OPEN_KNOB, LOGUP_KNOB, BLOCK_KNOB = "TS_MULTI_OPEN_GENERIC", "TS_MULTI_LOGUP_PER_TABLE", "TS_LOGUP_BLOCK_ROWS"


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(scope="module")
def accepted_b(ctx):
    """One accepted proof of case b at log_blowup 2: (config, tables, host-only AIRs, words)."""
    tables = bc.case("b")
    cfg = bc.config(ctx, 2)
    proof = bc.prove(cfg, bc.compiled(ctx, tables), tables)
    hairs = [ts.CompiledAir(None, t.tape) for t in tables]
    ts.verify_multi_bus(cfg, hairs, ts.BfChallenger(), proof, [t.pis for t in tables])
    proof.words.setflags(write=False)
    return cfg, tables, hairs, proof.words


def _verdict(cfg, airs, words, pis):
    try:
        ts.verify_multi_bus(cfg, airs, ts.BfChallenger(), words, pis, check_bus=False)
    except ts.VerificationError as e:
        return e.code
    return 0


def test_case_set_has_the_edges():
    a, b, c, e = (bc.case(n) for n in bc.CASE_NAMES)
    assert [(t.log_n, t.aux_width) for t in a] == [(5, 8), (5, 8)]
    assert [(t.log_n, t.aux_width) for t in b] == [(3, 8), (4, 0), (6, 8), (3, 16), (1, 8)]
    assert [t.log_n for t in c] == [12, 8, 10] and c[2].aux_width == 0
    assert len(e) == 32 and sum(1 << t.lqd for t in e) == 64 and {t.log_n for t in e} == {3}
    # every bus AIR has constraint degree 3: two chunks, fits log_blowup 1
    assert all(t.lqd == 1 for n in bc.CASE_NAMES for t in bc.case(n) if t.aux_width)
    assert all(t.lqd <= 1 for n in bc.CASE_NAMES for t in bc.case(n))
    # senders stay below the range table's height
    assert all(int(t.trace[:, 0::2].max()) < 8 for t in b[2:])
    # every sender sends and holds back (a selector column that is constant makes its value column free)
    assert all(0 < int(t.trace[:, 1::2][:, i].sum()) < t.trace.shape[0] for t in b[2:] for i in range(t.trace.shape[1] // 2))


# ------------------------------------------------------------------ 1. staged composition
@pytest.mark.parametrize("log_blowup", [1, 2])
@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_bus_proof_is_the_staged_composition(ctx, name, log_blowup):
    tables = bc.case(name)
    cfg = bc.config(ctx, log_blowup)
    cairs = bc.compiled(ctx, tables)
    staged_chal, chal = ts.BfChallenger(), ts.BfChallenger()
    root_t, root_a, exposed, root_q, opened, fri = bc.staged_proof(cfg.pcs, cairs, tables, staged_chal)
    proof = bc.prove(cfg, cairs, tables, chal)
    words, reg = proof.words, bc.regions(tables)
    assert list(words[:reg["tables"][1]]) == bc.header_words(tables)
    assert (words[slice(*reg["trace_root"])] == root_t).all(), "trace root differs"
    assert (words[slice(*reg["aux_root"])] == root_a).all(), "aux root differs"
    assert (words[slice(*reg["exposed"])].reshape(-1, 4) == exposed).all(), "exposed words differ"
    assert (words[slice(*reg["quotient_root"])] == root_q).all(), "quotient root differs"
    o = reg["fri"][0]
    assert (words[reg["opened"]:o].reshape(-1, 4) == opened).all(), "opened values differ"
    assert len(words) - o == len(fri) and (words[o:] == fri).all(), "FriProof words differ"
    assert (chal.state() == staged_chal.state()).all(), "final challenger state differs"
    # the parsed form
    assert isinstance(proof, ts.MultiBusProof)
    assert (proof.trace_commit == root_t).all() and (proof.aux_commit == root_a).all()
    assert (proof.quotient_commit == root_q).all() and (proof.exposed.reshape(-1, 4) == exposed).all()
    assert [(t.log_degree, t.width, t.qd, t.aux_width) for t in proof.tables] == \
        [(t.log_n, t.trace.shape[1], 1 << t.lqd, t.aux_width) for t in tables]
    k = 0
    for pt in proof.tables:
        assert (pt.aux_local == opened[k:k + pt.aux_width]).all()
        assert (pt.aux_next == opened[k + pt.aux_width:k + 2 * pt.aux_width]).all()
        k += 2 * pt.aux_width
    for pt in proof.tables:
        assert (pt.trace_local == opened[k:k + pt.width]).all()
        k += 2 * pt.width
    for pt in proof.tables:
        assert (pt.quotient_chunks.reshape(-1, 4) == opened[k:k + 4 * pt.qd]).all()
        k += 4 * pt.qd
    assert all(len(q.input_proof) == 3 for q in proof.query_proofs) and (proof.fri_words == fri).all()
    # balanced: everything sent is received
    got, bus_sum = bc.verify(cfg, tables, proof)
    assert (got.reshape(-1, 4) == exposed).all() and not bus_sum.any() and not proof.bus_sum.any()
    assert exposed.any(), "every table's own sum is zero: the case exercises no bus"


def test_golden_fixture_is_what_the_prover_writes(ctx):
    doc, tapes, pis, want = bc.load_golden()
    tables = bc.case("b")
    assert all((t.tape == tape).all() for t, tape in zip(tables, tapes))
    got = bc.prove(bc.config(ctx, 1), bc.compiled(ctx, tables), tables).words
    assert len(got) == len(want) and (got == want).all()


# ------------------------------------------------------------------ 2. degenerate form
def test_one_table_is_ts_prove_aux_behind_the_shape_words(ctx):
    (t,) = bc.case("t1")
    cfg = bc.config(ctx, 2)
    cair = bc.compiled(ctx, [t])[0]
    c4, c7 = ts.BfChallenger(), ts.BfChallenger()
    c4.observe(1)
    c4.observe(t.log_n)
    single = ts.prove(cfg, cair, c4, t.trace.copy(), t.pis, aux=t.logup.aux_source).words
    multi = bc.prove(cfg, [cair], [t], c7).words
    w, qd, aw = t.trace.shape[1], 1 << t.lqd, t.aux_width
    assert list(single[:8]) == [0x46505354, 4, t.log_n, w, qd, aw, 2, 4]
    assert list(multi[:8]) == [0x46505354, 7, 1, t.log_n, w, qd, aw, 4]
    assert len(multi) == len(single) and (multi[8:] == single[8:]).all()
    assert (c4.state() == c7.state()).all()


# ------------------------------------------------------------------ 3. the knobs
def _launches(ctx, cfg, cairs, tables):
    ctx.take_kernel_timings()
    ctx.set_kernel_timing(True)
    try:
        words = bc.prove(cfg, cairs, tables).words
        return words, {k: v[0] for k, v in ctx.take_kernel_timings().items()}
    finally:
        ctx.set_kernel_timing(False)


@pytest.mark.parametrize("name", ["b", "c"])
def test_class_path_and_generic_path_write_the_same_proof(ctx, monkeypatch, name):
    tables = bc.case(name)
    cfg = bc.config(ctx, 2)
    cairs = bc.compiled(ctx, tables)
    monkeypatch.delenv(OPEN_KNOB, raising=False)
    words, by_class = _launches(ctx, cfg, cairs, tables)
    monkeypatch.setenv(OPEN_KNOB, "1")
    generic, by_matrix = _launches(ctx, cfg, cairs, tables)
    assert len(words) == len(generic) and (words == generic).all()
    n_classes = len({t.log_n for t in tables})
    assert by_class.get("k_reduce_class", 0) == n_classes and by_class.get("k_bary_finish_jobs", 0) == 1
    assert "k_reduce_class" not in by_matrix
    n_mats = sum(1 for t in tables if t.aux_width) + len(tables) + sum(1 << t.lqd for t in tables)
    assert sum(v for k, v in by_matrix.items() if k.startswith("k_reduce<")) == n_mats


@pytest.mark.parametrize("name", ["b", "c", "e"])
def test_fused_builder_and_per_table_builder_write_the_same_proof(ctx, monkeypatch, name):
    tables = bc.case(name)
    cfg = bc.config(ctx, 1)
    cairs = bc.compiled(ctx, tables)
    n_aux = sum(1 for t in tables if t.aux_width)
    monkeypatch.delenv(LOGUP_KNOB, raising=False)
    words, fused = _launches(ctx, cfg, cairs, tables)
    monkeypatch.setenv(LOGUP_KNOB, "1")
    looped, per_table = _launches(ctx, cfg, cairs, tables)
    assert len(words) == len(looped) and (words == looped).all()
    # three launches for all tables against three per table
    assert [fused.get(k, 0) for k in ("k_logup_rows_jobs", "k_logup_totals_jobs", "k_logup_scan_jobs")] == [1, 1, 1]
    assert not any(k in fused for k in ("k_logup_rows", "k_logup_totals", "k_logup_scan"))
    assert [per_table.get(k, 0) for k in ("k_logup_rows", "k_logup_totals", "k_logup_scan")] == [n_aux] * 3
    assert not any(k.endswith("_jobs") and k.startswith("k_logup") for k in per_table)


@pytest.mark.parametrize("block_rows", [1, 3, 300])
@pytest.mark.parametrize("name", ["b", "c"])
def test_block_rows_do_not_change_the_proof(ctx, monkeypatch, name, block_rows):
    """Block rows 1 on the 2^8 range table of case c: 256 totals, two passes of the segmented totals scan, beside
    the 4096 totals of the 2^12 sender; 3: short last workgroups; 300: two rows per thread."""
    tables = bc.case(name)
    cfg = bc.config(ctx, 1)
    cairs = bc.compiled(ctx, tables)
    monkeypatch.delenv(BLOCK_KNOB, raising=False)
    want = bc.prove(cfg, cairs, tables).words
    monkeypatch.setenv(BLOCK_KNOB, str(block_rows))
    got = bc.prove(cfg, cairs, tables).words
    assert len(got) == len(want) and (got == want).all()


# ------------------------------------------------------------------ 4. ts_logup_aux_build_multi directly
def _challenges(seed):
    return (splitmix64_stream(seed, 8) % np.uint64(P)).astype(np.uint32)


def _build_and_compare(ctx, logups, traces, seed):
    ch = _challenges(seed)
    mats = [ts.DeviceMatrix.upload(ctx, t.copy()) for t in traces]
    auxs, S = logup_build_multi(logups, mats, ch)
    assert S.shape == (len(logups), 4)
    for k, (lu, t, m) in enumerate(zip(logups, traces, auxs)):
        want_aux, want_S = logup_reference(lu.interactions, t, ch[:4], ch[4:])
        got = m.download()
        assert got.shape == want_aux.shape == (t.shape[0], lu.aux_width)
        assert (got == want_aux).all(), f"table {k}: {int((got != want_aux).sum())} aux words differ"
        assert (S[k] == want_S).all(), f"table {k}: S differs"
    for m, t in zip(mats, traces):
        assert (m.download() == t).all()  # not consumed, not written


def test_builder_vs_python_integers_case_b(ctx):
    tables = [t for t in bc.case("b") if t.aux_width]
    assert [len(t.logup.interactions) for t in tables] == [1, 2, 5, 1]
    _build_and_compare(ctx, [t.logup for t in tables], [t.trace for t in tables], 300)


@pytest.mark.parametrize("block_rows", [1, 3])
def test_builder_vs_python_integers_small_blocks(ctx, monkeypatch, block_rows):
    """A 2^8 pair: at one row per workgroup each table has 256 totals (two passes of its own scan, and the second
    table's stretch starts where the first one's ends); at 3 both end on a short workgroup."""
    monkeypatch.setenv(BLOCK_KNOB, str(block_rows))
    s = bc.send(2, 8, 8, 61)
    r = bc.rng(8, [s])
    _build_and_compare(ctx, [s.logup, r.logup], [s.trace, r.trace], 310 + block_rows)


def test_builder_zero_denominator_names_the_table(ctx):
    """gamma = -v planted for the value of row 37 of the SECOND of three tables (as test_gpu_aux.py plants it): the
    report names that table, row and interaction, and nothing is handed out."""
    spec = LogUp([(("const", 1), [("col", 0)]), (("col", 3), [("col", 1)])])
    n = 128
    traces = []
    for k in range(3):
        t = (splitmix64_stream(70 + k, 4 * n) % np.uint64(P)).reshape(n, 4).astype(np.uint32)
        t[:, 0] = 1000 * (k + 1) + 3 * np.arange(n)  # distinct over all three tables
        traces.append(t)
    ch = _challenges(4)
    ch[:4] = (P - int(traces[1][37, 0]), 0, 0, 0)
    mats = [ts.DeviceMatrix.upload(ctx, t) for t in traces]
    with pytest.raises(_lib.TsError) as e:
        logup_build_multi([spec] * 3, mats, ch)
    assert e.value.code == TS_ERR_INVARIANT and "table 1, row 37, interaction 0" in str(e.value), str(e.value)
    out = (C.c_void_p * 3)(1, 1, 1)
    specs = [spec._spec_c() for _ in range(3)]
    ptrs = (C.POINTER(_lib.LogupSpecC) * 3)(*[C.pointer(s) for s, _ in specs])
    S = np.full(12, 0xABCD, dtype=np.uint32)
    rc = ctx._l.ts_logup_aux_build_multi(ctx.h, 3, ptrs, (C.c_void_p * 3)(*[m.h for m in mats]),
                                         ch.ctypes.data_as(_lib.u32p), out, S.ctypes.data_as(_lib.u32p))
    assert rc == TS_ERR_INVARIANT and list(out) == [None] * 3 and (S == 0xABCD).all()
    assert all(m.dims() == (n, 4) for m in mats)


def test_builder_refusals(ctx):
    spec = LogUp([(("const", 1), [("col", 0)])])
    m = ts.DeviceMatrix.upload(ctx, np.arange(16, dtype=np.uint32).reshape(8, 2))
    ch = _challenges(5)
    other = ts.DeviceMatrix.upload(ts.Context(0), np.zeros((8, 2), dtype=np.uint32))
    bad_challenge = ch.copy()
    bad_challenge[6] = P
    cases = {
        "a column outside the second trace": ([spec, LogUp([(("const", 1), [("col", 2)])])], [m, m], ch),
        "a kind-2 term": ([spec, LogUp([(("const", 1), [("prep", 0)])])], [m, m], ch),
        "a trace of another context": ([spec, spec], [m, other], ch),
        "a non-canonical challenge": ([spec], [m], bad_challenge),
        "65 tables": ([spec] * 65, [m] * 65, ch),
    }
    for what, (logups, mats, c) in cases.items():
        with pytest.raises(_lib.TsError) as e:
            logup_build_multi(logups, mats, c)
        assert e.value.code == TS_ERR_INVALID, what
    l = ctx._l
    assert l.ts_logup_aux_build_multi(None, 1, None, None, None, None, None) == TS_ERR_INVALID
    assert l.ts_logup_aux_build_multi(ctx.h, 0, None, None, None, None, None) == TS_ERR_INVALID
    assert (m.download() == np.arange(16, dtype=np.uint32).reshape(8, 2)).all()
    auxs, S = logup_build_multi([spec, spec], [m, m], ch)  # one trace may serve two tables: it is only read
    assert (auxs[0].download() == auxs[1].download()).all() and (S[0] == S[1]).all()


# ------------------------------------------------------------------ 5. unwritten memory
@pytest.fixture(scope="module")
def poison_contexts(ctx):
    return _poison.make_contexts()


@pytest.mark.parametrize("name", ["b", "c"])
def test_nothing_reads_unwritten_memory(poison_contexts, name):
    tables = bc.case(name)

    def run(c):
        return bc.prove(bc.config(c, 2), bc.compiled(c, tables), tables).words

    _poison.same_everywhere(poison_contexts, run, what=f"prove_multi_bus case {name}")


# ------------------------------------------------------------------ 6. balanced and unbalanced
def test_a_value_outside_the_table_verifies_and_does_not_balance(ctx):
    tables = bc.case("unbalanced")
    cfg = bc.config(ctx, 1)
    proof = bc.prove(cfg, bc.compiled(ctx, tables), tables)
    assert proof.bus_sum.any()
    with pytest.raises(ValueError, match="does not balance"):
        bc.verify(cfg, tables, proof)
    exposed, bus_sum = bc.verify(cfg, tables, proof, check_bus=False)
    assert bus_sum.any() and (bus_sum == proof.bus_sum).all() and (exposed == proof.exposed).all()
    # the balanced twin differs in that one row only
    good = bc.case("a")
    assert int((good[0].trace != tables[0].trace).any(axis=1).sum()) == 1
    assert not bc.prove(cfg, bc.compiled(ctx, good), good).bus_sum.any()


# ------------------------------------------------------------------ 7. rejections
def test_one_flipped_word_per_region_is_rejected(accepted_b):
    cfg, tables, hairs, words = accepted_b
    pis = [t.pis for t in tables]
    reg = bc.regions(tables)
    fri0 = reg["fri"][0]
    R = int(words[fri0])
    assert R == 6 and int(words[fri0 + 1 + 8 * R]) == bc.FRI_QUERIES
    n = len(words)
    tab = reg["tables"][0]
    # region -> (word index, the verdicts that region owns)
    flips = {
        "version": (1, {9}),
        "table count": (2, {1, 9}),
        "table width": (tab + 5 * 2 + 1, {1}),
        "table qd": (tab + 5 * 3 + 2, {1}),
        "table aux width": (tab + 5 * 0 + 3, {1}),
        "plain table's aux width": (tab + 5 * 1 + 3, {1}),
        "table n_exposed": (tab + 5 * 4 + 4, {1}),
        "table log_degree": (tab + 5 * 2, {7, 1, 9}),             # another transcript and another domain
        "trace root": (reg["trace_root"][0] + 3, {7, 4}),           # another gamma, beta, alpha and zeta
        "aux root": (reg["aux_root"][0] + 2, {7, 4}),               # another alpha and zeta
        "exposed word": (reg["exposed"][0] + 4 * 2 + 1, {7, 9}),    # another alpha, and another last-row constraint
        "quotient root": (reg["quotient_root"][0] + 5, {7, 4}),     # another zeta
        "aux value": (reg["aux_values"][3][0] + 9, {7, 9}),
        "trace value": (reg["trace_values"][4][0] + 1, {7, 9}),
        "plain table's trace value": (reg["trace_values"][1][0] + 2, {7, 9}),
        "chunk value": (reg["chunk_values"][2][0] + 6, {7, 9}),
        "FRI round root": (fri0 + 1 + 8 * 2, {3, 5, 8}),            # another transcript from that round on
        "final polynomial": (n - 5, {6, 9}),
        "PoW witness": (n - 1, {3, 4, 8}),
    }
    for what, (at, owned) in flips.items():
        bad = words.copy()
        bad[at] ^= 1
        v = _verdict(cfg, hairs, bad, pis)
        assert v != 0 and v in owned, f"{what}: verdict {v}"
    assert _verdict(cfg, hairs, words, pis) == 0


def test_swapped_exposed_words_are_rejected(accepted_b):
    """The exposed sums of two tables exchanged: the bus sum is the same, each table's last-row constraint is not."""
    cfg, tables, hairs, words = accepted_b
    pis = [t.pis for t in tables]
    e0 = bc.regions(tables)["exposed"][0]
    bad = words.copy()
    bad[e0:e0 + 4], bad[e0 + 4:e0 + 8] = words[e0 + 4:e0 + 8], words[e0:e0 + 4]
    assert not (bad == words).all()
    assert not ts.MultiBusProof(bad).bus_sum.any()
    assert _verdict(cfg, hairs, bad, pis) == 7


def test_other_verifiers_answer_a_v7_proof_with_9(ctx, accepted_b):
    cfg, tables, hairs, words = accepted_b
    l = _lib.lib()
    fri = cfg.pcs.fri._c()
    air, pis = hairs[1], tables[1].pis  # the plain Fibonacci table
    w = np.ascontiguousarray(words)
    wp, pp = w.ctypes.data_as(_lib.u32p), pis.ctypes.data_as(_lib.u32p)
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(cfg, air, ts.BfChallenger(), w, pis)
    assert e.value.code == 9
    with pytest.raises(ts.VerificationError) as e:
        ts.verify_multi(cfg, [air], ts.BfChallenger(), w, [pis])
    assert e.value.code == 9
    chals = [ts.BfChallenger() for _ in range(4)]  # kept alive across the calls
    v = C.c_int(-1)
    l.ts_verify_pre(C.byref(fri), air.h, chals[0].h, None, wp, len(w), pp, len(pis), C.byref(v))
    assert v.value == 9
    ex = np.zeros(4, dtype=np.uint32)
    v = C.c_int(-1)
    l.ts_verify_aux(C.byref(fri), hairs[0].h, chals[1].h, wp, len(w), None, 0, ex.ctypes.data_as(_lib.u32p), 4, C.byref(v))
    assert v.value == 9
    v = C.c_int(-1)
    l.ts_verify_pre_aux(C.byref(fri), hairs[0].h, chals[2].h, None, wp, len(w), None, 0, ex.ctypes.data_as(_lib.u32p), 4,
                        C.byref(v))
    assert v.value == 9
    v = C.c_int(-1)
    scripts, offsets = b"\0", (C.c_uint64 * 1)(0)  # an empty lock table
    rc = l.ts_verify_tap(C.byref(fri), air.h, chals[3].h, wp, len(w), pp, len(pis), scripts, offsets, 0, C.byref(v))
    assert rc == 0 and v.value == 9
    with pytest.raises(_lib.TsError) as e:
        ts.Proof(w).to_postcard()
    assert e.value.code == TS_ERR_UNSUPPORTED
    # and a v6 proof is no v7 proof
    plain = mc.case("b", 2)
    v6 = mc.prove(mc.config(ctx, 2), mc.compiled(ctx, plain), plain).words
    assert _verdict(cfg, hairs, v6, [t.pis for t in tables]) == 9


# ------------------------------------------------------------------ 8. refusals
def _call(ctx, cfg, entries, cap=1 << 17, chal=None, struct_size=None):
    """ts_prove_multi_bus on (CompiledAir, DeviceMatrix, pis, LogUp or None) entries: (status, text, words or the
    needed size)."""
    T = len(entries)
    tabs = (_lib.MultiBusTableC * max(T, 1))()
    keep = []
    for k, (a, m, p, lu) in enumerate(entries):
        p = np.asarray(p, dtype=np.uint32)
        keep.append(p)
        tabs[k].struct_size = C.sizeof(_lib.MultiBusTableC) if struct_size is None else struct_size
        tabs[k].n_public = len(p)
        tabs[k].air = a.h if a is not None else None
        tabs[k].trace = m.h if m is not None else None
        tabs[k].public_values = p.ctypes.data_as(_lib.u32p) if len(p) else None
        if lu is not None:
            keep.append(lu._spec_c())
            tabs[k].logup = C.pointer(keep[-1][0])
    out = np.zeros(max(cap, 1), dtype=np.uint32)
    n = C.c_size_t()
    fri = cfg.pcs.fri._c()
    chal = chal or ts.BfChallenger()
    rc = ctx._l.ts_prove_multi_bus(ctx.h, C.byref(fri), chal.h, tabs, T, out.ctypes.data_as(_lib.u32p), cap,
                                   C.byref(n))
    text = (ctx._l.ts_last_error(ctx.h) or b"").decode()
    return rc, text, (out[:n.value].copy() if rc == 0 else n.value)


def test_refusals_consume_nothing(ctx):
    cfg1, cfg2 = bc.config(ctx, 1), bc.config(ctx, 2)
    snd, rng_ = bc.case("a")
    fib = bc.fib(4)
    cs, cr, cf = (ts.CompiledAir(ctx, t.tape) for t in (snd, rng_, fib))
    high = mc.high(4)
    ch = ts.CompiledAir(ctx, high.tape)
    mats = {}

    def up(t, key):
        m = ts.DeviceMatrix.upload(ctx, t.trace.copy())
        mats[key] = (m, t.trace)
        return m

    s, r, f, h = up(snd, "send"), up(rng_, "range"), up(fib, "fib"), up(high, "high")
    other = ts.Context(0)
    s_other = ts.DeviceMatrix.upload(other, snd.trace.copy())
    cs_other = ts.CompiledAir(other, snd.tape)
    cs_host = ts.CompiledAir(None, snd.tape)
    sel = ts.CompiledAir(ctx, ts.air_tape(SelectorAir(), 2, 3))
    sel_trace, sel_pis = generate_selector_trace(generate_selector_preprocessed(8))
    sm = ts.DeviceMatrix.upload(ctx, sel_trace.copy())
    w3 = ts.DeviceMatrix.upload(ctx, np.zeros((32, 3), dtype=np.uint32))
    # a column-major matrix of the shape of a BusSendAir(2) trace: a quotient chunk (2^4 x 4, bit-reversed rows)
    snd2 = bc.send(2, 4, 5, 77)
    cs2 = ts.CompiledAir(ctx, snd2.tape)
    _, fib_alone = cfg2.pcs.commit([((fib.log_n, 1), fib.trace.copy())])
    (s_cols,) = cfg2.pcs.quotient_chunks(fib_alone, cf, fib.pis, np.array([3, 1, 4, 1], dtype=np.uint32))
    wide = BusSendAir(5).logup                                 # another aux width than the sender's AIR
    kind2 = LogUp([(("col", 1), [("const", 7), ("prep", 0)])])  # the right width, a preprocessed-column term
    outside = LogUp([(("col", 1), [("const", 7), ("col", 2)])])  # a column the trace does not have
    snd65 = [ts.DeviceMatrix.upload(ctx, snd.trace.copy()) for _ in range(65)]
    snd33 = snd65[:33]

    S, R, F = (cs, s, [], snd.logup), (cr, r, [], rng_.logup), (cf, f, fib.pis, None)
    cases = [
        ("no tables", cfg2, [], {}, TS_ERR_INVALID),
        ("65 tables", cfg2, [(cs, x, [], snd.logup) for x in snd65], {}, TS_ERR_INVALID),
        ("66 chunks", cfg2, [(cs, x, [], snd.logup) for x in snd33], {}, TS_ERR_INVALID),
        ("struct_size", cfg2, [S, R], {"struct_size": 32}, TS_ERR_INVALID),
        ("null air", cfg2, [S, (None, r, [], rng_.logup)], {}, TS_ERR_INVALID),
        ("null trace", cfg2, [S, (cr, None, [], rng_.logup)], {}, TS_ERR_INVALID),
        ("trace of another context", cfg2, [(cs, s_other, [], snd.logup), R], {}, TS_ERR_INVALID),
        ("air of another context", cfg2, [(cs_other, s, [], snd.logup), R], {}, TS_ERR_INVALID),
        ("host-only air", cfg2, [(cs_host, s, [], snd.logup), R], {}, TS_ERR_INVALID),
        ("width", cfg2, [(cs, w3, [], snd.logup), R], {}, TS_ERR_INVALID),
        ("n_public", cfg2, [S, R, (cf, f, fib.pis[:2], None)], {}, TS_ERR_INVALID),
        ("one handle twice", cfg2, [S, R, S], {}, TS_ERR_INVALID),
        ("no table with aux columns", cfg2, [F], {}, TS_ERR_INVALID),
        ("a spec is missing", cfg2, [(cs, s, [], None), R], {}, TS_ERR_INVALID),
        ("a spec where none is wanted", cfg2, [S, R, (cf, f, fib.pis, rng_.logup)], {}, TS_ERR_INVALID),
        ("a spec of another aux width", cfg2, [(cs, s, [], wide), R], {}, TS_ERR_INVALID),
        ("a spec that reads outside the trace", cfg2, [(cs, s, [], outside), R], {}, TS_ERR_INVALID),
        ("a kind-2 term", cfg2, [(cs, s, [], kind2), R], {}, TS_ERR_INVALID),
        ("a column-major trace under an aux table", cfg2, [(cs2, s_cols, [], snd2.logup), R], {}, TS_ERR_INVALID),
        ("preprocessed columns", cfg2, [S, R, (sel, sm, sel_pis, None)], {}, TS_ERR_UNSUPPORTED),
        ("lqd above the blowup", cfg1, [S, R, (ch, h, [], None)], {}, TS_ERR_INVARIANT),
    ]
    for what, cfg, entries, kw, want in cases:
        rc, text, _ = _call(ctx, cfg, entries, **kw)
        assert rc == want, f"{what}: status {rc} ({text})"
        assert text, f"{what}: no text"
        if what == "no table with aux columns":
            assert "ts_prove_multi" in text
    # every handle is still usable: download and compare, then prove with them
    for key, (mat, values) in mats.items():
        assert (mat.download() == values).all(), key
    assert (s_other.download() == snd.trace).all() and (sm.download() == sel_trace).all()
    assert s_cols.dims() == snd2.trace.shape
    assert all((x.download() == snd.trace).all() for x in snd65[::16])
    assert ctx._l.ts_prove_multi_bus(None, None, None, None, 0, None, 0, None) == TS_ERR_INVALID
    # ts_prove_multi keeps refusing aux AIRs
    with pytest.raises(_lib.TsError) as e:
        ts.prove_multi(cfg2, [cs, cr], ts.BfChallenger(), [s, r], [[], []])
    assert e.value.code == TS_ERR_UNSUPPORTED and (s.download() == snd.trace).all()
    rc, text, words = _call(ctx, cfg2, [S, R, F])
    assert rc == 0, text
    ts.verify_multi_bus(cfg2, [ts.CompiledAir(None, t.tape) for t in (snd, rng_, fib)], ts.BfChallenger(), words,
                        [[], [], fib.pis])


def test_short_buffer_reports_the_size(ctx):
    cfg = bc.config(ctx, 2)
    snd, rng_ = bc.case("a")
    cs, cr = ts.CompiledAir(ctx, snd.tape), ts.CompiledAir(ctx, rng_.tape)

    def entries():
        return [(cs, ts.DeviceMatrix.upload(ctx, snd.trace.copy()), [], snd.logup),
                (cr, ts.DeviceMatrix.upload(ctx, rng_.trace.copy()), [], rng_.logup)]

    rc, text, need = _call(ctx, cfg, entries(), cap=100)
    assert rc == TS_ERR_BUFFER and need > 100 and text
    rc, text, words = _call(ctx, cfg, entries(), cap=need)
    assert rc == 0 and len(words) == need
    assert need == ts.stark._multi_bus_capacity([(32, 2, 1, 8), (32, 2, 1, 8)], cfg.pcs.fri)
    bc.verify(cfg, [snd, rng_], words)


# ------------------------------------------------------------------ 9. nothing else moves
def test_other_proofs_are_unchanged_by_a_bus_proof(ctx, accepted_b):
    _, tables, _, words = accepted_b
    cfg = bc.config(ctx, 2)
    plain = mc.case("b", 2)
    (t1,) = bc.case("t1")
    c1 = bc.compiled(ctx, [t1])[0]

    def two():
        return [mc.prove(mc.config(ctx, 2), mc.compiled(ctx, plain), plain).words,
                ts.prove(cfg, c1, ts.BfChallenger(), t1.trace.copy(), t1.pis, aux=t1.logup.aux_source).words]

    before = two()
    mid = bc.prove(cfg, bc.compiled(ctx, tables), tables).words
    assert (mid == words).all()
    after = two()
    assert [int(w[1]) for w in before] == [6, 4]
    for b, a in zip(before, after):
        assert len(a) == len(b) and (a == b).all()


# ------------------------------------------------------------------ 10. the C++ example
def test_cpp_multi_bus_example(ctx, tmp_path):
    """examples/multi_bus.cpp: two sender tables and a range table of three heights in one proof; verified, the
    bus sum zero; then one sent value moved outside the table: verified again, the bus sum not zero."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "multi_bus")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "multi_bus.cpp"), "-L", libdir, "-ltapstark_hip",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TSPF v7" in r.stdout and "verify -> 0, bus sum zero" in r.stdout
    assert "value outside the table: verify -> 0, bus sum not zero" in r.stdout
