"""ts_prove_multi_key on the GPU: tables of mixed heights on a LogUp bus whose receiving tables are fixed columns of a
commit-once key, in one TSPF v8 proof; ts_logup_aux_build_multi_pre and ts_logup_multiplicities_bus_pre, the two
builders that read the key's values.

Exactness comes from composition, as in test_gpu_multi_bus.py: a key proof is, word for word, the Python staging of
tests/_key_cases.py -- ts_pcs_commit of the key list, the host challenger, the SINGLE-table ts_logup_aux_build_pre,
ts_quotient_chunks_pre_aux with key, aux and trace each committed ALONE, and ts_pcs_open over the three or four
rounds.  The CPU half is tests/test_multi_key_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.air import LogUp, logup_build_multi, logup_multiplicities_bus
from tapstark_amd.airs import (BUS_TAG, BusSendAir, fill_bus_key_multiplicities, generate_range_key, generate_xor_key,
                               splitmix64_stream)
import _bus_cases as bc
import _key_cases as kc
import _multi_cases as mc
import _poison
from _aux_airs import logup_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x78000001
TS_ERR_INVALID, TS_ERR_UNSUPPORTED, TS_ERR_INVARIANT, TS_ERR_BUFFER = 1, 4, 5, 6
OPEN_KNOB, LOGUP_KNOB, BLOCK_KNOB, HASH_KNOB = ("TS_MULTI_OPEN_GENERIC", "TS_MULTI_LOGUP_PER_TABLE", "TS_LOGUP_BLOCK_ROWS",
                                                "TS_LOGUP_HASH_BITS")


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(scope="module")
def accepted_kb(ctx):
    """One accepted proof of case kb at log_blowup 2: (config, tables, host-only AIRs, key root, words)."""
    tables = kc.case("kb")
    cfg = kc.config(ctx, 2)
    key = kc.make_key(cfg, tables)
    proof = kc.prove(cfg, key, kc.compiled(ctx, tables), tables)
    hairs = [ts.CompiledAir(None, t.tape) for t in tables]
    ts.verify_multi_key(cfg, key.root, hairs, ts.BfChallenger(), proof, [t.pis for t in tables])
    proof.words.setflags(write=False)
    return cfg, tables, hairs, key.root.copy(), proof.words


def _verdict(cfg, root, airs, words, pis):
    try:
        ts.verify_multi_key(cfg, root, airs, ts.BfChallenger(), words, pis, check_bus=False)
    except ts.VerificationError as e:
        return e.code
    return 0


def _shapes(tables):
    return [(*t.trace.shape, t.lqd, t.aux_width, t.prep_width) for t in tables]


# ------------------------------------------------------------------ 1. staged composition
@pytest.mark.parametrize("log_blowup", [1, 2])
@pytest.mark.parametrize("name", kc.CASE_NAMES + ("kt1",))
def test_key_proof_is_the_staged_composition(ctx, name, log_blowup):
    tables = kc.case(name)
    cfg = kc.config(ctx, log_blowup)
    cairs = kc.compiled(ctx, tables)
    key = kc.make_key(cfg, tables)
    staged_chal, chal = ts.BfChallenger(), ts.BfChallenger()
    root_k, root_t, root_a, exposed, root_q, opened, fri = kc.staged_proof(cfg.pcs, cairs, tables, staged_chal)
    assert (key.root == root_k).all(), "the key root is not ts_pcs_commit's of the same list"
    assert [key.info(i) for i in range(key.n)] == [m.shape for m in kc.key_matrices(tables)]
    proof = kc.prove(cfg, key, cairs, tables, chal)
    words, reg = proof.words, kc.regions(tables)
    A = sum(1 for t in tables if t.aux_width)
    assert list(words[:reg["tables"][1]]) == kc.header_words(tables)
    assert (words[slice(*reg["trace_root"])] == root_t).all(), "trace root differs"
    if A:
        assert (words[slice(*reg["aux_root"])] == root_a).all(), "aux root differs"
    assert (words[slice(*reg["exposed"])].reshape(-1, 4) == exposed).all(), "exposed words differ"
    assert (words[slice(*reg["quotient_root"])] == root_q).all(), "quotient root differs"
    o = reg["fri"][0]
    assert (words[reg["opened"]:o].reshape(-1, 4) == opened).all(), "opened values differ"
    assert len(words) - o == len(fri) and (words[o:] == fri).all(), "FriProof words differ"
    assert (chal.state() == staged_chal.state()).all(), "final challenger state differs"
    assert len(words) <= ts.stark._multi_key_capacity(_shapes(tables), cfg.pcs.fri)
    # the parsed form
    assert isinstance(proof, ts.MultiKeyProof)
    assert (proof.trace_commit == root_t).all() and (proof.quotient_commit == root_q).all()
    assert (proof.aux_commit == root_a).all() if A else proof.aux_commit is None
    assert (proof.exposed.reshape(-1, 4) == exposed).all()
    assert [(t.log_degree, t.width, t.qd, t.aux_width, t.preprocessed_width) for t in proof.tables] == \
        [(t.log_n, t.trace.shape[1], 1 << t.lqd, t.aux_width, t.prep_width) for t in tables]
    k = 0
    for pt in proof.tables:
        pw = pt.preprocessed_width
        assert (pt.preprocessed_local == opened[k:k + pw]).all() and (pt.preprocessed_next == opened[k + pw:k + 2 * pw]).all()
        k += 2 * pw
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
    assert all(len(q.input_proof) == (4 if A else 3) for q in proof.query_proofs) and (proof.fri_words == fri).all()
    # balanced: everything sent is received
    got, bus_sum = kc.verify(cfg, key.root, tables, proof)
    assert (got.reshape(-1, 4) == exposed).all() and not bus_sum.any() and not proof.bus_sum.any()
    if name not in ("k0", "kt1"):
        assert exposed.any(), "every table's own sum is zero: the case exercises no bus"
    # the key is not consumed: a second proof against it is the same proof
    again = kc.prove(cfg, key, cairs, tables).words
    assert len(again) == len(words) and (again == words).all()


def test_golden_fixture_is_what_the_prover_writes(ctx):
    doc, tapes, pis, want, root = kc.load_golden()
    tables = kc.case("kb")
    assert all((t.tape == tape).all() for t, tape in zip(tables, tapes))
    cfg = kc.config(ctx, 1)
    key = kc.make_key(cfg, tables)
    assert (key.root == root).all()
    got = kc.prove(cfg, key, kc.compiled(ctx, tables), tables).words
    assert len(got) == len(want) and (got == want).all()


# ------------------------------------------------------------------ 2. and 3. degenerate forms
def test_one_table_is_ts_prove_pre_aux_behind_the_shape_words(ctx):
    (t,) = kc.case("kt1")
    cfg = kc.config(ctx, 2)
    cair = kc.compiled(ctx, [t])[0]
    c5, c8 = ts.BfChallenger(), ts.BfChallenger()
    c5.observe(1)
    c5.observe(t.log_n)
    single_key = ts.PreprocessedKey(cfg, t.key.copy(), keep_values=True)
    single = ts.prove(cfg, cair, c5, t.trace.copy(), t.pis, preprocessed=single_key,
                      aux=t.logup.aux_source_with(single_key.values)).words
    key = kc.make_key(cfg, [t])
    assert (key.root == single_key.root).all()
    multi = kc.prove(cfg, key, [cair], [t], c8).words
    w, qd, aw = t.trace.shape[1], 1 << t.lqd, t.aux_width
    assert list(single[:9]) == [0x46505354, 5, t.log_n, w, qd, aw, 2, 4, 1]
    assert list(multi[:9]) == [0x46505354, 8, 1, t.log_n, w, qd, aw, 4, 1]
    assert len(multi) == len(single) and (multi[9:] == single[9:]).all()
    assert (c5.state() == c8.state()).all()


def test_without_aux_tables_the_challenge_phase_is_skipped(ctx):
    tables = kc.case("k0")
    cfg = kc.config(ctx, 1)
    key = kc.make_key(cfg, tables, keep_values=False)
    proof = kc.prove(cfg, key, kc.compiled(ctx, tables), tables)
    reg = kc.regions(tables)
    assert reg["aux_root"][0] == reg["aux_root"][1] == reg["exposed"][1] == reg["quotient_root"][0]
    assert proof.aux_commit is None and proof.exposed.size == 0
    assert all(len(q.input_proof) == 3 for q in proof.query_proofs)
    exposed, bus_sum = kc.verify(cfg, key.root, tables, proof)
    assert exposed.size == 0 and not bus_sum.any()
    with pytest.raises(_lib.TsError):
        key.values(0)


# ------------------------------------------------------------------ 4. the knobs
def _launches(ctx, cfg, key, cairs, tables):
    ctx.take_kernel_timings()
    ctx.set_kernel_timing(True)
    try:
        words = kc.prove(cfg, key, cairs, tables).words
        return words, {k: v[0] for k, v in ctx.take_kernel_timings().items()}
    finally:
        ctx.set_kernel_timing(False)


@pytest.mark.parametrize("name", ["kb", "kc", "ke"])
def test_class_path_and_generic_path_write_the_same_proof(ctx, monkeypatch, name):
    tables = kc.case(name)
    cfg = kc.config(ctx, 2)
    cairs = kc.compiled(ctx, tables)
    key = kc.make_key(cfg, tables)
    monkeypatch.delenv(OPEN_KNOB, raising=False)
    words, by_class = _launches(ctx, cfg, key, cairs, tables)
    monkeypatch.setenv(OPEN_KNOB, "1")
    generic, by_matrix = _launches(ctx, cfg, key, cairs, tables)
    assert len(words) == len(generic) and (words == generic).all()
    n_classes = len({t.log_n for t in tables})
    assert by_class.get("k_reduce_class", 0) == n_classes and by_class.get("k_bary_finish_jobs", 0) == 1
    assert "k_reduce_class" not in by_matrix
    n_mats = (sum(1 for t in tables if t.prep_width) + sum(1 for t in tables if t.aux_width) + len(tables) +
              sum(1 << t.lqd for t in tables))
    assert sum(v for k, v in by_matrix.items() if k.startswith("k_reduce<")) == n_mats


@pytest.mark.parametrize("name", ["kb", "kc", "ke"])
def test_fused_builder_and_per_table_builder_write_the_same_proof(ctx, monkeypatch, name):
    tables = kc.case(name)
    cfg = kc.config(ctx, 1)
    cairs = kc.compiled(ctx, tables)
    key = kc.make_key(cfg, tables)
    n_aux = sum(1 for t in tables if t.aux_width)
    n_aux_key = sum(1 for t in tables if t.aux_width and t.prep_width)
    monkeypatch.delenv(LOGUP_KNOB, raising=False)
    words, fused = _launches(ctx, cfg, key, cairs, tables)
    monkeypatch.setenv(LOGUP_KNOB, "1")
    looped, per_table = _launches(ctx, cfg, key, cairs, tables)
    assert len(words) == len(looped) and (words == looped).all()
    # three launches for all tables (the rows kernel in its instantiation with tables) against three per aux table
    assert [fused.get(k, 0) for k in ("k_logup_rows_jobs_pre", "k_logup_totals_jobs", "k_logup_scan_jobs")] == [1, 1, 1]
    assert not any(k in fused for k in ("k_logup_rows_jobs", "k_logup_rows", "k_logup_rows_pre", "k_logup_totals", "k_logup_scan"))
    assert per_table.get("k_logup_rows_pre", 0) == n_aux_key
    assert per_table.get("k_logup_rows", 0) == n_aux - n_aux_key
    assert [per_table.get(k, 0) for k in ("k_logup_totals", "k_logup_scan")] == [n_aux] * 2
    assert not any(k.endswith("_jobs") or k.endswith("_jobs_pre") for k in per_table if k.startswith("k_logup"))


@pytest.mark.parametrize("block_rows", [1, 3, 300])
@pytest.mark.parametrize("name", ["kb", "kc"])
def test_block_rows_do_not_change_the_proof(ctx, monkeypatch, name, block_rows):
    tables = kc.case(name)
    cfg = kc.config(ctx, 1)
    cairs = kc.compiled(ctx, tables)
    key = kc.make_key(cfg, tables)
    monkeypatch.delenv(BLOCK_KNOB, raising=False)
    want = kc.prove(cfg, key, cairs, tables).words
    monkeypatch.setenv(BLOCK_KNOB, str(block_rows))
    got = kc.prove(cfg, key, cairs, tables).words
    assert len(got) == len(want) and (got == want).all()


# ------------------------------------------------------------------ 5. ts_logup_aux_build_multi_pre directly
def _challenges(seed):
    return (splitmix64_stream(seed, 8) % np.uint64(P)).astype(np.uint32)


def _reference(logup, trace, table, ch):
    """tests/_aux_airs.logup_reference with table rows: a kind-2 term over `table` is a kind-1 term over the row
    (trace row ++ table row)."""
    w = trace.shape[1]
    move = lambda t: (1, w + t[1]) if t[0] == 2 else t
    its = [(move(m), [move(v) for v in vals]) for m, vals in logup.interactions]
    rows = trace if table is None else np.hstack([trace, table])
    return logup_reference(its, rows, ch[:4], ch[4:])


def _build_and_compare(ctx, tables, seed):
    ch = _challenges(seed)
    mats = [ts.DeviceMatrix.upload(ctx, t.trace.copy()) for t in tables]
    pre = [ts.DeviceMatrix.upload(ctx, t.key.copy()) if t.key is not None else None for t in tables]
    auxs, S = logup_build_multi([t.logup for t in tables], mats, ch, preprocessed=pre)
    assert S.shape == (len(tables), 4)
    for k, (t, m) in enumerate(zip(tables, auxs)):
        want_aux, want_S = _reference(t.logup, t.trace, t.key, ch)
        got = m.download()
        assert got.shape == want_aux.shape == (t.trace.shape[0], t.aux_width)
        assert (got == want_aux).all(), f"table {k}: {int((got != want_aux).sum())} aux words differ"
        assert (S[k] == want_S).all(), f"table {k}: S differs"
        # and the single call, word for word
        one, one_S = t.logup.build(mats[k], ch, preprocessed=pre[k])
        assert (one.download() == got).all() and (one_S == S[k]).all()
    for m, t in zip(mats, tables):
        assert (m.download() == t.trace).all()  # not consumed, not written
    for m, t in zip(pre, tables):
        assert m is None or (m.download() == t.key).all()


def test_builder_vs_python_integers_case_kb(ctx):
    """Jobs without a table (the senders) beside jobs with one (the two key tables)."""
    tables = [t for t in kc.case("kb") if t.aux_width]
    assert [t.key is not None for t in tables] == [True, False, False, True, False]
    _build_and_compare(ctx, tables, 400)


@pytest.mark.parametrize("block_rows", [1, 3])
def test_builder_vs_python_integers_small_blocks(ctx, monkeypatch, block_rows):
    monkeypatch.setenv(BLOCK_KNOB, str(block_rows))
    x = kc.xsend(2, 8, 4, 61)
    _build_and_compare(ctx, [x, kc.xor_key(4, [x])], 410 + block_rows)


def test_builder_zero_denominator_names_the_table(ctx):
    """The tuple is the one table value (prep 0), so d = gamma + v: gamma = -v planted for the TABLE value of row 37 of
    the SECOND of three tables.  The report names that table, row and interaction."""
    spec = LogUp([(("col", 0), [("prep", 0)])])
    n = 128
    traces = [np.ones((n, 1), dtype=np.uint32) for _ in range(3)]
    pres = [(1000 * (k + 1) + 3 * np.arange(n, dtype=np.uint32)).reshape(n, 1) for k in range(3)]
    ch = _challenges(4)
    ch[:4] = (P - int(pres[1][37, 0]), 0, 0, 0)
    mats = [ts.DeviceMatrix.upload(ctx, t) for t in traces]
    pm = [ts.DeviceMatrix.upload(ctx, t) for t in pres]
    with pytest.raises(_lib.TsError) as e:
        logup_build_multi([spec] * 3, mats, ch, preprocessed=pm)
    assert e.value.code == TS_ERR_INVARIANT and "table 1, row 37, interaction 0" in str(e.value), str(e.value)
    assert all(m.dims() == (n, 1) for m in mats + pm)


def test_builder_refusals_allocate_nothing(ctx):
    spec = LogUp([(("const", 1), [("col", 0)])])
    prep = LogUp([(("col", 1), [("prep", 0)])])
    m = ts.DeviceMatrix.upload(ctx, np.arange(16, dtype=np.uint32).reshape(8, 2))
    t1 = ts.DeviceMatrix.upload(ctx, np.arange(8, dtype=np.uint32).reshape(8, 1))
    short = ts.DeviceMatrix.upload(ctx, np.arange(4, dtype=np.uint32).reshape(4, 1))
    ch = _challenges(5)
    other = ts.DeviceMatrix.upload(ts.Context(0), np.zeros((8, 1), dtype=np.uint32))
    cases = {
        "a kind-2 term without a table": ([spec, prep], [m, m], [None, None]),
        "a kind-2 column outside the table": ([spec, LogUp([(("col", 1), [("prep", 1)])])], [m, m], [None, t1]),
        "a table of another height": ([prep], [m], [short]),
        "a table of another context": ([prep], [m], [other]),
        "65 tables": ([spec] * 65, [m] * 65, [None] * 65),
    }
    ctx.synchronize()
    before = ctx.stat(3)  # the pool's bytes: a refused call takes no block
    for what, (logups, mats, pre) in cases.items():
        with pytest.raises(_lib.TsError) as e:
            logup_build_multi(logups, mats, ch, preprocessed=pre)
        assert e.value.code == TS_ERR_INVALID, what
    assert ctx.stat(3) == before
    l = ctx._l
    assert l.ts_logup_aux_build_multi_pre(None, 1, None, None, None, None, None, None) == TS_ERR_INVALID
    assert l.ts_logup_aux_build_multi_pre(ctx.h, 1, None, None, None, None, None, None) == TS_ERR_INVALID
    assert (m.download() == np.arange(16, dtype=np.uint32).reshape(8, 2)).all()
    # a table serves a job, and a job without one keeps working beside it
    auxs, S = logup_build_multi([spec, prep], [m, m], ch, preprocessed=[None, t1])
    want, want_S = spec.build(m, ch)
    assert (auxs[0].download() == want.download()).all() and (S[0] == want_S).all()
    # ts_logup_aux_build_multi keeps refusing kind-2 terms
    with pytest.raises(_lib.TsError) as e:
        logup_build_multi([prep], [m], ch)
    assert e.value.code == TS_ERR_INVALID


# ------------------------------------------------------------------ 6. ts_logup_multiplicities_bus_pre
def _count(key, tuples, negate):
    """numpy: per class of equal key rows, on its lowest row, the number of `tuples` equal to it."""
    first, counts = {}, np.zeros(len(key), dtype=np.int64)
    for r, row in enumerate(key.tolist()):
        first.setdefault(tuple(row), r)
    for tup in tuples.tolist():
        counts[first[tuple(tup)]] += 1
    return ((P - counts) % P if negate else counts % P).astype(np.uint32)


@pytest.mark.parametrize("hash_bits", [None, 0, 3])
@pytest.mark.parametrize("negate", [0, 1])
def test_fill_vs_numpy_count(ctx, monkeypatch, negate, hash_bits):
    if hash_bits is None:
        monkeypatch.delenv(HASH_KNOB, raising=False)
    else:
        monkeypatch.setenv(HASH_KNOB, str(hash_bits))
    # a range key with duplicate entries (rows 8 .. 15 repeat 0 .. 7), senders of two heights and two k
    rkey = np.concatenate([generate_range_key(8), generate_range_key(8)])
    s2, s5 = kc.send(2, 6, 3, 21), kc.send(5, 3, 3, 22)
    table = ts.DeviceMatrix.upload(ctx, np.full((16, 1), 0xDEAD, dtype=np.uint32))
    pre = ts.DeviceMatrix.upload(ctx, rkey)
    lookers = []
    for s in (s2, s5):
        k = s.trace.shape[1] // 2
        lookers.append((ts.DeviceMatrix.upload(ctx, s.trace.copy()), [[("col", 2 * i)] for i in range(k)],
                        [("col", 2 * i + 1) for i in range(k)]))
    n_missing, first = logup_multiplicities_bus(table, [("prep", 0)], lookers, out_column=0, negate=negate,
                                                table_preprocessed=pre)
    sent = np.concatenate([kc.selected_tuples(s.trace, 1) for s in (s2, s5)])
    assert n_missing == 0 and first is None
    want = _count(rkey, sent, negate)
    assert (table.download()[:, 0] == want).all() and not want[8:].any() and want[:8].any()
    assert (pre.download() == rkey).all()
    # the xor key: tuples of three values from two matrices' worth of columns
    xkey = generate_xor_key(2)
    x = kc.xsend(2, 5, 2, 33)
    xt = ts.DeviceMatrix.upload(ctx, np.zeros((16, 1), dtype=np.uint32))
    xp = ts.DeviceMatrix.upload(ctx, xkey)
    xs = ts.DeviceMatrix.upload(ctx, x.trace.copy())
    if negate:
        assert fill_bus_key_multiplicities(xt, xp, [xs], n_values=3) == (0, None)
        assert (xt.download() == kc.xor_key(2, [x]).trace).all()
    else:
        lk = [(xs, [[("col", 4 * i + j) for j in range(3)] for i in range(2)], [("col", 4 * i + 3) for i in range(2)])]
        logup_multiplicities_bus(xt, [("prep", j) for j in range(3)], lk, out_column=0, negate=0, table_preprocessed=xp)
        assert (xt.download()[:, 0] == _count(xkey, kc.selected_tuples(x.trace, 3), 0)).all()


def test_fill_reports_a_miss_and_equals_the_plain_call_without_kind_2(ctx):
    bad = kc.case("unbalanced")[0]
    rkey = generate_range_key(32)
    table = ts.DeviceMatrix.upload(ctx, np.zeros((32, 1), dtype=np.uint32))
    pre = ts.DeviceMatrix.upload(ctx, rkey)
    s = ts.DeviceMatrix.upload(ctx, bad.trace.copy())
    n_missing, first = fill_bus_key_multiplicities(table, pre, [s], allow_missing=True)
    assert n_missing == 1 and first == (0, 3, 0)
    with pytest.raises(_lib.TsError) as e:
        fill_bus_key_multiplicities(table, pre, [s])
    assert e.value.code == TS_ERR_INVARIANT and "looker 0, row 3, lookup 0" in str(e.value)
    # no kind-2 term, no matrix: the column of ts_logup_multiplicities_bus
    good, rng_ = bc.case("a")
    a = ts.DeviceMatrix.upload(ctx, rng_.trace.copy())
    b = ts.DeviceMatrix.upload(ctx, rng_.trace.copy())
    g = ts.DeviceMatrix.upload(ctx, good.trace.copy())
    lk = [(g, [[("col", 0)]], [("col", 1)])]
    r1 = logup_multiplicities_bus(a, [("col", 0)], lk, out_column=1)
    r2 = logup_multiplicities_bus(b, [("col", 0)], lk, out_column=1, pre=True)
    assert r1 == r2 and (a.download() == b.download()).all() and (a.download() == rng_.trace).all()
    # refusals: a kind-2 term in the plain call, on a looker, without a matrix, outside it, a matrix of another height
    for what, call in {
        "plain call": lambda: logup_multiplicities_bus(table, [("prep", 0)], [(s, [[("col", 0)]], [("col", 1)])], 0),
        "looker term": lambda: logup_multiplicities_bus(table, [("prep", 0)], [(s, [[("prep", 0)]], [("col", 1)])], 0,
                                                        table_preprocessed=pre),
        "no matrix": lambda: logup_multiplicities_bus(table, [("prep", 0)], [(s, [[("col", 0)]], [("col", 1)])], 0, pre=True),
        "outside": lambda: logup_multiplicities_bus(table, [("prep", 1)], [(s, [[("col", 0)]], [("col", 1)])], 0,
                                                    table_preprocessed=pre),
        "height": lambda: logup_multiplicities_bus(a, [("prep", 0)], [(s, [[("col", 0)]], [("col", 1)])], 1,
                                                   table_preprocessed=ts.DeviceMatrix.upload(ctx, generate_range_key(16))),
    }.items():
        with pytest.raises(_lib.TsError) as e:
            call()
        assert e.value.code == TS_ERR_INVALID, what


# ------------------------------------------------------------------ 7. unwritten memory
@pytest.fixture(scope="module")
def poison_contexts(ctx):
    return _poison.make_contexts()


@pytest.mark.parametrize("name", ["kb", "kc"])
def test_nothing_reads_unwritten_memory(poison_contexts, name):
    tables = kc.case(name)
    aux_tables = [t for t in tables if t.aux_width]
    recv = next(t for t in tables if t.aux_width and t.prep_width == 1)
    senders = [t for t in tables if isinstance(t.air, BusSendAir)]

    def run(c):
        cfg = kc.config(c, 2)
        key = kc.make_key(cfg, tables)
        out = [kc.prove(cfg, key, kc.compiled(c, tables), tables).words]
        # both builders against the key's own values
        ki = {id(t): i for i, t in enumerate(t for t in tables if t.key is not None)}
        pre = [key.values(ki[id(t)]) if t.key is not None else None for t in aux_tables]
        auxs, S = logup_build_multi([t.logup for t in aux_tables], [ts.DeviceMatrix.upload(c, t.trace.copy()) for t in aux_tables],
                                    _challenges(9), preprocessed=pre)
        out += [m.download().reshape(-1) for m in auxs] + [S.reshape(-1)]
        col = ts.DeviceMatrix.upload(c, np.zeros_like(recv.trace))
        fill_bus_key_multiplicities(col, key.values(ki[id(recv)]), [ts.DeviceMatrix.upload(c, s.trace.copy()) for s in senders])
        out.append(col.download().reshape(-1))
        assert (out[-1] == recv.trace.reshape(-1)).all()
        return np.concatenate(out)

    _poison.same_everywhere(poison_contexts, run, what=f"prove_multi_key case {name}")


# ------------------------------------------------------------------ 8. soundness at the boundary
def test_a_changed_table_entry_is_another_key_and_rejects(ctx, accepted_kb):
    cfg, tables, hairs, root, words = accepted_kb
    pis = [t.pis for t in tables]
    mats = [m.copy() for m in kc.key_matrices(tables)]
    mats[2][5, 2] ^= 1  # one entry of the xor table: (a, b, a xor b) with the wrong xor
    other = ts.MultiKey(cfg, mats)
    assert not (other.root == root).all()
    v = _verdict(cfg, other.root, hairs, words, pis)
    assert v != 0 and v in {7, 4}, v
    assert _verdict(cfg, root, hairs, words, pis) == 0


def test_one_flipped_word_per_region_is_rejected(accepted_kb):
    cfg, tables, hairs, root, words = accepted_kb
    pis = [t.pis for t in tables]
    reg = kc.regions(tables)
    fri0 = reg["fri"][0]
    R = int(words[fri0])
    assert R == 6 and int(words[fri0 + 1 + 8 * R]) == kc.FRI_QUERIES
    q0 = fri0 + 1 + 8 * R + 1  # query 0: [4 batches][key round: n_mats, (len, values) ...]
    assert list(words[q0:q0 + 3]) == [4, 3, 1]
    n = len(words)
    tab = reg["tables"][0]
    # region -> (word index, the verdicts that region owns)
    flips = {
        "version": (1, {9}),
        "table count": (2, {1, 9}),
        "table width": (tab + 6 * 3 + 1, {1}),
        "table qd": (tab + 6 * 2 + 2, {1}),
        "table aux width": (tab + 6 * 0 + 3, {1}),
        "plain table's aux width": (tab + 6 * 1 + 3, {1}),
        "table n_exposed": (tab + 6 * 4 + 4, {1}),
        "table preprocessed width": (tab + 6 * 5 + 5, {1}),
        "plain table's preprocessed width": (tab + 6 * 1 + 5, {1}),
        "table log_degree": (tab + 6 * 3, {7, 1, 9}),               # another transcript and another domain
        "trace root": (reg["trace_root"][0] + 3, {7, 4}),           # another gamma, beta, alpha and zeta
        "aux root": (reg["aux_root"][0] + 2, {7, 4}),               # another alpha and zeta
        "exposed word": (reg["exposed"][0] + 4 * 2 + 1, {7, 9}),    # another alpha, and another last-row constraint
        "quotient root": (reg["quotient_root"][0] + 5, {7, 4}),     # another zeta
        "preprocessed value": (reg["key_values"][5][0] + 9, {7, 9}),
        "key-only table's preprocessed value": (reg["key_values"][2][0] + 1, {7, 9}),
        "aux value": (reg["aux_values"][4][0] + 9, {7, 9}),
        "trace value": (reg["trace_values"][6][0] + 1, {7, 9}),
        "plain table's trace value": (reg["trace_values"][1][0] + 2, {7, 9}),
        "chunk value": (reg["chunk_values"][2][0] + 6, {7, 9}),
        "key-round opening": (q0 + 3, {4, 9}),                      # the row no longer hashes to the key root
        "FRI round root": (fri0 + 1 + 8 * 2, {3, 5, 8}),            # another transcript from that round on
        "final polynomial": (n - 5, {6, 9}),
        "PoW witness": (n - 1, {3, 4, 8}),
    }
    for what, (at, owned) in flips.items():
        bad = words.copy()
        bad[at] ^= 1
        v = _verdict(cfg, root, hairs, bad, pis)
        assert v != 0 and v in owned, f"{what}: verdict {v}"
    bad_root = root.copy()
    bad_root[4] ^= 1
    assert _verdict(cfg, bad_root, hairs, words, pis) in {7, 4}
    assert _verdict(cfg, root, hairs, words, pis) == 0


def test_a_value_outside_the_table_verifies_and_does_not_balance(ctx):
    tables = kc.case("unbalanced")
    cfg = kc.config(ctx, 1)
    key = kc.make_key(cfg, tables)
    proof = kc.prove(cfg, key, kc.compiled(ctx, tables), tables)
    assert proof.bus_sum.any()
    with pytest.raises(ValueError, match="does not balance"):
        kc.verify(cfg, key.root, tables, proof)
    exposed, bus_sum = kc.verify(cfg, key.root, tables, proof, check_bus=False)
    assert bus_sum.any() and (bus_sum == proof.bus_sum).all() and (exposed == proof.exposed).all()
    good = kc.case("ka")
    assert int((good[0].trace != tables[0].trace).any(axis=1).sum()) == 1
    assert not kc.prove(cfg, key, kc.compiled(ctx, good), good).bus_sum.any()


# ------------------------------------------------------------------ 9. other calls
def test_other_verifiers_answer_a_v8_proof_with_9(ctx, accepted_kb):
    cfg, tables, hairs, root, words = accepted_kb
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
    with pytest.raises(ts.VerificationError) as e:
        ts.verify_multi_bus(cfg, [hairs[3], air], ts.BfChallenger(), w, [[], pis])
    assert e.value.code == 9
    chals = [ts.BfChallenger() for _ in range(4)]  # kept alive across the calls
    v = C.c_int(-1)
    l.ts_verify_pre(C.byref(fri), air.h, chals[0].h, None, wp, len(w), pp, len(pis), C.byref(v))
    assert v.value == 9
    ex = np.zeros(4, dtype=np.uint32)
    v = C.c_int(-1)
    l.ts_verify_aux(C.byref(fri), hairs[3].h, chals[1].h, wp, len(w), None, 0, ex.ctypes.data_as(_lib.u32p), 4, C.byref(v))
    assert v.value == 9
    v = C.c_int(-1)
    l.ts_verify_pre_aux(C.byref(fri), hairs[3].h, chals[2].h, None, wp, len(w), None, 0, ex.ctypes.data_as(_lib.u32p), 4,
                        C.byref(v))
    assert v.value == 9
    v = C.c_int(-1)
    scripts, offsets = b"\0", (C.c_uint64 * 1)(0)  # an empty lock table
    rc = l.ts_verify_tap(C.byref(fri), air.h, chals[3].h, wp, len(w), pp, len(pis), scripts, offsets, 0, C.byref(v))
    assert rc == 0 and v.value == 9
    with pytest.raises(_lib.TsError) as e:
        ts.Proof(w).to_postcard()
    assert e.value.code == TS_ERR_UNSUPPORTED
    # and v6 and v7 proofs are no v8 proofs
    plain = mc.case("b", 2)
    v6 = mc.prove(mc.config(ctx, 2), mc.compiled(ctx, plain), plain).words
    bus = bc.case("b")
    v7 = bc.prove(bc.config(ctx, 2), bc.compiled(ctx, bus), bus).words
    for other in (v6, v7):
        assert _verdict(cfg, root, hairs, other, [t.pis for t in tables]) == 9


def test_other_proofs_are_unchanged_by_a_key_proof(ctx, accepted_kb):
    _, tables, _, _, words = accepted_kb
    cfg = kc.config(ctx, 2)
    plain, bus = mc.case("b", 2), bc.case("b")
    (t1,) = kc.case("kt1")
    c1 = kc.compiled(ctx, [t1])[0]
    k1 = ts.PreprocessedKey(cfg, t1.key.copy(), keep_values=True)

    def three():
        return [mc.prove(mc.config(ctx, 2), mc.compiled(ctx, plain), plain).words,
                bc.prove(bc.config(ctx, 2), bc.compiled(ctx, bus), bus).words,
                ts.prove(cfg, c1, ts.BfChallenger(), t1.trace.copy(), t1.pis, preprocessed=k1,
                         aux=t1.logup.aux_source_with(k1.values)).words]

    before = three()
    key = kc.make_key(cfg, tables)
    mid = kc.prove(cfg, key, kc.compiled(ctx, tables), tables).words
    assert (mid == words).all()
    after = three()
    assert [int(w[1]) for w in before] == [6, 7, 5]
    for b, a in zip(before, after):
        assert len(a) == len(b) and (a == b).all()


# ------------------------------------------------------------------ 10. refusals
def _call(ctx, cfg, key, entries, cap=1 << 17, struct_size=None):
    """ts_prove_multi_key on (CompiledAir, DeviceMatrix, pis, LogUp or None) entries: (status, text, words or the
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
    chal = ts.BfChallenger()
    rc = ctx._l.ts_prove_multi_key(ctx.h, C.byref(fri), chal.h, key.h if key is not None else None, tabs, T,
                                   out.ctypes.data_as(_lib.u32p), cap, C.byref(n))
    text = (ctx._l.ts_last_error(ctx.h) or b"").decode()
    return rc, text, (out[:n.value].copy() if rc == 0 else n.value)


def test_refusals_consume_nothing(ctx):
    cfg1, cfg2 = kc.config(ctx, 1), kc.config(ctx, 2)
    snd, tab = kc.case("ka")
    fib = kc.fib(4)
    cs, ct, cf = (ts.CompiledAir(ctx, t.tape) for t in (snd, tab, fib))
    high = mc.high(4)
    ch = ts.CompiledAir(ctx, high.tape)
    mats = {}

    def up(t, name):
        m = ts.DeviceMatrix.upload(ctx, t.trace.copy())
        mats[name] = (m, t.trace)
        return m

    s, r, f, h = up(snd, "send"), up(tab, "table"), up(fib, "fib"), up(high, "high")
    key = ts.MultiKey(cfg2, [tab.key.copy()])
    key_b1 = ts.MultiKey(cfg1, [tab.key.copy()])
    key_novals = ts.MultiKey(cfg2, [tab.key.copy()], keep_values=False)
    key_two = ts.MultiKey(cfg2, [tab.key.copy(), tab.key.copy()])
    key_short = ts.MultiKey(cfg2, [tab.key[:16].copy()])
    key_wide = ts.MultiKey(cfg2, [np.hstack([tab.key, tab.key])])
    other = ts.Context(0)
    key_other = ts.MultiKey(kc.config(other, 2), [tab.key.copy()])
    s_other = ts.DeviceMatrix.upload(other, snd.trace.copy())
    kind2_no_prep = LogUp([(("col", 1), [("const", BUS_TAG), ("prep", 0)])])    # on the sender: no preprocessed columns
    kind2_outside = LogUp([(("col", 0), [("const", BUS_TAG), ("prep", 1)])])    # on the table: the key matrix has one column
    outside = LogUp([(("col", 0), [("const", BUS_TAG), ("col", 1)])])
    snd65 = [ts.DeviceMatrix.upload(ctx, snd.trace.copy()) for _ in range(65)]

    S, R, F = (cs, s, [], snd.logup), (ct, r, [], tab.logup), (cf, f, fib.pis, None)
    cases = [
        ("no tables", cfg2, key, [], {}, TS_ERR_INVALID),
        ("65 tables", cfg2, key, [(cs, x, [], snd.logup) for x in snd65], {}, TS_ERR_INVALID),
        ("66 chunks", cfg2, key, [R] + [(cs, x, [], snd.logup) for x in snd65[:33]], {}, TS_ERR_INVALID),
        ("struct_size", cfg2, key, [S, R], {"struct_size": 32}, TS_ERR_INVALID),
        ("null air", cfg2, key, [S, (None, r, [], tab.logup)], {}, TS_ERR_INVALID),
        ("null trace", cfg2, key, [S, (ct, None, [], tab.logup)], {}, TS_ERR_INVALID),
        ("trace of another context", cfg2, key, [(cs, s_other, [], snd.logup), R], {}, TS_ERR_INVALID),
        ("one handle twice", cfg2, key, [S, R, S], {}, TS_ERR_INVALID),
        ("n_public", cfg2, key, [S, R, (cf, f, fib.pis[:2], None)], {}, TS_ERR_INVALID),
        ("a spec is missing", cfg2, key, [S, (ct, r, [], None)], {}, TS_ERR_INVALID),
        ("a spec where none is wanted", cfg2, key, [S, R, (cf, f, fib.pis, snd.logup)], {}, TS_ERR_INVALID),
        ("a spec that reads outside the trace", cfg2, key, [S, (ct, r, [], outside)], {}, TS_ERR_INVALID),
        ("null key", cfg2, None, [S, R], {}, TS_ERR_INVALID),
        ("no table uses the key", cfg2, key, [S, F], {}, TS_ERR_INVALID),
        ("the key holds two matrices", cfg2, key_two, [S, R], {}, TS_ERR_INVALID),
        ("a key matrix of another height", cfg2, key_short, [S, R], {}, TS_ERR_INVALID),
        ("a key matrix of another width", cfg2, key_wide, [S, R], {}, TS_ERR_INVALID),
        ("a key of another context", cfg2, key_other, [S, R], {}, TS_ERR_INVALID),
        ("a key of another blowup", cfg2, key_b1, [S, R], {}, TS_ERR_INVALID),
        ("a kind-2 term on a table without preprocessed columns", cfg2, key, [(cs, s, [], kind2_no_prep), R], {}, TS_ERR_INVALID),
        ("a kind-2 column outside its matrix", cfg2, key, [S, (ct, r, [], kind2_outside)], {}, TS_ERR_INVALID),
        ("kind-2 terms against a key without kept values", cfg2, key_novals, [S, R], {}, TS_ERR_INVALID),
        ("lqd above the blowup", cfg1, key_b1, [S, R, (ch, h, [], None)], {}, TS_ERR_INVARIANT),
    ]
    for what, cfg, k, entries, kw, want in cases:
        rc, text, _ = _call(ctx, cfg, k, entries, **kw)
        assert rc == want, f"{what}: status {rc} ({text})"
        assert text, f"{what}: no text"
        if what in ("null key", "no table uses the key"):
            assert "ts_prove_multi_bus" in text
    # every handle is still usable: download and compare, then prove with them
    for name, (mat, values) in mats.items():
        assert (mat.download() == values).all(), name
    assert (s_other.download() == snd.trace).all()
    assert all((x.download() == snd.trace).all() for x in snd65[::16])
    assert (key.values(0).download() == tab.key).all()
    assert ctx._l.ts_prove_multi_key(None, None, None, None, None, 0, None, 0, None) == TS_ERR_INVALID
    # the calls without a key keep refusing preprocessed columns and kind-2 terms
    with pytest.raises(_lib.TsError) as e:
        ts.prove_multi_bus(cfg2, [cs, ct], ts.BfChallenger(), [s, r], [[], []], [snd.logup, tab.logup])
    assert e.value.code == TS_ERR_UNSUPPORTED and "no key round" in str(e.value) and (s.download() == snd.trace).all()
    with pytest.raises(_lib.TsError) as e:
        ts.prove_multi(cfg2, [cs, ct], ts.BfChallenger(), [s, r], [[], []])
    assert e.value.code == TS_ERR_UNSUPPORTED
    rc, text, words = _call(ctx, cfg2, key, [S, R, F])
    assert rc == 0, text
    kc.verify(cfg2, key.root, [snd, tab, fib], words)


def test_short_buffer_reports_the_size(ctx):
    cfg = kc.config(ctx, 2)
    snd, tab = kc.case("ka")
    cs, ct = ts.CompiledAir(ctx, snd.tape), ts.CompiledAir(ctx, tab.tape)
    key = kc.make_key(cfg, [snd, tab])

    def entries():
        return [(cs, ts.DeviceMatrix.upload(ctx, snd.trace.copy()), [], snd.logup),
                (ct, ts.DeviceMatrix.upload(ctx, tab.trace.copy()), [], tab.logup)]

    rc, text, need = _call(ctx, cfg, key, entries(), cap=100)
    assert rc == TS_ERR_BUFFER and need > 100 and text
    rc, text, words = _call(ctx, cfg, key, entries(), cap=need)
    assert rc == 0 and len(words) == need
    assert need == ts.stark._multi_key_capacity(_shapes([snd, tab]), cfg.pcs.fri)
    kc.verify(cfg, key.root, [snd, tab], words)


# ------------------------------------------------------------------ 11. the C++ example
def test_cpp_multi_key_example(ctx, tmp_path):
    """examples/multi_key.cpp: a 4-bit x 4-bit xor table in a key committed once, two statements with senders of two
    heights proved against it, the multiplicity column filled in HBM; verified against the key root with the bus sum
    zero, then against the root of a key with one entry changed: rejected."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "multi_key")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "multi_key.cpp"), "-L", libdir, "-ltapstark_hip",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("TSPF v8") == 2 and r.stdout.count("verify -> 0, bus sum zero") == 2
    assert "under a key with one entry changed: rejected" in r.stdout
