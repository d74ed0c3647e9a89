"""ts_verify_multi_key without a GPU: the case set's edges, argument refusals of every new call that needs no device,
the committed TSPF v8 fixture under host-only AIRs and its key root, and what the verifier answers to another key
root and to corrupted, truncated and over-long buffers.  The fixture tests/golden/multi_key_proof_small.json is this
library's own output for case kb of tests/_key_cases.py (write_golden there; tests/test_gpu_multi_key.py checks that
the prover still writes it).  None of this exists without the ts_multi_key_* / ts_prove_multi_key /
ts_verify_multi_key / ts_logup_aux_build_multi_pre / ts_logup_multiplicities_bus_pre symbols: they are new."""
import ctypes as C

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.airs import BusKeyTableAir, BusSendAir, BusTupleSendAir
import _bus_cases as bc
import _key_cases as kc
import _multi_cases as mc

TS_OK, TS_ERR_INVALID, TS_ERR_UNSUPPORTED = 0, 1, 4
NEW = ("ts_multi_key_commit", "ts_multi_key_info", "ts_multi_key_values", "ts_multi_key_free", "ts_prove_multi_key",
       "ts_verify_multi_key", "ts_logup_aux_build_multi_pre", "ts_logup_multiplicities_bus_pre")


@pytest.fixture(scope="module")
def golden():
    doc, tapes, pis, words, root = kc.load_golden()
    cfg = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*doc["fri"]), host_only=True))
    airs = [ts.CompiledAir(None, t) for t in tapes]
    words.setflags(write=False)
    root.setflags(write=False)
    return cfg, airs, pis, words, root


def _raw(cfg, root, airs, pis, words, n_words=None, n_tables=None, cap_exposed=None):
    """ts_verify_multi_key itself: (status, verdict, exposed words, bus sum)."""
    T = len(airs)
    handles = (C.c_void_p * max(T, 1))(*[a.h for a in airs])
    pv = (_lib.u32p * max(T, 1))(*[p.ctypes.data_as(_lib.u32p) if len(p) else None for p in pis])
    n_pub = np.array([len(p) for p in pis] or [0], dtype=np.uint32)
    w = np.ascontiguousarray(words, dtype=np.uint32)
    if len(w) == 0:
        w = np.zeros(1, dtype=np.uint32)
    r = np.ascontiguousarray(root, dtype=np.uint32)
    fri = cfg.pcs.fri._c()
    v = C.c_int(-1)
    exposed, bus_sum = np.full(4 * max(T, 1), 0xABCD, dtype=np.uint32), np.full(4, 0xABCD, dtype=np.uint32)
    chal = ts.BfChallenger()  # (kept alive across the call: its handle is freed with the object)
    rc = _lib.lib().ts_verify_multi_key(C.byref(fri), chal.h, r.ctypes.data_as(_lib.u32p), handles,
                                        T if n_tables is None else n_tables, pv, n_pub.ctypes.data_as(_lib.u32p),
                                        w.ctypes.data_as(_lib.u32p), len(words) if n_words is None else n_words,
                                        exposed.ctypes.data_as(_lib.u32p),
                                        len(exposed) if cap_exposed is None else cap_exposed,
                                        bus_sum.ctypes.data_as(_lib.u32p), C.byref(v))
    return rc, v.value, exposed, bus_sum


def _verdict(*a, **kw):
    rc, v, _, _ = _raw(*a, **kw)
    return rc, v


def test_case_set_has_the_edges():
    ka, kb, kc_, ke, k0 = (kc.case(n) for n in kc.CASE_NAMES)
    shape = lambda tables: [(t.log_n, t.aux_width, t.prep_width) for t in tables]
    assert shape(ka) == [(5, 8, 0), (5, 8, 1)]
    # kb: every table kind; key matrices of two heights and two widths; two buses; a receiver shorter than a sender
    assert shape(kb) == [(3, 8, 1), (4, 0, 0), (3, 0, 3), (6, 8, 0), (3, 16, 0), (4, 8, 3), (1, 8, 0)]
    assert {m.shape for m in kc.key_matrices(kb)} == {(8, 1), (8, 3), (16, 3)}
    assert {t.air.tag for t in kb if isinstance(t.air, BusKeyTableAir)} == {7, kc.XOR_TAG}
    assert shape(kc_) == [(12, 8, 0), (8, 8, 1), (10, 8, 0), (8, 8, 3)]
    # ke: 64 key + 64 aux + 64 trace + 64 chunk jobs in the one class
    assert len(ke) == 64 and {t.log_n for t in ke} == {3} and sum(1 << t.lqd for t in ke) == 64
    assert len(kc.key_matrices(ke)) == 64 and all(t.aux_width for t in ke)
    assert shape(k0) == [(3, 0, 3), (4, 0, 0)]
    assert shape(kc.case("kt1")) == [(4, 8, 1)]
    every = [t for n in kc.CASE_NAMES + ("kt1", "unbalanced") for t in kc.case(n)]
    assert all(t.lqd <= 1 for t in every)  # fits log_blowup 1
    # a key table and a one-lookup tuple sender have constraint degree 2: one chunk, no padding
    assert all(t.lqd == 0 for t in every if isinstance(t.air, BusKeyTableAir))
    assert [t.lqd for t in kb if isinstance(t.air, BusTupleSendAir)] == [0]
    assert [t.lqd for t in kc_ if isinstance(t.air, BusTupleSendAir)] == [1]
    # sender values lie in the key's table; every selector column is neither all 0 nor all 1
    for tables in (ka, kb, kc_):
        rows = {t.air.tag: {tuple(r) for r in t.key.tolist()} for t in tables if isinstance(t.air, BusKeyTableAir)}
        for t in tables:
            if isinstance(t.air, (BusSendAir, BusTupleSendAir)):
                nv = 1 if isinstance(t.air, BusSendAir) else 3
                tag = 7 if isinstance(t.air, BusSendAir) else t.air.tag
                groups = t.trace.reshape(t.trace.shape[0], -1, nv + 1)
                assert {tuple(r) for r in groups[:, :, :nv].reshape(-1, nv).tolist()} <= rows[tag]
                sel = groups[:, :, nv]
                assert set(np.unique(sel)) <= {0, 1}
                assert all(0 < int(sel[:, i].sum()) < sel.shape[0] for i in range(sel.shape[1]))
    bad = kc.case("unbalanced")
    assert int(bad[0].trace[3, 0]) == 32 and (32,) not in {tuple(r) for r in bad[1].key.tolist()}
    assert int((bad[0].trace != ka[0].trace).any(axis=1).sum()) == 1


def test_symbols_are_declared_and_exported():
    assert set(NEW) <= set(_lib.ABI_SYMBOLS)
    l = _lib.lib()
    assert all(hasattr(l, n) for n in NEW) and l.ts_abi_version() == 5
    assert C.sizeof(_lib.MultiBusTableC) == 40  # ts_multi_key_table is ts_multi_bus_table


def test_argument_refusals_touch_no_device(golden):
    cfg, airs, pis, words, root = golden
    l = _lib.lib()
    fri = cfg.pcs.fri._c()
    chal = ts.BfChallenger()
    v = C.c_int(-1)
    T = len(airs)
    handles = (C.c_void_p * T)(*[a.h for a in airs])
    pv = (_lib.u32p * T)(*[p.ctypes.data_as(_lib.u32p) if len(p) else None for p in pis])
    n_pub = np.array([len(p) for p in pis], dtype=np.uint32)
    exposed, bus_sum = np.zeros(4 * T, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    r = np.ascontiguousarray(root)
    npp, wp = n_pub.ctypes.data_as(_lib.u32p), np.ascontiguousarray(words).ctypes.data_as(_lib.u32p)
    args = [C.byref(fri), chal.h, r.ctypes.data_as(_lib.u32p), handles, T, pv, npp, wp, len(words),
            exposed.ctypes.data_as(_lib.u32p), 4 * T, bus_sum.ctypes.data_as(_lib.u32p), C.byref(v)]
    for k in (0, 1, 2, 3, 5, 6, 7, 9, 11, 12):  # every pointer argument in turn (five aux tables: exposed_out too)
        a = list(args)
        a[k] = None
        assert l.ts_verify_multi_key(*a) == TS_ERR_INVALID, k
    assert l.ts_verify_multi_key(*args) == TS_OK and v.value == 0
    # the calls that need a device, without a context; the key calls on null handles
    assert l.ts_prove_multi_key(None, C.byref(fri), chal.h, None, None, 1, wp, 1, None) == TS_ERR_INVALID
    assert l.ts_multi_key_commit(None, C.byref(fri), 1, None, 1, None, None) == TS_ERR_INVALID
    assert l.ts_logup_aux_build_multi_pre(None, 1, None, None, None, None, None, None) == TS_ERR_INVALID
    assert l.ts_logup_multiplicities_bus_pre(None, None, None, None, None, None, None) == TS_ERR_INVALID
    hh, ww, out = C.c_uint64(), C.c_uint32(), C.c_void_p(1)
    assert l.ts_multi_key_info(None, 0, C.byref(hh), C.byref(ww)) == TS_ERR_INVALID
    assert l.ts_multi_key_values(None, 0, C.byref(out)) == TS_ERR_INVALID and not out.value
    assert l.ts_multi_key_free(None, None) == TS_OK
    for n in (0, 65):
        rc, verdict = _verdict(cfg, root, airs, pis, words, n_tables=n)
        assert rc == TS_ERR_INVALID and verdict == -1
    assert (l.ts_last_error(None) or b"").decode()
    # a short buffer for the exposed words: five aux tables need 20
    rc, verdict = _verdict(cfg, root, airs, pis, words, cap_exposed=19)
    assert rc == TS_ERR_INVALID and verdict == -1
    assert _verdict(cfg, root, airs, pis, words, cap_exposed=20) == (TS_OK, 0)
    # AIRs the format does not take: no table with preprocessed columns (the text points at the calls without a key)
    rc, verdict = _verdict(cfg, root, [airs[1], airs[3]], [pis[1], pis[3]], words)
    assert rc == TS_ERR_INVALID and verdict == -1 and b"ts_verify_multi_bus" in l.ts_last_error(None)
    assert _verdict(cfg, root, airs, pis, words, n_words=0) == (TS_OK, 9)
    assert _verdict(cfg, root, airs, pis, np.zeros(0, dtype=np.uint32)) == (TS_OK, 9)
    # the calls without a key keep refusing preprocessed columns
    v7 = bc.load_golden()[3]
    with pytest.raises(_lib.TsError) as e:
        ts.verify_multi_bus(cfg, airs, ts.BfChallenger(), v7, pis)
    assert e.value.code == TS_ERR_UNSUPPORTED


def test_host_only_airs_accept_the_fixture_and_the_bus_balances(golden):
    cfg, airs, pis, words, root = golden
    tables = kc.case("kb")
    assert list(words[:3]) == [0x46505354, 8, 7] and list(words[:45]) == kc.header_words(tables)
    rc, verdict, exposed, bus_sum = _raw(cfg, root, airs, pis, words)
    assert (rc, verdict) == (TS_OK, 0) and not bus_sum.any()
    reg = kc.regions(tables)
    assert (exposed[:20] == words[slice(*reg["exposed"])]).all() and exposed[:20].any()
    assert (exposed[20:] == 0xABCD).all()
    got, s = ts.verify_multi_key(cfg, root, airs, ts.BfChallenger(), words, pis)
    assert (got == exposed[:20]).all() and not s.any()
    ts.verify_multi_key(cfg, root, airs, ts.BfChallenger(), ts.MultiKeyProof.parse(words), pis)
    pf = ts.MultiKeyProof(words)
    assert [(t.log_degree, t.width, t.qd, t.aux_width, t.n_exposed, t.preprocessed_width) for t in pf.tables] == \
        [(3, 1, 1, 8, 4, 1), (4, 2, 1, 0, 0, 0), (3, 3, 2, 0, 0, 3), (6, 4, 2, 8, 4, 0), (3, 10, 2, 16, 4, 0),
         (4, 1, 1, 8, 4, 3), (1, 4, 1, 8, 4, 0)]
    assert [t.preprocessed_local.shape for t in pf.tables] == [(t.prep_width, 4) for t in tables]
    assert len(pf.query_proofs) == 3 and len(pf.commit_phase_commits) == 6 and not pf.bus_sum.any()
    assert all(len(q.input_proof) == 4 for q in pf.query_proofs)
    # one flipped public value of the plain table, and of the key-only table
    for t in (1, 2):
        bad = [p.copy() for p in pis]
        bad[t][0] ^= 1
        assert _verdict(cfg, root, airs, bad, words) == (TS_OK, 7)
    # nothing is handed back on a rejection
    rc, verdict, exposed, bus_sum = _raw(cfg, root, airs, bad, words)
    assert (exposed == 0xABCD).all() and (bus_sum == 0xABCD).all()


def test_another_key_root_rejects(golden):
    """The key is part of the statement: its root is in the transcript and is the first commitment of the opening."""
    cfg, airs, pis, words, root = golden
    for word in range(8):
        other = root.copy()
        other[word] ^= 1
        rc, v = _verdict(cfg, other, airs, pis, words)
        assert rc == TS_OK and v != 0 and v in {7, 4}, (word, v)


def test_every_other_verify_call_answers_9(golden):
    cfg, airs, pis, words, root = golden
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(cfg, airs[1], ts.BfChallenger(), words, pis[1])
    assert e.value.code == 9
    with pytest.raises(ts.VerificationError) as e:
        ts.verify_multi(cfg, [airs[1]], ts.BfChallenger(), words, [pis[1]])
    assert e.value.code == 9
    with pytest.raises(ts.VerificationError) as e:
        ts.verify_multi_bus(cfg, [airs[3], airs[1]], ts.BfChallenger(), words, [pis[3], pis[1]])
    assert e.value.code == 9
    l, fri = _lib.lib(), cfg.pcs.fri._c()
    wp = np.ascontiguousarray(words).ctypes.data_as(_lib.u32p)
    ex = np.zeros(4, dtype=np.uint32)
    chal = ts.BfChallenger()
    v = C.c_int(-1)
    l.ts_verify_aux(C.byref(fri), airs[3].h, chal.h, wp, len(words), None, 0, ex.ctypes.data_as(_lib.u32p), 4, C.byref(v))
    assert v.value == 9
    with pytest.raises(_lib.TsError) as e:
        ts.Proof(words).to_postcard()
    assert e.value.code == TS_ERR_UNSUPPORTED
    # and the v6 and v7 fixtures are no v8 proofs
    v6, v7 = mc.load_golden()[3], bc.load_golden()[3]
    assert _verdict(cfg, root, airs, pis, v6) == (TS_OK, 9)
    assert _verdict(cfg, root, airs, pis, v7) == (TS_OK, 9)


def test_one_flipped_word_per_region_is_rejected(golden):
    cfg, airs, pis, words, root = golden
    tables = kc.case("kb")
    reg = kc.regions(tables)
    fri0 = reg["fri"][0]
    R = int(words[fri0])
    assert R == 6 and int(words[fri0 + 1 + 8 * R]) == kc.FRI_QUERIES
    q0 = fri0 + 1 + 8 * R + 1  # query 0: [4 batches][key round: n_mats, (len, values) ...]
    assert list(words[q0:q0 + 3]) == [4, 3, 1]
    n, tab = len(words), reg["tables"][0]
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
        "table log_degree": (tab + 6 * 3, {7, 1, 9}),
        "trace root": (reg["trace_root"][0] + 3, {7, 4}),
        "aux root": (reg["aux_root"][0] + 2, {7, 4}),
        "exposed word": (reg["exposed"][0] + 4 * 2 + 1, {7, 9}),
        "quotient root": (reg["quotient_root"][0] + 5, {7, 4}),
        "preprocessed value": (reg["key_values"][5][0] + 9, {7, 9}),
        "key-only table's preprocessed value": (reg["key_values"][2][0] + 1, {7, 9}),
        "aux value": (reg["aux_values"][4][0] + 9, {7, 9}),
        "trace value": (reg["trace_values"][6][0] + 1, {7, 9}),
        "plain table's trace value": (reg["trace_values"][1][0] + 2, {7, 9}),
        "chunk value": (reg["chunk_values"][2][0] + 6, {7, 9}),
        "key-round opening": (q0 + 3, {4, 9}),
        "FRI round root": (fri0 + 1 + 8 * 2, {3, 5, 8}),
        "final polynomial": (n - 5, {6, 9}),
        "PoW witness": (n - 1, {3, 4, 8}),
    }
    for what, (at, owned) in flips.items():
        bad = words.copy()
        bad[at] ^= 1
        rc, v = _verdict(cfg, root, airs, pis, bad)
        assert rc == TS_OK and v != 0 and v in owned, f"{what}: verdict {v}"
    # the exposed sums of two tables exchanged: the same bus sum, other last-row constraints
    e0 = reg["exposed"][0]
    bad = words.copy()
    bad[e0:e0 + 4], bad[e0 + 4:e0 + 8] = words[e0 + 4:e0 + 8], words[e0:e0 + 4]
    assert not (bad == words).all() and not ts.MultiKeyProof(bad).bus_sum.any()
    assert _verdict(cfg, root, airs, pis, bad) == (TS_OK, 7)
    # another table order: same tapes elsewhere
    assert _verdict(cfg, root, airs[::-1], pis[::-1], words)[1] != 0


def test_truncated_and_over_long_buffers_are_malformed(golden):
    cfg, airs, pis, words, root = golden
    for n in range(len(words)):
        rc, verdict = _verdict(cfg, root, airs, pis, words[:n])
        assert rc == TS_OK and verdict == 9, (n, rc, verdict)
    assert _verdict(cfg, root, airs, pis, np.concatenate([words, [0]])) == (TS_OK, 9)


def _fri_tail_words(pf):
    """The FriProof of a parsed proof, back in wire order."""
    out = [len(pf.commit_phase_commits), *pf.commit_phase_commits.reshape(-1), len(pf.query_proofs)]
    for q in pf.query_proofs:
        out.append(len(q.input_proof))
        for b in q.input_proof:
            out.append(len(b.opened_values))
            for v in b.opened_values:
                out += [len(v), *v]
            out += [len(b.opening_proof), *b.opening_proof.reshape(-1)]
        for vals, path in q.commit_phase_openings:
            out += [*vals.reshape(-1), len(path), *path.reshape(-1)]
    return out + [*pf.final_poly, pf.pow_witness]


@pytest.mark.parametrize("cls, load", [(ts.MultiProof, mc.load_golden), (ts.MultiBusProof, bc.load_golden),
                                       (ts.MultiKeyProof, kc.load_golden)])
def test_the_parsed_fields_are_the_words_in_wire_order(cls, load):
    """One parser reads TSPF v6, v7 and v8: every word of each committed fixture lands in exactly one field, in order."""
    from tapstark_amd.stark import TSPF_MAGIC
    words = load()[3]
    pf = cls.parse(words)
    header = ("log_degree", "width", "qd", "aux_width", "n_exposed", "preprocessed_width")[:{6: 3, 7: 5, 8: 6}[cls._VERSION]]
    out = [TSPF_MAGIC, cls._VERSION, len(pf.tables)]
    for t in pf.tables:
        out += [getattr(t, h) for h in header]
    out += [*pf.trace_commit]
    if cls._VERSION >= 7:  # both fixtures have aux tables: the v8 one carries its aux root too
        assert pf.aux_commit is not None and len(pf.exposed) == 4 * sum(1 for t in pf.tables if t.aux_width)
        out += [*pf.aux_commit, *pf.exposed]
    out += [*pf.quotient_commit, *pf.opened_words, *_fri_tail_words(pf)]
    assert np.array_equal(np.array(out, dtype=np.uint64), words)
    assert np.array_equal(pf.fri_words, np.array(_fri_tail_words(pf), dtype=np.uint64))
    for other in {ts.MultiProof, ts.MultiBusProof, ts.MultiKeyProof} - {cls}:
        with pytest.raises(ValueError, match=f"not a TSPF v{other._VERSION} proof"):
            other.parse(words)
