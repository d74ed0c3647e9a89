"""ts_verify_multi_bus without a GPU: argument refusals, the committed TSPF v7 fixture under host-only AIRs, and what
the verifier answers to corrupted, truncated and over-long buffers.  The fixture
tests/golden/multi_bus_proof_small.json is this library's own output for case b of tests/_bus_cases.py
(write_golden there; tests/test_gpu_multi_bus.py checks that the prover still writes it).  None of this exists
without ts_prove_multi_bus / ts_verify_multi_bus / ts_logup_aux_build_multi: the symbols are new."""
import ctypes as C

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
import _bus_cases as bc
import _multi_cases as mc

TS_OK, TS_ERR_INVALID, TS_ERR_UNSUPPORTED = 0, 1, 4


@pytest.fixture(scope="module")
def golden():
    doc, tapes, pis, words = bc.load_golden()
    cfg = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*doc["fri"]), host_only=True))
    airs = [ts.CompiledAir(None, t) for t in tapes]
    words.setflags(write=False)
    return cfg, airs, pis, words


def _raw(cfg, airs, pis, words, n_words=None, n_tables=None, cap_exposed=None):
    """ts_verify_multi_bus itself: (status, verdict, exposed words, bus sum)."""
    T = len(airs)
    handles = (C.c_void_p * max(T, 1))(*[a.h for a in airs])
    pv = (_lib.u32p * max(T, 1))(*[p.ctypes.data_as(_lib.u32p) if len(p) else None for p in pis])
    n_pub = np.array([len(p) for p in pis] or [0], dtype=np.uint32)
    w = np.ascontiguousarray(words, dtype=np.uint32)
    if len(w) == 0:
        w = np.zeros(1, dtype=np.uint32)
    fri = cfg.pcs.fri._c()
    v = C.c_int(-1)
    exposed, bus_sum = np.full(4 * max(T, 1), 0xABCD, dtype=np.uint32), np.full(4, 0xABCD, dtype=np.uint32)
    chal = ts.BfChallenger()  # (kept alive across the call: its handle is freed with the object)
    rc = _lib.lib().ts_verify_multi_bus(C.byref(fri), chal.h, handles, T if n_tables is None else n_tables, pv,
                                        n_pub.ctypes.data_as(_lib.u32p), w.ctypes.data_as(_lib.u32p),
                                        len(words) if n_words is None else n_words,
                                        exposed.ctypes.data_as(_lib.u32p),
                                        len(exposed) if cap_exposed is None else cap_exposed,
                                        bus_sum.ctypes.data_as(_lib.u32p), C.byref(v))
    return rc, v.value, exposed, bus_sum


def _verdict(*a, **kw):
    rc, v, _, _ = _raw(*a, **kw)
    return rc, v


def test_symbols_are_declared_and_exported():
    names = {"ts_prove_multi_bus", "ts_verify_multi_bus", "ts_logup_aux_build_multi"}
    assert names <= set(_lib.ABI_SYMBOLS)
    l = _lib.lib()
    assert all(hasattr(l, n) for n in names) and l.ts_abi_version() == 5
    assert C.sizeof(_lib.MultiBusTableC) == 40


def test_argument_refusals_touch_no_device(golden):
    cfg, airs, pis, words = golden
    l = _lib.lib()
    fri = cfg.pcs.fri._c()
    chal = ts.BfChallenger()
    v = C.c_int(-1)
    T = len(airs)
    handles = (C.c_void_p * T)(*[a.h for a in airs])
    pv = (_lib.u32p * T)(*[p.ctypes.data_as(_lib.u32p) if len(p) else None for p in pis])
    n_pub = np.array([len(p) for p in pis], dtype=np.uint32)
    exposed, bus_sum = np.zeros(4 * T, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    npp, wp = n_pub.ctypes.data_as(_lib.u32p), np.ascontiguousarray(words).ctypes.data_as(_lib.u32p)
    args = [C.byref(fri), chal.h, handles, T, pv, npp, wp, len(words), exposed.ctypes.data_as(_lib.u32p), 4 * T,
            bus_sum.ctypes.data_as(_lib.u32p), C.byref(v)]
    for k in (0, 1, 2, 4, 5, 6, 8, 10, 11):  # every pointer argument in turn
        a = list(args)
        a[k] = None
        assert l.ts_verify_multi_bus(*a) == TS_ERR_INVALID, k
    # the prover and the builder without a context, and with null tables
    assert l.ts_prove_multi_bus(None, C.byref(fri), chal.h, None, 1, wp, 1, None) == TS_ERR_INVALID
    assert l.ts_logup_aux_build_multi(None, 1, None, None, None, None, None) == TS_ERR_INVALID
    for n in (0, 65):
        rc, verdict = _verdict(cfg, airs, pis, words, n_tables=n)
        assert rc == TS_ERR_INVALID and verdict == -1
    assert (l.ts_last_error(None) or b"").decode()
    # a short buffer for the exposed words: four aux tables need 16
    rc, verdict = _verdict(cfg, airs, pis, words, cap_exposed=15)
    assert rc == TS_ERR_INVALID and verdict == -1
    assert _verdict(cfg, airs, pis, words, cap_exposed=16) == (TS_OK, 0)
    # AIRs the format does not take: no aux table at all; preprocessed columns
    fib = airs[1]
    rc, verdict = _verdict(cfg, [fib], [pis[1]], words)
    assert rc == TS_ERR_INVALID and verdict == -1 and b"ts_verify_multi" in l.ts_last_error(None)
    assert _verdict(cfg, airs, pis, words, n_words=0) == (TS_OK, 9)
    assert _verdict(cfg, airs, pis, np.zeros(0, dtype=np.uint32)) == (TS_OK, 9)


def test_host_only_airs_accept_the_fixture_and_the_bus_balances(golden):
    cfg, airs, pis, words = golden
    tables = bc.case("b")
    assert list(words[:3]) == [0x46505354, 7, 5] and list(words[:28]) == bc.header_words(tables)
    rc, verdict, exposed, bus_sum = _raw(cfg, airs, pis, words)
    assert (rc, verdict) == (TS_OK, 0) and not bus_sum.any()
    reg = bc.regions(tables)
    assert (exposed[:16] == words[slice(*reg["exposed"])]).all() and exposed[:16].any()
    assert (exposed[16:] == 0xABCD).all()
    got, s = ts.verify_multi_bus(cfg, airs, ts.BfChallenger(), words, pis)
    assert (got == exposed[:16]).all() and not s.any()
    ts.verify_multi_bus(cfg, airs, ts.BfChallenger(), ts.MultiBusProof.parse(words), pis)
    pf = ts.MultiBusProof(words)
    assert [(t.log_degree, t.width, t.qd, t.aux_width, t.n_exposed) for t in pf.tables] == \
        [(3, 2, 2, 8, 4), (4, 2, 1, 0, 0), (6, 4, 2, 8, 4), (3, 10, 2, 16, 4), (1, 2, 2, 8, 4)]
    assert len(pf.query_proofs) == 3 and len(pf.commit_phase_commits) == 6 and not pf.bus_sum.any()
    assert all(len(q.input_proof) == 3 for q in pf.query_proofs)
    # one flipped public value of the plain table
    bad = [p.copy() for p in pis]
    bad[1][0] ^= 1
    assert _verdict(cfg, airs, bad, words) == (TS_OK, 7)
    # nothing is handed back on a rejection
    rc, verdict, exposed, bus_sum = _raw(cfg, airs, bad, words)
    assert (exposed == 0xABCD).all() and (bus_sum == 0xABCD).all()


def test_every_other_verify_call_answers_9(golden):
    cfg, airs, pis, words = golden
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(cfg, airs[1], ts.BfChallenger(), words, pis[1])
    assert e.value.code == 9
    with pytest.raises(ts.VerificationError) as e:
        ts.verify_multi(cfg, [airs[1]], ts.BfChallenger(), words, [pis[1]])
    assert e.value.code == 9
    l, fri = _lib.lib(), cfg.pcs.fri._c()
    wp = np.ascontiguousarray(words).ctypes.data_as(_lib.u32p)
    ex = np.zeros(4, dtype=np.uint32)
    chal = ts.BfChallenger()
    v = C.c_int(-1)
    l.ts_verify_aux(C.byref(fri), airs[0].h, chal.h, wp, len(words), None, 0, ex.ctypes.data_as(_lib.u32p), 4, C.byref(v))
    assert v.value == 9
    with pytest.raises(_lib.TsError) as e:
        ts.Proof(words).to_postcard()
    assert e.value.code == TS_ERR_UNSUPPORTED
    # and the v6 fixture is no v7 proof
    _, _, _, v6 = mc.load_golden()
    assert _verdict(cfg, airs, pis, v6) == (TS_OK, 9)


def test_one_flipped_word_per_region_is_rejected(golden):
    cfg, airs, pis, words = golden
    tables = bc.case("b")
    reg = bc.regions(tables)
    fri0 = reg["fri"][0]
    R = int(words[fri0])
    assert R == 6 and int(words[fri0 + 1 + 8 * R]) == bc.FRI_QUERIES
    n, tab = len(words), reg["tables"][0]
    flips = {
        "version": (1, {9}),
        "table count": (2, {1, 9}),
        "table width": (tab + 5 * 2 + 1, {1}),
        "table qd": (tab + 5 * 3 + 2, {1}),
        "table aux width": (tab + 5 * 0 + 3, {1}),
        "plain table's aux width": (tab + 5 * 1 + 3, {1}),
        "table n_exposed": (tab + 5 * 4 + 4, {1}),
        "table log_degree": (tab + 5 * 2, {7, 1, 9}),
        "trace root": (reg["trace_root"][0] + 3, {7, 4}),
        "aux root": (reg["aux_root"][0] + 2, {7, 4}),
        "exposed word": (reg["exposed"][0] + 4 * 2 + 1, {7, 9}),
        "quotient root": (reg["quotient_root"][0] + 5, {7, 4}),
        "aux value": (reg["aux_values"][3][0] + 9, {7, 9}),
        "trace value": (reg["trace_values"][4][0] + 1, {7, 9}),
        "plain table's trace value": (reg["trace_values"][1][0] + 2, {7, 9}),
        "chunk value": (reg["chunk_values"][2][0] + 6, {7, 9}),
        "FRI round root": (fri0 + 1 + 8 * 2, {3, 5, 8}),
        "final polynomial": (n - 5, {6, 9}),
        "PoW witness": (n - 1, {3, 4, 8}),
    }
    for what, (at, owned) in flips.items():
        bad = words.copy()
        bad[at] ^= 1
        rc, v = _verdict(cfg, airs, pis, bad)
        assert rc == TS_OK and v != 0 and v in owned, f"{what}: verdict {v}"
    # the exposed sums of two tables exchanged: the same bus sum, other last-row constraints
    e0 = reg["exposed"][0]
    bad = words.copy()
    bad[e0:e0 + 4], bad[e0 + 4:e0 + 8] = words[e0 + 4:e0 + 8], words[e0:e0 + 4]
    assert not (bad == words).all() and not ts.MultiBusProof(bad).bus_sum.any()
    assert _verdict(cfg, airs, pis, bad) == (TS_OK, 7)
    # another table order: same tapes elsewhere
    assert _verdict(cfg, airs[::-1], pis[::-1], words)[1] != 0


def test_truncated_and_over_long_buffers_are_malformed(golden):
    cfg, airs, pis, words = golden
    for n in range(len(words)):
        rc, verdict = _verdict(cfg, airs, pis, words[:n])
        assert rc == TS_OK and verdict in (9, 1), (n, rc, verdict)
    assert _verdict(cfg, airs, pis, np.concatenate([words, [0]])) == (TS_OK, 9)


def test_corrupted_header_and_length_fields(golden):
    cfg, airs, pis, words = golden
    pf = ts.MultiBusProof.parse(words)
    first = len(words) - len(pf.fri_words)
    fields = list(range(3 + 5 * len(airs))) + mc.length_fields(words, first)
    rng = np.random.default_rng(0x627573)
    seen = set()
    for _ in range(200):
        at = int(fields[rng.integers(len(fields))])
        bad = words.copy()
        while bad[at] == words[at]:
            bad[at] = rng.integers(0, 1 << 32, dtype=np.uint64)
        rc, verdict = _verdict(cfg, airs, pis, bad)
        assert rc == TS_OK and verdict in (9, 1), (at, int(bad[at]), rc, verdict)
        seen.add(verdict)
    assert seen == {9, 1}
