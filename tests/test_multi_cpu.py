"""ts_verify_multi without a GPU: argument refusals, the committed TSPF v6 fixture under host-only AIRs, and what
the parser answers to truncated and corrupted buffers.  The fixture tests/golden/multi_proof_small.json is this
library's own output for case b of tests/_multi_cases.py (write_golden there; tests/test_gpu_multi.py checks that
the prover still writes it).  None of this exists without ts_prove_multi / ts_verify_multi: the symbols are new."""
import ctypes as C

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
import _multi_cases as mc

TS_OK, TS_ERR_INVALID = 0, 1


@pytest.fixture(scope="module")
def golden():
    doc, tapes, pis, words = mc.load_golden()
    cfg = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*doc["fri"]), host_only=True))
    airs = [ts.CompiledAir(None, t) for t in tapes]
    words.setflags(write=False)
    return cfg, airs, pis, words


def _raw(cfg, airs, pis, words, n_words=None, n_tables=None):
    """ts_verify_multi itself: (status, verdict)."""
    T = len(airs)
    handles = (C.c_void_p * max(T, 1))(*[a.h for a in airs])
    pv = (_lib.u32p * max(T, 1))(*[p.ctypes.data_as(_lib.u32p) if len(p) else None for p in pis])
    n_pub = np.array([len(p) for p in pis] or [0], dtype=np.uint32)
    w = np.ascontiguousarray(words, dtype=np.uint32)
    if len(w) == 0:
        w = np.zeros(1, dtype=np.uint32)
    fri = cfg.pcs.fri._c()
    v = C.c_int(-1)
    chal = ts.BfChallenger()  # (kept alive across the call: its handle is freed with the object)
    rc = _lib.lib().ts_verify_multi(C.byref(fri), chal.h, handles, T if n_tables is None else n_tables, pv,
                                    n_pub.ctypes.data_as(_lib.u32p), w.ctypes.data_as(_lib.u32p),
                                    len(words) if n_words is None else n_words, C.byref(v))
    return rc, v.value


def test_symbols_are_declared_and_exported():
    assert {"ts_prove_multi", "ts_verify_multi"} <= set(_lib.ABI_SYMBOLS)
    l = _lib.lib()
    assert hasattr(l, "ts_prove_multi") and hasattr(l, "ts_verify_multi") and l.ts_abi_version() == 5


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
    npp, wp = n_pub.ctypes.data_as(_lib.u32p), np.ascontiguousarray(words).ctypes.data_as(_lib.u32p)
    args = [C.byref(fri), chal.h, handles, T, pv, npp, wp, len(words), C.byref(v)]
    for k in (0, 1, 2, 4, 5, 6, 8):  # every pointer argument in turn
        a = list(args)
        a[k] = None
        assert l.ts_verify_multi(*a) == TS_ERR_INVALID, k
    assert l.ts_prove_multi(None, C.byref(fri), chal.h, None, 1, wp, 1, None) == TS_ERR_INVALID
    for n in (0, 65):
        rc, verdict = _raw(cfg, airs, pis, words, n_tables=n)
        assert rc == TS_ERR_INVALID and verdict == -1
    assert (l.ts_last_error(None) or b"").decode()
    assert _raw(cfg, airs, pis, words, n_words=0) == (TS_OK, 9)
    assert _raw(cfg, airs, pis, np.zeros(0, dtype=np.uint32)) == (TS_OK, 9)


def test_host_only_airs_accept_the_fixture(golden):
    cfg, airs, pis, words = golden
    assert list(words[:3]) == [0x46505354, 6, 3] and [int(words[3 + 3 * t]) for t in range(3)] == [3, 6, 3]
    assert _raw(cfg, airs, pis, words) == (TS_OK, 0)
    ts.verify_multi(cfg, airs, ts.BfChallenger(), words, pis)
    ts.verify_multi(cfg, airs, ts.BfChallenger(), ts.MultiProof.parse(words), pis)
    pf = ts.MultiProof(words)
    assert [(t.log_degree, t.width, t.qd) for t in pf.tables] == [(3, 2, 1), (6, 6, 2), (3, 2, 1)]
    assert len(pf.query_proofs) == 3 and len(pf.commit_phase_commits) == 6
    # one flipped public value of the last table
    bad = [p.copy() for p in pis]
    bad[2][0] ^= 1
    assert _raw(cfg, airs, bad, words) == (TS_OK, 7)
    assert _raw(cfg, airs, pis, np.concatenate([words, [0]])) == (TS_OK, 9)  # over-long
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(cfg, airs[0], ts.BfChallenger(), words, pis[0])
    assert e.value.code == 9


def test_every_truncation_is_malformed(golden):
    cfg, airs, pis, words = golden
    for n in range(len(words)):
        rc, verdict = _raw(cfg, airs, pis, words[:n])
        assert rc == TS_OK and verdict in (9, 1), (n, rc, verdict)


def test_corrupted_header_and_length_fields(golden):
    cfg, airs, pis, words = golden
    pf = ts.MultiProof.parse(words)
    first = len(words) - len(pf.fri_words)
    fields = list(range(3 + 3 * len(airs))) + mc.length_fields(words, first)
    rng = np.random.default_rng(0x6D756C74)
    seen = set()
    for _ in range(200):
        at = int(fields[rng.integers(len(fields))])
        bad = words.copy()
        while bad[at] == words[at]:
            bad[at] = rng.integers(0, 1 << 32, dtype=np.uint64)
        rc, verdict = _raw(cfg, airs, pis, bad)
        assert rc == TS_OK and verdict in (9, 1), (at, int(bad[at]), rc, verdict)
        seen.add(verdict)
    assert seen == {9, 1}
