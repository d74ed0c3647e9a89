"""AIRs with preprocessed columns on the CPU (no GPU): tape version 2 through the product's validation, degree
rules and lowering, the Python and C++ capture front ends, the refusals, the segment plan and the host-only
ts_verify_pre.  The reference's AIR language has such columns (PairBuilder::preprocessed, uni-stark/src/
symbolic_builder.rs:68-99,144-148; Entry::Preprocessed, symbolic_variable.rs:9-15,34-39) and its
get_log_quotient_degree takes their width (:15-21).  The frozen oracle knows version 1 only, so every check goes
through the joined AIR over hstack(preprocessed, main) (tests/_prep_airs.py).  The GPU half is
tests/test_gpu_preprocessed.py."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.airs import (FibonacciAir, HighDegreeAir, NumericBuilder, SelectorAir, SynthExtAir, SynthMulAir,
                               generate_fibonacci_trace, fibonacci_public_values, generate_selector_preprocessed,
                               generate_selector_trace, random_air_case, splitmix64_stream)
from _air_program import D_LOAD, run_program
from _air_segment import COMPUTED
from _prep_airs import join_program, join_tape, prep_width, split_tape

P = 0x78000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_UNSUPPORTED = 1, 4


def _rows(seed, w, m=8):
    """m (local, next, selector) inputs over the joined width, edge values mixed in."""
    vals = splitmix64_stream(seed + 177, 2 * m * w + 3 * m)
    local = vals[:m * w].reshape(m, w).copy()
    nxt = vals[m * w:2 * m * w].reshape(m, w).copy()
    sels = vals[2 * m * w:].reshape(m, 3).copy()
    local[0, :] = 0
    nxt[0, :] = P - 1
    local[1, :] = P - 1
    sels[0] = (1, 0, 1)
    sels[1] = (0, 1, 0)
    return local, nxt, sels


@pytest.mark.parametrize("chunk", range(6))
def test_degree_rules_and_lowered_program(orc, chunk):
    n_run = 0
    for seed in range(20 * chunk, 20 * chunk + 20):
        air, _ = random_air_case(seed)
        w = air.width()
        if w == 1:
            continue
        n_run += 1
        pw = prep_width(seed, w)
        v1 = ts.air_tape(air, air.n_public)
        v2 = split_tape(v1, pw)
        assert (join_tape(v2) == v1).all(), seed
        cair = ts.CompiledAir(None, v2)
        assert cair.preprocessed_width == pw and cair.width == w - pw, seed
        assert cair.max_constraint_degree == orc.max_constraint_degree(v1), seed
        assert cair.log_quotient_degree == orc.log_quotient_degree(v1), seed
        assert cair.log_quotient_degree == ts.get_log_quotient_degree(air, air.n_public, pw), seed
        prog = cair.program()
        loads = prog["code"][prog["code"][:, 0] == D_LOAD]
        assert (loads[:, 2] <= 3).all() and (loads[loads[:, 2] >= 2, 3] < pw).all(), seed
        assert (loads[loads[:, 2] < 2, 3] < w - pw).all(), seed
        local, nxt, sels = _rows(seed, w)
        pis = splitmix64_stream(seed + 5, max(air.n_public, 1))[:air.n_public]
        want = orc.constraint_values(v1, local, nxt, pis, sels)
        got = run_program(join_program(prog, pw), local, nxt, pis, sels, int(v1[5]))
        assert (got == want).all(), f"seed {seed}: constraint values differ"
    assert n_run >= 15


def test_python_degree_rules_with_preprocessed_width():
    air = SelectorAir()
    assert ts.get_max_constraint_degree(air, 2, 3) == 3 and ts.get_log_quotient_degree(air, 2, 3) == 1
    cair = ts.CompiledAir(None, ts.air_tape(air, 2, 3))
    assert (cair.width, cair.preprocessed_width, cair.n_public) == (3, 3, 2)
    assert (cair.max_constraint_degree, cair.log_quotient_degree) == (3, 1)


def test_version_2_with_width_0_is_version_1():
    for seed in (0, 1, 9, 14, 21):
        air, _ = random_air_case(seed)
        v1 = ts.air_tape(air, air.n_public)
        v2 = split_tape(v1, 0)
        assert v2[1] == 2 and v2[6] == 0 and len(v2) == len(v1) + 1
        a, b = ts.CompiledAir(None, v1), ts.CompiledAir(None, v2)
        pa, pb = a.program(), b.program()
        assert pa["n_regs"] == pb["n_regs"] and b.preprocessed_width == 0
        for k in ("code", "consts", "const_public"):
            assert (pa[k] == pb[k]).all(), (seed, k)
        assert a.jit_source() == b.jit_source()
        assert (a.width, a.n_public, a.max_constraint_degree, a.log_quotient_degree) == \
               (b.width, b.n_public, b.max_constraint_degree, b.log_quotient_degree)


def test_version_1_emitted_source_has_no_preprocessed_parameters():
    src = ts.CompiledAir(None, ts.air_tape(SynthMulAir(64), 0)).jit_source()
    assert "prep" not in src and "row2" not in src
    src2 = ts.CompiledAir(None, ts.air_tape(SelectorAir(), 2, 3)).jit_source()
    assert "const u32* __restrict__ prep, u64 prep_stride" in src2 and "row3[1ull * prep_stride]" in src2


def test_python_builder_output():
    """air_tape of the existing AIRs is what it was before preprocessed columns existed (digests recorded then:
    tests/golden/air_tapes_v1.json), and still version 1."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "air_tapes_v1.json")))
    cases = {"FibonacciAir/3": (FibonacciAir(), 3), "SynthMulAir(64)/0": (SynthMulAir(64), 0),
             "SynthMulAir(16)/0": (SynthMulAir(16), 0), "HighDegreeAir(33)/0": (HighDegreeAir(33), 0),
             "SynthExtAir(163)/0": (SynthExtAir(163), 0)}
    for seed in range(36):
        air, _ = random_air_case(seed)
        cases[f"random_air_case({seed})"] = (air, air.n_public)
    assert set(cases) == set(golden)
    for name, (air, k) in cases.items():
        t = ts.air_tape(air, k)
        assert t[1] == 1 and len(t) == 6 + 3 * int(t[4]) + int(t[5]) == golden[name]["n_words"], name
        assert hashlib.sha256(t.astype("<u4").tobytes()).hexdigest() == golden[name]["sha256"], name
    t = ts.air_tape(SelectorAir(), 2, preprocessed_width=3)
    assert t[1] == 2 and t[6] == 3 and len(t) == 7 + 3 * int(t[4]) + int(t[5])
    j = join_tape(t)
    assert j[1] == 1 and j[2] == 6 and (split_tape(j, 3) == t).all()


def test_selector_air_trace_satisfies_it(orc):
    air = SelectorAir()
    prep = generate_selector_preprocessed(32)
    assert set(np.unique(prep[:, 0])) == {0, 1}  # both kinds of row
    trace, pis = generate_selector_trace(prep)
    nb = NumericBuilder(trace.astype(np.uint64), pis, define=False, preprocessed=prep)
    air.eval(nb)
    joined = join_tape(ts.air_tape(air, 2, 3))
    assert nb.first_violation() == -1 == orc.check_constraints(joined, np.hstack([prep, trace]), pis)
    other = prep.copy()
    other[:, 0] ^= 1  # a trace made for another selector column
    nb = NumericBuilder(trace.astype(np.uint64), pis, define=False, preprocessed=other)
    air.eval(nb)
    assert nb.first_violation() == orc.check_constraints(joined, np.hstack([other, trace]), pis) >= 0


def test_cpp_capture():
    """include/tapstark_air.hpp: the C++ capture of SelectorAir (examples/selector_air.cpp, plain g++, no
    library) prints the words of the Python tape."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "selector_air")
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "selector_air.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = np.array([int(x) for x in out.split()], dtype=np.uint32)
    want = ts.air_tape(SelectorAir(), 2, 3)
    assert len(got) == len(want) and (got == want).all()


def _compile_status(tape):
    l = _lib.lib()
    h = C.c_void_p()
    t = np.ascontiguousarray(tape, dtype=np.uint32)
    rc = l.ts_air_compile(None, t.ctypes.data_as(_lib.u32p), len(t), C.byref(h))
    msg = (l.ts_last_error(None) or b"").decode()
    if rc == 0:
        l.ts_air_free(None, h)
    return rc, msg


def test_malformed_tapes():
    good = ts.air_tape(SelectorAir(), 2, 3)
    assert _compile_status(good)[0] == 0
    n_nodes = int(good[4])
    nodes = good[7:7 + 3 * n_nodes].reshape(n_nodes, 3)
    k_prep = int(np.flatnonzero(nodes[:, 0] == 10)[0])

    def mutated(f):
        t = good.copy()
        f(t)
        return t

    def set_node(t, field, value):
        t[7 + 3 * k_prep + field] = value

    v1_with_prep = np.concatenate([good[:6], good[7:]]).astype(np.uint32)
    v1_with_prep[1] = 1
    bad = {
        "PREP in a version-1 tape": v1_with_prep,
        "column >= preprocessed_width": mutated(lambda t: set_node(t, 2, 3)),
        "column far out of range": mutated(lambda t: set_node(t, 2, 0xFFFFFFFF)),
        "offset > 1": mutated(lambda t: set_node(t, 1, 2)),
        "a word too many": np.concatenate([good, [0]]).astype(np.uint32),
        "a word too few": good[:-1],
        "version-2 header cut short": good[:6],
        "preprocessed_width smaller than a used column": mutated(lambda t: t.__setitem__(6, 1)),
        "width == 0": mutated(lambda t: t.__setitem__(2, 0)),
        "version 3": mutated(lambda t: t.__setitem__(1, 3)),
    }
    for what, tape in bad.items():
        rc, msg = _compile_status(tape)
        assert rc == TS_ERR_INVALID and msg, what
    # declared and never referenced is fine, and so is a wider declaration
    assert _compile_status(mutated(lambda t: t.__setitem__(6, 7)))[0] == 0


def _oracle_fib_proof(orc):
    trace = generate_fibonacci_trace(0, 1, 8)
    pis = fibonacci_public_values(trace)
    tape = ts.air_tape(FibonacciAir(), 3)
    cfg = (1, 3, 1)
    return tape, pis, cfg, orc.prove(orc.FriConfig(*cfg), tape, trace, pis)


def _verify_pre(cfg, air_h, chal, root, words, pis, verdict=True):
    """ts_verify_pre with any argument None; `chal` is a BfChallenger (kept alive over the call) or None."""
    l = _lib.lib()
    chal_h = chal.h if chal is not None else None
    c = _lib.FriConfigC(*(cfg or (1, 1, 0)))
    v = C.c_int(-7)
    w = np.ascontiguousarray(words if words is not None else [], dtype=np.uint32)
    p = np.ascontiguousarray(pis, dtype=np.uint32)
    rc = l.ts_verify_pre(C.byref(c) if cfg else None, air_h, chal_h,
                         None if root is None else np.ascontiguousarray(root, dtype=np.uint32).ctypes.data_as(_lib.u32p),
                         None if words is None else w.ctypes.data_as(_lib.u32p), len(w) if words is not None else 0,
                         p.ctypes.data_as(_lib.u32p) if len(p) else None, len(p), C.byref(v) if verdict else None)
    return rc, v.value, (l.ts_last_error(None) or b"").decode()


def test_verify_pre_on_an_air_without_preprocessed_columns(orc):
    """ts_verify_pre with a null root is ts_verify but for the header: the oracle's TSPF v1 proof with the
    version word 3 and a zero preprocessed_width word is accepted, and every change ts_verify rejects is
    rejected."""
    tape, pis, cfg, v1 = _oracle_fib_proof(orc)
    v3 = np.concatenate([v1[:5], [0], v1[5:]]).astype(np.uint32)
    v3[1] = 3
    air = ts.CompiledAir(None, tape)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), None, host_only=True))
    ts.verify(config, air, ts.BfChallenger(), v1, pis)
    assert _verify_pre(cfg, air.h, ts.BfChallenger(), None, v3, pis)[:2] == (0, 0)
    bad = v3.copy()
    bad[30] ^= 1  # an opened value
    rc, verdict, _ = _verify_pre(cfg, air.h, ts.BfChallenger(), None, bad, pis)
    assert rc == 0 and verdict != 0
    with pytest.raises(ts.VerificationError):
        ts.verify(config, air, ts.BfChallenger(), np.concatenate([bad[:5], bad[6:]]) * 1, pis)
    # a proof of another version, or with another preprocessed width: refused as an argument, with the verdict
    rc, verdict, msg = _verify_pre(cfg, air.h, ts.BfChallenger(), None, v1, pis)
    assert (rc, verdict) == (TS_ERR_INVALID, 9) and "v3" in msg
    wrong_w = v3.copy()
    wrong_w[5] = 2
    rc, verdict, msg = _verify_pre(cfg, air.h, ts.BfChallenger(), None, wrong_w, pis)
    assert (rc, verdict) == (TS_ERR_INVALID, 1) and msg
    # and ts_verify refuses v3
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(config, air, ts.BfChallenger(), v3, pis)
    assert e.value.code == 9


def test_verify_pre_null_arguments_and_host_refusals(orc):
    tape, pis, cfg, v1 = _oracle_fib_proof(orc)
    v3 = np.concatenate([v1[:5], [0], v1[5:]]).astype(np.uint32)
    v3[1] = 3
    air = ts.CompiledAir(None, tape)
    chal = ts.BfChallenger()
    root = np.arange(8, dtype=np.uint32)
    cases = {
        "null config": (None, air.h, chal, None, v3, True),
        "null air": (cfg, None, chal, None, v3, True),
        "null challenger": (cfg, air.h, None, None, v3, True),
        "null proof": (cfg, air.h, chal, None, None, True),
        "null verdict": (cfg, air.h, chal, None, v3, False),
        "a root for an AIR without preprocessed columns": (cfg, air.h, chal, root, v3, True),
    }
    for what, (c, a, ch, r, w, v) in cases.items():
        rc, _, msg = _verify_pre(c, a, ch, r, w, pis, verdict=v)
        assert rc == TS_ERR_INVALID and msg, what
    sel = ts.CompiledAir(None, ts.air_tape(SelectorAir(), 2, 3))
    rc, _, msg = _verify_pre(cfg, sel.h, chal, None, v3, np.zeros(2, dtype=np.uint32))
    assert rc == TS_ERR_INVALID and "root" in msg  # null root for an AIR that has such columns
    # the host-only calls that take no root refuse such an AIR and say where to go
    l = _lib.lib()
    c = _lib.FriConfigC(*cfg)
    v = C.c_int(-1)
    z = np.zeros(2, dtype=np.uint32)
    rc = l.ts_verify(C.byref(c), sel.h, chal.h, v3.ctypes.data_as(_lib.u32p), len(v3), z.ctypes.data_as(_lib.u32p), 2,
                     C.byref(v))
    assert rc == TS_ERR_UNSUPPORTED and "ts_prove_pre" in (l.ts_last_error(None) or b"").decode()
    out = np.zeros(16 * len(v3), dtype=np.uint8)
    n = C.c_size_t()
    rc = l.ts_proof_to_postcard(v3.ctypes.data_as(_lib.u32p), len(v3), out.ctypes.data_as(C.POINTER(C.c_uint8)), len(out),
                                C.byref(n))
    assert rc == TS_ERR_UNSUPPORTED and (l.ts_last_error(None) or b"")


def test_null_arguments_of_the_accessor():
    l = _lib.lib()
    air = ts.CompiledAir(None, ts.air_tape(SelectorAir(), 2, 3))
    w = C.c_uint32(99)
    assert l.ts_air_preprocessed_width(None, C.byref(w)) == TS_ERR_INVALID
    assert l.ts_air_preprocessed_width(air.h, None) == TS_ERR_INVALID
    assert l.ts_air_preprocessed_width(air.h, C.byref(w)) == 0 and w.value == 3


def test_segment_plan_slots_no_load():
    """A version-2 AIR through the segment planner: no leaf (LOAD of either matrix, CONST, SEL) is slotted,
    and preprocessed LOADs do occur."""
    n_prep_loads = 0
    for seed in (1, 2, 3, 7, 11, 17):
        air, _ = random_air_case(seed)
        pw = prep_width(seed, air.width())
        cair = ts.CompiledAir(None, split_tape(ts.air_tape(air, air.n_public), pw), segment_instr=16)
        code = cair.program()["code"]
        n_prep_loads += int(((code[:, 0] == D_LOAD) & (code[:, 2] >= 2)).sum())
        plan = cair.segment_plan()
        assert len(plan["segments"]) > 1
        for sg in plan["segments"]:
            assert sg["end"] - sg["begin"] <= 16
            for v, _slot in sg["live_in"] + sg["live_out"]:
                assert code[v][0] in COMPUTED and code[v][0] != D_LOAD, seed
        # the segment sources name the preprocessed rows where they re-emit such a leaf
        src = cair.jit_source()
        assert src.count("k_quotient_seg") == len(plan["segments"])
        assert "prep_stride" in src
    assert n_prep_loads > 0
