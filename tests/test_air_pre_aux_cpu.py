"""AIRs with preprocessed AND challenge-phase (aux) columns on the CPU (no GPU): the lowering to a third matrix
(D_LOAD a = 4, 5), the emitted source, the host-only ts_verify_pre_aux and TSPF v5, the two capture front ends.
The frozen oracle knows one matrix, so every check goes through the joined AIR over hstack(pre, aux, main)
(tests/_pre_aux_airs.py).  The GPU half is tests/test_gpu_pre_aux.py."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.air import LogUp, aux_dims
from tapstark_amd.airs import (FibonacciAir, TableLookupAir, fibonacci_public_values, generate_fibonacci_trace,
                               generate_lookup_table, generate_table_lookup_trace, random_air_case, splitmix64_stream)
from _air_program import D_LOAD
from _aux_airs import logup_reference, split_counts
from _pre_aux_airs import join_tape_pre_aux, remap_logup, run_program6, split_tape_pre_aux, split_widths

P = 0x78000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_UNSUPPORTED = 1, 4
NEW_SYMBOLS = ("ts_prove_pre_aux", "ts_verify_pre_aux", "ts_quotient_chunks_pre_aux", "ts_check_constraints_pre_aux",
               "ts_logup_aux_build_pre")
# the seeds test_gpu_aux.py uses, restricted to AIRs wide enough for a three-way split
SEEDS = [s for s in range(36) if random_air_case(s)[0].width() >= 3]


def test_library_exports_and_header_declares_the_new_calls():
    l = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert name in _lib.ABI_SYMBOLS
        assert re.search(r"^ts_status " + name + r"\(", header, re.M), name
    assert l.ts_abi_version() == 5


def _rows(seed, w, m=8):
    vals = splitmix64_stream(seed + 177, 2 * m * w + 3 * m) % np.uint64(P)
    local = vals[:m * w].reshape(m, w).copy()
    nxt = vals[m * w:2 * m * w].reshape(m, w).copy()
    sels = vals[2 * m * w:].reshape(m, 3).copy()
    local[0, :] = 0
    nxt[0, :] = P - 1
    local[1, :] = P - 1
    sels[0] = (1, 0, 1)
    sels[1] = (0, 1, 0)
    return local, nxt, sels


def _program_digest(prog) -> str:
    h = hashlib.sha256()
    h.update(np.uint32(prog["n_regs"]).tobytes())
    for k in ("code", "consts", "const_public"):
        h.update(np.ascontiguousarray(prog[k], dtype=np.uint32).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("which", range(3))
def test_three_way_split_lowers_to_three_matrices(orc, which):
    """The lowered program of the (p, a, rest) split, run over six row arrays, is the joined tape's evaluation; the
    aux loads carry a = 4, 5, the preprocessed ones a = 2, 3, every column lies inside its matrix, and the public
    slots are public values ++ challenges ++ exposed."""
    n_aux_next = 0
    for seed in SEEDS:
        air, _ = random_air_case(seed)
        w = air.width()
        p, a = split_widths(seed, w, which)
        v1 = ts.air_tape(air, air.n_public)
        v3 = split_tape_pre_aux(v1, p, a)
        joined = join_tape_pre_aux(v3)
        keep, nc, ne = split_counts(air.n_public)
        cair = ts.CompiledAir(None, v3)
        assert (cair.width, cair.preprocessed_width, cair.aux_width) == (w - p - a, p, a), seed
        assert (cair.n_public, cair.n_challenges, cair.n_exposed) == (keep, nc, ne), seed
        assert cair.max_constraint_degree == orc.max_constraint_degree(joined), seed
        assert cair.log_quotient_degree == orc.log_quotient_degree(joined), seed
        prog = cair.program()
        loads = prog["code"][prog["code"][:, 0] == D_LOAD]
        assert (loads[:, 2] <= 5).all(), seed
        for base, width in ((0, w - p - a), (2, p), (4, a)):
            mine = loads[(loads[:, 2] >> 1) == (base >> 1)]
            assert (mine[:, 3] < width).all(), (seed, base)
        n_aux_next += int((loads[:, 2] == 5).any())
        slots = prog["const_public"][prog["const_public"] != 0xFFFFFFFF]
        assert (slots < keep + 4 * nc + ne).all(), seed
        local, nxt, sels = _rows(seed, w)
        pis = (splitmix64_stream(seed + 5, max(len(joined), 1)) % np.uint64(P))[:int(joined[3])]
        rows6 = (local[:, p + a:], nxt[:, p + a:], local[:, :p], nxt[:, :p], local[:, p:p + a], nxt[:, p:p + a])
        got = run_program6(prog, rows6, pis, sels, int(joined[5]))
        assert (got == orc.constraint_values(joined, local, nxt, pis, sels)).all(), f"seed {seed}: values differ"
    assert len(SEEDS) >= 25 and n_aux_next >= 5


def test_at_most_one_width_keeps_the_parent_program():
    """A pure-aux and a pure-preprocessed split of the same AIRs still load their second matrix with a = 2, 3, and
    program and emitted source are word for word what the library gave before a third matrix existed
    (tests/golden/pre_aux_parent_programs.json, made from that commit)."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pre_aux_parent_programs.json")))
    assert set(golden) == {str(s) for s in SEEDS}
    for seed in SEEDS:
        air, _ = random_air_case(seed)
        p, a = split_widths(seed, air.width(), 1)
        v1 = ts.air_tape(air, air.n_public)
        for key, tape in (("aux", split_tape_pre_aux(v1, 0, p + a)), ("pre", split_tape_pre_aux(v1, p + a, 0))):
            cair = ts.CompiledAir(None, tape)
            prog = cair.program()
            loads = prog["code"][prog["code"][:, 0] == D_LOAD]
            assert (loads[:, 2] <= 3).all() and (loads[:, 2] >= 2).any(), (seed, key)
            assert _program_digest(prog) == golden[str(seed)][key], (seed, key)
            src = cair.jit_source()
            assert hashlib.sha256(src.encode()).hexdigest() == golden[str(seed)]["jit_" + key], (seed, key)
            assert "aux_stride" not in src and "row4" not in src


def _both_tape(seed=6):
    air, _ = random_air_case(seed)
    p, a = split_widths(seed, air.width(), 1)
    return split_tape_pre_aux(ts.air_tape(air, air.n_public), p, a)


def test_jit_source_names_both_parameter_pairs():
    cair = ts.CompiledAir(None, _both_tape())
    src = cair.jit_source()
    assert "const u32* __restrict__ prep, u64 prep_stride, const u32* __restrict__ aux, u64 aux_stride" in src
    assert "row4 = aux + r;" in src and "row5 = aux + r_next;" in src
    assert re.search(r"row[45]\[\d+ull \* aux_stride\]", src) and re.search(r"row[23]\[\d+ull \* prep_stride\]", src)
    assert not re.search(r"row[45]\[\d+ull \* (prep|col)_stride\]", src)
    # the segmented kernels take the same pairs before their slab
    seg = ts.CompiledAir(None, _both_tape(), segment_instr=16)
    assert len(seg.segment_plan()["segments"]) > 1
    s = seg.jit_source()
    assert s.count("const u32* __restrict__ aux, u64 aux_stride, u32* __restrict__ slab, u32 slab_rows") == \
        len(seg.segment_plan()["segments"])


def _hiprtc_available() -> bool:
    for name in ("libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"):
        try:
            C.CDLL(name)
            return True
        except OSError:
            pass
    return False


def test_jit_source_compiles_for_gfx950():
    """hiprtc cross-compiles: no GPU needed.  Monolithic and segmented source, both parameter pairs in use."""
    if not _hiprtc_available():
        pytest.skip("hiprtc not available")
    for kw in ({}, {"segment_instr": 16}):
        code, seconds = ts.CompiledAir(None, _both_tape(), **kw).jit_compile("gfx950")
        assert len(code) > 64 and bytes(code[:4]) == b"\x7fELF"


# ------------------------------------------------------------------ ts_verify_pre_aux (host only)
def _verify_pre_aux(cfg, air_h, chal, root, words, pis, verdict=True, exposed=None):
    l = _lib.lib()
    c = _lib.FriConfigC(*(cfg or (1, 1, 0)))
    v = C.c_int(-7)
    w = np.ascontiguousarray(words if words is not None else [], dtype=np.uint32)
    p = np.ascontiguousarray(pis, dtype=np.uint32)
    r = None if root is None else np.ascontiguousarray(root, dtype=np.uint32)
    rc = l.ts_verify_pre_aux(C.byref(c) if cfg else None, air_h, chal.h if chal is not None else None,
                             None if r is None else r.ctypes.data_as(_lib.u32p),
                             None if words is None else w.ctypes.data_as(_lib.u32p), len(w),
                             p.ctypes.data_as(_lib.u32p) if len(p) else None, len(p),
                             None if exposed is None else exposed.ctypes.data_as(_lib.u32p),
                             0 if exposed is None else len(exposed), C.byref(v) if verdict else None)
    return rc, v.value, (l.ts_last_error(None) or b"").decode()


@pytest.fixture(scope="module")
def fib(orc):
    trace = generate_fibonacci_trace(0, 1, 8)
    pis = fibonacci_public_values(trace)
    tape = ts.air_tape(FibonacciAir(), 3)
    cfg = (1, 3, 1)
    v1 = orc.prove(orc.FriConfig(*cfg), tape, trace, pis)
    v5 = np.concatenate([v1[:5], [0, 0, 0, 0], v1[5:]]).astype(np.uint32)
    v5[1] = 5
    return tape, pis, cfg, v1, v5


def test_verify_pre_aux_on_an_air_with_neither_kind_of_column(fib):
    """All three widths 0, root NULL: ts_verify_pre_aux is ts_verify but for the header.  The oracle's TSPF v1 proof
    under the v5 header (version word 5, four zero words) is accepted and a changed opened value rejected."""
    tape, pis, cfg, v1, v5 = fib
    air = ts.CompiledAir(None, tape)
    assert _verify_pre_aux(cfg, air.h, ts.BfChallenger(), None, v5, pis)[:2] == (0, 0)
    bad = v5.copy()
    bad[33] ^= 1
    rc, verdict, _ = _verify_pre_aux(cfg, air.h, ts.BfChallenger(), None, bad, pis)
    assert rc == 0 and verdict not in (0, -1, -7)
    # a root for an AIR without preprocessed columns
    rc, _, msg = _verify_pre_aux(cfg, air.h, ts.BfChallenger(), np.zeros(8), v5, pis)
    assert rc == TS_ERR_INVALID and "root" in msg
    # another version: verdict 9; header words that are not the AIR's: verdict 1
    v3 = np.concatenate([v1[:5], [0], v1[5:]]).astype(np.uint32)
    v3[1] = 3
    v4 = np.concatenate([v1[:5], [0, 0, 0], v1[5:]]).astype(np.uint32)
    v4[1] = 4
    for other in (v1, v3, v4):
        rc, verdict, msg = _verify_pre_aux(cfg, air.h, ts.BfChallenger(), None, other, pis)
        assert (rc, verdict) == (TS_ERR_INVALID, 9) and "v5" in msg
    for k in (5, 6, 7, 8):
        wrong = v5.copy()
        wrong[k] = 1
        rc, verdict, msg = _verify_pre_aux(cfg, air.h, ts.BfChallenger(), None, wrong, pis)
        assert (rc, verdict) == (TS_ERR_INVALID, 1) and msg, k


def test_the_other_verify_calls_refuse_v5(fib):
    tape, pis, cfg, v1, v5 = fib
    air = ts.CompiledAir(None, tape)
    l, c, p = _lib.lib(), _lib.FriConfigC(*cfg), np.ascontiguousarray(pis, dtype=np.uint32)
    wp, pp = v5.ctypes.data_as(_lib.u32p), p.ctypes.data_as(_lib.u32p)
    chal = ts.BfChallenger()
    v = C.c_int(-1)
    assert l.ts_verify(C.byref(c), air.h, chal.h, wp, len(v5), pp, len(p), C.byref(v)) == 0 and v.value == 9
    v = C.c_int(-1)
    rc = l.ts_verify_pre(C.byref(c), air.h, ts.BfChallenger().h, None, wp, len(v5), pp, len(p), C.byref(v))
    assert (rc, v.value) == (TS_ERR_INVALID, 9)
    v = C.c_int(-1)
    rc = l.ts_verify_aux(C.byref(c), air.h, ts.BfChallenger().h, wp, len(v5), pp, len(p), None, 0, C.byref(v))
    assert (rc, v.value) == (TS_ERR_INVALID, 9)
    # the binding routes a v5 proof to ts_verify_pre_aux only together with a root
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), None, host_only=True))
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(config, air, ts.BfChallenger(), v5, pis)
    assert e.value.code == 9
    # v5 has no postcard form
    out, n = np.zeros(16 * len(v5), dtype=np.uint8), C.c_size_t()
    rc = l.ts_proof_to_postcard(wp, len(v5), out.ctypes.data_as(C.POINTER(C.c_uint8)), len(out), C.byref(n))
    assert rc == TS_ERR_UNSUPPORTED and b"v5" in (l.ts_last_error(None) or b"")


def test_verify_pre_aux_null_arguments_and_buffers(fib):
    tape, pis, cfg, v1, v5 = fib
    air = ts.CompiledAir(None, tape)
    chal = ts.BfChallenger()
    cases = {
        "null config": (None, air.h, chal, v5, True),
        "null air": (cfg, None, chal, v5, True),
        "null challenger": (cfg, air.h, None, v5, True),
        "null proof": (cfg, air.h, chal, None, True),
        "null verdict": (cfg, air.h, chal, v5, False),
    }
    for what, (c, a, ch, w, v) in cases.items():
        rc, _, msg = _verify_pre_aux(c, a, ch, None, w, pis, verdict=v)
        assert rc == TS_ERR_INVALID and msg, what
    lookup = ts.CompiledAir(None, ts.air_tape(TableLookupAir(), 0, 1, *aux_dims(TableLookupAir())))
    root = np.zeros(8, dtype=np.uint32)
    # an AIR with preprocessed columns needs the root; exposed words need a buffer that holds them
    rc, _, msg = _verify_pre_aux(cfg, lookup.h, chal, None, v5, [], exposed=np.zeros(4, dtype=np.uint32))
    assert rc == TS_ERR_INVALID and "root" in msg
    rc, _, msg = _verify_pre_aux(cfg, lookup.h, chal, root, v5, [])
    assert rc == TS_ERR_INVALID and "exposed" in msg
    rc, _, msg = _verify_pre_aux(cfg, lookup.h, chal, root, v5, [], exposed=np.zeros(3, dtype=np.uint32))
    assert rc == TS_ERR_INVALID and "exposed" in msg
    # the proof's header is not this AIR's
    rc, verdict, _ = _verify_pre_aux(cfg, lookup.h, chal, root, v5, [], exposed=np.zeros(4, dtype=np.uint32))
    assert (rc, verdict) == (TS_ERR_INVALID, 1)


def test_proof_parse_reads_v5():
    """A v5 word stream with every field present: widths w = 2, pw = 1, aw = 4, one exposed word, qd = 2, one FRI
    round, one query of four BatchOpenings.  Each field comes back as written."""
    w, pw, aw, ne, qd = 2, 1, 4, 1, 2
    ctr = iter(range(1000, 100000))
    take = lambda n: np.array([next(ctr) for _ in range(n)], dtype=np.uint32)
    parts = {"trace_commit": take(8), "aux_commit": take(8), "exposed": take(ne), "quotient_commit": take(8),
             "preprocessed_local": take(4 * pw), "preprocessed_next": take(4 * pw), "aux_local": take(4 * aw),
             "aux_next": take(4 * aw), "trace_local": take(4 * w), "trace_next": take(4 * w),
             "quotient_chunks": take(16 * qd)}
    words = [np.array([0x46505354, 5, 3, w, qd, aw, 2, ne, pw], dtype=np.uint32)] + list(parts.values())
    words.append(np.array([1], dtype=np.uint32))  # R
    commit = take(8)
    words += [commit, np.array([1], dtype=np.uint32)]  # Q
    rows = [take(pw), take(aw), take(w)] + [take(4) for _ in range(qd)]
    paths = [take(8 * 4) for _ in range(4)]
    q = [np.array([4], dtype=np.uint32)]
    for k, mats in enumerate(([rows[0]], [rows[1]], [rows[2]], rows[3:])):
        q.append(np.array([len(mats)], dtype=np.uint32))
        for m in mats:
            q += [np.array([len(m)], dtype=np.uint32), m]
        q += [np.array([4], dtype=np.uint32), paths[k]]
    step_vals, step_path = take(8), take(8 * 3)
    q += [step_vals, np.array([3], dtype=np.uint32), step_path]
    final = take(4)
    words += q + [final, np.array([77], dtype=np.uint32)]
    flat = np.concatenate(words).astype(np.uint32)
    pf = ts.Proof.parse(flat)
    assert (pf.version, pf.degree_bits, pf.preprocessed_width, pf.aux_width, pf.n_challenges) == (5, 3, pw, aw, 2)
    for name in ("trace_commit", "aux_commit", "exposed", "quotient_commit"):
        assert (getattr(pf, name) == parts[name]).all(), name
    for name in ("preprocessed_local", "preprocessed_next", "aux_local", "aux_next", "trace_local", "trace_next"):
        assert (getattr(pf, name).reshape(-1) == parts[name]).all(), name
    assert (pf.quotient_chunks.reshape(-1) == parts["quotient_chunks"]).all()
    assert (pf.commit_phase_commits == commit.reshape(1, 8)).all()
    (qp,) = pf.query_proofs
    assert len(qp.input_proof) == 4
    assert [len(b.opened_values) for b in qp.input_proof] == [1, 1, 1, qd]
    assert (qp.input_proof[0].opened_values[0] == rows[0]).all() and (qp.input_proof[1].opened_values[0] == rows[1]).all()
    assert all((b.opening_proof.reshape(-1) == paths[k]).all() for k, b in enumerate(qp.input_proof))
    assert (pf.final_poly == final).all() and pf.pow_witness == 77
    with pytest.raises(ValueError):
        ts.Proof.parse(flat[:-1])
    with pytest.raises(ValueError):
        ts.Proof.parse(np.concatenate([flat, [0]]).astype(np.uint32))


# ------------------------------------------------------------------ LogUp with table terms, TableLookupAir
def test_logup_accepts_prep_terms():
    lu = TableLookupAir.logup
    assert lu.interactions == [((0, 1), [(1, 0)]), ((1, 1), [(2, 0)])] and lu.reads_preprocessed
    assert (lu.aux_width, lu.n_groups) == (8, 1)
    assert not LogUp([(("const", 1), [("col", 0)])]).reads_preprocessed
    # ts_logup_aux_width keeps its limits: kind 2 is ts_logup_aux_build_pre's alone
    l, w = _lib.lib(), C.c_uint32()
    spec, keep = lu._spec_c()
    assert l.ts_logup_aux_width(C.byref(spec), C.byref(w)) == TS_ERR_INVALID


@pytest.mark.parametrize("n", [2, 4, 64])
def test_table_lookup_constraints_determine_the_aux_matrix(orc, n):
    """The version-3 tape with both widths, joined over hstack(table, aux, main): a true lookup satisfies it with
    sum zero, a changed aux word, multiplicity, table entry or sum does not; and the aux matrix is that of the
    remapped spec on hstack(trace, table)."""
    air = TableLookupAir()
    tape = ts.air_tape(air, 0, 1, *aux_dims(air))
    assert list(tape[:10]) == [0x54415354, 3, 2, 0, int(tape[4]), 16, 1, 8, 2, 4]
    joined = join_tape_pre_aux(tape)
    assert orc.max_constraint_degree(joined) == 3
    cair = ts.CompiledAir(None, tape)
    assert (cair.width, cair.preprocessed_width, cair.aux_width, cair.log_quotient_degree) == (2, 1, 8, 1)
    trace, table = generate_table_lookup_trace(n), generate_lookup_table(n)
    ch = (splitmix64_stream(9 + n, 8) % np.uint64(P)).astype(np.uint32)
    remapped = remap_logup(air.logup.interactions, trace.shape[1])
    assert remapped == [((0, 1), [(1, 0)]), ((1, 1), [(1, 2)])]
    aux, S = logup_reference(remapped, np.hstack([trace, table]), ch[:4], ch[4:])
    assert not S.any(), "a true lookup sums to zero"
    check = lambda tb, a, t, s: orc.check_constraints(joined, np.hstack([tb, a, t]).astype(np.uint32),
                                                      np.concatenate([ch, s]).astype(np.uint32))
    assert check(table, aux, trace, S) == -1
    for r, c in ((0, 0), (n - 1, 3), (n // 2, 4), (n - 1, 7)):
        bad = aux.copy()
        bad[r, c] = (int(bad[r, c]) + 1) % P
        assert check(table, bad, trace, S) >= 0, (r, c)
    bad_t = trace.copy()
    bad_t[n - 1, 1] = (int(bad_t[n - 1, 1]) + 1) % P
    assert check(table, aux, bad_t, S) >= 0
    bad_tb = table.copy()
    bad_tb[n // 2, 0] += 1
    assert check(bad_tb, aux, trace, S) >= 0
    out = generate_table_lookup_trace(n, outside_row=n - 1)
    aux_o, S_o = logup_reference(remapped, np.hstack([out, table]), ch[:4], ch[4:])
    assert check(table, aux_o, out, S_o) == -1 and S_o.any()


def test_cpp_capture_emits_the_python_tape(tmp_path):
    """examples/table_lookup_air.cpp builds with plain g++ and its --tape (no GPU) is air.py's tape word for word."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "table_lookup_air")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "table_lookup_air.cpp"), "-L", libdir, "-ltapstark_hip",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe, "--tape"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = np.array([int(x) for x in r.stdout.split()], dtype=np.uint32)
    air = TableLookupAir()
    want = ts.air_tape(air, 0, 1, *aux_dims(air))
    assert len(got) == len(want) and (got == want).all()
