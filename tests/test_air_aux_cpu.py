"""AIRs with challenge-phase (aux) columns on the CPU (no GPU): tape version 3 through the product's validation,
degree rules and lowering, ExtExpr and the LogUp constraints against Python integers, and the host-only
ts_verify_aux.  The frozen oracle knows version 1 only, so every check goes through the joined AIR over
hstack(aux, main) with the public vector pis ++ challenges ++ exposed (tests/_aux_airs.py).  The GPU half is
tests/test_gpu_aux.py."""
import ctypes as C

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.air import ExtExpr, LogUp, SymbolicAirBuilder, aux_dims
from tapstark_amd.airs import (FibonacciAir, RangeLookupAir, SelectorAir, fibonacci_public_values,
                               generate_fibonacci_trace, generate_range_lookup_trace, random_air_case,
                               splitmix64_stream)
from _air_program import D_CONST, D_LOAD, run_program
from _aux_airs import (aux_width_of, ef_add, ef_mul, ef_inv, ef_scale, ef_sub, join_program_aux, join_tape_aux,
                       logup_reference, split_counts, split_tape_aux)

P = 0x78000001
TS_ERR_INVALID, TS_ERR_UNSUPPORTED = 1, 4
SEEDS = [s for s in range(36) if random_air_case(s)[0].width() >= 2]


def _compile_status(tape):
    l = _lib.lib()
    h = C.c_void_p()
    t = np.ascontiguousarray(tape, dtype=np.uint32)
    rc = l.ts_air_compile(None, t.ctypes.data_as(_lib.u32p), len(t), C.byref(h))
    msg = (l.ts_last_error(None) or b"").decode()
    if rc == 0:
        l.ts_air_free(None, h)
    return rc, msg


def _lookup_tape():
    air = RangeLookupAir()
    return ts.air_tape(air, 0, 0, *aux_dims(air))


# ------------------------------------------------------------------ tape version 3
def test_split_set_is_what_the_tests_lean_on():
    n_chal = n_exp = 0
    for seed in SEEDS:
        air, _ = random_air_case(seed)
        _, nc, ne = split_counts(air.n_public)
        n_chal += nc > 0
        n_exp += ne > 0
    assert len(SEEDS) >= 33 and n_chal >= 12 and n_exp >= 2


def test_version_3_rejections():
    good = _lookup_tape()
    assert good[1] == 3 and list(good[6:10]) == [0, 8, 2, 4] and _compile_status(good)[0] == 0
    n_nodes = int(good[4])
    nodes = good[10:10 + 3 * n_nodes].reshape(n_nodes, 3)
    at = {op: int(np.flatnonzero(nodes[:, 0] == op)[0]) for op in (11, 12, 13)}

    def mutated(f):
        t = good.copy()
        f(t)
        return t

    def set_node(op, field, value):
        return mutated(lambda t: t.__setitem__(10 + 3 * at[op] + field, value))

    def as_version(v):  # the same nodes under a version-1 or version-2 header
        head = list(good[:6]) + ([0] if v == 2 else [])
        head[1] = v
        return np.concatenate([np.asarray(head, dtype=np.uint32), good[10:]]).astype(np.uint32)

    def only(op, v):  # a version-v tape whose one new leaf is `op` (the others become constants)
        t = as_version(v)
        hdr = 6 if v == 1 else 7
        nd = t[hdr:hdr + 3 * n_nodes].reshape(n_nodes, 3)
        for other in (11, 12, 13):
            if other != op:
                nd[nd[:, 0] == other] = (0, 1, 0)
        return t

    bad = {
        "AUX in a version-1 tape": only(11, 1), "AUX in a version-2 tape": only(11, 2),
        "CHALLENGE in a version-1 tape": only(12, 1), "CHALLENGE in a version-2 tape": only(12, 2),
        "EXPOSED in a version-1 tape": only(13, 1), "EXPOSED in a version-2 tape": only(13, 2),
        "aux column >= aux_width": set_node(11, 2, 8),
        "aux column far out of range": set_node(11, 2, 0xFFFFFFFF),
        "aux offset > 1": set_node(11, 1, 2),
        "challenge word >= 4 n_challenges": set_node(12, 1, 8),
        "exposed index >= n_exposed": set_node(13, 1, 4),
        "aux_width smaller than a used column": mutated(lambda t: t.__setitem__(7, 4)),
        "n_challenges smaller than a used word": mutated(lambda t: t.__setitem__(8, 1)),
        "n_exposed smaller than a used index": mutated(lambda t: t.__setitem__(9, 3)),
        "a word too many": np.concatenate([good, [0]]).astype(np.uint32),
        "a word too few": good[:-1],
        "version-3 header cut short": good[:9],
        "version 4": mutated(lambda t: t.__setitem__(1, 4)),
    }
    for what, tape in bad.items():
        rc, msg = _compile_status(tape)
        assert rc == TS_ERR_INVALID and msg, what
    # the controls: the mutation helpers alone do not break a tape
    assert _compile_status(set_node(11, 2, 7))[0] == 0
    assert _compile_status(mutated(lambda t: t.__setitem__(7, 12)))[0] == 0
    # a version-2 tape under the version word 3 is still invalid by its length
    v2 = ts.air_tape(SelectorAir(), 2, 3)
    v2[1] = 3
    assert _compile_status(v2)[0] == TS_ERR_INVALID


def test_versions_1_and_2_are_what_they_were():
    """A builder with no aux columns, challenges or exposed words emits the tape it always did."""
    for air, k, pw in ((FibonacciAir(), 3, 0), (SelectorAir(), 2, 3)):
        a = ts.air_tape(air, k, pw)
        b = ts.air_tape(air, k, pw, 0, 0, 0)
        assert (a == b).all() and a[1] == (2 if pw else 1)
    cair = ts.CompiledAir(None, ts.air_tape(FibonacciAir(), 3))
    assert (cair.aux_width, cair.n_challenges, cair.n_exposed) == (0, 0, 0)


def test_preprocessed_and_aux_together_compile():
    b = SymbolicAirBuilder(2, 1, preprocessed_width=1, aux_width=4, n_challenges=1, n_exposed=1)
    x = b.preprocessed().row_slice(0)[0] * b.aux().row_slice(1)[3] * b.main().row_slice(0)[1]
    b.assert_zero(x - b.exposed()[0] * b.challenges()[0].c[2] + b.public_values()[0])
    cair = ts.CompiledAir(None, b.tape())
    assert (cair.preprocessed_width, cair.aux_width, cair.n_challenges, cair.n_exposed) == (1, 4, 1, 1)
    assert cair.max_constraint_degree == 3 and cair.log_quotient_degree == 1


def test_aux_info_null_arguments():
    l = _lib.lib()
    cair = ts.CompiledAir(None, _lookup_tape())
    a, c, e = C.c_uint32(9), C.c_uint32(9), C.c_uint32(9)
    assert l.ts_air_aux_info(None, C.byref(a), C.byref(c), C.byref(e)) == TS_ERR_INVALID
    assert l.ts_air_aux_info(cair.h, C.byref(a), None, C.byref(e)) == 0 and (a.value, e.value) == (8, 4)
    assert l.ts_air_aux_info(cair.h, None, C.byref(c), None) == 0 and c.value == 2


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


@pytest.mark.parametrize("chunk", range(4))
def test_degree_rules_and_lowered_program(orc, chunk):
    """Degrees equal the oracle's for the joined tape; the lowered program IS the joined tape's program but for
    the documented mapping: AUX loads take a = 2, 3, main loads keep their (shifted) column, and CHALLENGE /
    EXPOSED take the public slots n_public + k and n_public + 4 n_challenges + e."""
    for seed in SEEDS[chunk::4]:
        air, _ = random_air_case(seed)
        w, A = air.width(), aux_width_of(seed, air.width())
        v1 = ts.air_tape(air, air.n_public)
        v3 = split_tape_aux(v1, A)
        joined = join_tape_aux(v3)
        keep, nc, ne = split_counts(air.n_public)
        cair = ts.CompiledAir(None, v3)
        assert (cair.width, cair.aux_width, cair.n_public, cair.n_challenges, cair.n_exposed) == (w - A, A, keep, nc, ne)
        assert cair.preprocessed_width == 0
        assert cair.max_constraint_degree == orc.max_constraint_degree(joined), seed
        assert cair.log_quotient_degree == orc.log_quotient_degree(joined), seed
        prog, want = cair.program(), ts.CompiledAir(None, joined).program()
        mapped = join_program_aux(prog, A)
        assert prog["n_regs"] == want["n_regs"] and (mapped["code"] == want["code"]).all(), seed
        assert (prog["consts"] == want["consts"]).all() and (prog["const_public"] == want["const_public"]).all(), seed
        loads = prog["code"][prog["code"][:, 0] == D_LOAD]
        assert (loads[:, 2] <= 3).all() and (loads[loads[:, 2] >= 2, 3] < A).all(), seed
        assert (loads[loads[:, 2] < 2, 3] < w - A).all(), seed
        slots = prog["const_public"][prog["const_public"] != 0xFFFFFFFF]
        assert (slots < keep + 4 * nc + ne).all(), seed
        # and it computes the oracle's constraint values on seeded rows
        local, nxt, sels = _rows(seed, w)
        pis = (splitmix64_stream(seed + 5, max(len(joined), 1)) % np.uint64(P))[:int(joined[3])]
        got = run_program(mapped, local, nxt, pis, sels, int(joined[5]))
        assert (got == orc.constraint_values(joined, local, nxt, pis, sels)).all(), seed


# ------------------------------------------------------------------ ExtExpr
EDGE = [(0, 0, 0, 0), (1, 0, 0, 0), (P - 1, P - 1, P - 1, P - 1), (0, 1, 0, P - 1), (P - 1, 0, 1, 0)]


def test_ext_expr_against_python_integers(orc):
    """x, y from aux columns, z from a challenge, e from exposed words, b a main column: the four coefficient
    constraints of each ExtExpr formula are the Python-integer EF4 value, at operands with coefficients 0, 1, p-1
    and at seeded ones."""
    b = SymbolicAirBuilder(1, 0, aux_width=8, n_challenges=1, n_exposed=4)
    aux = b.aux().row_slice(0)
    x, y = ExtExpr(b, aux[0:4]), ExtExpr(b, [aux[k] for k in range(4, 8)])
    z, e, base = b.challenges()[0], ExtExpr(b, b.exposed()), b.main().row_slice(0)[0]
    formulas = [
        (x + y, lambda X, Y, Z, E, B: ef_add(X, Y)),
        (x - y, lambda X, Y, Z, E, B: ef_sub(X, Y)),
        (x * y, lambda X, Y, Z, E, B: ef_mul(X, Y)),
        (x * y * z - e, lambda X, Y, Z, E, B: ef_sub(ef_mul(ef_mul(X, Y), Z), E)),
        (x.mul_base(base) + 3, lambda X, Y, Z, E, B: ef_add(ef_scale(X, B), (3, 0, 0, 0))),
        (-(x * base) + z * z, lambda X, Y, Z, E, B: ef_sub(ef_mul(Z, Z), ef_scale(X, B))),
        (5 - x * 7, lambda X, Y, Z, E, B: ef_sub((5, 0, 0, 0), ef_scale(X, 7))),
    ]
    for f, _ in formulas:
        b.assert_zero_ext(f)
    assert len(b.constraints) == 4 * len(formulas)
    joined = join_tape_aux(b.tape())
    rnd = (splitmix64_stream(77, 17 * 6) % np.uint64(P)).reshape(6, 17)
    ops = [(EDGE[i], EDGE[(i + 1) % 5], EDGE[(i + 2) % 5], EDGE[(i + 3) % 5], (0, 1, P - 1, 5, 7)[i]) for i in range(5)]
    ops += [(tuple(r[0:4]), tuple(r[4:8]), tuple(r[8:12]), tuple(r[12:16]), r[16]) for r in rnd.tolist()]
    for X, Y, Z, E, B in ops:
        local = np.array([list(X) + list(Y) + [B]], dtype=np.uint64)
        pis = np.array(list(Z) + list(E), dtype=np.uint64)
        got = orc.constraint_values(joined, local, local, pis, np.array([[1, 0, 1]], dtype=np.uint64))[0]
        want = [c for _, g in formulas for c in g(X, Y, Z, E, int(B))]
        assert got.tolist() == want, (X, Y, Z, E, B)


def test_python_ef4_inverse():
    for a in EDGE[1:] + [(5, 7, P - 1, 123456), (0, 0, 1, 0), (0, 0, 0, 1)]:
        assert ef_mul(a, ef_inv(a)) == (1, 0, 0, 0)


# ------------------------------------------------------------------ the LogUp constraints
@pytest.mark.parametrize("n", [2, 4, 64])
def test_logup_constraints_determine_the_aux_matrix(orc, n):
    air = RangeLookupAir()
    joined = join_tape_aux(_lookup_tape())
    assert orc.max_constraint_degree(joined) == 3
    trace = generate_range_lookup_trace(n)
    ch = (splitmix64_stream(9 + n, 8) % np.uint64(P)).astype(np.uint32)
    aux, S = logup_reference(air.logup.interactions, trace, ch[:4], ch[4:])
    assert not S.any(), "a true lookup sums to zero"
    check = lambda a, t, s: orc.check_constraints(joined, np.hstack([a, t]).astype(np.uint32),
                                                  np.concatenate([ch, s]).astype(np.uint32))
    assert check(aux, trace, S) == -1
    for r, c in ((0, 0), (n - 1, 3), (n // 2, 4), (n - 1, 7)):  # a word of h, of phi
        bad = aux.copy()
        bad[r, c] = (int(bad[r, c]) + 1) % P
        assert check(bad, trace, S) >= 0, (r, c)
    bad_t = trace.copy()
    bad_t[n - 1, 2] = (int(bad_t[n - 1, 2]) + 1) % P  # one multiplicity
    assert check(aux, bad_t, S) >= 0
    bad_S = S.copy()
    bad_S[2] = 1
    assert check(aux, trace, bad_S) >= 0
    LogUp.verify(S)
    with pytest.raises(ValueError):
        LogUp.verify(bad_S)
    # a value outside the table: the constraints still hold for the aux matrix built from it, the sum is not zero
    out = generate_range_lookup_trace(n, outside_row=n - 1)
    aux_o, S_o = logup_reference(air.logup.interactions, out, ch[:4], ch[4:])
    assert check(aux_o, out, S_o) == -1 and S_o.any()


def test_logup_helper_shapes():
    one = LogUp([(("const", P - 1), [("col", 0), ("const", 5), ("col", 1)])])
    assert (one.aux_width, one.n_groups) == (8, 1)
    three = LogUp([(("const", 1), [("col", 0)])] * 3)
    assert (three.aux_width, three.n_groups) == (12, 2)
    l = _lib.lib()
    w = C.c_uint32()
    for lu in (one, three, RangeLookupAir.logup):
        spec, keep = lu._spec_c()
        assert l.ts_logup_aux_width(C.byref(spec), C.byref(w)) == 0 and w.value == lu.aux_width
    # the limits: 16 interactions, 8 values, kinds 0 / 1
    for bad in (LogUp([(("const", 1), [("col", 0)])] * 17), LogUp([(("const", 1), [("col", 0)] * 9)]),
                LogUp([((2, 1), [("col", 0)])])):
        spec, keep = bad._spec_c()
        assert l.ts_logup_aux_width(C.byref(spec), C.byref(w)) == TS_ERR_INVALID
    assert l.ts_logup_aux_width(None, C.byref(w)) == TS_ERR_INVALID


# ------------------------------------------------------------------ ts_verify_aux (host only)
def _verify_aux(cfg, air_h, chal, words, pis, verdict=True, exposed=None):
    l = _lib.lib()
    c = _lib.FriConfigC(*(cfg or (1, 1, 0)))
    v = C.c_int(-7)
    w = np.ascontiguousarray(words if words is not None else [], dtype=np.uint32)
    p = np.ascontiguousarray(pis, dtype=np.uint32)
    rc = l.ts_verify_aux(C.byref(c) if cfg else None, air_h, chal.h if chal is not None else None,
                         None if words is None else w.ctypes.data_as(_lib.u32p), len(w),
                         p.ctypes.data_as(_lib.u32p) if len(p) else None, len(p),
                         None if exposed is None else exposed.ctypes.data_as(_lib.u32p),
                         0 if exposed is None else len(exposed), C.byref(v) if verdict else None)
    return rc, v.value, (l.ts_last_error(None) or b"").decode()


def _oracle_fib_proof(orc):
    trace = generate_fibonacci_trace(0, 1, 8)
    pis = fibonacci_public_values(trace)
    tape = ts.air_tape(FibonacciAir(), 3)
    cfg = (1, 3, 1)
    return tape, pis, cfg, orc.prove(orc.FriConfig(*cfg), tape, trace, pis)


def test_verify_aux_on_an_air_without_aux_columns(orc):
    """ts_verify_aux on an AIR with aux_width 0 is ts_verify but for the header: the oracle's TSPF v1 proof under
    the v4 header (version word 4, three zero words) is accepted, and a changed opened value is rejected."""
    tape, pis, cfg, v1 = _oracle_fib_proof(orc)
    v4 = np.concatenate([v1[:5], [0, 0, 0], v1[5:]]).astype(np.uint32)
    v4[1] = 4
    air = ts.CompiledAir(None, tape)
    assert _verify_aux(cfg, air.h, ts.BfChallenger(), v4, pis)[:2] == (0, 0)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), None, host_only=True))
    exposed = ts.verify(config, air, ts.BfChallenger(), v4, pis)
    assert exposed is not None and len(exposed) == 0
    assert ts.verify(config, air, ts.BfChallenger(), v1, pis) is None
    bad = v4.copy()
    bad[32] ^= 1
    rc, verdict, _ = _verify_aux(cfg, air.h, ts.BfChallenger(), bad, pis)
    assert rc == 0 and verdict != 0
    # a v1 or v3 proof: verdict 9; header words that disagree with the AIR: verdict 1
    v3 = np.concatenate([v1[:5], [0], v1[5:]]).astype(np.uint32)
    v3[1] = 3
    for other in (v1, v3):
        rc, verdict, msg = _verify_aux(cfg, air.h, ts.BfChallenger(), other, pis)
        assert (rc, verdict) == (TS_ERR_INVALID, 9) and "v4" in msg
    for k in (5, 6, 7):
        wrong = v4.copy()
        wrong[k] = 1
        rc, verdict, msg = _verify_aux(cfg, air.h, ts.BfChallenger(), wrong, pis)
        assert (rc, verdict) == (TS_ERR_INVALID, 1) and msg, k
    # ts_verify refuses v4, and v4 has no postcard form
    with pytest.raises(ts.VerificationError) as e:
        _raise_verdict(config, air, v4, pis)
    assert e.value.code == 9
    l = _lib.lib()
    out, n = np.zeros(16 * len(v4), dtype=np.uint8), C.c_size_t()
    rc = l.ts_proof_to_postcard(v4.ctypes.data_as(_lib.u32p), len(v4), out.ctypes.data_as(C.POINTER(C.c_uint8)), len(out),
                                C.byref(n))
    assert rc == TS_ERR_UNSUPPORTED and (l.ts_last_error(None) or b"")
    pf = ts.Proof.parse(v4)
    assert pf.version == 4 and pf.aux_width == 0 and pf.aux_commit is None and len(pf.aux_local) == 0


def _raise_verdict(config, air, words, pis):
    """ts_verify itself (the binding's verify routes a v4 proof to ts_verify_aux)."""
    l = _lib.lib()
    cfg = config.pcs.fri._c()
    v, chal = C.c_int(-1), ts.BfChallenger()  # (the challenger outlives the call)
    p = np.ascontiguousarray(pis, dtype=np.uint32)
    rc = l.ts_verify(C.byref(cfg), air.h, chal.h, words.ctypes.data_as(_lib.u32p), len(words),
                     p.ctypes.data_as(_lib.u32p), len(p), C.byref(v))
    assert rc == 0
    raise ts.VerificationError(v.value)


def test_verify_aux_null_arguments_and_host_refusals(orc):
    tape, pis, cfg, v1 = _oracle_fib_proof(orc)
    v4 = np.concatenate([v1[:5], [0, 0, 0], v1[5:]]).astype(np.uint32)
    v4[1] = 4
    air = ts.CompiledAir(None, tape)
    chal = ts.BfChallenger()
    cases = {
        "null config": (None, air.h, chal, v4, True),
        "null air": (cfg, None, chal, v4, True),
        "null challenger": (cfg, air.h, None, v4, True),
        "null proof": (cfg, air.h, chal, None, True),
        "null verdict": (cfg, air.h, chal, v4, False),
    }
    for what, (c, a, ch, w, v) in cases.items():
        rc, _, msg = _verify_aux(c, a, ch, w, pis, verdict=v)
        assert rc == TS_ERR_INVALID and msg, what
    lookup = ts.CompiledAir(None, _lookup_tape())
    # exposed words need a buffer
    rc, _, msg = _verify_aux(cfg, lookup.h, chal, v4, [])
    assert rc == TS_ERR_INVALID and "exposed" in msg
    rc, _, msg = _verify_aux(cfg, lookup.h, chal, v4, [], exposed=np.zeros(3, dtype=np.uint32))
    assert rc == TS_ERR_INVALID and "exposed" in msg
    # the proof's header is not this AIR's
    rc, verdict, _ = _verify_aux(cfg, lookup.h, chal, v4, [], exposed=np.zeros(4, dtype=np.uint32))
    assert (rc, verdict) == (TS_ERR_INVALID, 1)
    # the host-only calls that take no aux source refuse such an AIR and say where to go
    l = _lib.lib()
    c = _lib.FriConfigC(*cfg)
    v = C.c_int(-1)
    rc = l.ts_verify(C.byref(c), lookup.h, chal.h, v4.ctypes.data_as(_lib.u32p), len(v4), None, 0, C.byref(v))
    assert rc == TS_ERR_UNSUPPORTED and "ts_prove_aux" in (l.ts_last_error(None) or b"").decode()
    rc = l.ts_verify_pre(C.byref(c), lookup.h, chal.h, None, v4.ctypes.data_as(_lib.u32p), len(v4), None, 0, C.byref(v))
    assert rc == TS_ERR_UNSUPPORTED and "ts_prove_aux" in (l.ts_last_error(None) or b"").decode()
    # preprocessed and aux columns together: every aux call refuses
    b = SymbolicAirBuilder(1, 0, preprocessed_width=1, aux_width=4)
    b.assert_zero(b.preprocessed().row_slice(0)[0] - b.aux().row_slice(0)[0])
    both = ts.CompiledAir(None, b.tape())
    rc, _, msg = _verify_aux(cfg, both.h, chal, v4, [])
    assert rc == TS_ERR_UNSUPPORTED and msg
