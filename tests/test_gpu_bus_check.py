"""``ts_bus_check`` and ``ts_check_multi`` on the GPU: every report is compared field by field, shares included, with
the Python model of tests/_bus_check_cases.py (integers and a dictionary).  The statements are those of the bus and
key proofs (tests/_bus_cases.py, tests/_key_cases.py) and hand-made ones at the places where a hash join can go wrong:
zero padding, sums past p, the order of the first contribution, multiplicity words, probe chains, heights 1 and 2,
a table that is not on the bus, the widest spec.  The CPU half is tests/test_bus_check_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import _bus_cases as bc
import _bus_check_cases as m
import _key_cases as kc
import _poison
import tapstark_amd as ts
from tapstark_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = m.P
TS_ERR_INVALID = 1
CHALLENGES = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)  # any gamma, beta


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def run(ctx, tables):
    """(report, [(DeviceMatrix, uploaded array) ...]) of model tables on ``ctx``."""
    logups = [t[0] for t in tables]
    traces = [ts.DeviceMatrix.upload(ctx, t[1].copy()) for t in tables]
    pres = [ts.DeviceMatrix.upload(ctx, t[2].copy()) if t[2] is not None else None for t in tables]
    rep = ts.bus_check(logups, traces, pres if any(p is not None for p in pres) else None)
    return rep, list(zip(traces, [t[1] for t in tables])) + [(p, t[2]) for p, t in zip(pres, tables) if p is not None]


def check(ctx, tables, what=""):
    """The report equals the model's, and every matrix downloaded afterwards equals its upload."""
    rep, mats = run(ctx, tables)
    want = m.model(tables)
    got = rep.asdict()
    for field in want:
        assert got[field] == want[field], f"{what}: {field}: {got[field]} for {want[field]}"
    assert rep.balanced == (want["n_unbalanced"] == 0)
    for dm, up in mats:
        assert (dm.download() == up).all(), f"{what}: a matrix was written"
    return rep


def as_arrays(rep):
    """A report as integers only (None -> -1), for _poison.same_everywhere."""
    d = rep.asdict()
    first = list(d["first"]) if d["first"] is not None else [-1, -1, -1]
    shares = [[c, s, *(f if f is not None else (-1, -1))] for c, s, f in d["shares"]]
    return [d["n_contributions"], d["n_tuples"], d["n_unbalanced"], first, d["n_values"], d["tuple"], d["sum"], shares]


# ------------------------------------------------------------------ 1. the statements of the bus and key proofs
@pytest.mark.parametrize("name", ["a", "b", "c", "e", "t1"])
def test_balanced_bus_cases(ctx, name):
    tables = bc.case(name)
    rep = check(ctx, m.from_cases(tables), name)
    assert rep.n_unbalanced == 0 and rep.balanced and rep.first is None
    if name == "a":
        cfg = bc.config(ctx, 1)
        _, bus_sum = bc.verify(cfg, tables, bc.prove(cfg, bc.compiled(ctx, tables), tables))
        assert not bus_sum.any()


@pytest.mark.parametrize("name", ["ka", "kb", "kc", "kt1"])
def test_balanced_key_cases_with_the_keys_values(ctx, name):
    tables = kc.case(name)
    cfg = kc.config(ctx, 1)
    key = kc.make_key(cfg, tables)
    values, ki = [], 0
    for t in tables:
        values.append(key.values(ki) if t.key is not None else None)
        ki += t.key is not None
    traces = [ts.DeviceMatrix.upload(ctx, t.trace.copy()) for t in tables]
    rep = ts.bus_check([t.logup for t in tables], traces, values)
    want = m.model(m.from_cases(tables))
    assert rep.asdict() == want and rep.balanced
    for dm, t in zip(traces, tables):
        assert (dm.download() == t.trace).all()
    for v, t in zip(values, tables):
        assert v is None or (v.download() == t.key).all()
    if name == "ka":
        _, bus_sum = kc.verify(cfg, key.root, tables, kc.prove(cfg, key, kc.compiled(ctx, tables), tables))
        assert not bus_sum.any()


def test_no_table_on_the_bus(ctx):
    """Case k0 has no aux table: every spec is NULL, which ts_bus_check refuses; ts_check_multi answers it with the
    empty balanced report."""
    tables = kc.case("k0")
    traces = [ts.DeviceMatrix.upload(ctx, t.trace.copy()) for t in tables]
    with pytest.raises(_lib.TsError) as e:
        ts.bus_check([None] * len(tables), traces)
    assert e.value.code == TS_ERR_INVALID and "every spec is null" in str(e.value)
    cfg = kc.config(ctx, 1)
    key = kc.make_key(cfg, tables)
    bad, fv, rep = ts.check_multi(key, kc.compiled(ctx, tables), traces, [t.pis for t in tables],
                                  [t.logup for t in tables], CHALLENGES)
    assert (bad, fv) == (-1, -1) and rep.balanced
    assert rep.asdict() == {"n_contributions": 0, "n_tuples": 0, "n_unbalanced": 0, "first": None, "n_values": 0,
                            "tuple": [0] * 8, "sum": 0, "shares": [(0, 0, None)] * len(tables)}


UNBALANCED = {"n_unbalanced": 1, "first": (0, 3, 0), "n_values": 2, "tuple": [7, 32, 0, 0, 0, 0, 0, 0], "sum": 1,
              "shares": [(1, 1, (3, 0)), (0, 0, None)]}


def test_unbalanced_bus_case(ctx):
    tables = bc.case("unbalanced")
    got = check(ctx, m.from_cases(tables), "unbalanced").asdict()
    for field, want in UNBALANCED.items():
        assert got[field] == want, field
    cfg = bc.config(ctx, 1)
    _, bus_sum = bc.verify(cfg, tables, bc.prove(cfg, bc.compiled(ctx, tables), tables), check_bus=False)
    assert bus_sum.any()


def test_unbalanced_key_case(ctx):
    tables = kc.case("unbalanced")
    got = check(ctx, m.from_cases(tables), "unbalanced key").asdict()
    for field, want in UNBALANCED.items():
        assert got[field] == want, field
    cfg = kc.config(ctx, 1)
    key = kc.make_key(cfg, tables)
    _, bus_sum = kc.verify(cfg, key.root, tables, kc.prove(cfg, key, kc.compiled(ctx, tables), tables), check_bus=False)
    assert bus_sum.any()


# ------------------------------------------------------------------ 2. what the definitions say
def test_zero_padding(ctx):
    rep = check(ctx, m.padding(0), "(TAG, a) against (TAG, a, 0)")
    assert rep.balanced and rep.n_tuples == 1
    rep = check(ctx, m.padding(1), "(TAG, a) against (TAG, a, 1)")
    assert not rep.balanced and rep.n_tuples == 2 and rep.n_unbalanced == 2


def test_sums_past_p(ctx):
    rep = check(ctx, m.past_p(1 << 12), "2^12 rows of p - 1 against 2^12")
    assert rep.balanced and rep.n_contributions == (1 << 12) + 1 and rep.n_tuples == 1
    rep = check(ctx, m.past_p((1 << 12) - 1), "2^12 - 1 rows of p - 1 against 2^12")
    assert rep.n_unbalanced == 1 and rep.sum == 1 and rep.shares[0] == ((1 << 12) - 1, P - 4095, (0, 0))


def test_first_contribution_is_in_table_row_interaction_order(ctx):
    assert check(ctx, m.two_bad("second table"), "second table").first == (1, 2, 2)
    assert check(ctx, m.two_bad("late interaction"), "late interaction").first == (0, 1, 2)


def test_multiplicity_words(ctx):
    rep = check(ctx, m.non_canonical(), "0, p, p + 1, p + 2")
    assert rep.balanced and rep.n_contributions == 3
    assert check(ctx, m.cancels_inside(), "inside one table").balanced


# ------------------------------------------------------------------ 3. probe chains
def test_probe_chains_change_no_report(ctx, monkeypatch):
    s = bc.send(1, 8, 6, 71)
    balanced = m.from_cases([s, bc.rng(6, [s])])
    t = s.trace.copy()
    t[200] = (1 << 6, 1)  # one sent value outside the table
    bad = bc.Table(s.air, t)
    unbalanced = m.from_cases([bad, bc.rng(6, [bad])])
    equal = m.past_p(1 << 12)  # 2^12 rows of ONE tuple
    reports = []
    for bits in (None, "0", "3"):
        if bits is None:
            monkeypatch.delenv("TS_LOGUP_HASH_BITS", raising=False)
        else:
            monkeypatch.setenv("TS_LOGUP_HASH_BITS", bits)
        reports.append([check(ctx, tb, f"TS_LOGUP_HASH_BITS={bits}").asdict() for tb in (balanced, unbalanced, equal)])
    assert reports[0] == reports[1] == reports[2]
    assert reports[0][1]["first"] == (0, 200, 0) and reports[0][1]["tuple"][:2] == [7, 64]
    monkeypatch.setenv("TS_LOGUP_HASH_BITS", "33")
    with pytest.raises(_lib.TsError) as e:
        run(ctx, balanced)
    assert e.value.code == TS_ERR_INVALID and "TS_LOGUP_HASH_BITS" in str(e.value)


# ------------------------------------------------------------------ 4. heights and spec limits
def _wide_tables():
    """K = 16 interactions of 8 values over 2^10 rows (more than one workgroup), beside tables of 1 and 2 rows and a
    table that is not on the bus in the middle.  Small values, so that tuples meet across rows and interactions."""
    g = np.random.default_rng(5)
    big = np.concatenate([g.integers(0, 2, size=(1 << 10, 8)),
                          g.choice([0, 0, 1, 2, P - 1, P - 2], size=(1 << 10, 16))], axis=1).astype(np.uint32)
    wide = m.lg(*[(("col", 8 + i), [("col", (q + i) % 8) for q in range(8)]) for i in range(16)])
    short = m.lg((("col", 8), [("col", q) for q in range(8)]), (("const", P - 1), [("col", q) for q in range(4)]))
    one = big[:1].copy()
    two = big[5:7].copy()
    off = g.integers(0, P, size=(4, 3)).astype(np.uint32)
    return [(wide, big, None), (short, one, None), (None, off, None), (short, two, None)]


def test_heights_one_and_two_a_null_spec_and_the_widest_spec(ctx):
    tables = _wide_tables()
    rep = check(ctx, tables, "K = 16, n_values = 8")
    assert rep.n_contributions > 1 << 10 and rep.shares[2] == (0, 0, None)
    # the same with the null spec's trace left out altogether
    logups = [t[0] for t in tables]
    traces = [ts.DeviceMatrix.upload(ctx, t[1].copy()) if t[0] is not None else None for t in tables]
    assert ts.bus_check(logups, traces) == rep


# ------------------------------------------------------------------ 5. no state
def test_two_runs_in_one_context_agree(ctx):
    for tables in (m.from_cases(bc.case("b")), m.two_bad("second table")):
        assert run(ctx, tables)[0] == run(ctx, tables)[0]


def test_reads_no_unwritten_memory(ctx):
    targets = _poison.make_contexts()
    for what, tables in (("balanced", m.from_cases(bc.case("b"))), ("unbalanced", _wide_tables())):
        want = as_arrays(check(ctx, tables, what))
        _poison.same_everywhere(targets, lambda c: as_arrays(run(c, tables)[0]), want=want, what=what)


# ------------------------------------------------------------------ 6. refusals
def test_refusals(ctx):
    spec = m.lg((("col", 1), [("const", m.TAG), ("col", 0)]))
    host = m.u32([[5, 1], [5, P - 1]])
    t = ts.DeviceMatrix.upload(ctx, host.copy())
    other = ts.DeviceMatrix.upload(ts.Context(0), host.copy())
    # a column-major matrix: a quotient chunk (2^4 x 4, bit-reversed rows)
    fib = bc.fib(4)
    cfg = bc.config(ctx, 2)
    _, alone = cfg.pcs.commit([((fib.log_n, 1), fib.trace.copy())])
    (cols,) = cfg.pcs.quotient_chunks(alone, ts.CompiledAir(ctx, fib.tape), fib.pis, np.array([3, 1, 4, 1], dtype=np.uint32))
    kind2 = m.lg((("col", 1), [("const", m.TAG), ("prep", 0)]))
    outside = m.lg((("col", 1), [("const", m.TAG), ("col", 2)]))
    pre_short = ts.DeviceMatrix.upload(ctx, m.u32([[1], [2], [3], [4]]))
    k16 = m.lg(*[(("col", 1), [("col", 0)])] * 16)
    tall = ts.DeviceMatrix.synth_mul(ctx, 1 << 21, 8)  # 33 x 2^21 x 16 = 33 x 2^25 > 2^30; no device work is done
    cases = {
        "a column-major trace": lambda: ts.bus_check([spec], [cols]),
        "a trace of another context": lambda: ts.bus_check([spec, spec], [t, other]),
        "a kind-2 term without its matrix": lambda: ts.bus_check([kind2], [t]),
        "a kind-2 term, preprocessed given, its entry null": lambda: ts.bus_check([spec, kind2], [t, t], [t, None]),
        "a preprocessed matrix of another height": lambda: ts.bus_check([kind2], [t], [pre_short]),
        "a column outside the trace": lambda: ts.bus_check([outside], [t]),
        "17 interactions": lambda: ts.bus_check([m.lg(*[(("col", 1), [("col", 0)])] * 17)], [t]),
        "9 values": lambda: ts.bus_check([m.lg((("col", 1), [("col", 0)] * 9))], [t]),
        "every spec null": lambda: ts.bus_check([None, None], [t, t]),
        "a spec without a trace": lambda: ts.bus_check([spec, spec], [t, None]),
        "65 tables": lambda: ts.bus_check([spec] * 65, [t] * 65),
        "more than 2^30 possible contributions": lambda: ts.bus_check([k16] * 33, [tall] * 33),
    }
    for what, call in cases.items():
        with pytest.raises(_lib.TsError) as e:
            call()
        assert e.value.code == TS_ERR_INVALID and len(str(e.value)) > 20, f"{what}: {e.value}"
    assert "2^30" in str(e.value)
    # the arguments alone
    import ctypes as C
    sc, keep = spec._spec_c()
    specs = (C.POINTER(_lib.LogupSpecC) * 1)(C.pointer(sc))
    handles = (C.c_void_p * 1)(t.h)
    rep = _lib.BusReportC(struct_size=C.sizeof(_lib.BusReportC) - 8)
    assert ctx._l.ts_bus_check(ctx.h, 1, specs, None, handles, C.byref(rep), None) == TS_ERR_INVALID
    assert "struct_size" in (ctx._l.ts_last_error(ctx.h) or b"").decode()
    rep.struct_size += 8
    assert ctx._l.ts_bus_check(ctx.h, 1, None, None, handles, C.byref(rep), None) == TS_ERR_INVALID
    assert ctx._l.ts_bus_check(ctx.h, 1, specs, None, None, C.byref(rep), None) == TS_ERR_INVALID
    assert ctx._l.ts_bus_check(ctx.h, 1, specs, None, handles, C.byref(rep), None) == 0 and rep.n_unbalanced == 0
    del keep
    assert (t.download() == host).all()


# ------------------------------------------------------------------ 7. ts_check_multi
def _check_multi(ctx, cases, tables, traces=None):
    key = cases.make_key(cases.config(ctx, 1), tables) if cases is kc else None
    traces = traces or [t.trace for t in tables]
    mats = [ts.DeviceMatrix.upload(ctx, np.ascontiguousarray(t).copy()) for t in traces]
    out = ts.check_multi(key, cases.compiled(ctx, tables), mats, [t.pis for t in tables], [t.logup for t in tables],
                         CHALLENGES)
    for dm, t in zip(mats, traces):
        assert (dm.download() == t).all()  # not consumed, not written
    return out


@pytest.mark.parametrize("name", ["a", "b", "ka", "kb", "kt1"])
def test_check_multi_balanced(ctx, name):
    cases = kc if name.startswith("k") else bc
    tables = cases.case(name)
    bad, fv, rep = _check_multi(ctx, cases, tables)
    assert (bad, fv) == (-1, -1) and rep.balanced
    assert rep.asdict() == m.model(m.from_cases(tables))


def test_check_multi_names_the_table_with_a_violated_constraint(ctx):
    tables = kc.case("kb")
    k = 3  # BusSendAir(2) of 2^6 rows
    t = tables[k].trace.copy()
    t[9, 1] = 2  # a selector that is not boolean
    traces = [x.trace for x in tables]
    traces[k] = t
    bad, fv, rep = _check_multi(ctx, kc, tables, traces)
    dm = ts.DeviceMatrix.upload(ctx, t.copy())
    aux, exposed = tables[k].logup.build(dm, CHALLENGES)
    want = ts.check_constraints(ts.CompiledAir(ctx, tables[k].tape), dm, tables[k].pis, ctx, aux=aux,
                                challenges=CHALLENGES, exposed=exposed)
    assert want >= 0 and want >> 16 == 9
    assert (bad, fv) == (k, want)
    model_tables = m.from_cases(tables)
    model_tables[k] = (tables[k].logup, t, None)
    assert rep.asdict() == m.model(model_tables)


@pytest.mark.parametrize("cases", [bc, kc], ids=["bus", "key"])
def test_check_multi_unbalanced(ctx, cases):
    bad, fv, rep = _check_multi(ctx, cases, cases.case("unbalanced"))
    assert (bad, fv) == (-1, -1) and not rep.balanced
    got = rep.asdict()
    for field, want in UNBALANCED.items():
        assert got[field] == want, field


def test_check_multi_refusals(ctx):
    tables = kc.case("ka")
    cfg = kc.config(ctx, 1)
    cairs = kc.compiled(ctx, tables)
    mats = [ts.DeviceMatrix.upload(ctx, t.trace.copy()) for t in tables]
    args = ([t.pis for t in tables], [t.logup for t in tables], CHALLENGES)
    no_values = kc.make_key(cfg, tables, keep_values=False)
    for what, call in {
        "a null key beside preprocessed columns": lambda: ts.check_multi(None, cairs, mats, *args),
        "a key without kept values": lambda: ts.check_multi(no_values, cairs, mats, *args),
        "one trace handle twice": lambda: ts.check_multi(kc.make_key(cfg, tables), cairs, [mats[0], mats[0]], *args),
        "a spec for the wrong table": lambda: ts.check_multi(kc.make_key(cfg, tables), cairs, mats, args[0],
                                                            [tables[0].logup, None], CHALLENGES),
    }.items():
        with pytest.raises(_lib.TsError) as e:
            call()
        assert e.value.code == TS_ERR_INVALID, f"{what}: {e.value}"
    for dm, t in zip(mats, tables):
        assert (dm.download() == t.trace).all()


# ------------------------------------------------------------------ 8. the C++ example
def test_cpp_bus_check_example(ctx, tmp_path):
    """examples/bus_check.cpp: the statement of examples/multi_bus.cpp with one sent value outside the table names
    table 1, row 5 and the tuple (7, 256); with the value put right it says balanced."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "bus_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "bus_check.cpp"), "-L", libdir, "-ltapstark_hip",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unbalanced: table 1, row 5, interaction 0 sent (7, 256), multiplicity sum 1" in r.stdout
    assert "table 1: 1 contributions, sum 1, first at row 5, interaction 0" in r.stdout
    assert "table 0: no contribution" in r.stdout and "table 2: no contribution" in r.stdout
    assert r.stdout.count("constraints hold in every table") == 2
    assert r.stdout.rstrip().endswith("bus_check: balanced")
