"""ts_logup_multiplicities on the GPU (csrc/logup_mult.hip): every result -- the WHOLE trace after the call, the
miss count and the first miss -- is compared word for word with the integer reference of tests/_mult_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.air import aux_dims, logup_multiplicities
from tapstark_amd.airs import (FibonacciAir, RangeLookupAir, TableLookupAir, fibonacci_public_values,
                               fill_range_lookup_multiplicities, fill_table_lookup_multiplicities,
                               generate_fibonacci_trace, generate_lookup_table, generate_range_lookup_trace,
                               generate_table_lookup_trace)

import _mult_cases as mc
import _poison

pytestmark = pytest.mark.gpu
P = mc.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_OK, TS_ERR_INVALID, TS_ERR_INVARIANT = 0, 1, 5
# powers of two only: no call makes a matrix of another height (ts_matrix_upload and ts_matrix_from_device refuse
# it), so 255 and 1000 cannot be reached; 1, 2 and 128 are the heights below one workgroup, 2^10 and 2^12 span several
HEIGHTS = (1, 2, 1 << 7, 1 << 8, 1 << 10, 1 << 12)
HASH_KNOB = "TS_LOGUP_HASH_BITS"
CHALLENGES = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def run(ctx, case, allow_missing=True):
    """The case on the device: (the whole trace afterwards, n_missing, first_missing)."""
    trace, prep, spec = case
    d_trace = ts.DeviceMatrix.upload(ctx, trace)
    d_prep = ts.DeviceMatrix.upload(ctx, prep) if prep is not None else None
    n_missing, first = logup_multiplicities(d_trace, preprocessed=d_prep, allow_missing=allow_missing, **spec)
    if d_prep is not None:
        assert (d_prep.download() == prep).all(), "the preprocessed matrix changed"
    return d_trace.download(), n_missing, first


def want_of(case):
    trace, prep, spec = case
    return mc.reference(trace, preprocessed=prep, **spec)


def check(ctx, case, what=""):
    got, want = run(ctx, case), want_of(case)
    bad = np.argwhere(got[0] != want[0])
    assert len(bad) == 0, f"{what}: {len(bad)} words differ, first at (row, column) {bad[0].tolist()}"
    assert got[1:] == want[1:], f"{what}: (n_missing, first_missing) = {got[1:]}, not {want[1:]}"
    return want


# ------------------------------------------------------------------ 1. the range table
@pytest.mark.parametrize("n", HEIGHTS)
def test_range_table(ctx, n):
    want = check(ctx, mc.range_case(n), f"range table, n = {n}")
    assert want[1:] == (0, mc.NONE)
    assert int(want[0][:, 2].astype(np.int64).sum()) % P == (-n) % P  # every lookup was counted once


@pytest.mark.parametrize("log_n", [8, 10])
def test_range_table_is_the_generators_column(ctx, log_n):
    n = 1 << log_n
    want = generate_range_lookup_trace(n)
    trace = want.copy()
    trace[:, 2] = mc.JUNK
    d = ts.DeviceMatrix.upload(ctx, trace)
    assert fill_range_lookup_multiplicities(d) == (0, mc.NONE)
    assert (d.download() == want).all()


@pytest.mark.parametrize("bits", ["0", "1", "3", "8", None])
@pytest.mark.parametrize("n", [1 << 8, 1 << 7])
def test_hash_bits_change_nothing(ctx, monkeypatch, n, bits):
    """TS_LOGUP_HASH_BITS = 0 makes one probe chain through every entry, small values chains that wrap past the last
    slot."""
    if bits is None:
        monkeypatch.delenv(HASH_KNOB, raising=False)
    else:
        monkeypatch.setenv(HASH_KNOB, bits)
    check(ctx, mc.range_case(n), f"range table, n = {n}, {bits} hash bits")
    # few values: waves whose hits share one destination beside waves that mix them; a tuple table with duplicates
    check(ctx, mc.range_case(n, values=np.random.default_rng(2).integers(0, 4, size=n)), f"4 values, n = {n}")
    check(ctx, mc.tuple_case(n, 3, 3, seed=n, weights="field", alphabet=3), f"tuples, n = {n}, {bits} hash bits")


@pytest.mark.parametrize("value", ["33", "-1", "x", "8 "])
def test_knob_out_of_range_refused(ctx, monkeypatch, value):
    trace, _, spec = mc.range_case(16)
    d = ts.DeviceMatrix.upload(ctx, trace)
    monkeypatch.setenv(HASH_KNOB, value)
    with pytest.raises(_lib.TsError) as e:
        logup_multiplicities(d, **spec)
    assert e.value.code == TS_ERR_INVALID and HASH_KNOB in str(e.value)
    assert (d.download() == trace).all()


# ------------------------------------------------------------------ 2. tuples
@pytest.mark.parametrize("n", HEIGHTS)
@pytest.mark.parametrize("shape", ["w3_const_L3", "w8_L16", "w8_L1", "prep_w3_L3", "prep_w1_L1"])
def test_tuples(ctx, n, shape):
    case = {"w3_const_L3": lambda: mc.tuple_case(n, 3, 3, seed=10 + n, const_at=1),
            "w8_L16": lambda: mc.tuple_case(n, 8, 16, seed=20 + n),
            "w8_L1": lambda: mc.tuple_case(n, 8, 1, seed=30 + n, alphabet=2),
            "prep_w3_L3": lambda: mc.tuple_case(n, 3, 3, seed=40 + n, in_prep=True, alphabet=5),
            "prep_w1_L1": lambda: mc.tuple_case(n, 1, 1, seed=50 + n, in_prep=True)}[shape]()
    check(ctx, case, f"{shape}, n = {n}")


# ------------------------------------------------------------------ 3. weights
@pytest.mark.parametrize("n", HEIGHTS)
@pytest.mark.parametrize("negate", [0, 1])
@pytest.mark.parametrize("weights", ["one", "pm1", "selector", "field"])
def test_weights(ctx, n, weights, negate):
    check(ctx, mc.tuple_case(n, 2, 3, seed=60 + n, weights=weights, negate=negate, alphabet=6),
          f"weights {weights}, negate {negate}, n = {n}")


# ------------------------------------------------------------------ 4. duplicates
@pytest.mark.parametrize("n", [4, 1 << 8, 1 << 10, 1 << 12])
def test_every_entry_four_times(ctx, n):
    case = mc.duplicates_case(n)
    want = check(ctx, case, f"duplicates, n = {n}")
    table = case[0][:, 1]
    lowest = np.array([t == int(np.flatnonzero(table == table[t])[0]) for t in range(n)])
    assert not want[0][~lowest, 2].any(), "a row that is not its class's lowest holds a sum"
    assert np.count_nonzero(want[0][:, 2]) > 0


@pytest.mark.parametrize("n", HEIGHTS)
def test_all_table_rows_equal(ctx, n):
    want = check(ctx, mc.all_equal_table_case(n), f"one class, n = {n}")
    assert not want[0][1:, 3].any()


# ------------------------------------------------------------------ 5. one destination
def test_one_destination_sums_above_32_bits(ctx):
    """Every wave takes the one-add-per-wave path: 64 weights summed in 64 bits, 2^10 adds on one word."""
    case = mc.one_destination_case()
    want = check(ctx, case, "one destination")
    total = (1 << 12) * 16 * (P - 1)
    assert total > 1 << 32 and int(want[0][5, 1]) == total % P and np.count_nonzero(want[0][:, 1]) == 1


# ------------------------------------------------------------------ 6. misses
def _miss_case(n=1 << 10, L=3):
    trace, prep, spec = mc.tuple_case(n, 2, L, seed=70, weights="field", alphabet=9)
    w0 = spec["weights"][0][1]
    misses = [(977, 2), (41, 1), (41, 2), (500, 0)]
    for r, l in misses:
        trace[r, spec["lookups"][l][0][1]] = 1000 + r       # outside the alphabet
        trace[r, spec["weights"][l][1]] = 1 + r
    trace[7, spec["lookups"][0][1][1]] = 12345              # outside the table too, but of weight 0: not a miss
    trace[7, w0] = 0
    return (trace, prep, spec), misses


def test_misses_are_counted_and_the_hits_kept(ctx):
    case, misses = _miss_case()
    want = check(ctx, case, "misses")
    assert want[1:] == (len(misses), 41 * 3 + 1)
    assert np.count_nonzero(want[0][:, case[2]["out_column"]]) > 0


def test_a_miss_without_a_counter_is_an_invariant_error(ctx):
    case, misses = _miss_case()
    with pytest.raises(_lib.TsError) as e:
        run(ctx, case, allow_missing=False)
    assert e.value.code == TS_ERR_INVARIANT
    assert "row 41, lookup 1" in str(e.value), str(e.value)
    # the counter alone, and neither pointer with nothing missing, through the C ABI
    trace, prep, spec = mc.range_case(64)
    trace[9, 0] = 64
    d = ts.DeviceMatrix.upload(ctx, trace)
    spec_c, keep = _spec_c(spec)
    n_missing = C.c_uint64(77)
    assert ctx._l.ts_logup_multiplicities(ctx.h, C.byref(spec_c), None, d.h, C.byref(n_missing), None) == TS_OK
    assert n_missing.value == 1
    assert (d.download() == mc.reference(trace, **spec)[0]).all()
    trace[9, 0] = 63
    d = ts.DeviceMatrix.upload(ctx, trace)
    assert ctx._l.ts_logup_multiplicities(ctx.h, C.byref(spec_c), None, d.h, None, None) == TS_OK
    assert (d.download() == mc.reference(trace, **spec)[0]).all()


# ------------------------------------------------------------------ 7. refusals
def _spec_c(spec, struct_size=None, n_values=None, n_lookups=None):
    T = _lib.LogupTermC
    term = lambda t: T(mc.KINDS.get(t[0], t[0]), t[1])
    table = (T * len(spec["table"]))(*[term(t) for t in spec["table"]])
    flat = [term(t) for tup in spec["lookups"] for t in tup]
    lookups = (T * len(flat))(*flat)
    weights = (T * len(spec["weights"]))(*[term(t) for t in spec["weights"]])
    c = _lib.LogupMultSpecC(C.sizeof(_lib.LogupMultSpecC) if struct_size is None else struct_size,
                            len(spec["table"]) if n_values is None else n_values, table,
                            len(spec["lookups"]) if n_lookups is None else n_lookups, lookups, weights,
                            spec["out_column"], spec["negate"])
    return c, (table, lookups, weights)


def test_refusals_write_nothing(ctx):
    """Every TS_ERR_INVALID of the header, each followed by a download of the unchanged trace.  (A height outside
    [1, 2^27] cannot be reached: no call makes such a matrix.)"""
    trace, _, spec = mc.tuple_case(64, 2, 2, seed=80, weights="selector", alphabet=4)
    # columns: table 0 1, lookups 2 3 | 4 5, weights 6 7, out 8
    prep = np.arange(64 * 2, dtype=np.uint32).reshape(64, 2)
    d, d_prep = ts.DeviceMatrix.upload(ctx, trace), ts.DeviceMatrix.upload(ctx, prep)
    size = C.sizeof(_lib.LogupMultSpecC)

    def refused(spec_c, table=None, target=None, what=""):
        n_missing, first = C.c_uint64(0), C.c_uint64(0)
        rc = ctx._l.ts_logup_multiplicities(ctx.h, C.byref(spec_c[0]), table.h if table is not None else None,
                                            (target or d).h, C.byref(n_missing), C.byref(first))
        assert rc == TS_ERR_INVALID, f"{what}: status {rc}"
        assert (d.download() == trace).all(), f"{what}: the trace changed"

    def edited(**changes):
        s = {k: ([list(t) for t in v] if k == "lookups" else list(v) if isinstance(v, list) else v)
             for k, v in spec.items()}
        for k, v in changes.items():
            if k == "lookup00":
                s["lookups"][0][0] = v
            elif k in ("table0", "weight0"):
                s[{"table0": "table", "weight0": "weights"}[k]][0] = v
            else:
                s[k] = v
        return s

    for bad in (0, size - 8, size + 8):
        refused(_spec_c(spec, struct_size=bad), what=f"struct_size {bad}")
    for nv in (0, 9):
        refused(_spec_c(spec, n_values=nv), what=f"n_values {nv}")
    for nl in (0, 17):
        refused(_spec_c(spec, n_lookups=nl), what=f"n_lookups {nl}")
    refused(_spec_c(edited(negate=2)), what="negate 2")
    refused(_spec_c(edited(out_column=9)), what="out_column outside the trace")
    for key in ("table0", "lookup00", "weight0"):
        refused(_spec_c(edited(**{key: ("col", 9)})), what=f"{key}: a column outside the trace")
        refused(_spec_c(edited(**{key: ("const", P)})), what=f"{key}: a non-canonical constant")
        refused(_spec_c(edited(**{key: (3, 0)})), what=f"{key}: kind 3")
        refused(_spec_c(edited(**{key: ("prep", 0)})), what=f"{key}: kind 2 without a table matrix")
        refused(_spec_c(edited(**{key: ("prep", 2)})), table=d_prep, what=f"{key}: a column outside the table matrix")
        refused(_spec_c(edited(**{key: ("col", 8)})), what=f"{key}: reads out_column")
    for column in range(8):  # out_column among the columns the spec reads
        refused(_spec_c(edited(out_column=column)), what=f"out_column {column} is read")
    # a table of another height, and of another context
    short = ts.DeviceMatrix.upload(ctx, prep[:32])
    refused(_spec_c(spec), table=short, what="a table of another height")
    other = ts.Context(0)
    refused(_spec_c(spec), table=ts.DeviceMatrix.upload(other, prep), what="a table of another context")
    # a trace of another context, a consumed one, one that is not row-major
    foreign = ts.DeviceMatrix.upload(other, trace)
    refused(_spec_c(spec), target=foreign, what="a trace of another context")
    assert (foreign.download() == trace).all()
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 1), ctx)
    consumed = ts.DeviceMatrix.upload(ctx, trace)
    _, data = pcs.commit([((6, 1), consumed)])
    refused(_spec_c(spec), target=consumed, what="a consumed trace")
    fib = generate_fibonacci_trace(0, 1, 64)
    cair = ts.CompiledAir(ctx, ts.air_tape(FibonacciAir(), 3))
    _, fib_data = pcs.commit([((6, 1), fib)])
    chunk = pcs.quotient_chunks(fib_data, cair, fibonacci_public_values(fib), [1, 2, 3, 4])[0]
    one_column = dict(table=[("col", 0)], lookups=[[("col", 1)]], weights=[("const", 1)], out_column=2, negate=1)
    assert chunk.dims()[1] >= 3
    refused(_spec_c(one_column), target=chunk, what="a trace that is not row-major")
    # and the call itself still works on the matrix every refusal left alone
    assert logup_multiplicities(d, **spec) == mc.reference(trace, **spec)[1:]
    assert (d.download() == mc.reference(trace, **spec)[0]).all()


# ------------------------------------------------------------------ 8. the poisoned pool
@pytest.fixture(scope="module")
def poison_contexts(ctx):
    return _poison.make_contexts()


@pytest.mark.parametrize("name", ["range", "duplicates", "all_equal", "one_destination"])
def test_poisoned_pool(poison_contexts, name):
    """Slots, sums and the result block come from the pool and are initialised by the call: the clean context and the
    two filled ones, first use and recycled blocks, give the reference's words."""
    case = {"range": lambda: mc.range_case(1 << 8), "duplicates": lambda: mc.duplicates_case(1 << 8),
            "all_equal": lambda: mc.all_equal_table_case(1 << 8), "one_destination": mc.one_destination_case}[name]()
    words = lambda res: (res[0], res[1], np.array([res[2]], dtype=np.uint64))  # (2^64 - 1 is no int64)
    _poison.same_everywhere(poison_contexts, lambda c: words(run(c, case)), want=words(want_of(case)), what=name)


# ------------------------------------------------------------------ 9. end to end
def _table_lookup(ctx, n, outside_row=None, b=1):
    air = TableLookupAir()
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(b, 3, 2), ctx))
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0, 1, *aux_dims(air)))
    key = ts.PreprocessedKey(config, generate_lookup_table(n), keep_values=True)
    host = generate_table_lookup_trace(n, outside_row=outside_row)
    zeros = host.copy()
    zeros[:, 1] = 0
    return air, config, cair, key, host, zeros


def test_table_lookup_end_to_end(ctx):
    n = 1 << 8
    air, config, cair, key, host, zeros = _table_lookup(ctx, n)
    filled = ts.DeviceMatrix.upload(ctx, zeros)
    assert fill_table_lookup_multiplicities(filled, key.values) == (0, mc.NONE)
    assert (filled.download() == host).all()
    aux, exposed = air.logup.build(filled, CHALLENGES, preprocessed=key.values)
    assert ts.check_constraints(cair, filled, [], ctx, preprocessed=key.values, aux=aux, challenges=CHALLENGES,
                                exposed=exposed) == -1
    source = air.logup.aux_source_with(key.values)
    proof = ts.prove(config, cair, ts.BfChallenger(), filled, [], preprocessed=key, aux=source)
    S = ts.verify(config, cair, ts.BfChallenger(), proof, [], preprocessed_root=key.root)
    air.logup.verify(S)
    want = ts.prove(config, cair, ts.BfChallenger(), host.copy(), [], preprocessed=key, aux=source)
    assert len(proof.words) == len(want.words) and (proof.words == want.words).all()


def test_range_lookup_end_to_end(ctx):
    n = 1 << 8
    air = RangeLookupAir()
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(1, 3, 2), ctx))
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0, 0, *aux_dims(air)))
    host = generate_range_lookup_trace(n)
    zeros = host.copy()
    zeros[:, 2] = 0
    filled = ts.DeviceMatrix.upload(ctx, zeros)
    assert fill_range_lookup_multiplicities(filled) == (0, mc.NONE)
    aux, exposed = air.logup.build(filled, CHALLENGES)
    assert ts.check_constraints(cair, filled, [], ctx, aux=aux, challenges=CHALLENGES, exposed=exposed) == -1
    proof = ts.prove(config, cair, ts.BfChallenger(), filled, [], aux=air.logup.aux_source)
    air.logup.verify(ts.verify(config, cair, ts.BfChallenger(), proof, []))
    want = ts.prove(config, cair, ts.BfChallenger(), host.copy(), [], aux=air.logup.aux_source)
    assert len(proof.words) == len(want.words) and (proof.words == want.words).all()


def test_a_value_outside_the_table_end_to_end(ctx):
    n = 1 << 8
    air, config, cair, key, host, zeros = _table_lookup(ctx, n, outside_row=9)
    filled = ts.DeviceMatrix.upload(ctx, zeros)
    with pytest.raises(_lib.TsError) as e:
        fill_table_lookup_multiplicities(filled, key.values)
    assert e.value.code == TS_ERR_INVARIANT and "row 9, lookup 0" in str(e.value)
    assert fill_table_lookup_multiplicities(filled, key.values, allow_missing=True) == (1, 9)
    assert (filled.download() == host).all()
    proof = ts.prove(config, cair, ts.BfChallenger(), filled, [], preprocessed=key,
                     aux=air.logup.aux_source_with(key.values))
    S = ts.verify(config, cair, ts.BfChallenger(), proof, [], preprocessed_root=key.root)
    assert S.any()
    with pytest.raises(ValueError):
        air.logup.verify(S)


# ------------------------------------------------------------------ 10. the C++ example
def test_cpp_resident_example(ctx, tmp_path):
    """examples/table_lookup_resident.cpp: value columns uploaded with a zero multiplicity column, the column filled
    in HBM, the proof made with ts_prove_pre_aux and verified, the exposed sum zero."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "table_lookup_resident")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "table_lookup_resident.cpp"), "-L", libdir, "-ltapstark_hip",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 missing" in r.stdout and "verify -> 0" in r.stdout and "sum is zero" in r.stdout
