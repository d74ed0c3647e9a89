"""ts_logup_multiplicities_bus on the GPU: the multiplicity column of a table whose lookups are rows of OTHER traces
of other heights, against a Python dictionary count (`reference` below: nothing is compared against the code under
test), and against ts_logup_multiplicities where the one looker is the table trace itself."""
import ctypes as C

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.air import logup_multiplicities, logup_multiplicities_bus, mult_bus_spec_c
import _mult_cases as mcases

pytestmark = pytest.mark.gpu
P = 0x78000001
JUNK = mcases.JUNK
TS_ERR_INVALID, TS_ERR_INVARIANT = 1, 5
HASH_KNOB = "TS_LOGUP_HASH_BITS"


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def _value(term, row):
    kind, v = term
    return int(v) if kind in (0, "const") else int(row[v])


def reference(table_trace, table, lookers, out_column, negate):
    """(the table trace after the call, n_missing, least (looker, row, lookup) miss or None) over Python integers:
    a dictionary from the table's tuples to their lowest row, then one pass over every looker's rows."""
    rows = np.asarray(table_trace).tolist()
    lowest = {}
    for t, row in enumerate(rows):
        lowest.setdefault(tuple(_value(term, row) for term in table), t)
    sums = [0] * len(rows)
    misses = []
    for k, (trace, lookups, weights) in enumerate(lookers):
        for r, row in enumerate(np.asarray(trace).tolist()):
            for l, (tup, weight) in enumerate(zip(lookups, weights)):
                w = _value(weight, row) % P
                if w == 0:
                    continue
                rep = lowest.get(tuple(_value(term, row) for term in tup))
                if rep is None:
                    misses.append((k, r, l))
                else:
                    sums[rep] += w
    out = np.array(table_trace, dtype=np.uint32, copy=True)
    for t, s in enumerate(sums):
        out[t, out_column] = (P - s % P) % P if negate else s % P
    return out, len(misses), (min(misses) if misses else None)


def check(ctx, table_trace, table, lookers, out_column, negate=1, what=""):
    want, want_missing, want_first = reference(table_trace, table, lookers, out_column, negate)
    m = ts.DeviceMatrix.upload(ctx, table_trace.copy())
    mats = [(ts.DeviceMatrix.upload(ctx, np.ascontiguousarray(t)), lk, w) for t, lk, w in lookers]
    n_missing, first = logup_multiplicities_bus(m, table, mats, out_column, negate, allow_missing=True)
    got = m.download()
    assert (got == want).all(), f"{what}: {int((got != want).sum())} words differ"
    assert (n_missing, first) == (want_missing, want_first), what
    for (dm, _, _), (t, _, _) in zip(mats, lookers):
        assert (dm.download() == t).all(), f"{what}: a looker was written"
    return got


def _range_table(n):
    t = np.empty((n, 2), dtype=np.uint32)
    t[:, 0] = np.arange(n)
    t[:, 1] = JUNK
    return t


def _looker(n, width, below, seed, sel=True):
    """(value, weight) column pairs: values below `below`, weights 0 / 1 (or all 1)."""
    rng = np.random.default_rng(seed)
    t = np.empty((n, width), dtype=np.uint32)
    t[:, 0::2] = rng.integers(0, below, size=(n, width // 2))
    t[:, 1::2] = rng.integers(0, 2, size=(n, width // 2)) if sel else 1
    k = width // 2
    return t, [[("col", 2 * i)] for i in range(k)], [("col", 2 * i + 1) for i in range(k)]


@pytest.mark.parametrize("negate", [0, 1])
@pytest.mark.parametrize("bits", [None, "0", "2"])
def test_table_of_8_rows_lookers_of_64_and_2(ctx, monkeypatch, bits, negate):
    """The lookers are taller and shorter than the table; the 2-row looker runs the ballot with 62 dead lanes; the
    weight columns hold zeros.  TS_LOGUP_HASH_BITS 0 / 2: one probe chain through every entry / four of them."""
    if bits is None:
        monkeypatch.delenv(HASH_KNOB, raising=False)
    else:
        monkeypatch.setenv(HASH_KNOB, bits)
    big, small = _looker(64, 4, 8, 1), _looker(2, 2, 8, 2, sel=False)
    assert (big[0][:, 1::2] == 0).any() and (big[0][:, 1::2] == 1).any()
    check(ctx, _range_table(8), [("col", 0)], [big, small], 1, negate, f"bits {bits} negate {negate}")


def test_duplicate_table_rows_and_field_weights(ctx):
    """Every table tuple on four scattered rows: the lowest row of each class takes the sum, the others 0.  Weights
    are field elements (0 and p - 1 among them), tuples have a constant tag and two columns."""
    rng = np.random.default_rng(7)
    n = 32
    table = np.empty((n, 3), dtype=np.uint32)
    table[:, 0] = rng.permutation(np.repeat(np.arange(n // 4), 4))
    table[:, 1] = table[:, 0] * 3 + 1
    table[:, 2] = JUNK
    look = np.empty((128, 3), dtype=np.uint32)
    look[:, 0] = rng.integers(0, n // 4, size=128)
    look[:, 1] = look[:, 0] * 3 + 1
    look[:, 2] = rng.integers(0, P, size=128)
    look[0, 2], look[1, 2] = 0, P - 1
    spec_t = [("const", 9), ("col", 0), ("col", 1)]
    lookers = [(look, [[("const", 9), ("col", 0), ("col", 1)]], [("col", 2)])]
    got = check(ctx, table, spec_t, lookers, 2, 1, "duplicates")
    reps = {int(v): int(np.flatnonzero(table[:, 0] == v)[0]) for v in range(n // 4)}
    assert all(int(got[t, 2]) == 0 for t in range(n) if t not in reps.values())


def test_a_wave_that_hits_one_row(ctx):
    """Every row of a 256-row looker looks the same entry up (the one-destination path: one add per wave), beside a
    looker with 16 lookups per row; the sum passes 2^32 with weights p - 1."""
    one = np.empty((256, 1), dtype=np.uint32)
    one[:, 0] = 5
    wide = np.tile(np.arange(16, dtype=np.uint32), (64, 1))
    lookers = [(one, [[("col", 0)]], [("const", P - 1)]),
               (wide, [[("col", i)] for i in range(16)], [("const", P - 1)] * 16)]
    got = check(ctx, _range_table(16), [("col", 0)], lookers, 1, 0, "one destination")
    assert int(got[5, 1]) == (256 + 64) * (P - 1) % P


def test_the_table_trace_as_its_own_looker_is_ts_logup_multiplicities(ctx):
    for case in (mcases.range_case(1 << 8), mcases.duplicates_case(1 << 8),
                 mcases.tuple_case(1 << 7, 3, 3, 11, const_at=1, weights="field")):
        trace, prep, spec = case
        assert prep is None
        a = ts.DeviceMatrix.upload(ctx, trace.copy())
        b = ts.DeviceMatrix.upload(ctx, trace.copy())
        single = logup_multiplicities(a, allow_missing=True, **spec)
        bus = logup_multiplicities_bus(b, spec["table"], [(b, spec["lookups"], spec["weights"])], spec["out_column"],
                                       spec["negate"], allow_missing=True)
        assert (a.download() == b.download()).all()
        assert single[0] == bus[0] == 0 and bus[1] is None
        want, _, _ = mcases.reference(trace, **spec)
        assert (b.download() == want).all()


def test_the_bus_airs_fill_is_the_generators_column(ctx):
    import _bus_cases as bc
    from tapstark_amd.airs import fill_bus_range_multiplicities
    rng_t, _, s2, s5, s1 = bc.case("b")
    m = ts.DeviceMatrix.upload(ctx, np.where(np.arange(2) == 1, JUNK, rng_t.trace).astype(np.uint32))
    senders = [ts.DeviceMatrix.upload(ctx, s.trace.copy()) for s in (s2, s5, s1)]
    assert fill_bus_range_multiplicities(m, senders) == (0, None)
    assert (m.download() == rng_t.trace).all()


def test_a_planted_miss_reports_looker_row_lookup(ctx):
    a, b = _looker(64, 4, 8, 21), _looker(16, 6, 8, 22)
    b[0][9, 2], b[0][9, 3] = 8, 1      # looker 1, row 9, lookup 1: outside the table, weight 1
    b[0][12, 0], b[0][12, 1] = 1000, 1  # a later one
    b[0][3, 4], b[0][3, 5] = 77, 0      # weight 0: no miss
    want = reference(_range_table(8), [("col", 0)], [a, b], 1, 1)
    assert want[1] == 2 and want[2] == (1, 9, 1)
    check(ctx, _range_table(8), [("col", 0)], [a, b], 1, 1, "misses")
    m = ts.DeviceMatrix.upload(ctx, _range_table(8))
    mats = [(ts.DeviceMatrix.upload(ctx, t), lk, w) for t, lk, w in (a, b)]
    with pytest.raises(_lib.TsError) as e:
        logup_multiplicities_bus(m, [("col", 0)], mats, 1)
    assert e.value.code == TS_ERR_INVARIANT and "looker 1, row 9, lookup 1" in str(e.value), str(e.value)


def test_refusals_leave_the_column_untouched(ctx):
    table = _range_table(8)
    m = ts.DeviceMatrix.upload(ctx, table.copy())
    look, lk, w = _looker(16, 4, 8, 31)
    d = ts.DeviceMatrix.upload(ctx, look)
    other = ts.DeviceMatrix.upload(ts.Context(0), look)
    T = [("col", 0)]
    cases = {
        "no looker": lambda: logup_multiplicities_bus(m, T, [], 1),
        "17 lookers": lambda: logup_multiplicities_bus(m, T, [(d, lk, w)] * 17, 1),
        "17 lookups": lambda: logup_multiplicities_bus(m, T, [(d, [[("col", 0)]] * 17, [("const", 1)] * 17)], 1),
        "no values": lambda: logup_multiplicities_bus(m, [], [(d, [[]], [("const", 1)])], 1),
        "a looker of another context": lambda: logup_multiplicities_bus(m, T, [(d, lk, w), (other, lk, w)], 1),
        "out_column outside the table trace": lambda: logup_multiplicities_bus(m, T, [(d, lk, w)], 2),
        "out_column read by the table": lambda: logup_multiplicities_bus(m, T, [(d, lk, w)], 0),
        "out_column read by a looker that is the table trace":
            lambda: logup_multiplicities_bus(m, T, [(d, lk, w), (m, [[("col", 0)]], [("col", 1)])], 1),
        "a looker column outside its trace": lambda: logup_multiplicities_bus(m, T, [(d, [[("col", 4)]], [("const", 1)])], 1),
        "a table column outside its trace": lambda: logup_multiplicities_bus(m, [("col", 2)], [(d, lk, w)], 1),
        "a kind-2 term": lambda: logup_multiplicities_bus(m, T, [(d, [[("prep", 0)]], [("const", 1)])], 1),
        "negate 2": lambda: logup_multiplicities_bus(m, T, [(d, lk, w)], 1, negate=2),
    }
    for what, call in cases.items():
        with pytest.raises(_lib.TsError) as e:
            call()
        assert e.value.code == TS_ERR_INVALID, f"{what}: {e.value}"
    spec, keep = mult_bus_spec_c(T, [(lk, w)], 1)
    l = ctx._l
    handles = (C.c_void_p * 1)(d.h)
    assert l.ts_logup_multiplicities_bus(None, C.byref(spec), m.h, handles, None, None) == TS_ERR_INVALID
    assert l.ts_logup_multiplicities_bus(ctx.h, None, m.h, handles, None, None) == TS_ERR_INVALID
    assert l.ts_logup_multiplicities_bus(ctx.h, C.byref(spec), None, handles, None, None) == TS_ERR_INVALID
    assert l.ts_logup_multiplicities_bus(ctx.h, C.byref(spec), m.h, None, None, None) == TS_ERR_INVALID
    spec.struct_size -= 8
    assert l.ts_logup_multiplicities_bus(ctx.h, C.byref(spec), m.h, handles, None, None) == TS_ERR_INVALID
    assert (m.download() == table).all() and (d.download() == look).all()
    n_missing, first = logup_multiplicities_bus(m, T, [(d, lk, w)], 1)
    assert (n_missing, first) == (0, None) and not (m.download()[:, 1] == JUNK).any()
