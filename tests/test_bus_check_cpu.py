"""``ts_bus_check`` / ``ts_check_multi`` without a GPU: the two symbols are declared, exported and listed, the two
structs have the header's sizes, the refusals that need no device are made with a text, and the Python model the GPU
tests compare against gives the hand-written answers."""
import ctypes as C
import os
import re

import pytest

import _bus_check_cases as m
from tapstark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = m.P
INVALID = 1


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


def test_symbols_declared_exported_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    declared = set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ts_bus_check", "ts_check_multi"):
        assert name in declared
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name)
    assert lib.ts_abi_version() == 5  # additive


def test_struct_sizes():
    # ts_bus_share: u64 + 4 u32; ts_bus_report: 2 u32 + 3 u64 + 4 u32 + 8 u32 + 2 u32
    assert C.sizeof(_lib.BusShareC) == 24
    assert C.sizeof(_lib.BusReportC) == 8 + 24 + 16 + 32 + 8 == 88
    assert _lib.BusReportC.n_contributions.offset == 8 and _lib.BusReportC.first_table.offset == 32
    assert _lib.BusReportC.tuple.offset == 48 and _lib.BusReportC.sum.offset == 80
    assert _lib.BusShareC.sum.offset == 8 and _lib.BusShareC.first_interaction.offset == 16


def _text(lib):
    return (lib.ts_last_error(None) or b"").decode()


def test_bus_check_refusals_touch_no_device(lib):
    rep = _lib.BusReportC(struct_size=C.sizeof(_lib.BusReportC))
    specs = (C.POINTER(_lib.LogupSpecC) * 1)()
    traces = (C.c_void_p * 1)()
    # a null context
    assert lib.ts_bus_check(None, 1, specs, None, traces, C.byref(rep), None) == INVALID
    assert "ts_bus_check" in _text(lib) and "context" in _text(lib)
    # a null report
    assert lib.ts_bus_check(None, 1, specs, None, traces, None, None) == INVALID
    assert "ts_bus_check" in _text(lib) and "report" in _text(lib)
    # n = 0 and n = 65
    for n in (0, 65):
        assert lib.ts_bus_check(None, n, specs, None, traces, C.byref(rep), None) == INVALID
        assert "between 1 and 64 tables" in _text(lib)


def test_check_multi_refusals_touch_no_device(lib):
    rep = _lib.BusReportC(struct_size=C.sizeof(_lib.BusReportC))
    tabs = (_lib.MultiBusTableC * 1)()
    ch = (C.c_uint32 * 8)()
    bad, fv = C.c_int32(5), C.c_int64(5)
    assert lib.ts_check_multi(None, None, tabs, 1, ch, C.byref(bad), C.byref(fv), C.byref(rep), None) == INVALID
    assert "ts_check_multi" in _text(lib) and "context" in _text(lib)
    assert bad.value == -1 and fv.value == -1
    assert lib.ts_check_multi(None, None, tabs, 1, ch, C.byref(bad), C.byref(fv), None, None) == INVALID
    assert "ts_check_multi" in _text(lib) and "report" in _text(lib)
    for n in (0, 65):
        assert lib.ts_check_multi(None, None, tabs, n, ch, C.byref(bad), C.byref(fv), C.byref(rep), None) == INVALID
        assert "between 1 and 64 tables" in _text(lib)


# ---- the model against hand-written answers
def _balanced(n_contributions, n_tuples, n_tables):
    return {"n_contributions": n_contributions, "n_tuples": n_tuples, "n_unbalanced": 0, "first": None, "n_values": 0,
            "tuple": [0] * 8, "sum": 0, "shares": [(0, 0, None)] * n_tables}


def test_model_padding_equality():
    # (TAG, 5) twice against (TAG, 5, 0) with -2: one tuple
    assert m.model(m.padding(0)) == _balanced(3, 1, 2)
    # (TAG, 5, 1) is another tuple: both are out of balance, the sender's rows come first
    assert m.model(m.padding(1)) == {
        "n_contributions": 3, "n_tuples": 2, "n_unbalanced": 2, "first": (0, 0, 0), "n_values": 2,
        "tuple": [m.TAG, 5, 0, 0, 0, 0, 0, 0], "sum": 2, "shares": [(2, 2, (0, 0)), (0, 0, None)]}


def test_model_sum_of_exactly_p():
    spec = m.lg((("col", 1), [("const", m.TAG), ("col", 0)]))
    tables = [(spec, m.u32([[33, P - 1]]), None), (spec, m.u32([[33, 1]]), None)]
    assert m.model(tables) == _balanced(2, 1, 2)
    tables[1] = (spec, m.u32([[33, 2]]), None)
    got = m.model(tables)
    assert (got["n_unbalanced"], got["sum"], got["first"]) == (1, 1, (0, 0, 0))
    assert got["shares"] == [(1, P - 1, (0, 0)), (1, 2, (0, 0))]


def test_model_two_unbalanced_tuples():
    assert m.model(m.two_bad("second table")) == {
        "n_contributions": 8, "n_tuples": 5, "n_unbalanced": 2, "first": (1, 2, 2), "n_values": 2,
        "tuple": [m.TAG, 80, 0, 0, 0, 0, 0, 0], "sum": 5, "shares": [(0, 0, None), (1, 5, (2, 2))]}
    assert m.model(m.two_bad("late interaction")) == {
        "n_contributions": 3, "n_tuples": 2, "n_unbalanced": 2, "first": (0, 1, 2), "n_values": 2,
        "tuple": [m.TAG, 90, 0, 0, 0, 0, 0, 0], "sum": 6, "shares": [(1, 6, (1, 2)), (0, 0, None)]}


def test_model_cancels_inside_one_table():
    assert m.model(m.cancels_inside()) == _balanced(4, 2, 1)


def test_model_multiplicity_words():
    # 0 and p are no contribution; p + 1 and p + 2 count as 1 and 2 and meet p - 3
    assert m.model(m.non_canonical()) == _balanced(3, 1, 2)


def test_model_sums_past_p():
    assert m.model(m.past_p(1 << 12)) == _balanced((1 << 12) + 1, 1, 2)
    got = m.model(m.past_p((1 << 12) - 1))
    assert (got["n_unbalanced"], got["sum"], got["first"]) == (1, 1, (0, 0, 0))
    assert got["shares"] == [((1 << 12) - 1, P - 4095, (0, 0)), (1, 1 << 12, (0, 0))]
