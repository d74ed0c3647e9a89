"""CPU-side checks of ts_logup_multiplicities (include/tapstark.h): the reference of tests/_mult_cases.py against
the host generator it replaces, the spec LogUp.fill_multiplicities derives, the symbol, the ctypes layout of
ts_logup_mult_spec and the refusal that needs no context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tapstark_amd import _lib
from tapstark_amd.air import LogUp
from tapstark_amd.airs import RangeLookupAir, TableLookupAir, generate_range_lookup_trace

import _mult_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


@pytest.mark.parametrize("n", [1 << 8, 1 << 10])
@pytest.mark.parametrize("outside_row", [None, 0, 77])
def test_reference_is_the_generators_column(n, outside_row):
    want = generate_range_lookup_trace(n, outside_row=outside_row)
    trace = want.copy()
    trace[:, 2] = mc.JUNK
    spec = RangeLookupAir.logup.mult_spec(table=1)
    got, n_missing, first = mc.reference(trace, **spec)
    assert (got == want).all()
    assert (n_missing, first) == ((0, mc.NONE) if outside_row is None else (1, outside_row))


def test_reference_classes_weights_and_misses():
    """By hand: table rows 0 and 2 are equal (class of row 0), row 1 is alone, row 3 is looked up by nobody."""
    trace = np.array([[5, 5, 2, 0], [6, 6, 0, 0], [5, 9, mc.P - 1, 0], [8, 5, 3, 0]], dtype=np.uint32)
    spec = dict(table=[("col", 0)], lookups=[[("col", 1)]], weights=[("col", 2)], out_column=3)
    got, n_missing, first = mc.reference(trace, negate=0, **spec)
    # row 0: 5 -> class 0, w 2; row 1: weight 0, skipped; row 2: 9 missing; row 3: 5 -> class 0, w 3
    assert got[:, 3].tolist() == [5, 0, 0, 0] and (n_missing, first) == (1, 2)
    got, _, _ = mc.reference(trace, negate=1, **spec)
    assert got[:, 3].tolist() == [mc.P - 5, 0, 0, 0]
    assert (got[:, :3] == trace[:, :3]).all()


def test_spec_of_the_range_and_table_lookup_airs():
    assert RangeLookupAir.logup.mult_spec(table=1) == dict(
        table=[(1, 1)], lookups=[[(1, 0)]], weights=[(0, 1)], out_column=2, negate=1)
    assert TableLookupAir.logup.mult_spec(table=1) == dict(
        table=[(2, 0)], lookups=[[(1, 0)]], weights=[(0, 1)], out_column=1, negate=1)
    # the lookup side's multiplicity is a constant: it cannot be the table
    for air in (RangeLookupAir, TableLookupAir):
        with pytest.raises(ValueError):
            air.logup.mult_spec(table=0)


def test_spec_of_a_helper_with_three_interactions():
    """K = 3 without a preprocessed table: two lookups of pairs, a selector weight, and an interaction of another
    width that the default leaves out."""
    logup = LogUp([(("col", 6), [("col", 0), ("col", 1)]),           # the table: pairs, multiplicity in column 6
                   (("const", 1), [("col", 2), ("const", 4)]),       # a plain lookup
                   (("col", 5), [("col", 3), ("col", 4)]),           # a selected lookup
                   (("const", 1), [("col", 0)])])                    # width 1: not a lookup of this table
    want = dict(table=[(1, 0), (1, 1)], lookups=[[(1, 2), (0, 4)], [(1, 3), (1, 4)]], weights=[(0, 1), (1, 5)],
                out_column=6, negate=1)
    assert logup.mult_spec(table=0) == want
    assert logup.mult_spec(table=0, lookups=[2]) == dict(want, lookups=want["lookups"][1:], weights=want["weights"][1:])
    with pytest.raises(ValueError):
        logup.mult_spec(table=0, lookups=[3])   # another number of values
    with pytest.raises(ValueError):
        logup.mult_spec(table=0, lookups=[0])   # the table itself
    with pytest.raises(ValueError):
        logup.mult_spec(table=1)                # multiplicity not a column
    with pytest.raises(ValueError):
        logup.mult_spec(table=3, lookups=[])    # nothing to look up (the multiplicity is no column either)


def test_symbol_exported_and_declared(lib):
    assert hasattr(lib, "ts_logup_multiplicities")
    assert "ts_logup_multiplicities" in _lib.ABI_SYMBOLS
    assert lib.ts_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    assert "ts_status ts_logup_multiplicities(ts_ctx* ctx, const ts_logup_mult_spec* spec," in header


def test_ctypes_layout_matches_the_header(tmp_path):
    fields = [f for f, _ in _lib.LogupMultSpecC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tapstark.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(ts_logup_mult_spec));\n'
                   + "".join(f'    printf("%zu\\n", offsetof(ts_logup_mult_spec, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got[0] == C.sizeof(_lib.LogupMultSpecC)
    assert got[1:] == [getattr(_lib.LogupMultSpecC, f).offset for f in fields]


def test_null_arguments_refused(lib):
    T = _lib.LogupTermC
    terms = (T * 1)(T(1, 0))
    one = (T * 1)(T(0, 1))
    spec = _lib.LogupMultSpecC(C.sizeof(_lib.LogupMultSpecC), 1, terms, 1, terms, one, 1, 1)
    fake_trace = C.create_string_buffer(64)  # never dereferenced: the null context is refused first
    n_missing, first = C.c_uint64(12345), C.c_uint64(12345)
    assert lib.ts_logup_multiplicities(None, C.byref(spec), None, C.addressof(fake_trace), C.byref(n_missing),
                                       C.byref(first)) == TS_ERR_INVALID
    assert (n_missing.value, first.value) == (12345, 12345), "a refused call wrote its outputs"
