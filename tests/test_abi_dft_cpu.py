"""CPU-side checks of the on-device Dft / evaluations-on-domain surface (TwoAdicSubgroupDft, SURVEY.md
App. A.5; Pcs::get_evaluations_on_domain, fri/src/two_adic_pcs.rs:247-258): the five entry points are in
the header and exported, the Python names exist, and a call without a context is refused with a status
before anything touches a device.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest

import tapstark_amd as ts
from tapstark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ts_dft_batch", "ts_coset_lde_batch", "ts_matrix_bit_reverse_rows",
               "ts_pcs_data_evaluations_on_domain", "ts_matrix_device_ptr"]
TS_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


def test_dft_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    declared = set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/tapstark.h"
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.ts_abi_version() == 5  # additions only


def test_python_surface_exists():
    assert "Radix2Dft" in dir(ts)
    for m in ("dft_batch", "idft_batch", "coset_dft_batch", "coset_idft_batch", "lde_batch", "coset_lde_batch"):
        assert callable(getattr(ts.Radix2Dft, m)), m
    assert callable(ts.DeviceMatrix.bit_reverse_rows) and callable(ts.DeviceMatrix.device_ptr)
    assert callable(ts.TwoAdicFriPcs.get_evaluations_on_domain)
    import inspect
    assert inspect.signature(ts.Radix2Dft.coset_lde_batch).parameters["bit_reversed"].default is False


def test_null_context_is_refused_without_a_device(lib):
    out, ptr = C.c_void_p(0x1), C.c_void_p(0x1)
    m = C.c_void_p(0x10)  # never dereferenced: the context is checked first
    assert lib.ts_dft_batch(None, m, 0, 1, C.byref(out)) == TS_ERR_INVALID
    assert lib.ts_dft_batch(None, m, 1, 31, C.byref(out)) == TS_ERR_INVALID
    assert lib.ts_coset_lde_batch(None, m, 1, 31, 0, C.byref(out)) == TS_ERR_INVALID
    assert lib.ts_matrix_bit_reverse_rows(None, m, C.byref(out)) == TS_ERR_INVALID
    assert lib.ts_pcs_data_evaluations_on_domain(None, m, 0, 3, C.byref(out)) == TS_ERR_INVALID
    assert lib.ts_matrix_device_ptr(None, m, C.byref(ptr)) == TS_ERR_INVALID
