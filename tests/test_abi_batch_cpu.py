"""CPU-side checks of ts_prove_batch (include/tapstark.h): the symbol, the refusals of a meaningless call
(which return before any context is touched, so no GPU is needed), the ctypes layout of ts_batch_item and
the Python wrapper's own argument checks; and the same whole-call refusals of ts_prove_stream."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.airs import FibonacciAir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_OK, TS_ERR_INVALID = 0, 1


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


@pytest.fixture(scope="module")
def host_air(lib):
    return ts.CompiledAir(None, ts.air_tape(FibonacciAir(), 3))


# a stand-in context and trace: never dereferenced by the refusals below (they happen before any lane starts)
_FAKE_CTX = C.create_string_buffer(64)
_FAKE_TRACE = C.create_string_buffer(64)


def _call(lib, ctxs, airs, n_lanes, items, n_items, cfg=(2, 28, 8)):
    cfg_c = _lib.FriConfigC(*cfg) if cfg is not None else None
    return lib.ts_prove_batch(ctxs, airs, n_lanes, C.byref(cfg_c) if cfg_c is not None else None,
                              items, n_items, 0.0, 0)


def _stream(lib, ctxs, airs, n_lanes, lane_of, traces=True):
    n = len(lane_of) if lane_of is not None else 1
    mats = (C.c_void_p * n)(*([C.addressof(_FAKE_TRACE)] * n)) if traces else None
    lo = (C.c_uint32 * n)(*lane_of) if lane_of is not None else None
    cfg_c = _lib.FriConfigC(2, 28, 8)
    n_words = C.c_size_t(12345)
    return lib.ts_prove_stream(ctxs, airs, n_lanes, C.byref(cfg_c), mats, lo, n, None, 0, 0.0, None, 0,
                               C.byref(n_words), None, None)


def _lanes(host_air, n):
    ctxs = (C.c_void_p * n)(*([C.addressof(_FAKE_CTX)] * n))
    airs = (C.c_void_p * n)(*([host_air.h.value] * n))
    return ctxs, airs


def _item(lane=0, struct_size=None):
    it = _lib.BatchItemC()
    it.struct_size = C.sizeof(_lib.BatchItemC) if struct_size is None else struct_size
    it.lane = lane
    it.status = 12345  # a marker: the library writes every item of a call it accepts
    return it


def test_symbol_exported(lib):
    assert hasattr(lib, "ts_prove_batch")
    assert "ts_prove_batch" in _lib.ABI_SYMBOLS
    assert lib.ts_abi_version() == 5


def test_null_arrays_and_lane_counts_refused(lib, host_air):
    ctxs, airs = _lanes(host_air, 65)
    items = (_lib.BatchItemC * 1)(_item())
    assert _call(lib, None, airs, 1, items, 1) == TS_ERR_INVALID
    assert _call(lib, ctxs, None, 1, items, 1) == TS_ERR_INVALID
    assert _call(lib, ctxs, airs, 1, None, 1) == TS_ERR_INVALID
    assert _call(lib, ctxs, airs, 0, items, 1) == TS_ERR_INVALID
    assert _call(lib, ctxs, airs, 65, items, 1) == TS_ERR_INVALID
    null_ctx = (C.c_void_p * 1)(None)
    assert _call(lib, null_ctx, airs, 1, items, 1) == TS_ERR_INVALID
    # an invalid FriConfig makes the call meaningless too
    assert _call(lib, ctxs, airs, 1, items, 1, cfg=None) == TS_ERR_INVALID
    assert _call(lib, ctxs, airs, 1, items, 1, cfg=(0, 28, 8)) == TS_ERR_INVALID
    assert items[0].status == 12345, "a refused call wrote an item"
    # nothing to do is not an error
    assert _call(lib, ctxs, airs, 1, None, 0) == TS_OK


def test_struct_size_is_the_ctypes_size(lib, host_air):
    ctxs, airs = _lanes(host_air, 1)
    size = C.sizeof(_lib.BatchItemC)
    for bad in (0, size - 8, size + 8):
        items = (_lib.BatchItemC * 2)(_item(), _item(struct_size=bad))
        assert _call(lib, ctxs, airs, 1, items, 2) == TS_ERR_INVALID
        assert items[0].status == 12345 and items[1].status == 12345, "a refused call wrote an item"
    # the ctypes size is accepted: an item whose lane does not exist fails alone, in its own status, and
    # the lane thread never reaches the (stand-in) context because it has no item to prove
    items = (_lib.BatchItemC * 1)(_item(lane=5))
    assert _call(lib, ctxs, airs, 1, items, 1) == TS_ERR_INVALID
    assert items[0].status == TS_ERR_INVALID


def test_ctypes_layout_matches_the_header(lib, tmp_path):
    fields = [f for f, _ in _lib.BatchItemC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tapstark.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(ts_batch_item));\n'
                   + "".join(f'    printf("%zu\\n", offsetof(ts_batch_item, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got[0] == C.sizeof(_lib.BatchItemC)
    assert got[1:] == [getattr(_lib.BatchItemC, f).offset for f in fields]
    assert _lib.BATCH_DIGEST == 1


def test_wrapper_rejects_mismatched_lengths_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", no_library)
    lanes = [object()]  # never looked at: the lengths are checked first
    traces = [np.zeros((8, 2), dtype=np.uint32)] * 3
    with pytest.raises(ValueError, match="lane indices"):
        ts.prove_batch(lanes, traces, [0, 0])
    with pytest.raises(ValueError, match="public-value vectors"):
        ts.prove_batch(lanes, traces, [0, 0, 0], public_values=[[0, 1, 2], [0, 1, 2]])
    with pytest.raises(ValueError, match="challengers"):
        ts.prove_batch(lanes, traces, [0, 0, 0], challengers=[None, None])


def test_stream_refuses_before_any_lane_starts(lib, host_air):
    ctxs, airs = _lanes(host_air, 65)
    assert _stream(lib, None, airs, 1, [0]) == TS_ERR_INVALID
    assert _stream(lib, ctxs, None, 1, [0]) == TS_ERR_INVALID
    assert _stream(lib, ctxs, airs, 1, [0], traces=False) == TS_ERR_INVALID
    assert _stream(lib, ctxs, airs, 1, None) == TS_ERR_INVALID
    assert _stream(lib, ctxs, airs, 0, [0]) == TS_ERR_INVALID
    assert _stream(lib, ctxs, airs, 65, [0]) == TS_ERR_INVALID
    null_ctx = (C.c_void_p * 1)(None)
    assert _stream(lib, null_ctx, airs, 1, [0]) == TS_ERR_INVALID
    # a proof no lane can take refuses the whole call
    assert _stream(lib, ctxs, airs, 1, [0, 1]) == TS_ERR_INVALID


def test_one_context_on_two_lanes_refused(lib, host_air):
    # two lane threads would drive one context: both calls refuse it before any lane starts
    ctxs, airs = _lanes(host_air, 2)
    assert _stream(lib, ctxs, airs, 2, [0, 1]) == TS_ERR_INVALID
    items = (_lib.BatchItemC * 1)(_item(lane=5))
    assert _call(lib, ctxs, airs, 2, items, 1) == TS_ERR_INVALID
    assert items[0].status == 12345, "a refused call wrote an item"
    assert _call(lib, ctxs, airs, 2, None, 0) == TS_ERR_INVALID
