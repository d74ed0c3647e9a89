"""CPU-side checks of ts_prove_batch_lookup (include/tapstark.h): the symbol, the refusals of a meaningless call
(which return before any context is touched, so no GPU is needed), the ctypes layouts of ts_batch_lane and
ts_batch_lookup_item and the Python wrapper's own argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.airs import FibonacciAir, SelectorAir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_OK, TS_ERR_INVALID = 0, 1
MARK = 12345  # the library writes every item of a call it accepts


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


@pytest.fixture(scope="module")
def host_air(lib):
    return ts.CompiledAir(None, ts.air_tape(FibonacciAir(), 3))


@pytest.fixture(scope="module")
def keyed_air(lib):
    air = SelectorAir()
    return ts.CompiledAir(None, ts.air_tape(air, 2, air.preprocessed_width()))


# stand-in contexts: never dereferenced by the refusals below (they happen before any lane starts)
_FAKE_CTXS = [C.create_string_buffer(64) for _ in range(65)]


def _lanes(air, n, same_ctx=False):
    ctxs = (C.c_void_p * n)(*[C.addressof(_FAKE_CTXS[0 if same_ctx else k]) for k in range(n)])
    airs = (C.c_void_p * n)(*([air.h.value] * n))
    return ctxs, airs


def _lane_structs(n, struct_size=None):
    arr = (_lib.BatchLaneC * n)()
    for k in range(n):
        arr[k].struct_size = C.sizeof(_lib.BatchLaneC) if struct_size is None else struct_size
    return arr


def _item(lane=0, struct_size=None):
    it = _lib.BatchLookupItemC()
    it.struct_size = C.sizeof(_lib.BatchLookupItemC) if struct_size is None else struct_size
    it.lane = lane
    it.status = MARK
    return it


def _call(lib, ctxs, airs, lanes, n_lanes, items, n_items, cfg=(2, 28, 8)):
    cfg_c = _lib.FriConfigC(*cfg) if cfg is not None else None
    return lib.ts_prove_batch_lookup(ctxs, airs, lanes, n_lanes, C.byref(cfg_c) if cfg_c is not None else None,
                                     items, n_items, 0.0, 0)


def test_symbol_exported(lib):
    assert hasattr(lib, "ts_prove_batch_lookup")
    assert "ts_prove_batch_lookup" in _lib.ABI_SYMBOLS
    assert lib.ts_abi_version() == 5


def test_null_arrays_and_lane_counts_refused(lib, host_air):
    ctxs, airs = _lanes(host_air, 65)
    lanes = _lane_structs(65)
    items = (_lib.BatchLookupItemC * 1)(_item())
    assert _call(lib, None, airs, lanes, 1, items, 1) == TS_ERR_INVALID
    assert _call(lib, ctxs, None, lanes, 1, items, 1) == TS_ERR_INVALID
    assert _call(lib, ctxs, airs, lanes, 1, None, 1) == TS_ERR_INVALID
    assert _call(lib, ctxs, airs, lanes, 0, items, 1) == TS_ERR_INVALID
    assert _call(lib, ctxs, airs, lanes, 65, items, 1) == TS_ERR_INVALID
    null_ctx = (C.c_void_p * 1)(None)
    assert _call(lib, null_ctx, airs, lanes, 1, items, 1) == TS_ERR_INVALID
    assert _call(lib, ctxs, airs, lanes, 1, items, 1, cfg=None) == TS_ERR_INVALID
    assert _call(lib, ctxs, airs, lanes, 1, items, 1, cfg=(0, 28, 8)) == TS_ERR_INVALID
    assert items[0].status == MARK, "a refused call wrote an item"
    # nothing to do is not an error, with or without the lane array (no AIR here has preprocessed columns)
    assert _call(lib, ctxs, airs, lanes, 1, None, 0) == TS_OK
    assert _call(lib, ctxs, airs, None, 1, None, 0) == TS_OK


def test_one_context_on_two_lanes_refused(lib, host_air):
    ctxs, airs = _lanes(host_air, 2, same_ctx=True)
    items = (_lib.BatchLookupItemC * 1)(_item(lane=5))
    assert _call(lib, ctxs, airs, _lane_structs(2), 2, items, 1) == TS_ERR_INVALID
    assert items[0].status == MARK, "a refused call wrote an item"
    assert _call(lib, ctxs, airs, _lane_structs(2), 2, None, 0) == TS_ERR_INVALID


def test_struct_sizes_are_the_ctypes_sizes(lib, host_air):
    ctxs, airs = _lanes(host_air, 2)
    size = C.sizeof(_lib.BatchLookupItemC)
    for bad in (0, size - 8, size + 8, C.sizeof(_lib.BatchItemC)):
        items = (_lib.BatchLookupItemC * 2)(_item(), _item(struct_size=bad))
        assert _call(lib, ctxs, airs, _lane_structs(2), 2, items, 2) == TS_ERR_INVALID
        assert items[0].status == MARK and items[1].status == MARK, "a refused call wrote an item"
    lane_size = C.sizeof(_lib.BatchLaneC)
    for bad in (0, lane_size - 8, lane_size + 8):
        lanes = _lane_structs(2)
        lanes[1].struct_size = bad
        items = (_lib.BatchLookupItemC * 1)(_item(lane=5))
        assert _call(lib, ctxs, airs, lanes, 2, items, 1) == TS_ERR_INVALID
        assert items[0].status == MARK, "a refused call wrote an item"


def test_null_lane_array_refused_for_an_air_with_preprocessed_columns(lib, host_air, keyed_air):
    ctxs, _ = _lanes(host_air, 2)
    airs = (C.c_void_p * 2)(host_air.h.value, keyed_air.h.value)
    items = (_lib.BatchLookupItemC * 1)(_item(lane=5))
    assert _call(lib, ctxs, airs, None, 2, items, 1) == TS_ERR_INVALID
    assert items[0].status == MARK, "a refused call wrote an item"
    # with the lane array the call is accepted, and the item on a non-existent lane fails alone
    assert _call(lib, ctxs, airs, _lane_structs(2), 2, items, 1) == TS_ERR_INVALID
    assert items[0].status == TS_ERR_INVALID


def test_item_on_a_missing_lane_fails_alone(lib, host_air):
    # the lane threads never reach the (stand-in) contexts because they have no item to prove
    ctxs, airs = _lanes(host_air, 2)
    items = (_lib.BatchLookupItemC * 2)(_item(lane=2), _item(lane=7))
    assert _call(lib, ctxs, airs, _lane_structs(2), 2, items, 2) == TS_ERR_INVALID
    for it in items:
        assert it.status == TS_ERR_INVALID and it.n_words == 0 and it.n_exposed == 0
        assert it.n_missing == 0 and it.first_missing == 2**64 - 1


def _layout(tmp_path, c_name, struct):
    fields = [f for f, _ in struct._fields_]
    src = tmp_path / f"layout_{c_name}.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tapstark.h"\nint main(void) {\n'
                   f'    printf("%zu\\n", sizeof({c_name}));\n'
                   + "".join(f'    printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / f"layout_{c_name}")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got[0] == C.sizeof(struct)
    assert got[1:] == [getattr(struct, f).offset for f in fields]


def test_ctypes_layouts_match_the_header(lib, tmp_path):
    _layout(tmp_path, "ts_batch_lane", _lib.BatchLaneC)
    _layout(tmp_path, "ts_batch_lookup_item", _lib.BatchLookupItemC)


def test_wrapper_rejects_mismatched_lengths_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", no_library)
    lanes = [object(), object()]  # never looked at: the lengths are checked first
    traces = [np.zeros((8, 2), dtype=np.uint32)] * 3
    with pytest.raises(ValueError, match="lane indices"):
        ts.prove_batch_lookup(lanes, traces, [0, 0])
    with pytest.raises(ValueError, match="public-value vectors"):
        ts.prove_batch_lookup(lanes, traces, [0, 0, 0], public_values=[[0, 1, 2], [0, 1, 2]])
    with pytest.raises(ValueError, match="challengers"):
        ts.prove_batch_lookup(lanes, traces, [0, 0, 0], challengers=[None, None])
    with pytest.raises(ValueError, match="1 keys for 2 lanes"):
        ts.prove_batch_lookup(lanes, traces, [0, 0, 0], keys=[None])
    with pytest.raises(ValueError, match="3 LogUp specs for 2 lanes"):
        ts.prove_batch_lookup(lanes, traces, [0, 0, 0], logups=[None, None, None])
    with pytest.raises(ValueError, match="1 fill lists for 2 lanes"):
        ts.prove_batch_lookup(lanes, traces, [0, 0, 0], fills=[None])
    with pytest.raises(ValueError, match="no lanes"):
        ts.prove_batch_lookup([], [], [])
