"""CPU-side checks of packed / Montgomery trace ingest (ts_trace_format, include/tapstark.h): the five entry
points are declared, listed and exported, ts_trace_format_bytes gives hand-computed sizes, every refusal of a
format comes back as TS_ERR_INVALID without a context or a device, and TraceFormat.pack agrees with a
pure-numpy decoder.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ts_trace_format_bytes", "ts_matrix_upload_packed", "ts_matrix_upload_packed_async",
               "ts_matrix_from_device_packed", "ts_matrix_download_monty"]
TS_OK, TS_ERR_INVALID = 0, 1
U32, U16, U8, MONTY32, MONTY31 = range(5)
SIZE = {U32: 4, U16: 2, U8: 1, MONTY32: 4, MONTY31: 4}
ROWS, PLANAR = 0, 1


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


def c_format(kinds, layout=ROWS, stride=0, n_kinds=None, struct_size=None, reserved=0):
    arr = (C.c_uint8 * max(len(kinds), 1))(*kinds)
    f = _lib.TraceFormatC(C.sizeof(_lib.TraceFormatC) if struct_size is None else struct_size, layout, stride,
                          len(kinds) if n_kinds is None else n_kinds, reserved, C.cast(arr, C.POINTER(C.c_uint8)))
    f._keep = arr
    return f


def format_bytes(lib, f, height, width):
    n = C.c_uint64(12345)
    rc = lib.ts_trace_format_bytes(C.byref(f) if f is not None else None, height, width, C.byref(n))
    return rc, int(n.value)


def test_ingest_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    declared = set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/tapstark.h"
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.ts_abi_version() == 5  # additions only
    for name in ("TS_COL_U32 = 0", "TS_COL_U16 = 1", "TS_COL_U8 = 2", "TS_COL_MONTY32 = 3", "TS_COL_MONTY31 = 4",
                 "TS_LAYOUT_ROWS = 0", "TS_LAYOUT_PLANAR = 1"):
        assert name in hdr
    assert C.sizeof(_lib.TraceFormatC) == 32  # u32 u32 u64 u32 u32 pointer


def test_format_bytes_against_hand_computed_sizes(lib):
    kinds = [U8, U32, U16]  # a row is 1 + 4 + 2 = 7 bytes
    assert format_bytes(lib, c_format(kinds), 4, 3) == (TS_OK, 28)
    assert format_bytes(lib, c_format(kinds, stride=16), 4, 3) == (TS_OK, 64)
    # planar, height 2: u8 column 2 bytes at 0, u32 column 8 bytes at 16, u16 column 4 bytes at 32
    assert format_bytes(lib, c_format(kinds, layout=PLANAR), 2, 3) == (TS_OK, 16 + 16 + 4)
    assert format_bytes(lib, c_format([MONTY32]), 8, 3) == (TS_OK, 96)
    assert format_bytes(lib, c_format([U8]), 1, 1) == (TS_OK, 1)
    assert format_bytes(lib, c_format([U16], layout=PLANAR), 1 << 27, 2) == (TS_OK, 2 * (2 << 27))


REFUSALS = {
    "null format": lambda: (None, 4, 3),
    "struct_size": lambda: (c_format([U8, U32, U16], struct_size=C.sizeof(_lib.TraceFormatC) - 8), 4, 3),
    "struct_size 0": lambda: (c_format([U8, U32, U16], struct_size=0), 4, 3),
    "reserved": lambda: (c_format([U8, U32, U16], reserved=1), 4, 3),
    "unknown kind": lambda: (c_format([U8, 5, U16]), 4, 3),
    "unknown uniform kind": lambda: (c_format([255]), 4, 3),
    "unknown layout": lambda: (c_format([U8, U32, U16], layout=2), 4, 3),
    "n_kinds 2 of width 3": lambda: (c_format([U8, U32]), 4, 3),
    "n_kinds 0": lambda: (c_format([], n_kinds=0), 4, 3),
    "n_kinds above width": lambda: (c_format([U8, U32, U16, U8]), 4, 3),
    "stride below the row": lambda: (c_format([U8, U32, U16], stride=6), 4, 3),
    "height 3": lambda: (c_format([U8, U32, U16]), 3, 3),
    "height 0": lambda: (c_format([U8, U32, U16]), 0, 3),
    "height 2^28": lambda: (c_format([U8, U32, U16]), 1 << 28, 3),
    "width 0": lambda: (c_format([U8]), 4, 0),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_format_refusals_need_no_context(lib, what):
    f, height, width = REFUSALS[what]()
    rc, n = format_bytes(lib, f, height, width)
    assert rc == TS_ERR_INVALID, what
    assert n == 0
    assert (lib.ts_last_error(None) or b"") != b"", "the refusal left no text"
    assert lib.ts_trace_format_bytes(C.byref(c_format([U8])), 4, 1, None) == TS_ERR_INVALID  # null result


def test_null_context_is_refused_first(lib):
    out = C.c_void_p(0x1)
    good = c_format([U8, U32, U16])
    buf = C.c_void_p(0x1000)  # never dereferenced: the context is checked first
    for name in ("ts_matrix_upload_packed", "ts_matrix_upload_packed_async", "ts_matrix_from_device_packed"):
        fn = getattr(lib, name)
        assert fn(None, buf, C.byref(good), 4, 3, C.byref(out)) == TS_ERR_INVALID
        assert fn(None, buf, None, 4, 3, C.byref(out)) == TS_ERR_INVALID
        assert fn(None, C.c_void_p(0x1001), C.byref(good), 4, 3, C.byref(out)) == TS_ERR_INVALID
        assert fn(None, buf, C.byref(good), 4, 3, None) == TS_ERR_INVALID
    words = (C.c_uint32 * 4)()
    m = C.c_void_p(0x10)
    assert lib.ts_matrix_download_monty(None, m, 32, words) == TS_ERR_INVALID
    assert lib.ts_matrix_download_monty(None, m, 7, words) == TS_ERR_INVALID


def numpy_decode(buf, kinds, layout, stride, height, width):
    """The definition of the two layouts, independent of TraceFormat.pack: the raw column words."""
    kinds = list(kinds) * width if len(kinds) == 1 else list(kinds)
    out = np.zeros((height, width), dtype=np.uint64)
    row_bytes = sum(SIZE[k] for k in kinds)
    stride = stride or row_bytes
    off = 0
    for c, k in enumerate(kinds):
        s = SIZE[k]
        for r in range(height):
            if layout == ROWS:
                at = r * stride + off
            else:
                at = off + r * s
            out[r, c] = int.from_bytes(bytes(buf[at:at + s]), "little")
        off += s if layout == ROWS else height * s
        if layout == PLANAR:
            off = (off + 15) // 16 * 16
    return out.astype(np.uint32)


@pytest.mark.parametrize("layout,stride", [("rows", 0), ("rows", 23), ("planar", 0)])
def test_pack_round_trips_against_a_numpy_decoder(lib, layout, stride):
    rng = np.random.default_rng(7)
    kinds = [U8, U32, U16, MONTY32, U8, MONTY31, U16]
    height, width = 8, len(kinds)
    values = np.zeros((height, width), dtype=np.uint32)
    for c, k in enumerate(kinds):
        values[:, c] = rng.integers(0, 1 << (8 * SIZE[k]), size=height, dtype=np.uint64).astype(np.uint32)
    values[0] = [0xff, 0xffffffff, 0xffff, 0xffffffff, 0, 0x80000000, 1]
    fmt = ts.TraceFormat(kinds, layout=layout, row_stride=stride)
    buf = fmt.pack(values)
    assert buf.dtype == np.uint8 and buf.size == fmt.nbytes(height, width)
    # a row is 1 + 4 + 2 + 4 + 1 + 4 + 2 = 18 bytes; planar columns of 8, 32, 16, 32, 8, 32, 16 bytes start at
    # 0, 16, 48, 64, 96, 112, 144
    assert fmt.nbytes(height, width) == {"rows": height * (stride or 18), "planar": 160}[layout]
    got = numpy_decode(buf, kinds, ts.TraceFormat.LAYOUTS[layout], stride, height, width)
    assert (got == values).all()
    # one kind for every column
    uni = ts.TraceFormat("u16", layout=layout)
    v16 = rng.integers(0, 1 << 16, size=(4, 5), dtype=np.uint64).astype(np.uint32)
    got = numpy_decode(uni.pack(v16), [U16], ts.TraceFormat.LAYOUTS[layout], 0, 4, 5)
    assert (got == v16).all()


def test_python_surface_exists():
    import inspect

    for name in ("TraceFormat", "PinnedHostBytes"):
        assert name in dir(ts), name
    for m in ("nbytes", "pack"):
        assert callable(getattr(ts.TraceFormat, m)), m
    for m in ("upload_packed", "upload_packed_async", "from_device_packed"):
        assert callable(getattr(ts.DeviceMatrix, m)), m
    sig = inspect.signature(ts.TraceFormat.__init__).parameters
    assert sig["layout"].default == "rows" and sig["row_stride"].default == 0
    assert inspect.signature(ts.DeviceMatrix.download).parameters["monty_bits"].default is None
    with pytest.raises(_lib.TsError):
        ts.TraceFormat(["u8", "u32"]).nbytes(4, 3)
