"""Packed / Montgomery trace ingest on the GPU (ts_matrix_upload_packed and its async / device forms,
ts_matrix_download_monty).  Expected words come from the definition, in numpy uint64 / Python integers: a
column word x is x (u32, u16, u8), x * 2^-32 mod p (monty32) or x * 2^-31 mod p (monty31), p = 0x78000001 --
never from the code under test; equality is exact.  Shapes are the smallest at which the tile logic can go
wrong: heights below, at and above one tile, widths that are no multiple of anything, 4-byte columns at odd
byte offsets, row sizes that are no multiple of 4 or 16, a stride with slack, planar columns."""
import os
import sys

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.airs import (FibonacciAir, SynthMulAir, fibonacci_public_values, generate_fibonacci_trace,
                               generate_synth_mul_trace)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

P = 0x78000001
INV_2_32 = pow(2, -32, P)
INV_2_31 = pow(2, -31, P)
U32, U16, U8, MONTY32, MONTY31 = "u32", "u16", "u8", "monty32", "monty31"
BITS = {U32: 32, U16: 16, U8: 8, MONTY32: 32, MONTY31: 32}
EDGE_WORDS = [0, 1, P - 1, P, 1 << 31, (1 << 32) - 1]
HEIGHTS = [1, 2, 64, 4096]
WIDTHS = [1, 3, 5, 64, 163]
PATTERN = [U8, U32, U16, MONTY32, U8, MONTY31]  # 4-byte columns at byte offsets 1, 7 and 12 of every 16
KIND_SETS = {"u32": [U32], "u16": [U16], "u8": [U8], "monty32": [MONTY32], "monty31": [MONTY31], "alternating": None}
LAYOUTS = {"rows": ("rows", 0), "rows_stride": ("rows", 5), "planar": ("planar", 0)}
CFG = (2, 28, 8)


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def mulmod(x: np.ndarray, k: int) -> np.ndarray:
    """x * k mod p for 32-bit x and k < p, in uint64 without overflow: by 16-bit halves of x."""
    x = x.astype(np.uint64)
    k = np.uint64(k)
    p = np.uint64(P)
    hi = ((x >> np.uint64(16)) * k) % p  # < 2^16 * 2^31
    lo = ((x & np.uint64(0xffff)) * k) % p
    return ((hi * np.uint64(1 << 16)) % p + lo) % p


def expected(words: np.ndarray, kinds) -> np.ndarray:
    """The definition: what each column word stands for, canonical."""
    out = np.zeros(words.shape, dtype=np.uint32)
    for c in range(words.shape[1]):
        k = kinds[c if len(kinds) > 1 else 0]
        col = words[:, c]
        if k == MONTY32:
            out[:, c] = mulmod(col, INV_2_32)
        elif k == MONTY31:
            out[:, c] = mulmod(col, INV_2_31)
        else:
            out[:, c] = col
    return out


def column_words(rng, kinds, height, width) -> np.ndarray:
    """Random words over each column's full range, with the range ends (and for 4-byte kinds 0, 1, p-1, p,
    2^31, 2^32-1) cycled through the first rows."""
    words = np.zeros((height, width), dtype=np.uint32)
    for c in range(width):
        bits = BITS[kinds[c if len(kinds) > 1 else 0]]
        col = rng.integers(0, 1 << bits, size=height, dtype=np.uint64)
        edges = EDGE_WORDS if bits == 32 else [0, 1, (1 << bits) - 1, (1 << bits) - 2]
        for r in range(min(height, len(edges))):
            col[r] = edges[(r + c) % len(edges)]
        words[:, c] = col.astype(np.uint32)
    return words


def kinds_for(name, width):
    return KIND_SETS[name] or [PATTERN[c % len(PATTERN)] for c in range(width)]


def make_format(kinds, layout_name, width):
    layout, slack = LAYOUTS[layout_name]
    stride = 0
    if slack:
        per = kinds * width if len(kinds) == 1 else kinds
        stride = sum(BITS[k] // 8 for k in per) + slack
    return ts.TraceFormat(kinds, layout=layout, row_stride=stride)


def test_the_definition_helper_itself():
    # mulmod against Python integers, so that `expected` is the definition and not a second implementation to trust
    xs = np.array(EDGE_WORDS + [0x12345678, 0xfedcba98], dtype=np.uint32)
    for k in (INV_2_32, INV_2_31, pow(2, 32, P), pow(2, 31, P)):
        assert [int(v) for v in mulmod(xs, k)] == [int(x) * k % P for x in xs]
    assert (1 << 32) * INV_2_32 % P == 1 and (1 << 31) * INV_2_31 % P == 1


@pytest.mark.parametrize("layout_name", sorted(LAYOUTS))
@pytest.mark.parametrize("kind_name", sorted(KIND_SETS))
def test_upload_packed_is_the_definition(ctx, kind_name, layout_name):
    """Every height x width of the grid in one case per (kinds, layout): 20 small uploads."""
    rng = np.random.default_rng(sum(map(ord, kind_name + layout_name)))
    for height in HEIGHTS:
        for width in WIDTHS:
            kinds = kinds_for(kind_name, width)
            fmt = make_format(kinds, layout_name, width)
            words = column_words(rng, kinds, height, width)
            got = ts.DeviceMatrix.upload_packed(ctx, fmt.pack(words), fmt, height, width).download()
            want = expected(words, kinds)
            assert got.shape == want.shape
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (f"{kind_name} {layout_name} {height}x{width}: {len(bad)} words differ, first at "
                                   f"{bad[0]}: got {got[tuple(bad[0])]:#x}, want {want[tuple(bad[0])]:#x}")
            assert (got[:, [c for c in range(width) if kinds[c % len(kinds)] in (MONTY32, MONTY31)]] < P).all()


@pytest.mark.parametrize("shape", ["wide rows", "long stride", "wide planar"])
def test_the_other_tile_paths(ctx, shape):
    """Where the kernel tiles differently: a row of more columns than one tile takes (column tiles, rows layout),
    a stride longer than a tile's bytes (one row per tile) and more planar columns than a tile holds."""
    rng = np.random.default_rng(3)
    height, width, layout, stride = {"wide rows": (2, 5000, "rows", 0), "long stride": (4, 3, "rows", 40000),
                                     "wide planar": (128, 300, "planar", 0)}[shape]
    for kind_name in ("alternating", "u8"):
        kinds = kinds_for(kind_name, width)
        fmt = ts.TraceFormat(kinds, layout=layout, row_stride=stride)
        words = column_words(rng, kinds, height, width)
        got = ts.DeviceMatrix.upload_packed(ctx, fmt.pack(words), fmt, height, width).download()
        assert (got == expected(words, kinds)).all(), f"{shape} {kind_name}"


@pytest.mark.parametrize("layout_name", sorted(LAYOUTS))
def test_async_and_device_forms_give_the_same_words(ctx, layout_name):
    import torch

    rng = np.random.default_rng(11)
    for kind_name in ("alternating", "monty32", "u8"):
        for height, width in ((2, 5), (64, 163), (4096, 3)):
            kinds = kinds_for(kind_name, width)
            fmt = make_format(kinds, layout_name, width)
            words = column_words(rng, kinds, height, width)
            want = expected(words, kinds)
            pinned = ts.PinnedHostBytes(fmt.nbytes(height, width))
            fmt.pack(words, out=pinned.array)
            m = ts.DeviceMatrix.upload_packed_async(ctx, pinned, fmt, height, width)
            assert (m.download() == want).all(), f"async {kind_name} {height}x{width}"  # download synchronises
            dev = torch.from_numpy(fmt.pack(words)).to("cuda")
            torch.cuda.synchronize()
            assert dev.dtype == torch.uint8 and dev.data_ptr() % 16 == 0
            m = ts.DeviceMatrix.from_device_packed(ctx, dev.data_ptr(), fmt, height, width)
            assert (m.download() == want).all(), f"device {kind_name} {height}x{width}"


def test_refusals_with_a_context_leave_a_text(ctx):
    fmt = ts.TraceFormat([U8, U32, U16])
    buf = np.zeros(64 + 16, dtype=np.uint8)
    base = buf.ctypes.data
    aligned = buf[(-base) % 16:][:64]
    assert aligned.ctypes.data % 16 == 0
    ts.DeviceMatrix.upload_packed(ctx, aligned[:28], fmt, 4, 3)  # the same call, accepted
    cases = {
        "not 16-byte aligned": lambda: ts.DeviceMatrix.upload_packed(ctx, buf[(-base) % 16 + 1:][:28], fmt, 4, 3),
        "power of two": lambda: ts.DeviceMatrix.upload_packed(ctx, aligned, fmt, 3, 3),
        "n_kinds": lambda: ts.DeviceMatrix.upload_packed(ctx, aligned, fmt, 4, 2),
        "row_stride": lambda: ts.DeviceMatrix.upload_packed(ctx, aligned, ts.TraceFormat([U8, U32, U16], row_stride=6), 4, 3),
        "unknown column kind": lambda: ts.DeviceMatrix.upload_packed(ctx, aligned, ts.TraceFormat([9]), 4, 3),
        "unknown layout": lambda: ts.DeviceMatrix.upload_packed(ctx, aligned, ts.TraceFormat([U8], layout=7), 4, 3),
        "monty_bits": lambda: ts.DeviceMatrix.upload(ctx, np.ones((2, 2), dtype=np.uint32)).download(monty_bits=30),
    }
    for text, call in cases.items():
        with pytest.raises(_lib.TsError) as e:
            call()
        assert e.value.code == 1 and text in str(e.value), (text, str(e.value))


def test_download_monty_and_back(ctx):
    rng = np.random.default_rng(5)
    canon = rng.integers(0, P, size=(64, 37), dtype=np.uint64).astype(np.uint32)
    canon[0, :4] = [0, 1, P - 1, 2]
    m = ts.DeviceMatrix.upload(ctx, canon)
    for bits, inv in ((32, INV_2_32), (31, INV_2_31)):
        mont = m.download(monty_bits=bits)
        assert (mont < P).all()
        assert (mulmod(mont, inv) == canon).all(), f"radix {bits}: word * 2^-{bits} is not the value"
        kind = MONTY32 if bits == 32 else MONTY31
        fmt = ts.TraceFormat(kind)
        back = ts.DeviceMatrix.upload_packed(ctx, fmt.pack(mont), fmt, *canon.shape).download()
        assert (back == canon).all(), f"radix {bits}: upload of the download is not the identity"
    assert (m.download() == canon).all()


def same(proof, want):
    return len(proof.words) == len(want.words) and bool((proof.words == want.words).all())


def test_fibonacci_proof_from_monty_words_and_from_planar_u32(ctx):
    trace = generate_fibonacci_trace(0, 1, 1 << 8)
    pis = fibonacci_public_values(trace)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), ctx))
    air = ts.CompiledAir(ctx, ts.air_tape(FibonacciAir(), len(pis)))
    ch0 = ts.BfChallenger()
    want = ts.prove(config, air, ch0, ts.DeviceMatrix.upload(ctx, trace), pis)
    monty = mulmod(trace, pow(2, 32, P)).astype(np.uint32)  # the words a Montgomery host holds for these values
    for name, fmt, words in (("monty32", ts.TraceFormat(MONTY32), monty),
                             ("planar u32", ts.TraceFormat(U32, layout="planar"), trace)):
        m = ts.DeviceMatrix.upload_packed(ctx, fmt.pack(words), fmt, *trace.shape)
        ch = ts.BfChallenger()
        proof = ts.prove(config, air, ch, m, pis)
        assert same(proof, want), f"{name}: proof words differ from the proof of the uploaded trace"
        assert (ch.state() == ch0.state()).all(), f"{name}: final challenger state"


def test_synth_mul_trace_enters_prove_batch_through_upload_packed_async(ctx):
    trace = generate_synth_mul_trace(1 << 10)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), ctx))
    air = ts.CompiledAir(ctx, ts.air_tape(SynthMulAir(64), 0))
    ch0 = ts.BfChallenger()
    want = ts.prove(config, air, ch0, ts.DeviceMatrix.upload(ctx, trace), [])
    # columns at the smallest size that holds them (the `a` columns are 16-bit at this height), Montgomery words
    # for every fourth of the rest
    kinds, words = [], trace.copy()
    for c in range(trace.shape[1]):
        top = int(trace[:, c].max())
        if top < (1 << 16):
            kinds.append(U16)
        elif c % 4 == 1:
            kinds.append(MONTY31)
            words[:, c] = mulmod(trace[:, c], pow(2, 31, P))
        else:
            kinds.append(U32)
    assert U16 in kinds and MONTY31 in kinds and U32 in kinds
    fmt = ts.TraceFormat(kinds)
    pinned = ts.PinnedHostBytes(fmt.nbytes(*trace.shape))
    fmt.pack(words, out=pinned.array)
    m = ts.DeviceMatrix.upload_packed_async(ctx, pinned, fmt, *trace.shape)
    res = ts.prove_batch([(config, air)], [m], [0])
    assert res.rc == 0 and same(res.proofs[0], want)
    assert (res.final_states[0] == ch0.state()).all()


def test_cpp_stream_example_packed_mode(ctx, tmp_path):
    """examples/prove_stream.cpp `packed`: the lanes of its `pinned` mode with the trace held at its columns'
    own sizes in page-locked memory; the same proofs."""
    import re
    import subprocess

    from test_abi_cpu import _build_example
    exe = _build_example(tmp_path, "prove_stream")
    digests, dumps = {}, {}
    for mode in ("pinned", "packed"):
        out_bin = str(tmp_path / f"stream_{mode}.bin")
        r = subprocess.run([exe, "10", "6", "2", mode, out_bin], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "all proofs identical" in r.stdout and "verify -> 0" in r.stdout
        digests[mode] = re.search(r"proof digest ([0-9a-f]{16})", r.stdout).group(1)
        dumps[mode] = np.fromfile(out_bin, dtype=np.uint32)
    assert "ts_matrix_upload_packed_async" in r.stdout and re.search(r"packed to \d+ of \d+ bytes", r.stdout)
    assert digests["packed"] == digests["pinned"]
    assert len(dumps["packed"]) == len(dumps["pinned"]) and (dumps["packed"] == dumps["pinned"]).all()
