"""CPU-side checks of ts_matrix_collect_rows (include/tapstark.h "collected rows"): the reference of
tests/_collect_cases.py against hand-written values, ts_collect_rows_host -- the library's sequential loop over host
rows -- against that reference at every source count, height, emitter count and term kind, the height rules, every
refusal that needs no matrix, the symbols, the builders, and the same loop in a stand-alone program under the
sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tapstark_amd import _lib
from tapstark_amd._lib import TsError
from tapstark_amd.airs import (MEM_TAG, MemoryAccessAir, MemoryCpuAir, generate_memory_cpu_trace,
                               memory_cpu_collect_spec)
from tapstark_amd.collect import ALWAYS, MAGIC, ROW, CollectSpec, col, collect_check, collect_rows_host, const

import _collect_cases as cc
from _collect_cases import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_BUFFER = 1, 6


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]}: "
                           f"{int(got[tuple(bad[0])]):#x} for {int(want[tuple(bad[0])]):#x}")


def check(spec, sources, out_height=0, what=""):
    got, live = collect_rows_host(spec, sources, out_height)
    want, want_live = cc.reference(spec, sources, out_height)
    assert live == want_live, what
    same(got, want, what)
    return got, live


# ------------------------------------------------------------------ 1. the reference, by hand
def test_reference_by_hand():
    a = np.array([[10, 1, 7], [11, 0, 8], [12, P, 9], [13, 0xFFFFFFFF, P + 5]], dtype=np.uint32)
    b = np.array([[100, 2 * P], [101, P + 1]], dtype=np.uint32)
    spec = CollectSpec([3, 2], 3, pad=[5, 6, 7])
    spec.emit(1, when=col(1), terms=[col(0), ROW, 1])            # written first, comes last: source 1
    spec.emit(0, when=col(1), terms=[col(0), ROW, col(2)])
    spec.emit(0, when=ALWAYS, terms=[const(P + 3), col(1), ROW])
    out, live = cc.reference(spec, [a, b])
    assert live == 7 and out.tolist() == [
        [10, 0, 7], [3, 1, 0],                    # row 0 of source 0: both emitters, in spec order
        [3, 0, 1],                                # row 1: column 1 is 0
        [3, P, 2],                                # row 2: p is a zero; the copied word stays p
        [13, 3, P + 5], [3, 0xFFFFFFFF, 3],       # row 3: 0xFFFFFFFF fires; words are copied as stored
        [101, 1, 1],                              # source 1: 2p is a zero, p + 1 fires
        [5, 6, 7]]                                # padded to 8 rows
    assert cc.reference(spec, [a, b], 16)[0].shape == (16, 3) and cc.reference(spec, [a, b], 16)[0][7:].tolist() == [[5, 6, 7]] * 9
    with pytest.raises(ValueError, match="7 rows selected, out_height 4"):
        cc.reference(spec, [a, b], 4)
    nothing = CollectSpec([2], 2, pad=[9, 8]).emit(0, when=col(1), terms=[1, 2])
    assert cc.reference(nothing, [b[:1]])[0].tolist() == [[9, 8]] and cc.reference(nothing, [b[:1]])[1] == 0


def test_host_loop_by_hand(lib):
    a = np.array([[10, 1, 7], [11, 0, 8], [12, P, 9], [13, 0xFFFFFFFF, P + 5]], dtype=np.uint32)
    spec = CollectSpec([3], 2).emit(0, when=col(1), terms=[col(2), ROW]).emit(0, terms=[7, col(0)])
    got, live = collect_rows_host(spec, [a])
    assert live == 6 and got.tolist() == [[7, 0], [7, 10], [7, 11], [7, 12], [P + 5, 3], [7, 13], [0, 0], [0, 0]]


# ------------------------------------------------------------------ 2. the host loop against the reference
@pytest.mark.parametrize("height", [1, 3, 1000])
@pytest.mark.parametrize("n_emitters", [1, 16])
@pytest.mark.parametrize("n_sources", [1, 2, 3, 4])
def test_host_loop_against_the_reference(lib, n_sources, n_emitters, height):
    widths = [3, 1, 17, 6][:n_sources]
    heights = [height, 3, 1, 100][:n_sources]
    kinds = set()
    for seed in range(2):
        sources = [cc.random_rows(100 * seed + s, heights[s], widths[s], density=[0.5, 0.9][seed])
                   for s in range(n_sources)]
        for out_width in (1, 5, 64):
            spec = cc.random_spec(seed + out_width, widths, n_emitters, out_width)
            kinds |= {(k, s[0]) for _, s, terms in spec.emitters for k, _ in terms}
            check(spec, sources, what=f"seed {seed} out_width {out_width}")
    assert {k for k, _ in kinds} == {0, 1, 2}, "every term kind"


def test_selector_words_decide_mod_p(lib):
    words = np.array(cc.SELECTOR_WORDS + [2, P - 1, P + 2, 1 << 31], dtype=np.uint32)
    rows = np.stack([words, np.arange(len(words), dtype=np.uint32)], axis=1)
    got, live = check(CollectSpec([2], 2).emit(0, when=col(0), terms=[col(0), col(1)]), [rows])
    fired = [int(w) for w in words if int(w) % P]
    assert live == len(fired) == 7 and got[:live, 0].tolist() == fired  # 0, p and 2p are silent, the rest is kept as stored


def test_one_array_as_two_sources(lib):
    rows = cc.random_rows(5, 37, 4)
    spec = CollectSpec([4, 4], 3).emit(1, when=col(0), terms=[col(1), ROW, 1]).emit(0, when=col(0), terms=[col(2), ROW, 0])
    got, live = check(spec, [rows, rows])
    assert (got[:live // 2, 2] == 0).all() and (got[live // 2:live, 2] == 1).all()


# ------------------------------------------------------------------ 3. heights
def test_heights(lib):
    rows = cc.random_rows(9, 100, 3, density=0.4)
    spec = CollectSpec([3], 2, pad=[P - 1, 3]).emit(0, when=col(0), terms=[ROW, col(1)])
    _, live = cc.reference(spec, [rows])
    assert 20 < live < 64
    got, _ = check(spec, [rows], 0)
    assert got.shape == (64, 2) and (got[live:] == [P - 1, 3]).all()
    assert check(spec, [rows], 64)[0].shape == (64, 2)
    assert check(spec, [rows], 1 << 10)[0].shape == (1 << 10, 2)
    exact = rows[:64].copy()
    exact[:, 0] = 1
    got, live = check(spec, [exact], 64)
    assert live == 64 and got.shape == (64, 2), "no pad row"
    assert check(spec, [exact], 0)[0].shape == (64, 2)
    assert check(spec, [np.concatenate([exact, exact[:1]])], 0)[0].shape == (128, 2)


def test_too_small_is_refused_and_nothing_is_written(lib):
    rows = np.ones((9, 1), dtype=np.uint32)
    t = CollectSpec([1], 1).emit(0, when=col(0), terms=[ROW]).tape()
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    used, live = C.c_uint64(77), C.c_uint64(77)
    ptrs = (_lib.u32p * 1)(rows.ctypes.data_as(_lib.u32p))
    heights = (C.c_uint64 * 1)(9)

    def call(out_height, cap=64):
        return lib.ts_collect_rows_host(t.ctypes.data_as(_lib.u32p), len(t), ptrs, heights, out_height,
                                        out.ctypes.data_as(_lib.u32p), cap, C.byref(used), C.byref(live))

    assert call(8) == TS_ERR_INVALID
    assert lib.ts_last_error(None).decode() == "collect: 9 rows selected, out_height 8"
    assert (out == 0xABABABAB).all() and used.value == 0 and live.value == 0
    assert call(16, cap=15) == TS_ERR_BUFFER
    assert "fewer than height * out_width words" in lib.ts_last_error(None).decode()
    assert (out == 0xABABABAB).all(), "a call that found the buffer too small wrote into it"
    assert call(0, cap=15) == TS_ERR_BUFFER and (out == 0xABABABAB).all()
    assert call(16, cap=16) == 0 and (used.value, live.value) == (16, 9)
    assert out[:16].tolist() == list(range(9)) + [0] * 7 and (out[16:] == 0xABABABAB).all()


def test_nothing_selected_gives_one_pad_row(lib):
    rows = np.zeros((50, 2), dtype=np.uint32)
    rows[::2, 0] = P
    got, live = check(CollectSpec([2], 3, pad=[4, 5, 6]).emit(0, when=col(0), terms=[1, 2, 3]), [rows])
    assert live == 0 and got.tolist() == [[4, 5, 6]]


# ------------------------------------------------------------------ 4. refusals
def good():
    return CollectSpec([3, 2], 2, pad=[1, 2]).emit(0, when=col(2), terms=[col(0), ROW]).emit(1, terms=[const(5), col(1)])


def words(**changes):
    """The good tape with single words replaced: index -> word."""
    t = good().tape().copy()
    for at, word in changes.items():
        t[int(at[1:])] = word
    return t


# the good tape: [0..4] header, [5..6] src widths, [7..8] pad, emitter 0 at 9 (source, sel kind, sel value, 2 terms),
# emitter 1 at 16
REFUSALS = [
    ("bad magic", words(w0=MAGIC + 1)),
    ("unknown spec version 2", words(w1=2)),
    ("n_sources 0 outside [1, 4]", words(w2=0)),
    ("n_sources 5 outside [1, 4]", words(w2=5)),
    ("n_emitters 0 outside [1, 16]", words(w3=0)),
    ("n_emitters 17 outside [1, 16]", words(w3=17)),
    ("out_width 0 outside [1, 64]", words(w4=0)),
    ("out_width 65 outside [1, 64]", words(w4=65)),
    ("23 words, the header asks for 30", words(w3=3)),
    ("22 words, the header asks for 23", good().tape()[:-1]),
    ("shorter than its header", good().tape()[:4]),
    ("source 1: src_width outside [1, 2^16]", words(w6=0)),
    ("source 0: src_width outside [1, 2^16]", words(w5=(1 << 16) + 1)),
    ("pad word 1 is not below p", words(w8=P)),
    ("emitter 0: source 2 outside the spec's sources", words(w9=2)),
    ("emitter 0: selector kind must be 0 (always) or 1 (column)", words(w10=2)),
    ("emitter 1: a constant selector must be 1", words(w18=0)),
    ("emitter 1: a constant selector must be 1", words(w18=2)),
    ("emitter 0: the selector column is outside the source", words(w11=3)),
    ("emitter 0: term 1: kind must be 0 (constant), 1 (column) or 2 (row index)", words(w14=3)),
    ("emitter 1: term 0: the constant is not below p", words(w20=P)),
    ("emitter 1: term 1: the column is outside the source", words(w22=2)),
    ("emitter 0: term 0: the column is outside the source", words(w13=3)),
    ("emitter 0: term 1: the value word of a row index must be 0", words(w15=1)),
]


@pytest.mark.parametrize("text,tape", REFUSALS, ids=[f"{k}-{t[:40]}" for k, (t, _) in enumerate(REFUSALS)])
def test_every_matrix_free_refusal(lib, text, tape):
    assert collect_check(good()) == (2, 2)
    with pytest.raises(TsError) as e:
        collect_check(tape)
    assert e.value.code == TS_ERR_INVALID and text in str(e.value), str(e.value)
    # the host loop makes the same checks first and writes nothing
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    a, b = np.ones((2, 3), dtype=np.uint32), np.ones((2, 2), dtype=np.uint32)
    ptrs = (_lib.u32p * 4)(*[m.ctypes.data_as(_lib.u32p) for m in (a, b, b, b)])
    heights = (C.c_uint64 * 4)(2, 2, 2, 2)
    used, live = C.c_uint64(), C.c_uint64()
    tape = np.ascontiguousarray(tape, dtype=np.uint32)
    assert lib.ts_collect_rows_host(tape.ctypes.data_as(_lib.u32p), len(tape), ptrs, heights, 0,
                                    out.ctypes.data_as(_lib.u32p), 64, C.byref(used), C.byref(live)) == TS_ERR_INVALID
    assert text in lib.ts_last_error(None).decode() and (out == 0xABABABAB).all()


def test_host_call_refusals(lib):
    t = good().tape()
    a, b = np.ones((2, 3), dtype=np.uint32), np.ones((2, 2), dtype=np.uint32)
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    used, live = C.c_uint64(), C.c_uint64()
    p = lambda m: m.ctypes.data_as(_lib.u32p)  # noqa: E731

    def refused(text, spec_p=p(t), srcs=(a, b), hs=(2, 2), out_height=0, out_p=p(out), used_p=C.byref(used),
                live_p=C.byref(live), null_sources=False, null_heights=False):
        ptrs = (_lib.u32p * 2)(*[p(m) if m is not None else None for m in srcs])
        heights = (C.c_uint64 * 2)(*hs)
        st = lib.ts_collect_rows_host(spec_p, len(t), None if null_sources else ptrs, None if null_heights else heights,
                                      out_height, out_p, 64, used_p, live_p)
        assert st == TS_ERR_INVALID and text in lib.ts_last_error(None).decode(), lib.ts_last_error(None)
        assert (out == 0xABABABAB).all(), "a refused call wrote into the buffer"

    refused("null", spec_p=None)
    refused("null argument", null_sources=True)
    refused("null argument", null_heights=True)
    refused("null argument", out_p=None)
    refused("null argument", used_p=None)
    refused("null argument", live_p=None)
    refused("null argument", srcs=(a, None))
    refused("the height of source 1 must be in [1, 2^27]", hs=(2, 0))
    refused("the height of source 0 must be in [1, 2^27]", hs=((1 << 27) + 1, 2))
    for bad in (3, 6, (1 << 27) + 1, 1 << 28, 1 << 63):
        refused(f"out_height {bad} is neither 0 nor a power of two in [1, 2^27]", out_height=bad)
    assert lib.ts_collect_check(None, 5, None, None) == TS_ERR_INVALID
    assert lib.ts_collect_check(p(t), len(t), None, None) == 0, "both outputs may be null"


def test_null_context_refused(lib):
    t = good().tape()
    fake = C.create_string_buffer(64)  # never dereferenced: the null context is refused first
    handles = (C.c_void_p * 4)(C.addressof(fake), C.addressof(fake))
    out, live = C.c_void_p(12345), C.c_uint64(77)
    assert lib.ts_matrix_collect_rows(None, t.ctypes.data_as(_lib.u32p), len(t), handles, 0, C.byref(out),
                                      C.byref(live)) == TS_ERR_INVALID
    assert out.value is None and live.value == 0, "a refused call left a handle"
    assert lib.ts_matrix_collect_rows(None, None, 0, None, 0, None, None) == TS_ERR_INVALID


# ------------------------------------------------------------------ 5. the ABI and the builders
def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "tapstark-gpu", "src", "ffi.rs")).read()
    for name in ("ts_matrix_collect_rows", "ts_collect_check", "ts_collect_rows_host"):
        assert hasattr(lib, name) and name in _lib.ABI_SYMBOLS
        assert f"ts_status {name}(" in header and f"pub fn {name}(" in ffi
    assert lib.ts_abi_version() == 5
    assert "enum { TS_COLLECT_MAX_SOURCES = 4, TS_COLLECT_MAX_EMITTERS = 16, TS_COLLECT_MAX_WIDTH = 64 };" in header
    assert "has not been compiled" in ffi
    assert header.index("---- scanned columns") < header.index("---- collected rows") < header.index("ts_abi_version")


CPP_COLLECT = r"""
#include <stdio.h>
#include "tapstark_air.hpp"
int main() {
    using ts::air::Collect;
    Collect c({10, 3}, 3, {7});
    c.emit(1, Collect::col(2), {Collect::col(0), Collect::row(), Collect::constant(0x78000001ull + 3)});
    c.emit(0, Collect::always(), {Collect::constant(1), Collect::col(9), Collect::row()});
    for (uint32_t w : c.tape()) printf("%u\n", w);
    return 0;
}
"""


def test_cpp_builder_writes_the_python_tape(lib, tmp_path):
    src = tmp_path / "collect.cpp"
    src.write_text(CPP_COLLECT)
    exe = str(tmp_path / "collect")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    spec = CollectSpec([10, 3], 3, pad=[7, 0, 0]).emit(1, when=col(2), terms=[col(0), ROW, const(P + 3)])
    spec.emit(0, when=ALWAYS, terms=[1, col(9), ROW])
    assert got == spec.tape().tolist()
    assert collect_check(spec) == (2, 3)


def test_memory_cpu_trace_collects_to_the_access_table(lib):
    """The two slots of every CPU row, selected, reshaped and stacked by the host loop: an access table in execution
    order whose first access of every address is a write and whose reads return the last written value."""
    A, M = MemoryCpuAir, MemoryAccessAir
    n = 300
    cpu = generate_memory_cpu_trace(n, 9, 5)
    assert cpu.shape == (n, A.WIDTH) and (cpu[:, A.CLK] == np.arange(n)).all()
    assert (cpu[:, A.TS_A] == 2 * np.arange(n)).all() and (cpu[:, A.TS_B] == 2 * np.arange(n) + 1).all()
    for c in (A.SEL_A, A.SEL_B, A.WR_B):
        assert set(cpu[:, c].tolist()) == {0, 1}
    table, live = collect_rows_host(memory_cpu_collect_spec(), [cpu])
    assert live == int(cpu[:, A.SEL_A].sum() + cpu[:, A.SEL_B].sum()) and 0 < live < 2 * n
    assert table.shape == (512, 5) and not table[live:].any()
    acc = table[:live]
    assert (np.diff(acc[:, M.CLK].astype(np.int64)) > 0).all(), "execution order: timestamps ascend"
    assert (acc[:, M.SEL] == 1).all()
    memory = {}
    for addr, _, value, is_write, _ in acc.tolist():
        if is_write:
            memory[addr] = value
        else:
            assert memory[addr] == value, "a read returns the last written value"
    same(table, cc.reference(memory_cpu_collect_spec(), [cpu])[0])
    assert MEM_TAG == 11


# ------------------------------------------------------------------ 6. under the sanitizers
def _case_words(tape, sources, heights, out_height):
    out = [len(tape), *[int(w) for w in tape], out_height, len(sources)]
    for rows, h in zip(sources, heights):
        out += [h, rows.size, *rows.reshape(-1).tolist()]
    return out


def test_checks_and_host_loop_are_clean_under_the_sanitizers(lib, tmp_path):
    """csrc/collect.cpp and tap-stark_amd/probe/collect_probe.cpp built together with AddressSanitizer and UBSan into
    a stand-alone program and run over the seeded cases above, the height cases and every refused tape, each in
    buffers of exactly its size: every line is what the reference gives and no sanitizer report ends the run."""
    from tapstark_amd import build as b

    exe = str(tmp_path / "collect_probe")
    cmd = [b._clangxx(), "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(b._rocm(), "include"), "-I", b.CSRC,
           "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(b.PKG, "probe", "collect_probe.cpp"),
           os.path.join(b.CSRC, "collect.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def fnv(a):
        h = 0xcbf29ce484222325
        for byte in np.ascontiguousarray(a, dtype="<u4").tobytes():
            h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return h

    cases, want = [], []
    widths, heights = [3, 1, 17, 6], [1000, 3, 1, 37]
    for seed in range(4):
        for n_sources, n_emitters, out_width in ((1, 1, 1), (2, 16, 5), (4, 16, 64), (3, 7, 2)):
            sources = [cc.random_rows(seed + 10 * s, heights[s], widths[s], density=0.3 * seed) for s in range(n_sources)]
            spec = cc.random_spec(seed, widths[:n_sources], n_emitters, out_width)
            for out_height in (0, 1 << 15, 4):
                cases.append(_case_words(spec.tape(), sources, heights, out_height))
                try:
                    m, live = cc.reference(spec, sources, out_height)
                    want.append(f"{m.shape[0]} {live} {fnv(m):016x}")
                except ValueError as e:
                    want.append(f"refused: {e}")
    a, b2 = np.ones((2, 3), dtype=np.uint32), np.ones((2, 2), dtype=np.uint32)
    for text, tape in REFUSALS:
        cases.append(_case_words(tape, [a, b2], [2, 2], 0))
        want.append(text)
    path = tmp_path / "cases.bin"
    np.array([len(cases)] + [w for c in cases for w in c], dtype="<u4").tofile(str(path))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(want)
    for k, (got, w) in enumerate(zip(lines, want)):
        assert (w in got and got.startswith("refused: ")) if k >= len(want) - len(REFUSALS) else got == w, (k, got, w)
    assert any(l.startswith("refused: collect: ") and "rows selected, out_height 4" in l for l in lines)
