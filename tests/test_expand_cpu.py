"""CPU-side checks of ts_matrix_expand_rows (include/tapstark.h "expanded rows"): the reference of
tests/_expand_cases.py against hand-written values, ts_expand_rows_host -- the library's sequential loop over host rows
-- against that reference at every width and term kind, the height rules, every refusal that needs no matrix, the two
late refusals with their exact numbers, the symbols, the builders, the span AIRs on host-made traces, and the same loop
in a stand-alone program under the sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tapstark_amd import _lib
from tapstark_amd._lib import TsError
from tapstark_amd.air import aux_dims, get_symbolic_constraints
from tapstark_amd.airs import (BUS_TAG, SPAN_TAG, BusRangeAir, NumericBuilder, SpanCallAir, SpanChipAir,
                               generate_span_call_trace, generate_span_chip_trace, span_expand_spec)
from tapstark_amd.expand import (ALWAYS, FIRST, J, LAST, MAGIC, REMAINING, ROW, ExpandSpec, col, const, expand_check,
                                 expand_rows_host, stepped)

import _expand_cases as xc
from _expand_cases import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_INVARIANT, TS_ERR_BUFFER = 1, 5, 6


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


def check(spec, src, out_height=0, what=""):
    got, live = expand_rows_host(spec, src, out_height)
    want, want_live = xc.reference(spec, src, out_height)
    assert live == want_live, what
    same(got, want, what)
    return got, live


ALL_TERMS = [const(P + 3), col(0), ROW, J, REMAINING, FIRST, LAST, stepped(0, 1), stepped(0, P - 1)]


# ------------------------------------------------------------------ 1. by hand
def by_hand():
    src = np.array([[10, 2, 1], [P - 1, 5, 0], [12, P + 3, 0xFFFFFFFF], [13, P, 1], [0xFFFFFFFF, 1, P + 1]],
                   dtype=np.uint32)
    spec = ExpandSpec(3, 9, count=col(1), when=col(2), max_count=3, pad=[9, 8, 7, 6, 5, 4, 3, 2, 1], terms=ALL_TERMS)
    want = [
        [3, 10, 0, 0, 1, 1, 0, 10, 10], [3, 10, 0, 1, 0, 0, 1, 11, 9],          # row 0 asks for 2
        # row 1 takes no part: its 5 is over max_count and is not looked at
        [3, 12, 2, 0, 2, 1, 0, 12, 12], [3, 12, 2, 1, 1, 0, 0, 13, 11], [3, 12, 2, 2, 0, 0, 1, 14, 10],  # p + 3 is 3
        # row 3 asks for p rows: 0
        [3, 0xFFFFFFFF, 4, 0, 0, 1, 1, (1 << 28) - 3, (1 << 28) - 3],             # 0xFFFFFFFF mod p; kept as stored
        [9, 8, 7, 6, 5, 4, 3, 2, 1], [9, 8, 7, 6, 5, 4, 3, 2, 1]]
    return spec, src, want


def test_reference_by_hand():
    spec, src, want = by_hand()
    out, live = xc.reference(spec, src)
    assert live == 6 and out.tolist() == want
    assert xc.reference(spec, src, 16)[0].shape == (16, 9) and xc.reference(spec, src, 16)[0][6:].tolist() == [want[-1]] * 10
    with pytest.raises(ValueError, match="6 rows asked for, out_height 4"):
        xc.reference(spec, src, 4)
    src[1, 2] = 1
    with pytest.raises(ValueError, match="row 1 asks for 5 rows, max_count 3"):
        xc.reference(spec, src, 4)  # the first refusal wins
    assert 0xFFFFFFFF % P == (1 << 28) - 3


def test_host_loop_by_hand(lib):
    spec, src, want = by_hand()
    got, live = expand_rows_host(spec, src)
    assert live == 6 and got.tolist() == want
    # the stepped word wraps at p: p - 1 + 1 = 0, and p - 1 steps of p - 1 back
    wrap = ExpandSpec(1, 3, count=3, max_count=3, terms=[stepped(0, 1), stepped(0, P - 1), col(0)])
    got, live = expand_rows_host(wrap, np.array([[P - 1], [P]], dtype=np.uint32))
    assert live == 6 and got[:6].tolist() == [[P - 1, P - 1, P - 1], [0, P - 2, P - 1], [1, P - 3, P - 1],
                                              [0, 0, P], [1, P - 1, P], [2, P - 2, P]]


# ------------------------------------------------------------------ 2. the host loop against the reference
@pytest.mark.parametrize("height", [1, 3, 1000, (1 << 12) + 1])
@pytest.mark.parametrize("src_width", [1, 3, 17])
def test_host_loop_against_the_reference(lib, src_width, height):
    kinds = set()
    for seed in range(2):
        src = xc.random_rows(100 * seed + src_width, height, src_width, density=[0.5, 0.9][seed])
        for out_width in (1, 5, 64):
            spec = xc.random_spec(seed + out_width, src_width, out_width)
            kinds |= {xc._term(t)[0] for t in spec.terms}
            check(spec, src, what=f"seed {seed} out_width {out_width}")
    assert kinds == set(range(8)), "every term kind"


def test_words_decide_mod_p(lib):
    sel = np.array(xc.QUIET + xc.LOUD + [2, P - 1], dtype=np.uint32)
    cnt = np.array([1, 2, 3, P, P + 3, 2 * P, 2 * P + 1, 0], dtype=np.uint32)
    src = np.stack([sel, cnt, np.arange(8, dtype=np.uint32)], axis=1)
    got, live = check(ExpandSpec(3, 3, count=col(1), when=col(0), max_count=3, terms=[col(2), col(1), J]), src)
    # rows 0 .. 2 are quiet; p and 2p ask for nothing, p + 3 for 3, 2p + 1 for 1; the copied word stays as stored
    assert live == 4 and got[:4].tolist() == [[4, P + 3, 0], [4, P + 3, 1], [4, P + 3, 2], [6, 2 * P + 1, 0]]
    got, live = check(ExpandSpec(3, 1, count=col(1), when=ALWAYS, max_count=3, terms=[col(2)]), src)
    assert got[:live, 0].tolist() == [0, 1, 1, 2, 2, 2, 4, 4, 4, 6]


# ------------------------------------------------------------------ 3. heights
def test_heights(lib):
    src = xc.random_rows(9, 20, 3, max_count=4)
    spec = ExpandSpec(3, 2, count=col(1), when=col(0), max_count=4, pad=[P - 1, 3], terms=[ROW, J])
    _, live = xc.reference(spec, src)
    assert 8 < live < 32
    got, _ = check(spec, src, 0)
    assert got.shape == (32, 2) and (got[live:] == [P - 1, 3]).all()
    assert check(spec, src, 32)[0].shape == (32, 2)
    assert check(spec, src, 1 << 10)[0].shape == (1 << 10, 2)
    exact = np.ones((16, 3), dtype=np.uint32)
    exact[:, 1] = 4
    got, live = check(spec, exact, 64)
    assert live == 64 and got.shape == (64, 2), "no pad row"
    assert check(spec, exact, 0)[0].shape == (64, 2)
    exact[0, 1] = 3
    assert check(spec, exact, 0)[0].shape == (64, 2)
    assert check(spec, np.concatenate([exact, exact[1:3]]), 0)[0].shape == (128, 2)


def test_nothing_asked_for_gives_one_pad_row(lib):
    src = np.zeros((50, 2), dtype=np.uint32)
    src[::2, 1] = P
    src[:, 0] = 1
    got, live = check(ExpandSpec(2, 3, count=col(1), when=col(0), max_count=1, pad=[4, 5, 6], terms=[1, 2, 3]), src)
    assert live == 0 and got.tolist() == [[4, 5, 6]]


def _host_call(lib, tape, src, out_height, out, cap, used, live):
    tape = np.ascontiguousarray(tape, dtype=np.uint32)
    return lib.ts_expand_rows_host(tape.ctypes.data_as(_lib.u32p), len(tape), src.ctypes.data_as(_lib.u32p), len(src),
                                   out_height, out.ctypes.data_as(_lib.u32p), cap, C.byref(used), C.byref(live))


def test_late_refusals_on_the_host_loop_and_nothing_is_written(lib):
    src = np.full((9, 1), 2, dtype=np.uint32)
    t = ExpandSpec(1, 1, count=col(0), max_count=5, terms=[J]).words()
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    used, live = C.c_uint64(77), C.c_uint64(77)
    call = lambda out_height, cap=64, s=src: _host_call(lib, t, s, out_height, out, cap, used, live)  # noqa: E731

    assert call(16) == TS_ERR_INVALID
    assert lib.ts_last_error(None).decode() == "expand: 18 rows asked for, out_height 16"
    assert (out == 0xABABABAB).all() and used.value == 0 and live.value == 0
    two = src.copy()
    two[[3, 7], 0] = [6, 0xFFFFFFFF]
    assert call(16, s=two) == TS_ERR_INVARIANT, "the first refusal wins"
    assert lib.ts_last_error(None).decode() == "expand: row 3 asks for 6 rows, max_count 5"
    two[3, 0] = 5
    assert call(0, s=two) == TS_ERR_INVARIANT
    assert lib.ts_last_error(None).decode() == f"expand: row 7 asks for {(1 << 28) - 3} rows, max_count 5"
    assert (out == 0xABABABAB).all() and used.value == 0 and live.value == 0
    assert call(32, cap=31) == TS_ERR_BUFFER
    assert "fewer than height * out_width words" in lib.ts_last_error(None).decode()
    assert (out == 0xABABABAB).all(), "a call that found the buffer too small wrote into it"
    assert call(0, cap=31) == TS_ERR_BUFFER and (out == 0xABABABAB).all()
    assert call(32, cap=32) == 0 and (used.value, live.value) == (32, 18)
    assert out[:32].tolist() == [0, 1] * 9 + [0] * 14 and (out[32:] == 0xABABABAB).all()


def test_the_total_is_exact_past_32_bits(lib):
    """64 rows of 2^26 and 1024 rows of 2^22: 2^32 rows each, a total that a 32-bit sum would wrap to 0."""
    out = np.full(4, 0xABABABAB, dtype=np.uint32)
    used, live = C.c_uint64(), C.c_uint64()
    for rows, each in ((64, 1 << 26), (1024, 1 << 22), (3, (1 << 27) - 1)):
        t = ExpandSpec(1, 1, count=col(0), max_count=1 << 27, terms=[J]).words()
        src = np.full((rows, 1), each, dtype=np.uint32)
        for out_height, said in ((0, 1 << 27), (1 << 20, 1 << 20)):
            assert _host_call(lib, t, src, out_height, out, 4, used, live) == TS_ERR_INVALID
            assert lib.ts_last_error(None).decode() == f"expand: {rows * each} rows asked for, out_height {said}"
    assert 64 * (1 << 26) == 1024 * (1 << 22) == 4294967296 and (out == 0xABABABAB).all()


# ------------------------------------------------------------------ 4. refusals
def good():
    return ExpandSpec(3, 2, count=col(1), when=col(2), max_count=8, pad=[1, 2], terms=[col(0), stepped(0, 5)])


def words(**changes):
    """The good tape with single words replaced: index -> word."""
    t = good().words().copy()
    for at, word in changes.items():
        t[int(at[1:])] = word
    return t


# the good tape: [0..8] header, [9..10] pad, term 0 at 11 (kind, value, step), term 1 at 14
REFUSALS = [
    ("bad magic", words(w0=MAGIC + 1)),
    ("unknown spec version 2", words(w1=2)),
    ("src_width 0 outside [1, 2^16]", words(w2=0)),
    ("src_width 65537 outside [1, 2^16]", words(w2=(1 << 16) + 1)),
    ("out_width 0 outside [1, 64]", words(w3=0)),
    ("out_width 65 outside [1, 64]", words(w3=65)),
    ("17 words, the header asks for 21", words(w3=3)),
    ("16 words, the header asks for 17", good().words()[:-1]),
    ("shorter than its header", good().words()[:8]),
    ("selector kind must be 0 (always) or 1 (column)", words(w4=2)),
    ("a constant selector must be 1", words(w4=0, w5=0)),
    ("a constant selector must be 1", words(w4=0, w5=2)),
    ("the selector column is outside the source", words(w5=3)),
    ("count kind must be 0 (constant) or 1 (column)", words(w6=2)),
    ("a constant count must be in [1, max_count]", words(w6=0, w7=0)),
    ("a constant count must be in [1, max_count]", words(w6=0, w7=9)),
    ("the count column is outside the source", words(w7=3)),
    ("max_count 0 outside [1, 2^27]", words(w8=0)),
    ("max_count 134217729 outside [1, 2^27]", words(w8=(1 << 27) + 1)),
    ("pad word 1 is not below p", words(w10=P)),
    ("term 0: kind must be in [0, 7]", words(w11=8)),
    ("term 0: the constant is not below p", words(w11=0, w12=P)),
    ("term 0: the column is outside the source", words(w12=3)),
    ("term 1: the column is outside the source", words(w15=3)),
    ("term 0: the value word of kinds 2 to 6 must be 0", words(w11=2, w12=1)),
    ("term 0: the value word of kinds 2 to 6 must be 0", words(w11=6, w12=1)),
    ("term 0: the step word must be 0 for every kind but 7", words(w13=1)),
    ("term 0: the step word must be 0 for every kind but 7", words(w11=3, w12=0, w13=1)),
    ("term 1: the step is not below p", words(w16=P)),
]


@pytest.mark.parametrize("text,tape", REFUSALS, ids=[f"{k}-{t[:40]}" for k, (t, _) in enumerate(REFUSALS)])
def test_every_matrix_free_refusal(lib, text, tape):
    assert expand_check(good()) == (3, 2)
    with pytest.raises(TsError) as e:
        expand_check(tape)
    assert e.value.code == TS_ERR_INVALID and text in str(e.value), str(e.value)
    # the host loop makes the same checks first and writes nothing
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    used, live = C.c_uint64(), C.c_uint64()
    src = np.ones((2, 3), dtype=np.uint32)  # (never read: the tape is refused first)
    assert _host_call(lib, tape, src, 0, out, 64, used, live) == TS_ERR_INVALID
    assert text in lib.ts_last_error(None).decode() and (out == 0xABABABAB).all()


def test_host_call_refusals(lib):
    t = good().words()
    src = np.ones((2, 3), dtype=np.uint32)
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    used, live = C.c_uint64(), C.c_uint64()
    p = lambda m: m.ctypes.data_as(_lib.u32p)  # noqa: E731

    def refused(text, spec_p=p(t), src_p=p(src), height=2, out_height=0, out_p=p(out), used_p=C.byref(used),
                live_p=C.byref(live)):
        st = lib.ts_expand_rows_host(spec_p, len(t), src_p, height, out_height, out_p, 64, used_p, live_p)
        assert st == TS_ERR_INVALID and text in lib.ts_last_error(None).decode(), lib.ts_last_error(None)
        assert (out == 0xABABABAB).all(), "a refused call wrote into the buffer"

    refused("null", spec_p=None)
    refused("null argument", src_p=None)
    refused("null argument", out_p=None)
    refused("null argument", used_p=None)
    refused("null argument", live_p=None)
    refused("the height of the source must be in [1, 2^27]", height=0)
    refused("the height of the source must be in [1, 2^27]", height=(1 << 27) + 1)
    for bad in (3, 6, (1 << 27) + 1, 1 << 28, 1 << 63):
        refused(f"out_height {bad} is neither 0 nor a power of two in [1, 2^27]", out_height=bad)
    assert lib.ts_expand_check(None, 9, None, None) == TS_ERR_INVALID
    assert lib.ts_expand_check(p(t), len(t), None, None) == 0, "both outputs may be null"


def test_null_context_refused(lib):
    t = good().words()
    fake = C.create_string_buffer(64)  # never dereferenced: the null context is refused first
    out, live = C.c_void_p(12345), C.c_uint64(77)
    assert lib.ts_matrix_expand_rows(None, t.ctypes.data_as(_lib.u32p), len(t), C.addressof(fake), 0, C.byref(out),
                                     C.byref(live)) == TS_ERR_INVALID
    assert out.value is None and live.value == 0, "a refused call left a handle"
    assert lib.ts_matrix_expand_rows(None, None, 0, None, 0, None, None) == TS_ERR_INVALID


# ------------------------------------------------------------------ 5. the ABI and the builders
def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "tapstark-gpu", "src", "ffi.rs")).read()
    for name in ("ts_matrix_expand_rows", "ts_expand_check", "ts_expand_rows_host"):
        assert hasattr(lib, name) and name in _lib.ABI_SYMBOLS
        assert f"ts_status {name}(" in header and f"pub fn {name}(" in ffi
    assert lib.ts_abi_version() == 5 and len(_lib.ABI_SYMBOLS) == 161
    assert header.index("---- joined rows") < header.index("---- expanded rows") < header.index("ts_abi_version")


CPP_EXPAND = r"""
#include <stdio.h>
#include "tapstark_air.hpp"
int main() {
    using ts::air::Expand;
    Expand a(10, 9, 24, {7});
    a.count(Expand::col(2)).when(Expand::col(3));
    a.terms({Expand::constant(0x78000001ull + 3), Expand::col(9), Expand::row(), Expand::inner(), Expand::remaining(),
             Expand::first(), Expand::last(), Expand::stepped(1), Expand::stepped(4, 0x78000001ull + 5)});
    for (uint32_t w : a.tape()) printf("%u\n", w);
    Expand b(2, 1, 24);
    b.count(Expand::times(24)).terms({Expand::inner()});
    for (uint32_t w : b.tape()) printf("%u\n", w);
    return 0;
}
"""


def test_cpp_builder_writes_the_python_words(lib, tmp_path):
    src = tmp_path / "expand.cpp"
    src.write_text(CPP_EXPAND)
    exe = str(tmp_path / "expand")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    a = ExpandSpec(10, 9, count=col(2), when=col(3), max_count=24, pad=[7] + [0] * 8,
                   terms=[const(P + 3), col(9), ROW, J, REMAINING, FIRST, LAST, stepped(1, 1), stepped(4, P + 5)])
    b = ExpandSpec(2, 1, count=24, max_count=24, terms=[J])
    assert got == a.words().tolist() + b.words().tolist()
    assert expand_check(a) == (10, 9) and expand_check(b) == (2, 1)


# ------------------------------------------------------------------ 6. the span AIRs
def violations(air, trace):
    nb = NumericBuilder(np.asarray(trace).astype(np.uint64), [], define=False)
    air.eval_main(nb)
    return nb.first_violation()


@pytest.mark.parametrize("n,max_len,table", [(256, 7, 64), (32, 24, 24), (16, 1, 4)])
def test_span_airs_hold_on_the_generated_traces(lib, n, max_len, table):
    A, T = SpanCallAir, SpanChipAir
    calls = generate_span_call_trace(n, max_len, table, 5)
    assert violations(SpanCallAir(), calls) == -1
    picked = calls[calls[:, A.SEL] == 1]
    assert 0 < len(picked) < n and picked[:, A.LEN].min() >= 1 and picked[:, A.LEN].max() <= max_len
    assert (picked[:, A.BASE].astype(np.int64) + picked[:, A.LEN] <= table).all()
    chip = generate_span_chip_trace(calls)
    assert violations(SpanChipAir(), chip) == -1
    n_live = int(picked[:, A.LEN].sum())
    assert chip[:n_live, T.LIVE].all() and not chip[n_live:].any() and chip[:, T.ADDR].max() < table
    # the host loop and one appended column make the same table
    rows, live = expand_rows_host(span_expand_spec(max_len), calls)
    assert live == n_live
    same(np.concatenate([rows, ((P - rows[:, T.FIRST].astype(np.int64)) % P).astype(np.uint32)[:, None]], axis=1), chip)
    # the chip receives what the machine sends: one tuple per selected call
    sent = sorted(map(tuple, picked[:, :3].tolist()))
    assert sorted(map(tuple, chip[chip[:, T.FIRST] == 1][:, :3].tolist())) == sent
    full = generate_span_chip_trace(calls, out_height=1 << 12)
    assert violations(SpanChipAir(), full) == -1 and full.shape == (1 << 12, 9)


def test_span_chip_constraints_catch_what_they_are_for(lib):
    T, air = SpanChipAir, SpanChipAir()
    chip = generate_span_chip_trace(generate_span_call_trace(64, 7, 64, 5))
    inside = int(np.flatnonzero((chip[:, T.FIRST] == 0) & (chip[:, T.LIVE] == 1))[0])
    for column, row in ((T.J, inside), (T.ADDR, inside), (T.LEN, inside), (T.BASE, inside), (T.ID, inside)):
        bad = chip.copy()
        bad[row, column] += 1
        assert violations(air, bad) != -1, column
    cut = chip.copy()  # a span that stops short of its length
    last = int(np.flatnonzero((chip[:, T.LAST] == 1) & (chip[:, T.FIRST] == 0))[0])
    cut[last, T.LAST] = 0
    assert violations(air, cut) != -1


def test_span_airs_have_constraint_degree_three():
    for air in (SpanCallAir(), SpanChipAir(), BusRangeAir()):
        aw, nc, ne = aux_dims(air)
        assert get_symbolic_constraints(air, 0, 0, aw, nc, ne).max_constraint_degree() == 3, type(air).__name__
    assert len({SPAN_TAG, BUS_TAG, 11, 13}) == 4


# ------------------------------------------------------------------ 7. under the sanitizers
def _case_words(tape, src, height, out_height):
    return [len(tape), *[int(w) for w in tape], out_height, height, src.size, *src.reshape(-1).tolist()]


def test_checks_and_host_loop_are_clean_under_the_sanitizers(lib, tmp_path):
    """csrc/expand.cpp and tap-stark_amd/probe/expand_probe.cpp built together with AddressSanitizer and UBSan into a
    stand-alone program and run over the seeded grid, the height cases, the late refusals and every refused tape, each in
    buffers of exactly its size: every line is what the reference gives and no sanitizer report ends the run."""
    from tapstark_amd import build as b

    exe = str(tmp_path / "expand_probe")
    cmd = [b._clangxx(), "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(b._rocm(), "include"), "-I", b.CSRC,
           "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(b.PKG, "probe", "expand_probe.cpp"),
           os.path.join(b.CSRC, "expand.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def fnv(a):
        h = 0xcbf29ce484222325
        for byte in np.ascontiguousarray(a, dtype="<u4").tobytes():
            h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return h

    cases, want = [], []
    for seed in range(4):
        for src_width, out_width, height in ((1, 1, 1), (3, 5, 1000), (17, 64, 37), (2, 9, 3)):
            src = xc.random_rows(seed + 10 * src_width, height, src_width, density=0.3 * seed)
            spec = xc.random_spec(seed, src_width, out_width)
            for out_height in (0, 1 << 13, 4):
                cases.append(_case_words(spec.words(), src, height, out_height))
                try:
                    m, live = xc.reference(spec, src, out_height)
                    want.append(f"{m.shape[0]} {live} {fnv(m):016x}")
                except ValueError as e:
                    want.append(f"refused: {e}")
    big = ExpandSpec(1, 1, count=col(0), max_count=1 << 27, terms=[J])
    cases.append(_case_words(big.words(), np.full((64, 1), 1 << 26, dtype=np.uint32), 64, 0))
    want.append("refused: expand: 4294967296 rows asked for, out_height 134217728")
    over = ExpandSpec(1, 1, count=col(0), max_count=2, terms=[J])
    cases.append(_case_words(over.words(), np.array([[1], [3], [0xFFFFFFFF]], dtype=np.uint32), 3, 2))
    want.append("refused: expand: row 1 asks for 3 rows, max_count 2")
    src = np.ones((2, 3), dtype=np.uint32)
    for text, tape in REFUSALS:
        cases.append(_case_words(tape, src, 2, 0))
        want.append(text)
    path = tmp_path / "cases.bin"
    np.array([len(cases)] + [w for c in cases for w in c], dtype="<u4").tofile(str(path))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(want)
    for k, (got, w) in enumerate(zip(lines, want)):
        assert (w in got and got.startswith("refused: ")) if k >= len(want) - len(REFUSALS) else got == w, (k, got, w)
    assert any("rows asked for, out_height 4" in l for l in lines)
