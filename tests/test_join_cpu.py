"""CPU-side checks of ts_matrix_join_rows (include/tapstark.h "joined rows"): the reference of tests/_join_cases.py
against hand-written values, ts_join_rows_host -- the library's sequential loop over host rows -- against that
reference over the case grid, every refusal that needs no device, the symbols, the builders, the ROM statement, and the
same loop in a stand-alone program under the sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tapstark_amd import _lib
from tapstark_amd._lib import TsError
from tapstark_amd.airs import (ROM_TAG, BusTupleSendAir, generate_key_table_trace, generate_rom_fetch_trace,
                               generate_rom_key, rom_join_spec, selected_tuples)
from tapstark_amd.join import ALWAYS, HIT, KEEP, TABLE_ROW, JoinSpec, col, const, join_check, join_rows_host

import _join_cases as jc
from _join_cases import P

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


def check(spec, src, table, what=""):
    got = join_rows_host(spec, src, table)
    want = jc.reference(spec, src, table)
    assert got[1:] == want[1:], (what, got[1:], want[1:])
    same(got[0], want[0], what)
    return got


# ------------------------------------------------------------------ 1. the reference, by hand
TABLE = np.array([[1, 10, 20], [P + 1, 11, 21], [0xFFFFFFFF, 12, 22], [1, 13, 23], [2 * P, 14, P + 7], [P, 15, 25]],
                 dtype=np.uint32)
#                 key          when  a   b
SRC = np.array([[1,            1,    90, 91],    # the class {0, 3}: row 0
                [P + 1,        P + 1, 90, 91],   # matched as stored: row 1, not the rows that hold 1
                [0xFFFFFFFF,   0xFFFFFFFF, 90, 91],
                [2 * P,        5,    90, 91],    # row 4; the fetched word p + 7 arrives as stored
                [0,            1,    90, 91],    # 0 is not p nor 2p: a miss
                [P,            0,    90, 91],    # takes no part: `when` is 0
                [P,            P,    90, 91],    # takes no part: p is a zero
                [7,            2 * P, 90, 91],   # takes no part (and would miss): not counted
                [P,            P - 1, 90, 91]],  # row 5
               dtype=np.uint32)


def test_reference_by_hand():
    spec = JoinSpec(keys=[(col(0), col(0))], when=col(1), fetch=[(2, 3, 77), (1, 4, 78)], flags=TABLE_ROW | HIT)
    out, n_missing, first = jc.reference(spec, SRC, TABLE)
    assert (n_missing, first) == (1, 4)
    assert out.tolist() == [
        [1, 1, 90, 20, 10, 0, 1],
        [P + 1, P + 1, 90, 21, 11, 1, 1],
        [0xFFFFFFFF, 0xFFFFFFFF, 90, 22, 12, 2, 1],
        [2 * P, 5, 90, P + 7, 14, 4, 1],
        [0, 1, 90, 77, 78, 0, 0],
        [P, 0, 90, 77, 78, 0, 0],
        [P, P, 90, 77, 78, 0, 0],
        [7, 2 * P, 90, 77, 78, 0, 0],
        [P, P - 1, 90, 25, 15, 5, 1]]
    keep, _, _ = jc.reference(JoinSpec(keys=[(col(0), col(0))], when=col(1), fetch=[(2, 3, 77), (1, 4, 78)], flags=KEEP),
                              SRC, TABLE)
    assert keep[4:8].tolist() == [[0, 1, 90, 91, 78], [P, 0, 90, 91, 78], [P, P, 90, 91, 78], [7, 2 * P, 90, 91, 78]]
    # only rows [0, 3) are entered: the class of 1 is {0}, and 2p and p are in no entered row
    short = JoinSpec(keys=[(col(0), col(0))], when=col(1), fetch=[(1, 2, 0)], table_rows=3)
    out, n_missing, first = jc.reference(short, SRC, TABLE)
    assert (n_missing, first) == (3, 3) and out[:, 2].tolist() == [10, 11, 12, 0, 0, 0, 0, 0, 0]
    # constants on either side, and a constant `when`
    two = JoinSpec(keys=[(col(0), col(0)), (const(P + 13), col(1))], when=ALWAYS, fetch=[(2, 0, 5)])
    out, n_missing, first = jc.reference(two, SRC, TABLE)
    assert (n_missing, first) == (8, 1) and out[:, 0].tolist() == [23, 5, 5, 5, 5, 5, 5, 5, 5]
    never = JoinSpec(keys=[(col(0), col(0))], when=0, fetch=[(2, 0, 5)])
    assert jc.reference(never, SRC, TABLE)[1:] == (0, None)


def test_host_loop_by_hand(lib):
    for flags in range(8):
        check(JoinSpec(keys=[(col(0), col(0))], when=col(1), fetch=[(2, 3, 77), (1, 4, 78)], flags=flags), SRC, TABLE,
              f"flags {flags}")
    check(JoinSpec(keys=[(col(0), col(0))], when=col(1), fetch=[(1, 2, 0)], table_rows=3), SRC, TABLE, "short")
    check(JoinSpec(keys=[(col(0), col(0)), (const(P + 13), col(1))], fetch=[(2, 0, 5)]), SRC, TABLE, "constants")
    got = check(JoinSpec(keys=[(col(0), col(0))], when=0, fetch=[(2, 0, 5)]), SRC, TABLE, "never")
    assert (got[0][:, 0] == 5).all()


# ------------------------------------------------------------------ 2. the host loop against the reference
GRID = list(jc.grid())


@pytest.mark.parametrize("name,case", GRID, ids=[name for name, _ in GRID])
def test_host_loop_against_the_reference(lib, name, case):
    check(*case, what=name)


def test_the_grid_covers_what_it_should():
    flags = {c[0].flags for _, c in GRID}
    assert flags == set(range(8))
    assert any(c[0].table_rows for _, c in GRID) and any(not c[0].table_rows for _, c in GRID)
    assert any(s[0] == 0 for _, c in GRID for s, _ in c[0].keys) and any(t[0] == 0 for _, c in GRID for _, t in c[0].keys)
    assert {len(c[0].fetch) for _, c in GRID} == {0, 1, 32} and {len(c[0].keys) for _, c in GRID} == {1, 3, 8}
    small = [jc.reference(*c) for _, c in GRID[:54]]  # the source heights 1 and 3
    assert any(n for _, n, _ in small) and any(n == 0 for _, n, _ in small)


def test_duplicate_tuples_lowest_row_wins(lib):
    rng = np.random.default_rng(5)
    tuples = rng.integers(0, 1 << 32, size=(8, 2), dtype=np.uint32)
    table = np.concatenate([np.repeat(tuples, 16, axis=0), np.arange(128, dtype=np.uint32).reshape(128, 1)], axis=1)
    table = table[rng.permutation(128)]
    src = tuples[rng.integers(0, 8, size=50)]
    out, n_missing, _ = check(JoinSpec(keys=[(col(0), col(0)), (col(1), col(1))], fetch=[(2, 2, 0)], flags=TABLE_ROW),
                              src, table)
    assert n_missing == 0
    for r in range(50):
        rows = np.flatnonzero((table[:, :2] == src[r]).all(axis=1))
        assert out[r, 3] == rows.min() and out[r, 2] == table[rows.min(), 2]


def test_src_is_table(lib):
    spec, m = jc.chase(3, 200)
    out, n_missing, first = check(spec, m, m, "chase")
    assert 0 < n_missing < 200 and out.shape == (200, 5)
    again = join_rows_host(spec, m, m.copy())
    same(again[0], out)


def test_pad_row_that_would_match_is_not_entered(lib):
    spec, src, table = jc.case(1, 40, 5, 1, 1, flags=HIT, pad_row=True, hit=1.0)
    assert spec.table_rows == 4
    asks = src[:, 0] == table[4, 0]
    assert asks.any() and not asks.all()
    out, n_missing, first = check(spec, src, table)
    fires = src[:, 1] % P != 0
    assert n_missing == int((asks & fires).sum()) > 0 and first == int(np.flatnonzero(asks & fires)[0])
    spec.table_rows = 0
    assert check(spec, src, table)[1] == 0


# ------------------------------------------------------------------ 3. the refusals
def good(**kw):
    args = dict(keys=[(col(0), col(1)), (5, col(0))], when=col(2), fetch=[(2, 3, 0), (0, 4, 9)], flags=0)
    args.update(kw)
    return JoinSpec(**args)


def bad_size():
    s = good()
    s.struct_size -= 8
    return s


SRC_W, TABLE_W = 4, 3
REFUSALS = [
    ("bad struct_size", bad_size),
    ("n_keys 0 outside [1, 8]", lambda: good(keys=[])),
    ("n_keys 9 outside [1, 8]", lambda: good(keys=[(col(0), col(0))] * 9)),
    ("n_fetch 33 outside [0, 32]", lambda: good(fetch=[(0, 4 + f, 0) for f in range(33)])),
    ("nothing to write", lambda: good(fetch=[])),
    ("nothing to write", lambda: good(fetch=[], flags=KEEP)),
    ("unknown flag", lambda: good(flags=8)),
    ("unknown flag", lambda: good(flags=1 << 31)),
    ("source key 0: kind must be 0 (constant) or 1 (column)", lambda: good(keys=[((2, 0), col(0))])),
    ("table key 1: kind must be 0 (constant) or 1 (column)", lambda: good(keys=[(col(0), col(0)), (col(0), (2, 0))])),
    ("when: kind must be 0 (constant) or 1 (column)", lambda: good(when=(2, 0))),
    ("source key 0: the column is outside the source", lambda: good(keys=[(col(4), col(0))])),
    ("table key 0: the column is outside the table", lambda: good(keys=[(col(0), col(3))])),
    ("when: the column is outside the source", lambda: good(when=col(4))),
    ("fetch 1: the column is outside the table", lambda: good(fetch=[(2, 3, 0), (3, 4, 9)])),
    ("source key 0: the constant is not below p", lambda: good(keys=[((0, P), col(0))])),
    ("table key 0: the constant is not below p", lambda: good(keys=[(col(0), (0, 0xFFFFFFFF))])),
    ("when: the constant is not below p", lambda: good(when=(0, P))),
    ("fetch 0: the default is not below p", lambda: good(fetch=[(2, 3, P)])),
    ("dst column 3 appears twice", lambda: good(fetch=[(2, 3, 0), (0, 3, 9)])),
    ("column 4 of the result is neither the source's nor a dst column", lambda: good(fetch=[(2, 5, 0)])),
    ("column 5 of the result is neither the source's nor a dst column", lambda: good(fetch=[(2, 4, 0), (2, 6, 0)])),
    ("wider than 2^16", lambda: good(fetch=[(2, 1 << 16, 0)])),
]


@pytest.mark.parametrize("text,make", REFUSALS, ids=[f"{k}-{t[:40]}" for k, (t, _) in enumerate(REFUSALS)])
def test_every_matrix_free_refusal(lib, text, make):
    with pytest.raises(TsError) as e:
        join_check(make(), SRC_W, TABLE_W)
    assert e.value.code == TS_ERR_INVALID and text in str(e.value), str(e.value)
    src, table = np.ones((2, SRC_W), dtype=np.uint32), np.ones((2, TABLE_W), dtype=np.uint32)
    with pytest.raises(TsError) as e:
        join_rows_host(make(), src, table, capacity_words=64)
    assert e.value.code == TS_ERR_INVALID and text in str(e.value)


def test_widths_and_the_widest_result(lib):
    assert join_check(good(), SRC_W, TABLE_W) == 5
    assert join_check(good(flags=TABLE_ROW | HIT), SRC_W, TABLE_W) == 7
    assert join_check(good(fetch=[(0, 1, 0)]), 1 << 16, TABLE_W) == 1 << 16
    for flags in (TABLE_ROW, HIT, TABLE_ROW | HIT):
        with pytest.raises(TsError, match="wider than 2\\^16"):
            join_check(good(fetch=[(0, 1, 0)], flags=flags), 1 << 16, TABLE_W)
    with pytest.raises(TsError, match="the source's width outside"):
        join_check(good(), (1 << 16) + 1, TABLE_W)
    for sw, tw in ((0, 3), (4, 0)):
        with pytest.raises(TsError, match="width"):
            join_check(good(), sw, tw)


def _host(lib, spec, src, src_h, table, table_h, out, n_missing=True):
    s, _keep = spec.c_spec()
    p = lambda a: a.ctypes.data_as(_lib.u32p)
    n, first = C.c_uint64(7), C.c_uint64(7)
    st = lib.ts_join_rows_host(C.byref(s), p(src), src_h, src.shape[1], p(table), table_h, table.shape[1], p(out),
                               out.size, C.byref(n) if n_missing else None, C.byref(first))
    return st, n.value, first.value, (lib.ts_last_error(None) or b"").decode()


def test_host_call_refusals(lib):
    src, table = np.ones((4, SRC_W), dtype=np.uint32), np.ones((2, TABLE_W), dtype=np.uint32)
    out = np.full(4 * 5, 0xABCD, dtype=np.uint32)
    for src_h, table_h, text in ((0, 2, "the height of the source"), ((1 << 27) + 1, 2, "the height of the source"),
                                 (4, 0, "the height of the table"), (4, (1 << 27) + 1, "the height of the table")):
        st, n, first, err = _host(lib, good(), src, src_h, table, table_h, out)  # (refused before a row is read)
        assert st == TS_ERR_INVALID and text in err and (n, first) == (0, 2 ** 64 - 1)
    st, _, _, err = _host(lib, good(table_rows=3), src, 4, table, 2, out)
    assert st == TS_ERR_INVALID and "table_rows 3 above the table's height 2" in err
    assert _host(lib, good(table_rows=2), src, 4, table, 2, out)[0] == 0
    out[:] = 0xABCD
    st, _, _, err = _host(lib, good(), src, 4, table, 2, out[:19])
    assert st == TS_ERR_BUFFER and "fewer than height * out_width words" in err and (out == 0xABCD).all()
    # a miss without a count is an error that names the row, and writes nothing
    src[:, 2] = (0, 1, 1, 1)
    st, _, first, err = _host(lib, good(), src, 4, table, 2, out, n_missing=False)
    assert st == TS_ERR_INVARIANT and "source row 1 is in no table row (3 such rows)" in err and (out == 0xABCD).all()
    st, n, first, _ = _host(lib, good(), src, 4, table, 2, out)
    assert (st, n, first) == (0, 3, 1)
    assert lib.ts_join_rows_host(None, None, 0, 0, None, 0, 0, None, 0, None, None) == TS_ERR_INVALID
    assert lib.ts_join_check(None, 1, 1, None) == TS_ERR_INVALID


def test_null_context_refused(lib):
    s, _keep = good().c_spec()
    fake = C.create_string_buffer(64)  # never dereferenced: the null context is refused first
    out, n, first = C.c_void_p(12345), C.c_uint64(77), C.c_uint64(77)
    assert lib.ts_matrix_join_rows(None, C.byref(s), C.addressof(fake), C.addressof(fake), C.byref(out), C.byref(n),
                                   C.byref(first)) == TS_ERR_INVALID
    assert out.value is None and n.value == 0 and first.value == 2 ** 64 - 1, "a refused call left a handle"
    assert lib.ts_matrix_join_rows(None, None, None, None, None, None, None) == TS_ERR_INVALID


# ------------------------------------------------------------------ 4. the ABI and the builders
def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "tapstark-gpu", "src", "ffi.rs")).read()
    for name in ("ts_matrix_join_rows", "ts_join_check", "ts_join_rows_host"):
        assert hasattr(lib, name) and name in _lib.ABI_SYMBOLS
        assert f"ts_status {name}(" in header and f"pub fn {name}(" in ffi
    assert lib.ts_abi_version() == 5
    for line in ("#define TS_JOIN_MAX_KEYS   8u", "#define TS_JOIN_MAX_FETCH  32u", "#define TS_JOIN_TABLE_ROW  1u",
                 "#define TS_JOIN_HIT        2u", "#define TS_JOIN_KEEP       4u"):
        assert line in header
    for line in ("TS_JOIN_MAX_KEYS: usize = 8", "TS_JOIN_MAX_FETCH: usize = 32", "TS_JOIN_TABLE_ROW: u32 = 1",
                 "TS_JOIN_HIT: u32 = 2", "TS_JOIN_KEEP: u32 = 4", "pub struct ts_join_spec"):
        assert line in ffi
    assert "has not been compiled" in ffi
    assert header.index("---- collected rows") < header.index("---- joined rows") < header.index("ts_abi_version")
    assert C.sizeof(_lib.JoinSpecC) == 80


CPP_JOIN = r"""
#include <stdio.h>
#include "tapstark_air.hpp"
int main() {
    using ts::air::Join;
    Join j(TS_JOIN_TABLE_ROW | TS_JOIN_KEEP, 300);
    j.key(Join::col(4), Join::col(0)).key(Join::constant(0x78000001ull + 3), Join::col(2)).key(Join::col(1), Join::constant(9));
    j.when(Join::col(7)).fetch(1, 5, 0).fetch(2, 6, 77);
    const ts_join_spec* s = j.spec();
    printf("%u %u\n", s->struct_size, (unsigned)sizeof(ts_join_spec));
    printf("%u\n", s->n_keys);
    for (uint32_t q = 0; q < s->n_keys; q++) printf("%u %u\n", s->src_keys[q].kind, s->src_keys[q].value);
    for (uint32_t q = 0; q < s->n_keys; q++) printf("%u %u\n", s->table_keys[q].kind, s->table_keys[q].value);
    printf("%u %u %u\n", s->when.kind, s->when.value, s->n_fetch);
    for (uint32_t f = 0; f < s->n_fetch; f++) printf("%u %u %u\n", s->table_columns[f], s->dst_columns[f], s->defaults[f]);
    printf("%u %llu\n", s->flags, (unsigned long long)s->table_rows);
    return 0;
}
"""


def test_cpp_builder_writes_the_python_spec(lib, tmp_path):
    src = tmp_path / "join.cpp"
    src.write_text(CPP_JOIN)
    exe = str(tmp_path / "join")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    spec = JoinSpec(keys=[(col(4), col(0)), (const(P + 3), col(2)), (col(1), 9)], when=col(7),
                    fetch=[(1, 5, 0), (2, 6, 77)], flags=TABLE_ROW | KEEP, table_rows=300)
    assert got[:2] == [C.sizeof(_lib.JoinSpecC)] * 2
    s, _keep = spec.c_spec()  # the struct the library is given, field after field
    want = [s.n_keys]
    for terms in (s.src_keys, s.table_keys):
        for q in range(s.n_keys):
            want += [terms[q].kind, terms[q].value]
    want += [s.when.kind, s.when.value, s.n_fetch]
    for f in range(s.n_fetch):
        want += [s.table_columns[f], s.dst_columns[f], s.defaults[f]]
    want += [s.flags, s.table_rows]
    assert got[2:] == want and want[:5] == [3, 1, 4, 0, 3] and want[-2:] == [5, 300]  # (the constant is reduced mod p)
    assert join_check(spec, 8, 3) == 9


# ------------------------------------------------------------------ 5. the ROM statement
def test_rom_trace_is_filled_by_the_join(lib):
    key = generate_rom_key(16, 3)
    assert key.shape == (16, 3) and len(set(key[:, 0].tolist())) == 16
    assert (np.diff(key[:, 0].astype(np.int64)) < 0).any() and (key[:, 0] != np.arange(16)).all(), "sparse, unordered"
    k = 2
    want = generate_rom_fetch_trace(64, k, key, 4)
    unfilled = generate_rom_fetch_trace(64, k, key, 4, unfilled=True)
    assert want.shape == (64, 4 * k) == unfilled.shape and BusTupleSendAir(ROM_TAG, k, 3).width() == 4 * k
    assert not unfilled[:, [1, 2, 5, 6]].any() and (unfilled[:, [0, 3, 4, 7]] == want[:, [0, 3, 4, 7]]).all()
    assert set(want[:, 3].tolist()) == {0, 1} and want[:, [1, 2]][want[:, 3] == 1].any()
    trace = unfilled
    for spec in rom_join_spec(k):
        trace, n_missing, first = join_rows_host(spec, trace, key)
        assert (n_missing, first) == (0, None)
    same(trace, want)
    # every selected tuple is a ROM row: the table's multiplicities count them all
    sent = selected_tuples(want, 3)
    mult = generate_key_table_trace(key, sent)
    assert int(((P - mult.astype(np.int64)) % P).sum()) == len(sent) > 0
    # a pc that is not in the ROM is the miss the join names
    bad = unfilled.copy()
    row = int(np.flatnonzero(bad[:, 3] == 1)[5])
    bad[row, 0] = 7
    _, n_missing, first = join_rows_host(rom_join_spec(k)[0], bad, key)
    assert (n_missing, first) == (1, row)
    assert ROM_TAG == 13


# ------------------------------------------------------------------ 6. under the sanitizers
def _case_words(spec, src, table):
    w = [1 if spec.struct_size == C.sizeof(_lib.JoinSpecC) else 0, len(spec.keys)]
    for s, _ in spec.keys:
        w += list(s)
    for _, t in spec.keys:
        w += list(t)
    w += [*spec.when, len(spec.fetch)]
    for k in range(3):
        w += [f[k] for f in spec.fetch]
    w += [spec.flags, spec.table_rows, src.shape[0], src.shape[1], *src.reshape(-1).tolist()]
    if table is src:
        return w + [1]
    return w + [0, table.shape[0], table.shape[1], *table.reshape(-1).tolist()]


def test_checks_and_host_loop_are_clean_under_the_sanitizers(lib, tmp_path):
    """csrc/join.cpp and tap-stark_amd/probe/join_probe.cpp built together with AddressSanitizer and UBSan into a
    stand-alone program and run over the grid above, the hand-written cases, src-is-table and every refused spec, each
    in buffers of exactly its size: every line is what the reference gives and no sanitizer report ends the run."""
    from tapstark_amd import build as b

    exe = str(tmp_path / "join_probe")
    cmd = [b._clangxx(), "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(b._rocm(), "include"), "-I", b.CSRC,
           "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(b.PKG, "probe", "join_probe.cpp"),
           os.path.join(b.CSRC, "join.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def fnv(a):
        h = 0xcbf29ce484222325
        for byte in np.ascontiguousarray(a, dtype="<u4").tobytes():
            h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return h

    runs = [c for _, c in GRID]
    runs += [(JoinSpec(keys=[(col(0), col(0))], when=col(1), fetch=[(2, 3, 77), (1, 4, 78)], flags=f), SRC, TABLE)
             for f in range(8)]
    chase_spec, m = jc.chase(3, 200)
    runs.append((chase_spec, m, m))
    cases, want = [], []
    for spec, src, table in runs:
        cases.append(_case_words(spec, src, table))
        out, n_missing, first = jc.reference(spec, src, table)
        want.append(f"{out.shape[1]} {n_missing} {-1 if first is None else first} {fnv(out):016x}")
    src, table = np.ones((2, SRC_W), dtype=np.uint32), np.ones((2, TABLE_W), dtype=np.uint32)
    for text, make in REFUSALS:
        cases.append(_case_words(make(), src, table))
        want.append(text)
    cases.append(_case_words(good(table_rows=3), src, table))
    want.append("table_rows 3 above the table's height 2")
    n_refused = len(REFUSALS) + 1
    path = tmp_path / "cases.bin"
    np.array([len(cases)] + [w for c in cases for w in c], dtype="<u4").tofile(str(path))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(want)
    for k, (got, w) in enumerate(zip(lines, want)):
        assert (w in got and got.startswith("refused: join: ")) if k >= len(want) - n_refused else got == w, (k, got, w)
