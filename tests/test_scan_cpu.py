"""CPU-side checks of the scans of ts_matrix_scan (include/tapstark.h "scanned columns"): the reference of
tests/_scan_cases.py against hand-written values, ts_scan_rows_host -- the library's sequential loop over host rows --
against that reference at every height, flag, term kind and edge word, every refusal that needs no matrix, the symbols,
the struct layout, the Python helpers and the C++ builder."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from tapstark_amd import _lib
from tapstark_amd.airs import (MemoryTableAir, generate_memory_accesses, generate_memory_table,
                               memory_fill_helper_program, memory_fill_scan)
from tapstark_amd.derive import derive_rows_host
from tapstark_amd.scan import NO_RESET, ScanSpec, carry_last, col, running_product, running_sum, scan_rows_host

import _scan_cases as sc
from _scan_cases import EDGE, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_BUFFER = 1, 6
HEIGHTS = [1, 2, 3, 63, 64, 65, 1000, 4097]


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


def check(spec, rows, what=""):
    got, last = scan_rows_host(spec, rows, finals=True)
    want, want_last = sc.reference(spec, rows, finals=True)
    same(got, want, what)
    assert last.tolist() == want_last.tolist(), what
    same(scan_rows_host(spec, rows), want, what + " (no finals)")
    return got


# ------------------------------------------------------------------ 1. the reference, by hand
def test_reference_by_hand():
    rows = np.array([[2, 5, 0], [3, 7, 0], [0, 1, 1], [4, P + 2, 0]], dtype=np.uint32)
    spec = ScanSpec().add(3, a=col(0), b=col(1), init=1).add(4, a=col(0), b=col(1), init=1, exclusive=True)
    spec.add(5, a=1, b=col(1), reset=2).add(6, a=col(0), b=0, init=1)
    out, last = sc.reference(spec, rows, finals=True)
    assert out[:, 3].tolist() == [7, 28, 1, 6]           # 2*1+5, 3*7+7, 0*28+1, 4*1+2
    assert out[:, 4].tolist() == [1, 7, 28, 1]           # the state before each row
    assert out[:, 5].tolist() == [5, 12, 1, 3]           # a sum that starts over on row 2; p + 2 reads as 2
    assert out[:, 6].tolist() == [2, 6, 0, 0]            # a product stays 0 after a zero
    assert last.tolist() == [6, 6, 3, 0], "finals are y[h-1], for an exclusive scan too"
    assert (out[:, :3] == rows).all(), "untouched columns are copied as stored"


def test_reference_reset_on_an_exclusive_scan_gives_init():
    rows = np.array([[1, 0], [1, 1], [1, 0]], dtype=np.uint32)
    spec = ScanSpec().add(2, a=1, b=col(0), init=9, reset=1, exclusive=True)
    assert sc.reference(spec, rows)[:, 2].tolist() == [9, 9, 10]


# ------------------------------------------------------------------ 2. ts_scan_rows_host against the reference
@pytest.mark.parametrize("height", HEIGHTS)
def test_host_rows_heights(lib, height):
    for seed in range(6):
        width = (1, 3, 17)[seed % 3]
        check(sc.random_spec(seed + height, width), sc.random_rows(seed + height, height, width), f"seed {seed}")


@pytest.mark.parametrize("a_kind,b_kind,exclusive,reset", list(itertools.product((0, 1), (0, 1), (False, True), (False, True))))
def test_host_rows_every_kind_and_flag(lib, a_kind, b_kind, exclusive, reset):
    rows = sc.random_rows(7, 257, 4)
    for init in (0, 1, P - 1):
        for const in (0, 1, P - 1, 12345):
            spec = ScanSpec().add(4, a=col(0) if a_kind else const, b=col(1) if b_kind else const, init=init,
                                  reset=2 if reset else None, exclusive=exclusive)
            check(spec, rows, f"init {init} constant {const}")


def test_host_rows_edge_words_in_a_b_and_reset(lib):
    """Every triple of edge words as (a, b, reset) of one row, each followed by a plain row that shows what state the
    edge row left: p reads as 0 (no reset, a zero factor), p + 1 as 1, 0xFFFFFFFF as 268435453."""
    triples = list(itertools.product(EDGE, repeat=3))
    rows = np.zeros((2 * len(triples), 4), dtype=np.uint32)
    rows[0::2, :3] = triples
    rows[1::2, :3] = [3, 5, 0]
    rows[:, 3] = 0xFFFFFFFF
    for init in (0, 1, P - 1):
        spec = ScanSpec().add(4, a=col(0), b=col(1), init=init, reset=2).add(5, a=col(0), b=col(1), init=init, reset=2,
                                                                             exclusive=True)
        got = check(spec, rows, f"init {init}")
        assert got[:, 4:].max() < P and (got[:, 3] == 0xFFFFFFFF).all()
    assert 0xFFFFFFFF % P == 268435453


def test_host_rows_zero_factors_mid_run(lib):
    rows = sc.random_rows(11, 1000, 2)
    rows[:, 0] = np.where(np.arange(1000) % 97 == 13, 0, rows[:, 0] | 1)
    rows[500, 0] = P  # a zero factor that is not stored as 0
    got = check(ScanSpec().add(2, a=col(0), b=col(1), init=5), rows)
    assert got[500, 2] == rows[500, 1] % P

    ones = np.ones((300, 1), dtype=np.uint32) * 2
    ones[150, 0] = 0
    got = check(running_product(0, dst=1), ones)
    assert got[149, 1] == pow(2, 150, P) and not got[150:, 1].any(), "a running product stays 0 after a zero"


@pytest.mark.parametrize("where", ["every row", "no row", "row 0 only"])
def test_host_rows_reset_placements(lib, where):
    rows = sc.random_rows(5, 200, 3)
    rows[:, 2] = {"every row": 1, "no row": 0, "row 0 only": (np.arange(200) == 0)}[where]
    spec = running_sum(0, reset=2, dst=3, init=7).extend(running_sum(0, reset=2, dst=4, init=7, exclusive=True))
    got = check(spec, rows, where)
    c0 = rows[:, 0].astype(object) % P
    if where == "every row":
        assert got[:, 3].tolist() == [int((7 + v) % P) for v in c0] and (got[:, 4] == 7).all()
    else:
        assert got[:, 3].tolist() == [int(v % P) for v in 7 + np.cumsum(c0)]


def test_host_rows_reads_see_the_source(lib):
    """Two scans read column 1, a third overwrites it: all three see the source's words."""
    rows = sc.random_rows(6, 130, 3)
    spec = running_sum(1, dst=3).extend(running_product(1, dst=0)).extend(running_sum(2, dst=1))
    got = check(spec, rows)
    assert got[:, 3].tolist() == [int(v % P) for v in np.cumsum(rows[:, 1].astype(object) % P)]
    assert got[:, 1].tolist() == [int(v % P) for v in np.cumsum(rows[:, 2].astype(object) % P)]


@pytest.mark.parametrize("kind", ["appended", "overwriting", "truncated", "truncated to the dst"])
def test_host_rows_appended_overwritten_and_truncated(lib, kind):
    rows = sc.random_rows(8, 65, 6)
    spec = {"appended": ScanSpec().add(6, a=col(4), b=col(5)).add(7, a=1, b=1),
            "overwriting": ScanSpec().add(2, a=col(4), b=col(5)).add(0, a=1, b=1),
            "truncated": ScanSpec(out_width=4).add(2, a=col(4), b=col(5)),
            "truncated to the dst": ScanSpec(out_width=3).add(2, a=col(4), b=col(5))}[kind]
    got = check(spec, rows, kind)
    assert got.shape[1] == {"appended": 8, "overwriting": 6, "truncated": 4, "truncated to the dst": 3}[kind]


def test_host_rows_untouched_columns_keep_non_canonical_words(lib):
    edge = np.array(EDGE, dtype=np.uint32)
    rows = edge[(np.arange(5 * 300) * 3 % len(edge))].reshape(300, 5)
    got = check(running_sum(0, dst=2).extend(running_sum(3, dst=5)), rows)
    assert (got[:, [0, 1, 3, 4]] == rows[:, [0, 1, 3, 4]]).all(), "copied as stored, not reduced"
    assert got[:, [2, 5]].max() < P


def test_eight_scans_and_the_all_ones_sum(lib):
    rows = np.ones((4097, 2), dtype=np.uint32)
    spec = ScanSpec()
    for k in range(8):
        spec.add(2 + k, a=1, b=col(k % 2), init=k)
    got, last = scan_rows_host(spec, rows, finals=True)
    assert last.tolist() == [4097 + k for k in range(8)] and got[-1, 2:].tolist() == last.tolist()


# ------------------------------------------------------------------ 3. refusals
def good():
    return ScanSpec().add(2, a=col(0), b=col(1), init=1, reset=0)


def broken(**kw):
    s = good()
    s.columns[0].update(kw)
    return s


def nine():
    s = ScanSpec()
    for k in range(9):
        s.add(2 + k)
    return s


REFUSALS = {
    "no scans": (lambda: ScanSpec(), "n_columns 0"),
    "nine scans": (lambda: nine(), "n_columns 9"),
    "kind of a": (lambda: broken(a=(2, 0)), "term kind"),
    "kind of b": (lambda: broken(b=(2, 0)), "term kind"),
    "constant a": (lambda: broken(a=(0, P)), "constant a is not below p"),
    "constant b": (lambda: broken(b=(0, 0xFFFFFFFF)), "constant b is not below p"),
    "init": (lambda: broken(init=P), "init is not below p"),
    "column of a": (lambda: broken(a=(1, 2)), "column of a is outside the source"),
    "column of b": (lambda: broken(b=(1, 7)), "column of b is outside the source"),
    "reset column": (lambda: broken(reset=2), "reset column is outside the source"),
    "flag bit 1": (lambda: broken(flags=2), "unknown flag bits"),
    "a gap beyond the source": (lambda: broken(dst=3), "column 2 is beyond the source"),
    "a column written twice": (lambda: good().add(2), "dst of two scans"),
    "out_width below the dst": (lambda: ScanSpec(out_width=1).add(1), "out_width 1 outside [2, 2]"),
    "out_width above the width": (lambda: ScanSpec(out_width=4).add(2), "out_width 4 outside [3, 3]"),
    "wider than 2^16": (lambda: broken(dst=1 << 16), "2^16"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_rows_host_refuses(lib, name):
    make, text = REFUSALS[name]
    spec = make()
    rows = sc.random_rows(1, 4, 2)
    out = np.full(4 * 70000, 0xABABABAB, dtype=np.uint32)
    last = np.full(8, 0xABABABAB, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(_lib.u32p)
    assert lib.ts_scan_rows_host(C.byref(spec.c_spec()), p(rows), 4, 2, p(out), out.size, p(last)) == TS_ERR_INVALID
    assert text in lib.ts_last_error(None).decode(), lib.ts_last_error(None)
    assert (out == 0xABABABAB).all() and (last == 0xABABABAB).all(), "a refused call wrote into the buffer"
    with pytest.raises(_lib.TsError, match="TS_ERR_INVALID"):
        scan_rows_host(spec, rows)


def test_rows_host_refuses_arguments(lib):
    spec, rows = good().c_spec(), sc.random_rows(1, 4, 2)
    out = np.full(12, 0xABABABAB, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(_lib.u32p)

    def refused(text, code=TS_ERR_INVALID, spec_p=C.byref(spec), rows_p=p(rows), height=4, width=2, out_p=p(out), cap=12):
        assert lib.ts_scan_rows_host(spec_p, rows_p, height, width, out_p, cap, None) == code
        assert text in lib.ts_last_error(None).decode(), lib.ts_last_error(None)
        assert (out == 0xABABABAB).all(), "a refused call wrote into the buffer"

    refused("null argument", spec_p=None)
    refused("null argument", rows_p=None)
    refused("null argument", out_p=None)
    refused("height", height=0)
    refused("height", height=(1 << 27) + 1)
    refused("src_width", width=0)
    refused("src_width", width=(1 << 16) + 1)
    refused("fewer than height * out_width words", code=TS_ERR_BUFFER, cap=11)
    bad = good().c_spec()
    bad.struct_size -= 4
    refused("struct_size", spec_p=C.byref(bad))
    assert lib.ts_scan_rows_host(C.byref(spec), p(rows), 4, 2, p(out), 12, None) == 0
    assert (out.reshape(4, 3) == sc.reference(good(), rows)).all()


def test_null_context_refused(lib):
    fake = C.create_string_buffer(64)  # never dereferenced: the null context is refused first
    out = C.c_void_p(12345)
    assert lib.ts_matrix_scan(None, C.byref(good().c_spec()), C.addressof(fake), C.byref(out), None) == TS_ERR_INVALID
    assert out.value is None, "a refused call left a handle"
    assert lib.ts_matrix_scan(None, None, None, None, None) == TS_ERR_INVALID


# ------------------------------------------------------------------ 4. the ABI, the helpers and the builders
def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "tapstark-gpu", "src", "ffi.rs")).read()
    for name in ("ts_matrix_scan", "ts_scan_rows_host"):
        assert hasattr(lib, name) and name in _lib.ABI_SYMBOLS
        assert f"ts_status {name}(" in header and f"pub fn {name}(" in ffi
    assert lib.ts_abi_version() == 5
    assert "enum { TS_SCAN_MAX_COLUMNS = 8, TS_SCAN_EXCLUSIVE = 1 };" in header
    assert C.sizeof(_lib.ScanColumnC) == 32 and C.sizeof(_lib.ScanSpecC) == 272
    assert "prefix sums" not in header[header.index("ts_status ts_matrix_derive(") - 1500:header.index("ts_status ts_matrix_derive(")]


def test_carry_last_fills_the_memory_table(lib):
    """The sorted table with 0 in `value` on every read, the helper columns from the row program, the scan: the table of
    the host generator again.  All on the host: the lowered program and the sequential loop."""
    A = MemoryTableAir
    want = generate_memory_table(generate_memory_accesses(300, 9, 5))
    unfilled = want.copy()
    unfilled[unfilled[:, A.IS_WRITE] == 0, A.VALUE] = 0
    assert (unfilled != want).any()
    same(scan_rows_host(memory_fill_scan(), derive_rows_host(memory_fill_helper_program(), unfilled)), want)
    program, spec = carry_last(A.IS_WRITE, A.VALUE, src_width=8, reset=A.START)
    same(scan_rows_host(spec, derive_rows_host(program, unfilled)), want, "carry_last")


CPP_SCAN = r"""
#include <stdio.h>
#include <string.h>
#include "tapstark_air.hpp"
int main() {
    using ts::air::Scan;
    Scan s(8);
    s.add(2, Scan::col(8), Scan::col(9), 0, 7);
    s.running_sum(0, 4, 7).running_product(1, 5);
    s.add(6, Scan::constant(0x78000001ull + 3), Scan::col(1), 5, TS_SCAN_NO_RESET, true);
    const ts_scan_spec& spec = s.spec();
    uint32_t words[sizeof(ts_scan_spec) / 4];
    memcpy(words, &spec, sizeof spec);
    for (uint32_t w : words) printf("%u\n", w);
    return 0;
}
"""


def test_cpp_builder_fills_the_python_spec(tmp_path):
    src = tmp_path / "scan.cpp"
    src.write_text(CPP_SCAN)
    exe = str(tmp_path / "scan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    spec = ScanSpec(out_width=8).add(2, a=col(8), b=col(9), init=0, reset=7)
    spec.extend(running_sum(0, dst=4, reset=7)).extend(running_product(1, dst=5))
    spec.add(6, a=3, b=col(1), init=5, exclusive=True)
    want = np.frombuffer(bytes(spec.c_spec()), dtype=np.uint32).tolist()
    assert got == want
    assert spec.columns[0]["reset"] == 7 and spec.columns[2]["reset"] == NO_RESET
