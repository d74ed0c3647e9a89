"""CPU-side checks of ts_matrix_sort_rows / ts_matrix_gather_rows (include/tapstark.h): the numpy reference of
tests/_sort_cases.py against plain Python ``sorted`` on every case family, the memory-table AIR pair on the generated
tables, the symbols, the ctypes layout of ts_sort_spec and the refusals that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tapstark_amd import _lib
from tapstark_amd.air import aux_dims, get_symbolic_constraints
from tapstark_amd.airs import (BUS_TAG, MEM_TAG, BusRangeAir, MemoryAccessAir, MemoryTableAir, NumericBuilder,
                               fill_memory_gaps, generate_memory_accesses, generate_memory_table, memory_table_source)

import _sort_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID = 1
P = sc.P


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


# ------------------------------------------------------------------ 1. the reference
def check_reference(src, keys, group_keys, n_live):
    got = sc.reference(src, keys, group_keys=group_keys, n_live=n_live, source_row=True, group_start=True)
    order = sc.python_order(src, keys, n_live)
    w = src.shape[1]
    assert got[:, w].tolist() == order
    assert (got[:, :w] == src[order]).all()
    rows = [[int(x) for x in r] for r in src]
    lead = lambda r: tuple(rows[r][k] for k in keys[:group_keys])
    start = [int(i < n_live and (i == 0 or lead(order[i]) != lead(order[i - 1]))) for i in range(len(order))]
    assert got[:, w + 1].tolist() == start
    for flags in ((False, False), (True, False), (False, True)):
        part = sc.reference(src, keys, group_keys=group_keys, n_live=n_live, source_row=flags[0], group_start=flags[1])
        cols = list(range(w)) + ([w] if flags[0] else []) + ([w + 1] if flags[1] else [])
        assert (part == got[:, cols]).all()


@pytest.mark.parametrize("family", sc.KEY_FAMILIES)
def test_reference_against_python_sorted_key_families(family):
    for length in (1, 2, 65, 300):
        src, n_live = sc.tail_case(sc.key_family(family, length), sc.pow2_at_least(length))
        check_reference(src, [2], 1, n_live)


def test_reference_against_python_sorted_multi_key_and_n_live():
    for n_keys in (2, 4):
        src, columns = sc.multi_key_case(256, n_keys)
        for group_keys in (0, 1, n_keys):
            for n_live in (0, 1, 255, 256):
                check_reference(src, columns, group_keys, n_live)
    for width in (1, 3, 17):
        check_reference(sc.matrix(sc.key_family("uniform", 64), width), [width - 1], 1, 64)


def test_families_are_what_their_names_say():
    n = 1024
    byte = lambda w, b: (w >> np.uint32(8 * b)) & np.uint32(255)
    for name, moving in (("top_byte", 3), ("byte1", 1), ("byte0", 0)):
        w = sc.key_family(name, n)
        for b in range(4):
            assert (len(np.unique(byte(w, b))) > 1) == (b == moving), (name, b)
    assert set(sc.key_family("edge_words", n).tolist()) == set(sc.EDGE_WORDS.tolist())
    one = byte(sc.key_family("wave_one_digit", n), 0).reshape(-1, 64)
    assert (one == one[:, :1]).all() and len(np.unique(one[:, 0])) > 1
    many = byte(sc.key_family("wave_64_digits", n), 0).reshape(-1, 64)
    assert all(len(np.unique(r)) == 64 for r in many)
    assert set(byte(sc.key_family("digits_0_255", n), 0).tolist()) == {0, 255}
    assert len(np.unique(sc.key_family("all_equal", n))) == 1
    # the tail rows of a case would sort first
    src, n_live = sc.tail_case(sc.key_family("uniform", 100) | np.uint32(1), 128)
    assert (src[n_live:, 2] < src[:n_live, 2].min()).all()


# ------------------------------------------------------------------ 2. the memory tables
def violations(air, trace):
    nb = NumericBuilder(np.asarray(trace).astype(np.uint64), [], define=False)
    air.eval_main(nb)
    return nb.first_violation()


def bus_tuples(trace, mult_col, value_cols, tag):
    """{tuple: multiplicity sum mod p} of one interaction over a host trace."""
    out = {}
    for row in np.asarray(trace).astype(np.int64):
        if row[mult_col] % P:
            key = (tag,) + tuple(int(row[c]) for c in value_cols)
            out[key] = (out.get(key, 0) + int(row[mult_col])) % P
    return out


@pytest.mark.parametrize("n,n_addr,n_selected", [(256, 16, None), (256, 16, 200), (64, 5, 1), (16, 16, 0)])
def test_memory_airs_hold_on_the_generated_tables(n, n_addr, n_selected):
    acc = generate_memory_accesses(n, n_addr, 77, n_selected=n_selected)
    assert violations(MemoryAccessAir(), acc) == -1
    table = generate_memory_table(acc)
    assert violations(MemoryTableAir(), table) == -1
    A = MemoryTableAir
    n_live = int(table[:, A.LIVE].sum())
    assert n_live == (n if n_selected is None else n_selected)
    # sorted, strictly, and a group starts exactly where the address changes
    live = table[:n_live].astype(np.int64)
    keys = live[:, A.ADDR] * (1 << 32) + live[:, A.CLK]
    assert (np.diff(keys) > 0).all()
    assert live[:, A.GAP].max(initial=0) < n
    # the reference of the sort gives the same table from the generator's source matrix
    src, n_live2 = memory_table_source(acc)
    want = sc.reference(src, [0, 1], group_keys=1, n_live=n_live2, group_start=True)
    assert n_live2 == n_live and (fill_memory_gaps(want) == table).all()
    # the memory bus balances: every sent access is received once
    sent = bus_tuples(acc, 4, (0, 1, 2, 3), MEM_TAG)
    got = bus_tuples(table, A.RECV, (A.ADDR, A.CLK, A.VALUE, A.IS_WRITE), MEM_TAG)
    assert set(sent) == set(got) and all((sent[k] + got[k]) % P == 0 for k in sent)
    # reads return the last write, by replay
    memory = {}
    for addr, clk, value, is_write, sel in acc.tolist():
        if sel:
            if is_write:
                memory[addr] = value
            assert memory[addr] == value


def test_memory_table_constraints_catch_what_they_are_for():
    acc = generate_memory_accesses(256, 16, 77)
    table = generate_memory_table(acc)
    A, air = MemoryTableAir, MemoryTableAir()
    reads = np.flatnonzero((table[:, A.IS_WRITE] == 0) & (table[:, A.LIVE] == 1))
    bad = table.copy()
    bad[reads[0], A.VALUE] ^= 1  # a read that does not return the last value
    assert violations(air, bad) >> 16 == reads[0] - 1
    bad = table.copy()
    starts = np.flatnonzero(table[:, A.START] == 1)
    bad[starts[1], A.IS_WRITE] = 0  # the first access of an address is a read
    assert violations(air, bad) >> 16 in (starts[1] - 1, starts[1])
    inside = np.flatnonzero((table[:-1, A.START] == 0) & (table[1:, A.START] == 0) & (table[1:, A.LIVE] == 1))[1]
    swapped = table.copy()
    swapped[[inside, inside + 1]] = swapped[[inside + 1, inside]]
    swapped = fill_memory_gaps(swapped)
    assert swapped[inside + 1, A.GAP] >= P - 256  # the clock went back: no range table holds this gap
    assert (np.delete(swapped[:, A.GAP], inside + 1) < 256).all()


def test_memory_airs_have_constraint_degree_three():
    for air in (MemoryAccessAir(), MemoryTableAir(), BusRangeAir()):
        aw, nc, ne = aux_dims(air)
        assert get_symbolic_constraints(air, 0, 0, aw, nc, ne).max_constraint_degree() == 3, type(air).__name__
    assert MEM_TAG != BUS_TAG


# ------------------------------------------------------------------ 3. the ABI
def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    for name in ("ts_matrix_sort_rows", "ts_matrix_gather_rows"):
        assert hasattr(lib, name) and name in _lib.ABI_SYMBOLS
    assert lib.ts_abi_version() == 5
    assert ("ts_status ts_matrix_sort_rows(ts_ctx* ctx, const ts_sort_spec* spec, const ts_matrix* src, "
            "ts_matrix** out);") in header
    assert "ts_status ts_matrix_gather_rows(ts_ctx* ctx, const ts_matrix* src, const ts_matrix* index, " in header


def test_ctypes_layout_matches_the_header(tmp_path):
    fields = [f for f, _ in _lib.SortSpecC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tapstark.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(ts_sort_spec));\n'
                   + "".join(f'    printf("%zu\\n", offsetof(ts_sort_spec, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got[0] == C.sizeof(_lib.SortSpecC) == 40
    assert got[1:] == [getattr(_lib.SortSpecC, f).offset for f in fields]


def test_null_context_refused(lib):
    spec = _lib.SortSpecC(struct_size=C.sizeof(_lib.SortSpecC), n_keys=1, n_live=1)
    fake = C.create_string_buffer(64)  # never dereferenced: the null context is refused first
    out = C.c_void_p(12345)
    assert lib.ts_matrix_sort_rows(None, C.byref(spec), C.addressof(fake), C.byref(out)) == TS_ERR_INVALID
    assert out.value is None, "a refused call left a handle"
    out = C.c_void_p(12345)
    assert lib.ts_matrix_gather_rows(None, C.addressof(fake), C.addressof(fake), 0, C.byref(out)) == TS_ERR_INVALID
    assert out.value is None
    assert lib.ts_matrix_sort_rows(None, None, None, None) == TS_ERR_INVALID
    assert lib.ts_matrix_gather_rows(None, None, None, 0, None) == TS_ERR_INVALID
