"""CPU-side checks of the row programs of ts_matrix_derive (include/tapstark.h "derived columns"): the reference of
tests/_derive_cases.py against hand-written values, ts_derive_rows_host -- the library's own lowered program over host
rows -- against that reference, every refusal of ts_derive_check, the slot count of the lowering, the symbols, and the
C++ builder against the Python one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tapstark_amd import _lib
from tapstark_amd.airs import (MemoryTableAir, fill_memory_gaps, generate_memory_accesses, generate_memory_table,
                               memory_gap_program, memory_table_source, memory_table_source_program)
from tapstark_amd.derive import DeriveBuilder, derive_check, derive_rows_host

import _derive_cases as dc
from _derive_cases import ADD, AND, BITS, COL, CONST, INV, IS_ZERO, LT, MUL, NEG, ROW, SUB, XOR
from _field_cases import E, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID = 1
FUZZ = int(os.environ.get("TS_DERIVE_FUZZ", "100"))


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


def col2(prog, rows):
    return [int(x) for x in dc.reference(prog, rows)[:, 2]]


# ------------------------------------------------------------------ 1. the reference, by hand
def test_reference_reads_stored_words_reduced():
    rows = np.array([[0xFFFFFFFF, P], [P + 1, 1 << 31], [5, P - 1]], dtype=np.uint32)
    prog = dc.tape(2, [(COL, 0, 0), (COL, 0, 1)], [(0, 2), (1, 3)])
    got = dc.reference(prog, rows)
    assert got[:, 2].tolist() == [268435453, 1, 5]
    assert got[:, 3].tolist() == [0, (1 << 31) - P, P - 1]
    assert (got[:, :2] == rows).all(), "untouched columns are copied as stored"
    assert 0xFFFFFFFF % P == 268435453


def test_reference_field_ops_by_hand():
    rows = np.array([[P - 1, 2], [0, 0], [7, P - 3]], dtype=np.uint32)
    assert col2(dc.op_program(ADD), rows) == [1, 0, 4]
    assert col2(dc.op_program(SUB), rows) == [P - 3, 0, 10]
    assert col2(dc.op_program(NEG), rows) == [1, 0, P - 7]
    assert col2(dc.op_program(MUL), rows) == [P - 2, 0, P - 21]
    assert col2(dc.op_program(IS_ZERO), rows) == [0, 1, 0]
    assert col2(dc.op_program(LT), rows) == [0, 0, 1]
    assert col2(dc.op_program(ROW), rows) == [0, 1, 2]
    assert col2(dc.op_program(dc.IS_FIRST), rows) == [1, 0, 0]
    assert col2(dc.op_program(dc.IS_LAST), rows) == [0, 0, 1]
    assert col2(dc.op_program(dc.IS_TRANS), rows) == [1, 1, 0]
    assert col2(dc.op_program(CONST), rows) == [P - 1] * 3
    assert col2(dc.op_program(COL), rows) == [0, P - 3, 2], "column 1 of the NEXT row, cyclic"


def test_reference_integer_ops_by_hand():
    rows = np.array([[0x40000000, 0x3FFFFFFF], [0x55555555, 0x2AAAAAAA], [P - 1, 1], [0b1011 << 7, 0]], dtype=np.uint32)
    # 0x7FFFFFFF >= p reduces: 0x7FFFFFFF - p = 0x07FFFFFE; (p - 1) ^ 1 = p reduces to 0
    assert col2(dc.op_program(XOR), rows) == [0x07FFFFFE, 0x7FFFFFFF - P, 0, 0b1011 << 7]
    assert 0x7FFFFFFF >= P
    assert col2(dc.op_program(AND), rows) == [0, 0, 0, 0]
    assert col2(dc.op_program(BITS), rows)[3] == 0b1011
    assert col2(dc.op_program(BITS), rows)[2] == ((P - 1) >> 7) & 0xFFF


def test_reference_inverse_and_limbs_on_the_edge_set():
    rows = np.array([[e, 0] for e in E], dtype=np.uint32)
    nodes = [(COL, 0, 0), (INV, 0, 0), (MUL, 0, 1), (BITS, 0, 0 | 16 << 8), (BITS, 0, 16 | 15 << 8),
             (CONST, 1 << 16, 0), (MUL, 4, 5), (ADD, 3, 6)]
    for force in ("int", "u64"):
        got = dc.reference(dc.tape(2, nodes, [(1, 2), (2, 3), (7, 4)]), rows, force=force)
        for e, (inv, one, back) in zip(E, got[:, 2:].tolist()):
            assert inv == (pow(e, -1, P) if e else 0)
            assert one == (1 if e else 0)
            assert back == e, "BITS(0,16) + 2^16 BITS(16,15) recomposes the value"


def test_reference_two_evaluators_agree():
    for seed in range(20):
        prog = dc.random_program(seed, 3)
        rows = dc.random_rows(seed, 33, 3)
        assert (dc.reference(prog, rows, force="int") == dc.reference(prog, rows, force="u64")).all()


def test_random_programs_are_what_they_claim():
    ops, offsets, over, app = set(), set(), 0, 0
    for seed in range(100):
        w, nodes, outputs = dc.parse(dc.random_program(seed, 5))
        assert 4 <= len(nodes) <= 60 and 1 <= len(outputs) <= 6
        ops |= {n[0] for n in nodes}
        offsets |= {n[1] for n in nodes if n[0] == COL}
        over += sum(d < w for _, d in outputs)
        app += sum(d >= w for _, d in outputs)
        derive_check(dc.random_program(seed, 5), 5)
    assert ops == set(dc.ALL_OPS) and offsets == {0, 1, 2} and over and app


# ------------------------------------------------------------------ 2. ts_derive_rows_host against the reference
@pytest.mark.parametrize("op", dc.ALL_OPS)
def test_host_rows_each_op_on_planted_pairs(lib, op):
    prog = dc.op_program(op)
    pairs = dc.planted_pairs()
    assert len(pairs) == len(dc.STORED) ** 2
    for rows in (pairs, pairs[1234:1235], pairs[777:779]):
        got, want = derive_rows_host(prog, rows), dc.reference(prog, rows)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (op, rows[bad[0][0]].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


@pytest.mark.parametrize("height", [1, 2, 8])
def test_host_rows_cyclic_neighbours(lib, height):
    b = DeriveBuilder(2)
    b.output(b.next(0) - b.prev(0), 2)
    b.output(b.next(1), 0)
    b.output(b.prev(1), 3)
    rows = np.stack([np.arange(height) + 10, 100 - np.arange(height)], axis=1).astype(np.uint32)
    got = derive_rows_host(b, rows)
    assert (got == dc.reference(b.tape(), rows)).all()
    assert got[:, 0].tolist() == np.roll(rows[:, 1], -1).tolist()
    assert got[:, 3].tolist() == np.roll(rows[:, 1], 1).tolist()
    assert got[0, 2] == (int(rows[1 % height, 0]) - int(rows[-1, 0])) % P


def test_host_rows_random_programs(lib):
    for seed in range(FUZZ):
        width = (1, 3, 5, 17)[seed % 4]
        prog = dc.random_program(seed, width)
        rows = dc.random_rows(seed, (1, 2, 37, 64)[(seed // 4) % 4], width)
        got, want = derive_rows_host(prog, rows), dc.reference(prog, rows)
        assert got.shape == want.shape and (got == want).all(), seed


def test_host_rows_memory_programs(lib):
    acc = generate_memory_accesses(256, 16, 77, n_selected=200)
    src, n_live = memory_table_source(acc)
    assert n_live == 200
    assert (derive_rows_host(memory_table_source_program(), acc) == src).all()
    table = generate_memory_table(acc)
    blank = table.copy()
    blank[:, MemoryTableAir.GAP] = 12345  # whatever stood there is overwritten
    got = derive_rows_host(memory_gap_program(), blank)
    assert (got == table).all() and (got == fill_memory_gaps(blank)).all()


def test_host_rows_refusals(lib):
    prog = dc.op_program(ADD)
    rows = np.zeros((4, 2), dtype=np.uint32)
    out = np.zeros((4, 3), dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(_lib.u32p)
    assert lib.ts_derive_rows_host(p(prog), len(prog), p(rows), 4, 2, p(out), 11) == 6  # TS_ERR_BUFFER
    assert lib.ts_derive_rows_host(p(prog), len(prog), p(rows), 0, 2, p(out), 12) == TS_ERR_INVALID
    assert b"height" in lib.ts_last_error(None)
    assert lib.ts_derive_rows_host(p(prog), len(prog), None, 4, 2, p(out), 12) == TS_ERR_INVALID
    assert lib.ts_derive_rows_host(p(prog), len(prog), p(rows), 4, 2, p(out), 12) == 0


# ------------------------------------------------------------------ 3. ts_derive_check
ADD_NODES = [(COL, 0, 0), (COL, 0, 1), (ADD, 0, 1)]
REFUSALS = {
    "magic": (lambda: np.concatenate([[0x54415354], dc.tape(2, ADD_NODES, [(2, 2)])[1:]]).astype(np.uint32), "magic"),
    "version": (lambda: np.concatenate([[dc.MAGIC, 2], dc.tape(2, ADD_NODES, [(2, 2)])[2:]]).astype(np.uint32), "version"),
    "word count": (lambda: dc.tape(2, ADD_NODES, [(2, 2)])[:-1], "words"),
    "short header": (lambda: dc.tape(2, ADD_NODES, [(2, 2)])[:4], "header"),
    "source width": (lambda: dc.tape(3, ADD_NODES, [(2, 3)]), "columns"),
    "unknown op 2": (lambda: dc.tape(2, ADD_NODES + [(2, 0, 0)], [(2, 2)]), "unknown op 2"),
    "unknown op 39": (lambda: dc.tape(2, ADD_NODES + [(39, 0, 0)], [(2, 2)]), "unknown op 39"),
    "operand is the node itself": (lambda: dc.tape(2, [(COL, 0, 0), (NEG, 1, 0)], [(1, 2)]), "earlier node"),
    "second operand later": (lambda: dc.tape(2, [(COL, 0, 0), (ADD, 0, 2), (COL, 0, 1)], [(1, 2)]), "earlier node"),
    "COL offset": (lambda: dc.tape(2, [(COL, 3, 0)], [(0, 2)]), "offset"),
    "COL column": (lambda: dc.tape(2, [(COL, 0, 2)], [(0, 2)]), "outside the source"),
    "CONST": (lambda: dc.tape(2, [(CONST, P, 0)], [(0, 2)]), "below p"),
    "BITS nbits 0": (lambda: dc.tape(2, [(COL, 0, 0), (BITS, 0, 3)], [(1, 2)]), "BITS"),
    "BITS past bit 31": (lambda: dc.tape(2, [(COL, 0, 0), (BITS, 0, 16 | 16 << 8)], [(1, 2)]), "BITS"),
    "no nodes": (lambda: dc.tape(2, [], [(0, 2)]), "n_nodes"),
    "no outputs": (lambda: dc.tape(2, ADD_NODES, []), "n_outputs"),
    "too many nodes": (lambda: dc.tape(2, [(COL, 0, 0)] * 4097, [(0, 2)]), "4096"),
    "too many outputs": (lambda: dc.tape(2, [(COL, 0, 0)], [(0, c) for c in range(257)]), "256"),
    "output node": (lambda: dc.tape(2, ADD_NODES, [(3, 2)]), "names no node"),
    "a gap beyond the source": (lambda: dc.tape(2, ADD_NODES, [(2, 3)]), "column 2"),
    "a column named twice": (lambda: dc.tape(2, ADD_NODES, [(2, 1), (0, 1)]), "two outputs"),
    "wider than 2^16": (lambda: dc.tape(2, ADD_NODES, [(2, 1 << 16)]), "2^16"),
    "49 values at once": (lambda: dc.sum_of_loads_program(49), "49 values at once, the limit is 48"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_check_refuses(lib, name):
    make, text = REFUSALS[name]
    prog = np.ascontiguousarray(make(), dtype=np.uint32)
    src_width = 49 if name.startswith("49") else 2
    w, n, live = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    st = lib.ts_derive_check(prog.ctypes.data_as(_lib.u32p), len(prog), src_width, C.byref(w), C.byref(n), C.byref(live))
    assert st == TS_ERR_INVALID
    assert text in lib.ts_last_error(None).decode(), lib.ts_last_error(None)
    assert (w.value, n.value, live.value) == (0, 0, 0)
    with pytest.raises(_lib.TsError, match="TS_ERR_INVALID"):
        derive_check(prog, src_width)


def test_check_null_program(lib):
    assert lib.ts_derive_check(None, 8, 2, None, None, None) == TS_ERR_INVALID
    assert b"null" in lib.ts_last_error(None)
    ok = dc.op_program(ADD)
    assert lib.ts_derive_check(ok.ctypes.data_as(_lib.u32p), len(ok), 2, None, None, None) == 0


@pytest.mark.parametrize("k", [1, 2, 48])
def test_check_counts_live_values(lib, k):
    info = derive_check(dc.sum_of_loads_program(k), k)
    assert info == {"out_width": k + 1, "n_instructions": 2 * k - 1, "n_live": k}


def test_check_does_not_count_dead_nodes(lib):
    live = dc.tape(2, ADD_NODES, [(2, 2)])
    dead = [(COL, 0, 0), (COL, 1, 1), (MUL, 0, 1), (INV, 2, 0), (COL, 0, 1), (XOR, 3, 4), (ADD, 0, 4)]
    padded = dc.tape(2, dead, [(6, 2)])
    assert derive_check(padded, 2) == derive_check(live, 2) == {"out_width": 3, "n_instructions": 3, "n_live": 2}
    rows = dc.random_rows(3, 16, 2)
    assert (derive_rows_host(padded, rows) == derive_rows_host(live, rows)).all()
    # a dead node is still checked
    with pytest.raises(_lib.TsError, match="unknown op"):
        derive_check(dc.tape(2, ADD_NODES + [(99, 0, 0)], [(2, 2)]), 2)


def test_check_one_node_into_two_columns(lib):
    prog = dc.tape(2, ADD_NODES, [(2, 2), (2, 0), (0, 3)])
    assert derive_check(prog, 2) == {"out_width": 4, "n_instructions": 3, "n_live": 2}
    rows = dc.random_rows(5, 9, 2)
    assert (derive_rows_host(prog, rows) == dc.reference(prog, rows)).all()


# ------------------------------------------------------------------ 4. the ABI and the builders
def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    for name in ("ts_matrix_derive", "ts_derive_check", "ts_derive_rows_host"):
        assert hasattr(lib, name) and name in _lib.ABI_SYMBOLS
        assert f"ts_status {name}(" in header
    assert lib.ts_abi_version() == 5
    assert "enum { TS_DERIVE_MAX_NODES = 4096, TS_DERIVE_MAX_OUTPUTS = 256, TS_DERIVE_MAX_LIVE = 48 };" in header
    ffi = open(os.path.join(ROOT, "bindings", "rust", "tapstark-gpu", "src", "ffi.rs")).read()
    for name in ("ts_matrix_derive", "ts_derive_check", "ts_derive_rows_host"):
        assert f"pub fn {name}(" in ffi


def test_null_context_refused(lib):
    prog = dc.op_program(ADD)
    fake = C.create_string_buffer(64)  # never dereferenced: the null context is refused first
    out = C.c_void_p(12345)
    assert lib.ts_matrix_derive(None, prog.ctypes.data_as(_lib.u32p), len(prog), C.addressof(fake),
                                C.byref(out)) == TS_ERR_INVALID
    assert out.value is None, "a refused call left a handle"
    assert lib.ts_matrix_derive(None, None, 0, None, None) == TS_ERR_INVALID


def test_python_builder_operators():
    b = DeriveBuilder(3)
    x, y = b.col(0), b.next(1)
    b.output((x + y) * 3 - (-x), 3)
    b.output((x & y) ^ 5, 4)
    b.output(x.lt(y) + x.inv() * x.is_zero() + b.row() + b.is_last_row() + b.prev(2).bits(3, 4), 0)
    w, nodes, outputs = dc.parse(b.tape())
    assert w == 3 and [d for _, d in outputs] == [3, 4, 0]
    assert {n[0] for n in nodes} >= {CONST, COL, ADD, SUB, NEG, MUL, AND, XOR, LT, INV, IS_ZERO, ROW, BITS, dc.IS_LAST}
    assert any(n[0] == BITS and n[2] == 3 | 4 << 8 for n in nodes)
    derive_check(b, 3)
    rows = dc.random_rows(9, 8, 3)
    x0, y1 = rows[:, 0].astype(object) % P, np.roll(rows[:, 1], -1).astype(object) % P
    assert dc.reference(b.tape(), rows)[:, 3].tolist() == [int(v) for v in ((x0 + y1) * 3 + x0) % P]


CPP_GAP = r"""
#include <stdio.h>
#include "tapstark_air.hpp"
int main() {
    using ts::air::DExpr;
    ts::air::Derive b(8);
    // addr 0, clk 1, live 4, gap 6, start 7; one operation per statement, in the order the Python program makes them
    DExpr start = b.col(7);
    DExpr addr = b.col(0);
    DExpr addr_prev = b.prev(0);
    DExpr addr_step = addr - addr_prev;
    DExpr by_addr = start * addr_step;
    DExpr not_start = 1 - start;
    DExpr clk = b.col(1);
    DExpr clk_prev = b.prev(1);
    DExpr clk_step = clk - clk_prev;
    DExpr by_clk = not_start * clk_step;
    DExpr both = by_addr + by_clk;
    DExpr step = both - 1;
    DExpr live = b.col(4);
    DExpr first = b.is_first_row();
    DExpr not_first = 1 - first;
    DExpr gated = live * not_first;
    b.output(gated * step, 6);
    for (uint32_t w : b.tape()) printf("%u\n", w);
    return 0;
}
"""


def test_cpp_builder_emits_the_python_tape(tmp_path):
    src = tmp_path / "gap.cpp"
    src.write_text(CPP_GAP)
    exe = str(tmp_path / "gap")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == memory_gap_program().tape().tolist()
