"""CPU-side checks of the iterate form of ts_matrix_derive (include/tapstark.h "iterated columns"): the reference of
tests/_iterate_cases.py against hand-written values, ts_derive_rows_host -- the library's own lowered list walked down
host rows -- against that reference, the slot count of the lowering, every refusal with its text, TDER tapes unchanged,
the builders, the sponge AIRs, and the checks and the host loop under the sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tapstark_amd import _lib
from tapstark_amd.air import get_symbolic_constraints
from tapstark_amd.airs import (SPONGE_IV, NumericBuilder, SpongeCallAir, SpongeChipAir, generate_sponge_call_trace,
                               generate_sponge_chip_trace, sponge_expand_spec, sponge_program)
from tapstark_amd.derive import DeriveBuilder, derive_check, derive_rows_host
from tapstark_amd.expand import expand_rows_host
from tapstark_amd.iterate import IterateBuilder, iterate_check, iterate_rows_host
from tapstark_amd.join import KEEP, JoinSpec, col, join_rows_host

import _derive_cases as dc
import _iterate_cases as ic
from _bus_cases import aux_dims
from _derive_cases import ADD, COL, CONST, MUL
from _field_cases import P
from _iterate_cases import CARRY, IS_GROUP_FIRST, IS_GROUP_LAST, NO_RESET, STEP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_INVARIANT = 1, 5
FUZZ = int(os.environ.get("TS_ITERATE_FUZZ", "100"))


@pytest.fixture(scope="module")
def lib():
    from tapstark_amd.build import build

    build()
    return _lib.lib()


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def grouped(seed, width, lengths, column=0):
    starts, height = ic.starts_of_lengths(lengths)
    return ic.with_resets(dc.random_rows(seed, height, width), column, starts, seed)


# ------------------------------------------------------------------ 1. the reference, by hand
def test_reference_running_sum_by_hand():
    rows = np.array([[1, 5], [0, 7], [P, 1], [P + 1, P - 1], [0, 2], [0xFFFFFFFF, 3], [2 * P, 4]], dtype=np.uint32)
    prog = ic.tape(2, [(CARRY, 0, 0), (COL, 0, 1), (ADD, 0, 1), (STEP, 0, 0), (IS_GROUP_FIRST, 0, 0), (IS_GROUP_LAST, 0, 0)],
                   [(2, 2), (0, 3), (3, 4), (4, 5), (5, 6)], [(2, 10)], 0)
    got = ic.reference(prog, rows)
    # groups start on rows 0, 3 (p + 1) and 5 (0xFFFFFFFF); 0, p and 2p do not fire
    assert got[:, 2].tolist() == [15, 22, 23, 9, 11, 13, 17]
    assert got[:, 3].tolist() == [10, 15, 22, 10, 9, 10, 13], "CARRY reads the value from before the row"
    assert got[:, 4].tolist() == [0, 1, 2, 0, 1, 0, 1]
    assert got[:, 5].tolist() == [1, 0, 0, 1, 0, 1, 0]
    assert got[:, 6].tolist() == [0, 0, 1, 0, 1, 0, 1]
    assert (got[:, :2] == rows).all()
    assert ic.group_starts(rows.tolist(), 0) == [0, 3, 5] and ic.group_starts(rows.tolist(), NO_RESET) == [0]


def test_reference_fibonacci_is_the_closed_loop():
    rows = np.zeros((40, 1), dtype=np.uint32)
    rows[[0, 25], 0] = 1
    got = ic.reference(ic.fibonacci(1, 0), rows)
    a, b, want = 0, 1, []
    for r in range(40):
        if r == 25:
            a, b = 0, 1
        want.append([a, b])
        a, b = b, (a + b) % P
    assert got[:, 1:].tolist() == want


def test_random_programs_are_what_they_claim():
    ops, resets, n_carries = set(), set(), set()
    for seed in range(100):
        w, nodes, outputs, carries, reset, _ = ic.parse(ic.random_program(seed, 5))
        ops |= {n[0] for n in nodes}
        resets.add(reset == NO_RESET)
        n_carries.add(len(carries))
        iterate_check(ic.random_program(seed, 5), 5)
    assert ops == set(ic.ALL_OPS) and resets == {True, False} and n_carries == {1, 2, 3, 4}


# ------------------------------------------------------------------ 2. ts_derive_rows_host against the reference
@pytest.mark.parametrize("op", ic.ALL_OPS)
def test_host_rows_each_op(lib, op):
    prog = ic.op_program(op)
    for lengths in ([1], [2, 1], [1, 2, 5, 64, 1, 70, 13]):
        rows = grouped(op, 3, lengths)
        same(iterate_rows_host(prog, rows), ic.reference(prog, rows), (op, lengths))
    pairs = dc.planted_pairs()  # every ordered pair of stored words in (x, y), a group start every third row
    rows = np.concatenate([np.zeros((len(pairs), 1), dtype=np.uint32), pairs], axis=1)
    rows[::3, 0] = 1
    same(iterate_rows_host(prog, rows), ic.reference(prog, rows), op)


def test_host_rows_random_programs(lib):
    for seed in range(FUZZ):
        width = (1, 3, 5, 17)[seed % 4]
        prog = ic.random_program(seed, width)
        rows = ic.random_rows(seed, (1, 2, 37, 64, 100)[(seed // 4) % 5], width, ic.parse(prog)[4])
        same(iterate_rows_host(prog, rows), ic.reference(prog, rows), seed)


@pytest.mark.parametrize("height", [1, 2, 3, 37, 100])
def test_host_rows_two_carries_swapped(lib, height):
    rows = grouped(height, 2, [height])
    got = iterate_rows_host(ic.fibonacci(2, NO_RESET), rows)
    a, b = 0, 1
    for r in range(height):
        assert (int(got[r, 2]), int(got[r, 3])) == (a, b)
        a, b = b, (a + b) % P
    rows = grouped(height, 2, [1] * height)  # every row a start
    got = iterate_rows_host(ic.fibonacci(2, 0), rows)
    assert (got[:, 2] == 0).all() and (got[:, 3] == 1).all()


def test_host_rows_sixteen_carries_and_carries_no_output_reaches(lib):
    rows = grouped(16, 2, [7, 1, 90, 31])
    prog = ic.sixteen_carries(2, 0)
    same(iterate_rows_host(prog, rows), ic.reference(prog, rows))
    assert iterate_check(prog, 2)["n_live"] >= 32, "16 carry slots and 16 copies held to the latches"
    nodes = [(CARRY, 0, 0), (COL, 0, 1), (ADD, 0, 1), (CARRY, 1, 0), (CONST, 1, 0), (ADD, 3, 4)]
    prog = ic.tape(2, nodes, [(2, 2)], [(2, 0), (5, 9)], 0)
    same(iterate_rows_host(prog, rows), ic.reference(prog, rows))
    assert iterate_check(prog, 2)["n_instructions"] == 6, "the nodes of a carry are kept though no output reaches them"


def test_host_rows_reset_words_and_a_start_on_the_last_row(lib):
    words = [0, P, 2 * P, P + 1, 0xFFFFFFFF, 0, 1]
    rows = np.array([[w, r + 1] for r, w in enumerate(words)], dtype=np.uint32)
    prog = ic.tape(2, [(CARRY, 0, 0), (COL, 0, 1), (ADD, 0, 1), (IS_GROUP_LAST, 0, 0)], [(2, 2), (3, 3)], [(2, 0)], 0)
    got = iterate_rows_host(prog, rows)
    same(got, ic.reference(prog, rows))
    assert got[:, 2].tolist() == [1, 3, 6, 4, 5, 11, 7], "0, p and 2p do not fire; p + 1 and 0xFFFFFFFF do"
    assert got[:, 3].tolist() == [0, 0, 1, 1, 0, 1, 1], "the start on row h-1 is a group of one row"
    prog = ic.tape(2, [(CARRY, 0, 0), (COL, 0, 1), (ADD, 0, 1)], [(2, 2)], [(2, 0)], NO_RESET)
    assert iterate_rows_host(prog, rows)[:, 2].tolist() == [1, 3, 6, 10, 15, 21, 28], "no reset column: one group"


def test_builder_program_overwrites_what_it_reads(lib):
    rows = grouped(5, 3, [4, 1, 1, 66, 130, 3])
    b = IterateBuilder(3, reset_column=0, max_group_rows=130)
    acc = b.carry(7)
    new = acc * 3 + b.col(1) + b.next(1) + b.prev(0)
    b.set_carry(acc, new)
    b.output(new, 0)
    b.output(b.step() + new * b.is_group_first() + b.is_group_last(), 1)
    got = iterate_rows_host(b, rows)
    same(got, ic.reference(b.tape(), rows))
    assert (got[:, 2] == rows[:, 2]).all()
    with pytest.raises(ValueError, match="never set"):
        c = IterateBuilder(1)
        c.carry(0)
        c.tape()


# ------------------------------------------------------------------ 3. ts_derive_check of a TITR tape
def test_check_counts_the_carry_slots(lib):
    assert iterate_check(ic.carry_and_loads_program(47), 47) == {"out_width": 48, "n_instructions": 93, "n_live": 48}
    with pytest.raises(_lib.TsError, match="iterate: the program holds 49 values at once, the limit is 48"):
        iterate_check(ic.carry_and_loads_program(48), 48)
    assert iterate_check(ic.sponge_like(2, 0), 2) == {"out_width": 3, "n_instructions": 7, "n_live": 3}


SPONGE_NODES = [(CARRY, 0, 0), (COL, 0, 1), (ADD, 0, 1)]


def _t(nodes=SPONGE_NODES, outputs=((2, 2),), carries=((2, 0),), reset=0, rows=64, width=2):
    return ic.tape(width, list(nodes), list(outputs), list(carries), reset, rows)


REFUSALS = {
    "no carries": (lambda: _t(carries=()), "iterate: n_carries 0 outside [1, 16]"),
    "17 carries": (lambda: _t(carries=[(2, 0)] * 17), "iterate: n_carries 17 outside [1, 16]"),
    "carry node": (lambda: _t(carries=[(3, 0)]), "iterate: carry 0 names no node"),
    "init": (lambda: _t(carries=[(2, P)]), "iterate: carry 0: init is not below p"),
    "CARRY index": (lambda: _t(nodes=[(CARRY, 1, 0), (COL, 0, 1), (ADD, 0, 1)]), "iterate: node 0: CARRY names no carry"),
    "reset column": (lambda: _t(reset=2), "iterate: reset_column 2 is outside the source"),
    "max_group_rows 0": (lambda: _t(rows=0), "iterate: max_group_rows is 0"),
    # three nodes and one latch: 4 instructions
    "work": (lambda: _t(rows=(1 << 18) + 1),
             "iterate: max_group_rows 262145 x 4 instructions is above the work limit of 1048576"),
    "word count": (lambda: _t()[:-1], "iterate: 20 words, the header asks for 21"),
    "short header": (lambda: _t()[:7], "iterate: the program is shorter than its header"),
    "version": (lambda: np.concatenate([[ic.MAGIC, 2], _t()[2:]]).astype(np.uint32), "iterate: unknown program version 2"),
    "source width": (lambda: _t(width=3, outputs=[(2, 3)]), "iterate: the program is written for a source of 3 columns"),
    "unknown op 39": (lambda: _t(nodes=SPONGE_NODES + [(39, 0, 0)]), "iterate: node 3: unknown op 39"),
    "unknown op 44": (lambda: _t(nodes=SPONGE_NODES + [(44, 0, 0)]), "iterate: node 3: unknown op 44"),
    "the latch is no op of a tape": (lambda: _t(nodes=SPONGE_NODES + [(62, 0, 0)]), "unknown op 62"),
    "operand later": (lambda: _t(nodes=[(CARRY, 0, 0), (ADD, 0, 2), (COL, 0, 1)]), "earlier node"),
    "a column named twice": (lambda: _t(outputs=[(2, 2), (0, 2)]), "iterate: column 2 is named by two outputs"),
    "CARRY in a TDER tape": (lambda: dc.tape(2, [(CARRY, 0, 0)], [(0, 2)]), "derive: node 0: unknown op 40"),
    "STEP in a TDER tape": (lambda: dc.tape(2, [(STEP, 0, 0)], [(0, 2)]), "derive: node 0: unknown op 41"),
    "IS_GROUP_FIRST in a TDER tape": (lambda: dc.tape(2, [(IS_GROUP_FIRST, 0, 0)], [(0, 2)]), "unknown op 42"),
    "IS_GROUP_LAST in a TDER tape": (lambda: dc.tape(2, [(IS_GROUP_LAST, 0, 0)], [(0, 2)]), "unknown op 43"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_check_refuses(lib, name):
    make, text = REFUSALS[name]
    prog = np.ascontiguousarray(make(), dtype=np.uint32)
    w, n, live = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    st = lib.ts_derive_check(prog.ctypes.data_as(_lib.u32p), len(prog), 2, C.byref(w), C.byref(n), C.byref(live))
    assert st == TS_ERR_INVALID
    assert text in lib.ts_last_error(None).decode(), lib.ts_last_error(None)
    assert (w.value, n.value, live.value) == (0, 0, 0), "a refused check zeroes its outputs"
    rows, out = np.zeros((4, 2), dtype=np.uint32), np.full((4, 4), 9, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(_lib.u32p)
    assert lib.ts_derive_rows_host(p(prog), len(prog), p(rows), 4, 2, p(out), out.size) == TS_ERR_INVALID
    assert (out == 9).all(), "a refused host call writes nothing"


def test_the_work_limit_is_exact(lib):
    assert iterate_check(_t(rows=1 << 18), 2)["n_live"] == 3  # 2^18 rows x 4 instructions = 2^20
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    assert "enum { TS_ITERATE_MAX_CARRIES = 16, TS_ITERATE_MAX_WORK = 1 << 20 };" in header


def test_the_over_long_group_with_the_least_start_row_is_named(lib):
    rows = grouped(3, 3, [40] * 3 + [41] + [40] * 2 + [300] + [50])
    prog = ic.sponge_like(3, 0, max_group_rows=40)
    text = "iterate: the group that starts at row 120 has 41 rows, max_group_rows is 40"
    assert ic.longest_refusal(rows.tolist(), 0, 40) == text
    out = np.full((len(rows), 4), 9, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(_lib.u32p)
    assert lib.ts_derive_rows_host(p(prog), len(prog), p(rows), len(rows), 3, p(out), out.size) == TS_ERR_INVARIANT
    assert lib.ts_last_error(None).decode() == text and (out == 9).all()
    rows = grouped(3, 3, [40] * 3 + [50])  # only the final group, which no start ends
    with pytest.raises(_lib.TsError, match="iterate: the group that starts at row 120 has 50 rows, max_group_rows is 40"):
        iterate_rows_host(prog, rows)
    same(iterate_rows_host(ic.sponge_like(3, 0, max_group_rows=50), rows), ic.reference(prog, rows))


def test_tder_tapes_are_unchanged(lib):
    for seed in range(40):
        width = (1, 3, 5, 17)[seed % 4]
        prog = dc.random_program(seed, width)
        rows = dc.random_rows(seed, (1, 2, 37, 64)[(seed // 4) % 4], width)
        same(derive_rows_host(prog, rows), dc.reference(prog, rows), seed)
    assert derive_check(dc.sum_of_loads_program(48), 48) == {"out_width": 49, "n_instructions": 95, "n_live": 48}
    with pytest.raises(_lib.TsError, match="derive: bad magic"):
        derive_check(np.concatenate([[0x54415354], dc.op_program(ADD)[1:]]).astype(np.uint32), 2)


# ------------------------------------------------------------------ 4. the ABI and the builders
def test_no_entry_point_was_added(lib):
    assert lib.ts_abi_version() == 5 and len(_lib.ABI_SYMBOLS) == 161
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    assert (header.index("---- derived columns") < header.index("---- iterated columns: a row program with carried state, "
                                                                 "per group, in HBM ----")
            < header.index("---- scanned columns"))


CPP_SPONGE = r"""
#include <stdio.h>
#include "tapstark_air.hpp"
int main() {
    using ts::air::DExpr;
    ts::air::Iterate b(6, 0, 12);
    // first 0, word 3, acc 4, state 5; one operation per statement, in the order the Python program makes them
    DExpr state = b.carry(0x5EED);
    DExpr word = b.col(3);
    DExpr acc = state + word;
    DExpr a2 = acc * acc;
    DExpr a4 = a2 * a2;
    DExpr a6 = a4 * a2;
    DExpr next = a6 * acc;
    b.set_carry(state, next);
    b.output(acc, 4);
    b.output(next, 5);
    for (uint32_t w : b.tape()) printf("%u\n", w);
    ts::air::Iterate c(2);
    DExpr x = c.carry(0x78000001ull + 3);
    DExpr y = c.carry(1);
    DExpr s = c.step();
    DExpr f = c.is_group_first();
    DExpr l = c.is_group_last();
    DExpr t = s + f;
    c.set_carry(x, y);
    c.set_carry(y, t * l);
    c.output(x, 2);
    for (uint32_t w : c.tape()) printf("%u\n", w);
    return 0;
}
"""


def test_cpp_builder_writes_the_python_words(lib, tmp_path):
    src = tmp_path / "iterate.cpp"
    src.write_text(CPP_SPONGE)
    exe = str(tmp_path / "iterate")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    c = IterateBuilder(2)
    x, y = c.carry(P + 3), c.carry(1)
    s, f, l = c.step(), c.is_group_first(), c.is_group_last()
    t = s + f
    c.set_carry(x, y)
    c.set_carry(y, t * l)
    c.output(x, 2)
    assert got == sponge_program(12).tape().tolist() + c.tape().tolist()
    assert iterate_check(c, 2) == {"out_width": 3, "n_instructions": 7, "n_live": 6}


# ------------------------------------------------------------------ 5. the sponge AIRs
def violations(air, trace):
    nb = NumericBuilder(np.asarray(trace).astype(np.uint64), [], define=False)
    air.eval_main(nb)
    return nb.first_violation()


@pytest.mark.parametrize("n,max_len", [(32, 12), (256, 7), (16, 1)])
def test_sponge_airs_hold_and_the_host_route_makes_the_tables(lib, n, max_len):
    A, T = SpongeCallAir, SpongeChipAir
    calls = generate_sponge_call_trace(n, max_len, 5)
    assert violations(SpongeCallAir(), calls) == -1
    chip = generate_sponge_chip_trace(calls)
    assert violations(SpongeChipAir(), chip) == -1
    for first, last, _, word, acc, state in chip.tolist():
        assert state == pow(acc, 7, P)
    # expand -> iterate -> join on the host: the chip's table, then the digests back by id
    blank = generate_sponge_call_trace(n, max_len, 5, unfilled=True)
    rows, live = expand_rows_host(sponge_expand_spec(max_len), blank)
    assert live == int(calls[calls[:, A.SEL] == 1][:, A.LEN].sum())
    same(iterate_rows_host(sponge_program(max_len), rows), chip)
    spec = JoinSpec(keys=[(col(A.ID), col(T.ID)), (1, col(T.LAST))], when=col(A.SEL), fetch=[(T.STATE, A.DIGEST, 0)], flags=KEEP)
    same(join_rows_host(spec, blank, chip)[0], calls)
    # the chip sends what the machine receives: one tuple per selected call
    sent = sorted(map(tuple, chip[chip[:, T.LAST] == 1][:, [T.ID, T.STATE]].tolist()))
    assert sent == sorted(map(tuple, calls[calls[:, A.SEL] == 1][:, [A.ID, A.DIGEST]].tolist()))
    bad = chip.copy()
    bad[int(np.flatnonzero(chip[:, T.FIRST] == 0)[0]) if max_len > 1 else 0, T.STATE] += 1
    assert violations(SpongeChipAir(), bad) != -1
    assert pow(SPONGE_IV, 7, P) == int(chip[-1, T.STATE]) or live == len(chip)


def test_sponge_constraint_degrees():
    for air, degree in ((SpongeCallAir(), 3), (SpongeChipAir(), 7)):
        aw, nc, ne = aux_dims(air)
        assert get_symbolic_constraints(air, 0, 0, aw, nc, ne).max_constraint_degree() == degree, type(air).__name__


# ------------------------------------------------------------------ 6. under the sanitizers
def test_checks_lowering_and_host_loop_are_clean_under_the_sanitizers(lib, tmp_path):
    """csrc/derive.cpp, csrc/iterate.cpp and tap-stark_amd/probe/iterate_probe.cpp built together with AddressSanitizer
    and UBSan into a stand-alone program and run over seeded programs of both kinds, the planted layouts, the over-long
    group and every refused tape, each in buffers of exactly its size: every line is what the reference gives and no
    sanitizer report ends the run."""
    from tapstark_amd import build as b

    exe = str(tmp_path / "iterate_probe")
    cmd = [b._clangxx(), "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(b._rocm(), "include"), "-I", b.CSRC,
           "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(b.PKG, "probe", "iterate_probe.cpp"),
           os.path.join(b.CSRC, "derive.cpp"), os.path.join(b.CSRC, "iterate.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def fnv(a):
        h = 0xcbf29ce484222325
        for byte in np.ascontiguousarray(a, dtype="<u4").tobytes():
            h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return h

    def words(tape, rows):
        return [len(tape), *[int(w) for w in tape], rows.shape[1], rows.shape[0], rows.size, *rows.reshape(-1).tolist()]

    cases, want = [], []

    def accepted(tape, rows, ref):
        info = derive_check(tape, rows.shape[1])
        cases.append(words(tape, rows))
        want.append(f"{info['out_width']} {info['n_instructions']} {info['n_live']} {fnv(ref(tape, rows)):016x}")

    for seed in range(24):
        width = (1, 3, 5, 17)[seed % 4]
        height = (1, 2, 37, 100)[(seed // 4) % 4]
        prog = ic.random_program(seed, width)
        accepted(prog, ic.random_rows(seed, height, width, ic.parse(prog)[4]), ic.reference)
        accepted(dc.random_program(seed, width), dc.random_rows(seed, height, width), dc.reference)
    accepted(ic.sixteen_carries(2, 0), grouped(1, 2, [7, 1, 90, 31]), ic.reference)
    accepted(ic.carry_and_loads_program(47), dc.random_rows(2, 5, 47), ic.reference)
    accepted(ic.fibonacci(1, 0), grouped(3, 1, [1] * 9 + [3]), ic.reference)
    n_accepted = len(cases)
    cases.append(words(ic.sponge_like(3, 0, max_group_rows=40), grouped(3, 3, [40] * 3 + [41] + [50])))
    want.append("refused: iterate: the group that starts at row 120 has 41 rows, max_group_rows is 40")
    rows = np.ones((2, 2), dtype=np.uint32)
    for make, text in REFUSALS.values():
        cases.append(words(np.ascontiguousarray(make(), dtype=np.uint32), rows))
        want.append(text)
    path = tmp_path / "cases.bin"
    np.array([len(cases)] + [w for c in cases for w in c], dtype="<u4").tofile(str(path))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(want)
    for k, (got, w) in enumerate(zip(lines, want)):
        assert got == w if k <= n_accepted else (w in got and got.startswith("refused: ")), (k, got, w)
