"""CPU-side checks of the TGRP tape of the three collect calls (include/tapstark.h "grouped rows"): the reference of
tests/_group_cases.py against hand-written values, the library's sequential loop over host rows against that reference
at every height, width, key count and term kind, the edge words, the height rules, every refusal that needs no matrix,
the TCOL form unchanged, the header, the builders, and the final state of memory as a statement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tapstark_amd import _lib
from tapstark_amd._lib import TsError
from tapstark_amd.air import aux_dims, get_symbolic_constraints
from tapstark_amd.airs import (FIN_TAG, MEM_TAG, MemoryFinalAir, MemoryTableAir, MemoryTableFinalAir, NumericBuilder,
                               generate_memory_accesses, generate_memory_final, generate_memory_table,
                               generate_memory_table_final, memory_final_group_spec, memory_last_program)
from tapstark_amd.collect import ALWAYS, ROW, CollectSpec, col, collect_check, collect_rows_host, const
from tapstark_amd.derive import derive_rows_host
from tapstark_amd.group import (COUNT, FIRST_ROW, INDEX, LAST_ROW, MAGIC, GroupSpec, first, greatest, group_check,
                                group_rows_host, last, least, total)

import _collect_cases as cc
import _group_cases as gc
from _group_cases import P

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


def check(spec, rows, out_height=0, what=""):
    got, live = group_rows_host(spec, rows, out_height)
    want, want_live = gc.reference(spec, rows, out_height)
    assert live == want_live, what
    same(got, want, what)
    return got, live


# ------------------------------------------------------------------ 1. by hand
ROWS = np.array([[7, 1, 10], [9, 0, 11], [7, P, 12], [P + 7, 1, P - 1], [7, 0xFFFFFFFF, P + 2], [9, 5, 13], [P + 7, 2, P - 1],
                 [P + 7, 3, P - 1]], dtype=np.uint32)
TERMS = [first(0), last(2), FIRST_ROW, LAST_ROW, COUNT, total(2), least(2), greatest(2), INDEX, const(P + 4)]


def test_reference_and_host_loop_by_hand(lib):
    spec = GroupSpec(3, 10, [col(0)], when=col(1), pad=list(range(10)), terms=TERMS)
    want = [[7, P + 2, 0, 4, 2, 12, 2, 10, 0, 4],                                # rows 0 and 4; row 2's selector is p
            [P + 7, P - 1, 3, 7, 3, (3 * (P - 1)) % P, P - 1, P - 1, 1, 4],   # p + 7 is not 7; three words p - 1
            [9, 13, 5, 5, 1, 13, 13, 13, 2, 4]]                                  # row 1's selector is 0
    for got, live in (gc.reference(spec, ROWS), group_rows_host(spec, ROWS)):
        assert live == 3 and got[:3].tolist() == want and got[3].tolist() == list(range(10)) and got.shape == (4, 10)
    assert (3 * (P - 1)) % P == P - 3 and 3 * (P - 1) >= 1 << 32, "a 32-bit accumulator would show"


# ------------------------------------------------------------------ 2. the host loop against the reference
@pytest.mark.parametrize("height", [1, 2, 3, 37, 1000, (1 << 12) + 1])
def test_host_loop_against_the_reference(lib, height):
    kinds = set()
    for name, spec, rows in gc.grid((height,)):
        kinds |= {int(k) for k in spec.tape()[7 + 2 * len(spec.keys) + spec.out_width::2]}
        check(spec, rows, what=name)
    assert kinds == set(range(10)), "every term kind"


def test_edge_words_as_selectors_keys_and_aggregates(lib):
    edge = np.array(gc.EDGE_WORDS, dtype=np.uint32)
    n = len(edge)
    rows = np.stack([np.repeat(edge, n), np.tile(edge, n), np.tile(edge[::-1], n)], axis=1)  # every (key, selector)
    spec = GroupSpec(3, 5, [col(0)], when=col(1), terms=[first(0), COUNT, total(2), least(2), greatest(2)])
    got, live = check(spec, rows)
    assert live == n and got[:live, 0].tolist() == gc.EDGE_WORDS, "p + 1 and 1, 0 and p and 2p: groups of their own"
    assert (got[:live, 1] == 4).all(), "selector words 0, p and 2p do not fire; 1, p - 1, p + 1 and 0xFFFFFFFF do"
    three = np.full((3, 1), P - 1, dtype=np.uint32)
    got, _ = check(GroupSpec(1, 1, [const(0)], terms=[total(0)]), three)
    assert got.tolist() == [[P - 3]]


# ------------------------------------------------------------------ 3. heights
def test_heights_and_the_buffer(lib):
    rows = np.stack([np.arange(100, dtype=np.uint32) % 9, np.arange(100, dtype=np.uint32)], axis=1)
    spec = GroupSpec(2, 2, [col(0)], pad=[P - 1, 3], terms=[first(0), COUNT])
    got, live = check(spec, rows)
    assert live == 9 and got.shape == (16, 2) and (got[9:] == [P - 1, 3]).all()
    assert check(spec, rows, 16)[0].shape == (16, 2) and check(spec, rows, 64)[0].shape == (64, 2)
    with pytest.raises(ValueError, match="9 groups, out_height 8"):
        gc.reference(spec, rows, 8)
    t = spec.tape()
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    used, live_c = C.c_uint64(), C.c_uint64()
    p = lambda m: m.ctypes.data_as(_lib.u32p)  # noqa: E731

    def call(out_height, cap=64):
        return lib.ts_collect_rows_host(p(t), len(t), (_lib.u32p * 1)(p(rows)), (C.c_uint64 * 1)(100), out_height, p(out), cap,
                                        C.byref(used), C.byref(live_c))

    assert call(8) == TS_ERR_INVALID
    assert lib.ts_last_error(None).decode() == "group: 9 groups, out_height 8"
    assert (out == 0xABABABAB).all() and used.value == 0 and live_c.value == 0
    assert call(16, cap=31) == TS_ERR_BUFFER
    assert "fewer than height * out_width words" in lib.ts_last_error(None).decode()
    assert (out == 0xABABABAB).all(), "a call that found the buffer too small wrote into it"
    assert call(0, cap=31) == TS_ERR_BUFFER and (out == 0xABABABAB).all()
    assert call(16, cap=32) == 0 and (used.value, live_c.value) == (16, 9)
    assert (out[32:] == 0xABABABAB).all()
    for bad in (3, 6, (1 << 27) + 1, 1 << 28):
        assert call(bad) == TS_ERR_INVALID
        assert f"out_height {bad} is neither 0 nor a power of two in [1, 2^27]" in lib.ts_last_error(None).decode()


def test_no_row_taking_part_gives_one_pad_row(lib):
    rows = np.zeros((50, 2), dtype=np.uint32)
    rows[::2, 0] = P
    got, live = check(GroupSpec(2, 3, [col(1)], when=col(0), pad=[4, 5, 6], terms=[COUNT, first(1), INDEX]), rows)
    assert live == 0 and got.tolist() == [[4, 5, 6]]


# ------------------------------------------------------------------ 4. refusals
def good():
    return GroupSpec(3, 2, [col(0), const(5)], when=col(2), pad=[1, 2], terms=[last(1), COUNT])


def words(**changes):
    """The good tape with single words replaced: index -> word."""
    t = good().tape().copy()
    for at, word in changes.items():
        t[int(at[1:])] = word
    return t


def many_aggregates(n):
    return GroupSpec(3, n, [col(0)], terms=[total(1)] * n).tape()


# the good tape: [0..6] header, keys at 7 and 9, pad at 11 and 12, terms at 13 and 15: 17 words
REFUSALS = [
    ("group: unknown spec version 2", words(w1=2)),
    ("group: src_width 0 outside [1, 2^16]", words(w2=0)),
    ("group: src_width 65537 outside [1, 2^16]", words(w2=(1 << 16) + 1)),
    ("group: out_width 0 outside [1, 64]", words(w3=0)),
    ("group: out_width 65 outside [1, 64]", words(w3=65)),
    ("group: n_keys 0 outside [1, 8]", words(w4=0)),
    ("group: n_keys 9 outside [1, 8]", words(w4=9)),
    ("group: 17 words, the header asks for 20", words(w3=3)),
    ("group: 17 words, the header asks for 19", words(w4=3)),
    ("group: 16 words, the header asks for 17", good().tape()[:-1]),
    ("group: the spec is shorter than its header", good().tape()[:6]),
    ("group: the spec is shorter than its header", good().tape()[:1]),
    ("group: selector kind must be 0 (always) or 1 (column)", words(w5=2)),
    ("group: a constant selector must be 1", words(w5=0, w6=0)),
    ("group: a constant selector must be 1", words(w5=0, w6=2)),
    ("group: the selector column is outside the source", words(w6=3)),
    ("group: key 0: kind must be 0 (constant) or 1 (column)", words(w7=2)),
    ("group: key 0: the column is outside the source", words(w8=3)),
    ("group: key 1: the constant is not below p", words(w10=P)),
    ("group: pad word 1 is not below p", words(w12=P)),
    ("group: term 0: kind must be in [0, 9]", words(w13=10)),
    ("group: term 0: the column is outside the source", words(w14=3)),
    ("group: term 0: the column is outside the source", words(w13=1, w14=3)),
    ("group: term 0: the column is outside the source", words(w13=8, w14=3)),
    ("group: term 1: the constant is not below p", words(w15=0, w16=P)),
    ("group: term 1: the value word of kinds 3, 4, 5 and 9 must be 0", words(w16=1)),
    ("group: term 1: the value word of kinds 3, 4, 5 and 9 must be 0", words(w15=9, w16=1)),
    ("group: 17 terms of kinds 6 to 8, more than 16", many_aggregates(17)),
]


@pytest.mark.parametrize("text,tape", REFUSALS, ids=[f"{k}-{t[:40]}" for k, (t, _) in enumerate(REFUSALS)])
def test_every_matrix_free_refusal(lib, text, tape):
    assert group_check(good()) == (1, 2) and group_check(many_aggregates(16)) == (1, 16)
    with pytest.raises(TsError) as e:
        group_check(tape)
    assert e.value.code == TS_ERR_INVALID and text in str(e.value), str(e.value)
    # the host loop makes the same checks first and writes nothing
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    a = np.ones((2, 3), dtype=np.uint32)
    used, live = C.c_uint64(), C.c_uint64()
    tape = np.ascontiguousarray(tape, dtype=np.uint32)
    assert lib.ts_collect_rows_host(tape.ctypes.data_as(_lib.u32p), len(tape), (_lib.u32p * 1)(a.ctypes.data_as(_lib.u32p)),
                                    (C.c_uint64 * 1)(2), 0, out.ctypes.data_as(_lib.u32p), 64, C.byref(used),
                                    C.byref(live)) == TS_ERR_INVALID
    assert text in lib.ts_last_error(None).decode() and (out == 0xABABABAB).all()


def test_host_call_refusals(lib):
    t = good().tape()
    a = np.ones((2, 3), dtype=np.uint32)
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    used, live = C.c_uint64(), C.c_uint64()
    p = lambda m: m.ctypes.data_as(_lib.u32p)  # noqa: E731

    def refused(text, src=a, h=2, out_p=p(out), used_p=C.byref(used), live_p=C.byref(live), null_sources=False,
                null_heights=False):
        ptrs = (_lib.u32p * 1)(p(src) if src is not None else None)
        st = lib.ts_collect_rows_host(p(t), len(t), None if null_sources else ptrs,
                                      None if null_heights else (C.c_uint64 * 1)(h), 0, out_p, 64, used_p, live_p)
        assert st == TS_ERR_INVALID and text in lib.ts_last_error(None).decode(), lib.ts_last_error(None)
        assert (out == 0xABABABAB).all(), "a refused call wrote into the buffer"

    refused("null argument", null_sources=True)
    refused("null argument", null_heights=True)
    refused("null argument", out_p=None)
    refused("null argument", used_p=None)
    refused("null argument", live_p=None)
    refused("null argument", src=None)
    refused("group: the height of source 0 must be in [1, 2^27]", h=0)
    refused("group: the height of source 0 must be in [1, 2^27]", h=(1 << 27) + 1)
    assert lib.ts_collect_check(p(t), len(t), None, None) == 0, "both outputs may be null"
    fake = C.create_string_buffer(64)  # never dereferenced: the null context is refused first
    out_h, n_live = C.c_void_p(12345), C.c_uint64(77)
    assert lib.ts_matrix_collect_rows(None, p(t), len(t), (C.c_void_p * 4)(C.addressof(fake)), 0, C.byref(out_h),
                                      C.byref(n_live)) == TS_ERR_INVALID
    assert out_h.value is None and n_live.value == 0, "a refused call left a handle"


# ------------------------------------------------------------------ 5. the TCOL form is what it was
def collect_good():  # the good() tape of tests/test_collect_cpu.py
    return CollectSpec([3, 2], 2, pad=[1, 2]).emit(0, when=col(2), terms=[col(0), ROW]).emit(1, terms=[const(5), col(1)])


def test_tcol_tapes_still_collect(lib):
    assert collect_check(collect_good()) == (2, 2)
    for seed in range(3):
        widths = [5, 2, 9][:1 + seed]
        sources = [cc.random_rows(seed + 7 * s, 100 + 37 * s, w) for s, w in enumerate(widths)]
        spec = cc.random_spec(seed, widths, 6, 7)
        got, live = collect_rows_host(spec, sources)
        want, want_live = cc.reference(spec, sources)
        assert live == want_live
        same(got, want, f"seed {seed}")
    for magic, text in ((0x4C4F4354 + 1, "collect: bad magic (not a TCOL spec)"), (MAGIC + 1, "collect: bad magic"),
                        (MAGIC - 1, "collect: bad magic")):
        t = collect_good().tape().copy()
        t[0] = magic
        with pytest.raises(TsError, match="collect: bad magic") as e:
            collect_check(t)
        assert text in str(e.value)
    with pytest.raises(TsError, match="collect: the spec is shorter than its header"):
        collect_check(collect_good().tape()[:4])
    assert lib.ts_collect_check(None, 5, None, None) == TS_ERR_INVALID and "collect: null spec" in lib.ts_last_error(None).decode()


# ------------------------------------------------------------------ 6. the ABI, the header and the builders
def test_abi_and_header(lib):
    header = open(os.path.join(ROOT, "include", "tapstark.h")).read()
    assert lib.ts_abi_version() == 5 and len(_lib.ABI_SYMBOLS) == 161
    section = "---- grouped rows: one row per distinct key tuple, in HBM ----"
    assert header.count(section) == 1
    assert (header.index("---- collected rows") < header.index("ts_status ts_collect_rows_host(") < header.index(section)
            < header.index("---- joined rows") < header.index("---- expanded rows") < header.index("ts_abi_version"))
    assert "enum { TS_GROUP_MAX_KEYS = 8, TS_GROUP_MAX_AGGREGATES = 16, TS_GROUP_MAX_WIDTH = 64 };" in header
    between = header[header.index(section):header.index("---- joined rows")]
    assert re.findall(r"\bts_\w+\(", between) == [], "the new section declares and names no call"
    rust = open(os.path.join(ROOT, "bindings", "rust", "tapstark-gpu", "src", "ffi.rs")).read()
    assert "GROUP_MAX_KEYS" in rust and "has not been compiled" in rust


CPP_GROUP = r"""
#include <stdio.h>
#include "tapstark_air.hpp"
int main() {
    using ts::air::Group;
    Group g(9, 11, {Group::col(2), Group::constant(0x78000001ull + 3)}, Group::col(4), {7, 8});
    g.terms({Group::first(0), Group::last(1), Group::first_row(), Group::last_row(), Group::count(), Group::total(3),
             Group::least(5), Group::greatest(6), Group::index(), Group::constant(12), Group::col(8)});
    for (uint32_t w : g.tape()) printf("%u\n", w);
    Group all(1, 1, {Group::col(0)});
    all.terms({Group::count()});
    for (uint32_t w : all.tape()) printf("%u\n", w);
    return 0;
}
"""


def test_cpp_builder_writes_the_python_tape(lib, tmp_path):
    src = tmp_path / "group.cpp"
    src.write_text(CPP_GROUP)
    exe = str(tmp_path / "group")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    spec = GroupSpec(9, 11, [col(2), const(P + 3)], when=col(4), pad=[7, 8] + [0] * 9,
                     terms=[first(0), last(1), FIRST_ROW, LAST_ROW, COUNT, total(3), least(5), greatest(6), INDEX, 12, col(8)])
    every = GroupSpec(1, 1, [col(0)], when=ALWAYS, terms=[COUNT])
    assert got == spec.tape().tolist() + every.tape().tolist()
    assert len(spec.tape()) == 7 + 2 * 2 + 3 * 11 and group_check(spec) == (1, 11) and group_check(every) == (1, 1)


# ------------------------------------------------------------------ 7. the statement
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


@pytest.mark.parametrize("n,n_addr,n_selected", [(256, 16, None), (256, 16, 200), (64, 5, 1), (64, 8, None)])
def test_memory_final_airs_hold_and_the_bus_balances(lib, n, n_addr, n_selected):
    acc = generate_memory_accesses(n, n_addr, 77, n_selected=n_selected)
    table = generate_memory_table_final(acc)
    T, F = MemoryTableFinalAir, MemoryFinalAir
    same(table[:, :8], generate_memory_table(acc), "MemoryTableAir's columns")
    assert violations(MemoryTableFinalAir(), table) == -1
    same(derive_rows_host(memory_last_program(), table[:, :8]), table, "`last` by one derive over the next row")
    final, n_groups = group_rows_host(memory_final_group_spec(), table)
    same(final, generate_memory_final(table), "ONE group call over the sorted table")
    same(final, gc.reference(memory_final_group_spec(), table)[0])
    assert violations(MemoryFinalAir(), final) == -1
    # final value, last clock and number of accesses of every touched address, by replay
    memory = {}
    for addr, clk, value, is_write, sel in acc.tolist():
        if sel:
            memory[addr] = (clk, value, memory.get(addr, (0, 0, 0))[2] + 1)
    assert n_groups == len(memory) and {r[0]: (r[1], r[2], r[3]) for r in final[:n_groups].tolist()} == memory
    assert not final[n_groups:].any()
    # the FIN bus balances: every address group sends its last access once, the final table receives it once
    sent = bus_tuples(table, T.LAST, (T.ADDR, T.CLK, T.VALUE), FIN_TAG)
    got = bus_tuples(final, F.RECV, (F.ADDR, F.CLK, F.VALUE), FIN_TAG)
    assert set(sent) == set(got) and len(sent) == n_groups and all((sent[k] + got[k]) % P == 0 for k in sent)
    # a changed final value: every constraint still holds, the bus does not balance
    if n_groups > 1:
        bad = final.copy()
        bad[1, F.VALUE] = (int(bad[1, F.VALUE]) + 1) % P
        assert violations(MemoryFinalAir(), bad) == -1
        assert set(bus_tuples(bad, F.RECV, (F.ADDR, F.CLK, F.VALUE), FIN_TAG)) != set(sent)
    # `last` on a row that is not the last of its address is a violated constraint
    inside = np.flatnonzero((table[:-1, T.LIVE] == 1) & (table[1:, T.START] == 0) & (table[1:, T.LIVE] == 1))
    if len(inside):
        bad = table.copy()
        bad[inside[0], T.LAST] = 1
        assert violations(MemoryTableFinalAir(), bad) >> 16 == inside[0]


def test_memory_final_airs_have_constraint_degree_three():
    for air in (MemoryTableFinalAir(), MemoryFinalAir()):
        aw, nc, ne = aux_dims(air)
        assert get_symbolic_constraints(air, 0, 0, aw, nc, ne).max_constraint_degree() == 3, type(air).__name__
    assert FIN_TAG not in (MEM_TAG, 7, 13, 17, 19) and MemoryTableFinalAir.LAST == MemoryTableAir.START + 1
