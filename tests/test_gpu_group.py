"""The TGRP tape of ts_matrix_collect_rows on the GPU against the exact reference of tests/_group_cases.py and the
library's host loop, word for word: the shapes that break the kernels (every row its own group, one group, groups
alternating by lane, group sizes astride waves and workgroups, a sorted source, nothing taking part), every value of the
two knobs, the height rules, pool poison, composition with the sort and the join, and the final state of memory proved
as a table of its own without the access table leaving HBM.  Source heights are powers of two: no call makes a matrix
of another height (the host loop is tested at other heights in tests/test_group_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd._lib import TsError
from tapstark_amd.airs import (BusRangeAir, MemoryFinalAir, MemoryTableFinalAir, generate_memory_accesses,
                               memory_final_group_spec, memory_final_tables)
from tapstark_amd.collect import ALWAYS, col, const
from tapstark_amd.group import (COUNT, FIRST_ROW, INDEX, LAST_ROW, GroupSpec, first, greatest, group_rows_host, last, least,
                                total)
from tapstark_amd.join import TABLE_ROW, JoinSpec

import _bus_cases as bc
import _group_cases as gc
import _poison
from _group_cases import P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_KNOB, HASH_KNOB = "TS_COLLECT_BLOCK_ROWS", "TS_LOGUP_HASH_BITS"
STAT_POOL_BYTES = 3  # ts_ctx_stat: bytes the device pool has reserved, handed out or not
STAT_LIVE_BLOCKS = 11  # ts_ctx_stat: pool blocks handed out and not yet given back


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv(BLOCK_KNOB, raising=False)
    monkeypatch.delenv(HASH_KNOB, raising=False)


def group(ctx, spec, rows, out_height=0):
    got, live = ts.group_rows(ctx, spec, ts.DeviceMatrix.upload(ctx, rows), out_height)
    return got.download(), live


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]}: "
                           f"{int(got[tuple(bad[0])]):#x} for {int(want[tuple(bad[0])]):#x}")


def check(ctx, spec, rows, out_height=0, what=""):
    got, live = group(ctx, spec, rows, out_height)
    want, want_live = gc.reference(spec, rows, out_height)
    assert live == want_live, what
    same(got, want, what)
    return got, live


# ------------------------------------------------------------------ 1. the grid
GRID = list(gc.grid((1 << 8, 1 << 10, 1 << 12)))


@pytest.mark.parametrize("name", [g[0] for g in GRID])
def test_grid_against_the_reference_and_the_host_loop(ctx, name):
    _, spec, rows = next(g for g in GRID if g[0] == name)
    d_src = ts.DeviceMatrix.upload(ctx, rows)
    d_out, live = ts.group_rows(ctx, spec, d_src)
    got = d_out.download()
    want, want_live = gc.reference(spec, rows)
    same(got, want, "device against the reference")
    host, host_live = group_rows_host(spec, rows)
    same(got, host, "device against the library's host loop")
    assert live == want_live == host_live
    same(d_src.download(), rows, "the source after the call")
    again, live_again = ts.group_rows(ctx, spec, d_src)
    same(again.download(), got, "a second call")
    assert live_again == live


# ------------------------------------------------------------------ 2. shapes that break the kernels
N = 1 << 12
ALL_TERMS = [first(0), last(1), FIRST_ROW, LAST_ROW, COUNT, total(2), least(2), greatest(2), INDEX, const(5), last(3)]


def _spec(width=4, keys=(col(0),), when=ALWAYS, terms=ALL_TERMS):
    return GroupSpec(width, len(terms), list(keys), when=when, pad=[P - 1] + [0] * (len(terms) - 1), terms=terms)


def _data(seed=1, height=N, width=4):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=(height, width), dtype=np.uint64).astype(np.uint32)


def test_every_row_its_own_group(ctx):
    rows = _data()
    rows[:, 0] = np.random.default_rng(2).permutation(N).astype(np.uint32) + 7
    got, live = check(ctx, _spec(), rows)
    assert live == N and (got[:, 2] == np.arange(N)).all() and (got[:, 4] == 1).all()


def test_all_rows_one_group(ctx):
    """The combined path of every wave, and one slot under all inserts."""
    rows = _data()
    rows[:, 0] = P + 1
    rows[:, 2] = P - 1  # the sum of 4096 words p - 1 needs more than 32 bits
    got, live = check(ctx, _spec(), rows)
    assert live == 1 and got.shape[0] == 1 and got[0, 4] == N and got[0, 5] == (N * (P - 1)) % P


def test_two_groups_alternating_by_lane(ctx):
    """No wave is uniform: one atomic per row and accumulator on two records."""
    rows = _data()
    rows[:, 0] = np.where(np.arange(N) % 2 == 0, 1, P + 1)  # equal mod p, two groups as stored
    got, live = check(ctx, _spec(), rows)
    assert live == 2 and got[:2, 4].tolist() == [N // 2, N // 2]


def test_group_sizes_astride_waves_and_workgroups(ctx):
    sizes = [63, 64, 65, 255, 256, 257]
    key = np.repeat(np.arange(len(sizes)), sizes)  # 960 rows
    key = np.concatenate([key, len(sizes) + np.arange(1024 - len(key)) // 3])
    rows = _data(3, 1024)
    rows[:, 0] = key.astype(np.uint32) * 3 + 1
    got, _ = check(ctx, _spec(), rows)
    assert got[:6, 4].tolist() == sizes


def test_sorted_source(ctx):
    rows = _data(4)
    rows[:, 0] = np.sort(np.random.default_rng(5).integers(0, 40, size=N)).astype(np.uint32)
    got, live = check(ctx, _spec(), rows)
    assert (np.diff(got[:live, 0].astype(np.int64)) > 0).all(), "key order on a sorted source"


def test_no_row_taking_part(ctx):
    rows = _data(5)
    rows[:, 1] = np.array([0, P, 2 * P], dtype=np.uint32)[np.arange(N) % 3]
    got, live = check(ctx, _spec(when=col(1)), rows)
    assert live == 0 and got.tolist() == [[P - 1] + [0] * (len(ALL_TERMS) - 1)], "height 1, all pad"


def test_when_on_some_rows_and_edge_words(ctx):
    rows = _data(6)
    edge = np.array(gc.EDGE_WORDS, dtype=np.uint32)
    rows[:, 0] = edge[np.random.default_rng(7).integers(0, len(edge), size=N)]
    rows[:, 1] = edge[np.arange(N) % len(edge)]
    rows[:, 2] = edge[np.random.default_rng(8).integers(0, len(edge), size=N)]
    got, live = check(ctx, _spec(when=col(1)), rows)
    assert live == len(edge), "p + 1 and 1 are two groups"


@pytest.mark.parametrize("n_keys", [1, 3, 8])
def test_keys_with_a_constant_among_them(ctx, n_keys):
    rows = gc.random_rows(20 + n_keys, N, 9, n_values=9)
    keys = [col(q) for q in range(n_keys)]
    if n_keys > 1:
        keys[1] = const(P - 1)
    check(ctx, _spec(9, keys=keys), rows)


def test_sixteen_aggregates_at_width_64(ctx):
    rows = gc.random_rows(31, N, 6)
    terms = []
    for a in range(16):
        terms.append([total, least, greatest][a % 3](a % 6))
    for c in range(48):
        terms.append([first(c % 6), last(c % 6), FIRST_ROW, LAST_ROW, COUNT, INDEX, const(c)][c % 7])
    rng = np.random.default_rng(9)
    terms = [terms[i] for i in rng.permutation(64)]
    check(ctx, GroupSpec(6, 64, [col(0), col(1)], when=col(2), pad=list(range(64)), terms=terms), rows)


def test_2_16_rows_1024_groups_8_aggregates_against_the_host_loop(ctx):
    rows = _data(10, 1 << 16, 8)
    rows[:, 0] = np.random.default_rng(11).integers(0, 1 << 10, size=1 << 16).astype(np.uint32)
    terms = [first(0), COUNT, last(7)] + [[total, least, greatest][a % 3](1 + a % 7) for a in range(8)]
    spec = _spec(8, terms=terms)
    got, live = group(ctx, spec, rows)
    host, host_live = group_rows_host(spec, rows)
    assert live == host_live == 1 << 10
    same(got, host)


# ------------------------------------------------------------------ 3. the knobs change no word
def _knob_case(height):
    rows = gc.random_rows(42, height, 6, n_values=20)
    spec = gc.random_spec(42, 6, 2)
    return spec, rows


@pytest.mark.parametrize("bits", [0, 3, 32])
def test_same_words_for_every_hash_bits(ctx, monkeypatch, bits):
    """2^8 rows: with 0 bits every tuple starts at slot 0 and the probe chains are as long as the groups are many."""
    spec, rows = _knob_case(1 << 8)
    default, live = check(ctx, spec, rows, what="default")
    monkeypatch.setenv(HASH_KNOB, str(bits))
    got, live_knob = group(ctx, spec, rows)
    same(got, default, f"{HASH_KNOB}={bits}")
    assert live_knob == live


@pytest.mark.parametrize("block_rows", [1, 7, 256, 1024])
def test_same_words_for_every_block_rows(ctx, monkeypatch, block_rows):
    """2^12 rows: with 1 row per block there are 4096 blocks and 16 trips of the offsets loop; 7 leaves a short last
    block."""
    spec, rows = _knob_case(N)
    default, live = check(ctx, spec, rows, what="default")
    monkeypatch.setenv(BLOCK_KNOB, str(block_rows))
    got, live_knob = group(ctx, spec, rows)
    same(got, default, f"{BLOCK_KNOB}={block_rows}")
    assert live_knob == live


@pytest.mark.parametrize("knob,value,text", [
    (BLOCK_KNOB, "0", r"TS_COLLECT_BLOCK_ROWS must be in \[1, 1024\]"),
    (BLOCK_KNOB, "1025", r"TS_COLLECT_BLOCK_ROWS must be in \[1, 1024\]"),
    (BLOCK_KNOB, "x", r"TS_COLLECT_BLOCK_ROWS must be in \[1, 1024\]"),
    (HASH_KNOB, "33", r"TS_LOGUP_HASH_BITS must be in \[0, 32\]"),
    (HASH_KNOB, "-1", r"TS_LOGUP_HASH_BITS must be in \[0, 32\]"),
])
def test_knob_outside_its_range_is_refused(ctx, monkeypatch, knob, value, text):
    spec, rows = _knob_case(16)
    monkeypatch.setenv(knob, value)
    with pytest.raises(TsError, match=text):
        group(ctx, spec, rows)


# ------------------------------------------------------------------ 4. heights
def test_out_heights_and_the_refusal_returns_every_block(ctx):
    rows = _data(12)
    rows[:, 0] = (np.arange(N) % 2048).astype(np.uint32)  # 2048 groups of two rows
    spec = _spec()
    got, live = check(ctx, spec, rows, out_height=2048, what="out_height = n_live: no pad row")
    assert live == 2048 and got.shape[0] == 2048
    got, _ = check(ctx, spec, rows, out_height=4096, what="out_height = 2 n_live")
    assert (got[2048:] == [P - 1] + [0] * (len(ALL_TERMS) - 1)).all()
    odd = rows.copy()
    odd[5, 0] = 1 << 20  # 2049 groups
    check(ctx, spec, odd, out_height=0, what="one more: 4096 rows, 2047 of them pad")
    # the refusal after the wait, on a context of its own: its pool holds only what this test took and gave back
    own = ts.Context(0)
    d = ts.DeviceMatrix.upload(own, odd)
    t = spec.tape()
    handles = (C.c_void_p * 4)(d.h)
    out, n_live = C.c_void_p(12345), C.c_uint64(77)
    live_before = own.stat(STAT_LIVE_BLOCKS)
    assert live_before >= 1, "the source is a live block"
    reserved = []
    for _ in range(4):
        out.value = 12345
        st = own._l.ts_matrix_collect_rows(own.h, t.ctypes.data_as(ts._lib.u32p), len(t), handles, 2048, C.byref(out),
                                           C.byref(n_live))
        assert st == 1 and own._l.ts_last_error(own.h).decode() == "group: 2049 groups, out_height 2048"
        assert not out.value and n_live.value == 0, "a refused call left a handle"
        assert own.stat(STAT_LIVE_BLOCKS) == live_before, "a refused call kept pool blocks"
        reserved.append(own.stat(STAT_POOL_BYTES))
    assert reserved[1:] == reserved[:-1], "a refused call kept pool blocks"
    for bad in (3, 1 << 28):
        with pytest.raises(TsError, match="neither 0 nor a power of two"):
            ts.group_rows(own, spec, d, bad)
        assert own.stat(STAT_LIVE_BLOCKS) == live_before
    d_out, _ = ts.group_rows(own, spec, d)
    assert own.stat(STAT_LIVE_BLOCKS) == live_before + 1, "an accepted call keeps its result and nothing else"
    same(d_out.download(), gc.reference(spec, odd)[0], "the matrix still groups")


def test_refusals_leave_no_handle(ctx):
    rows = _data(13, 16)
    d = ts.DeviceMatrix.upload(ctx, rows)
    good = _spec()
    lib, out, live = ctx._l, C.c_void_p(), C.c_uint64()

    def refused(text, spec=good, ctx_h=ctx.h, handles=(d.h,)):
        out.value = 12345
        t = spec.tape()
        st = lib.ts_matrix_collect_rows(ctx_h, t.ctypes.data_as(ts._lib.u32p), len(t), (C.c_void_p * 4)(*handles), 0,
                                        C.byref(out), C.byref(live))
        assert st == 1 and text in lib.ts_last_error(ctx_h).decode(), lib.ts_last_error(ctx_h)
        assert not out.value, "a refused call left a handle"

    refused("null argument", handles=(None,))
    refused("group: the spec is written for a source 0 of 5 columns, this one has 4", spec=_spec(5))
    refused("group: the selector column is outside the source", spec=_spec(when=col(4)))
    other = ts.Context(0)
    refused("made on this context", ctx_h=other.h)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 1), ctx)
    consumed = ts.DeviceMatrix.upload(ctx, rows)
    _, consumed_data = pcs.commit([((4, 1), consumed)])
    refused("unconsumed", handles=(consumed.h,))
    same(ts.group_rows(ctx, good, d)[0].download(), gc.reference(good, rows)[0], "the matrix still groups")


# ------------------------------------------------------------------ 5. pool poison
def test_pool_poison_changes_nothing():
    """Every slot, class word, block count, offset, record word and output word -- pad rows included -- is written by a
    fill or a kernel of the call before it is read: the same matrices on a clean context and on contexts whose pool
    hands out blocks full of 0x00000001 and 0xFFFFFFFF (stat 9 is above 0 there)."""
    from tapstark_amd.build import build

    build()
    trio = _poison.make_contexts()
    cases = [(gc.random_spec(seed, 5, 1 + seed % 3), gc.random_rows(seed, 1 << 10, 5)) for seed in (3, 7)]
    quiet = np.zeros((1 << 10, 2), dtype=np.uint32)
    cases.append((GroupSpec(2, 3, [col(1)], when=col(0), pad=[9, 8, 7], terms=[COUNT, first(1), total(1)]), quiet))

    def run(c):
        out = []
        for spec, rows in cases:
            for out_height in (0, 1 << 11):
                m, live = ts.group_rows(c, spec, ts.DeviceMatrix.upload(c, rows), out_height)
                out += [m.download(), live]
        return out

    want = []
    for spec, rows in cases:
        for out_height in (0, 1 << 11):
            want += list(gc.reference(spec, rows, out_height))
    _poison.same_everywhere(trio, run, want=want, what="group")
    assert all(c.stat(_poison.STAT_FILLS) > 0 for c in trio[1:])


# ------------------------------------------------------------------ 6. composition
def test_group_of_sorted_is_sorted_group(ctx):
    """group(sort(x)) and group(x) hold the same rows up to their order, on the terms that do not name rows: sorted by
    key, word for word."""
    rows = _data(14)
    rows[:, 0] = np.random.default_rng(15).integers(0, 300, size=N).astype(np.uint32)
    terms = [first(0), COUNT, total(1), least(2), greatest(3)]
    spec = _spec(terms=terms)
    plain, live = group(ctx, spec, rows)
    d_sorted = ts.DeviceMatrix.upload(ctx, rows).sort_rows([0])
    sorted_first, live_sorted = ts.group_rows(ctx, spec, d_sorted)
    assert live == live_sorted
    want = plain[:live][np.argsort(plain[:live, 0], kind="stable")]
    same(sorted_first.download()[:live], want)


def test_join_against_the_result_gives_every_row_its_group_index(ctx):
    rows = gc.random_rows(16, N, 4, n_values=30)
    spec = _spec(keys=[col(0), col(1)], terms=[first(0), first(1), INDEX])
    d_src = ts.DeviceMatrix.upload(ctx, rows)
    d_groups, live = ts.group_rows(ctx, spec, d_src)
    joined, n_missing, _ = d_src.join_rows(d_groups, JoinSpec(keys=[(col(0), col(0)), (col(1), col(1))], fetch=[],
                                                              flags=TABLE_ROW, table_rows=live))
    assert n_missing == 0
    assert joined.download()[:, 4].tolist() == gc.group_index_of_rows(spec, rows)


# ------------------------------------------------------------------ 7. the final state of memory as a table of its own
N_ACC, N_ADDR = 1 << 6, 8
CHALLENGES = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)


def _range_table(ctx, d_table, height):
    from tapstark_amd.airs import fill_memory_range_multiplicities
    from tapstark_amd.derive import DeriveBuilder
    index = DeriveBuilder(2)
    index.output(index.row(), 0)
    d_rng = ts.DeviceMatrix.upload(ctx, np.zeros((height, 2), dtype=np.uint32)).derive(index)  # (zeros: no trace)
    fill_memory_range_multiplicities(d_rng, d_table, allow_missing=True)
    return d_rng


def _statement(ctx, acc):
    """sort -> derive -> derive -> group: the four resident traces, the tables, the number of touched addresses."""
    from tapstark_amd.airs import MemoryAccessAir
    d_acc = ts.DeviceMatrix.upload(ctx, acc)
    d_table, d_final, n_addr = memory_final_tables(ctx, d_acc, N_ACC)
    d_rng = _range_table(ctx, d_table, N_ACC)
    airs = [MemoryAccessAir(), MemoryTableFinalAir(), MemoryFinalAir(), BusRangeAir()]
    heights = [N_ACC, N_ACC, N_ADDR, N_ACC]
    tabs = [bc.Table(a, np.zeros((h, a.width()), dtype=np.uint32)) for a, h in zip(airs, heights)]
    return [d_acc, d_table, d_final, d_rng], tabs, n_addr


def test_memory_final_statement_is_built_in_hbm_proved_and_verified(ctx):
    from tapstark_amd.airs import generate_memory_final, generate_memory_table_final
    acc = generate_memory_accesses(N_ACC, N_ADDR, 77)
    traces, tabs, n_addr = _statement(ctx, acc)
    assert n_addr == N_ADDR == len(set(acc[:, 0].tolist()))
    table = traces[1].download()
    same(table, generate_memory_table_final(acc), "the sorted table with `last`")
    final = traces[2].download()
    same(final, generate_memory_final(table), "the final table against the host's")
    memory = {}
    for addr, clk, value, is_write, sel in acc.tolist():
        memory[addr] = (clk, value)
    assert {r[0]: (r[1], r[2]) for r in final.tolist()} == memory, "final value and last clock of every address, by replay"
    cairs = bc.compiled(ctx, tabs)
    bad, fv, rep = ts.check_multi(None, cairs, traces, [t.pis for t in tabs], [t.logup for t in tabs], CHALLENGES, ctx=ctx)
    assert (bad, fv) == (-1, -1) and rep.balanced
    config = bc.config(ctx, 1)
    proof = ts.prove_multi_bus(config, cairs, ts.BfChallenger(), traces, [t.pis for t in tabs], [t.logup for t in tabs])
    bc.verify(config, tabs, proof)  # raises unless accepted with the bus sum at zero


def test_memory_final_one_final_value_changed_is_named(ctx):
    from tapstark_amd.airs import FIN_TAG
    acc = generate_memory_accesses(N_ACC, N_ADDR, 77)
    traces, tabs, _ = _statement(ctx, acc)
    final = traces[2].download()
    row = 3
    bad_final = final.copy()
    bad_final[row, MemoryFinalAir.VALUE] = (int(final[row, MemoryFinalAir.VALUE]) + 1) % P
    traces[2] = ts.DeviceMatrix.upload(ctx, bad_final)
    cairs = bc.compiled(ctx, tabs)
    bad, fv, rep = ts.check_multi(None, cairs, traces, [t.pis for t in tabs], [t.logup for t in tabs], CHALLENGES, ctx=ctx)
    assert (bad, fv) == (-1, -1), "every constraint holds: the value is tied by the bus alone"
    assert not rep.balanced and rep.n_unbalanced == 2
    # the sorted table sends the true final tuple (table 1 comes first in the report's order), which nobody receives
    addr, clk, value = (int(final[row, c]) for c in (0, 1, 2))
    assert list(rep.tuple[:rep.n_values]) == [FIN_TAG, addr, clk, value] and rep.sum == 1
    assert rep.first[0] == 1 and rep.first[2] == 2


def test_cpp_memory_final_resident_example(ctx, tmp_path):
    """examples/memory_final_resident.cpp: sort, derive and ONE group call make the final table in HBM; proved and
    verified; one changed final value named."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "memory_final_resident")
    source = os.path.join(ROOT, "examples", "memory_final_resident.cpp")
    text = open(source).read()
    # two uploads in the text: the access table -- the only trace -- and a matrix of zeros the range table is derived from
    assert text.count("ts_matrix_upload(") == 2 and text.count("ts_matrix_upload(ctx, trace.data()") == 1
    assert "ts_matrix_upload(ctx, zeros.data()" in text and "ts_matrix_download(" not in text
    assert "ts_matrix_sort_rows(" in text and "ts_matrix_collect_rows(" in text and "Group::last(2)" in text
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source,
                           "-L", libdir, "-ltapstark_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "64 accesses over 8 addresses: 8 groups, final table of 8 rows x 6 grouped in HBM" in r.stdout
    assert "verify -> 0, bus sum zero" in r.stdout
    assert "constraints hold in every table; 2 tuples out of balance" in r.stdout
    assert "unbalanced: table 1, row " in r.stdout and "sent (23, " in r.stdout
    assert r.stdout.rstrip().endswith("memory_final_resident: as expected")
