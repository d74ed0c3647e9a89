"""ts_matrix_collect_rows on the GPU against the exact reference of tests/_collect_cases.py, word for word: source
heights and widths around the lane group, the wave and the workgroup, every density, every value of the
TS_COLLECT_BLOCK_ROWS knob, several sources, sixteen emitters, the height rules, pool poison, and the memory table of a
CPU trace made and proved without the trace leaving HBM.  Source heights are powers of two: no call makes a matrix of
another height (the host loop is tested at other heights in tests/test_collect_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd._lib import TsError
from tapstark_amd.airs import (BusRangeAir, MemoryCpuAir, MemoryTableAir, fill_memory_range_multiplicities,
                               generate_memory_cpu_trace, memory_cpu_collect_spec, memory_cpu_table)
from tapstark_amd.collect import ALWAYS, ROW, CollectSpec, col, collect_rows_host
from tapstark_amd.derive import DeriveBuilder

import _bus_cases as bc
import _collect_cases as cc
import _poison
from _collect_cases import P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "TS_COLLECT_BLOCK_ROWS"
STAT_POOL_BYTES = 3  # ts_ctx_stat: bytes the device pool has reserved, handed out or not
STAT_LIVE_BLOCKS = 11  # ts_ctx_stat: pool blocks handed out and not yet given back


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(autouse=True)
def default_knob(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


def collect(ctx, spec, sources, out_height=0):
    got, live = ts.collect_rows(ctx, spec, [ts.DeviceMatrix.upload(ctx, s) for s in sources], out_height)
    return got.download(), live


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]}: "
                           f"{int(got[tuple(bad[0])]):#x} for {int(want[tuple(bad[0])]):#x}")


def check(ctx, spec, sources, out_height=0, what=""):
    got, live = collect(ctx, spec, sources, out_height)
    want, want_live = cc.reference(spec, sources, out_height)
    assert live == want_live, what
    same(got, want, what)
    return got, live


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("width", [1, 3, 17])
@pytest.mark.parametrize("height", [1, 2, 64, 128, 256, 512, 1024, 2048, 1 << 12, 1 << 14])
def test_heights_and_widths(ctx, height, width):
    rows = cc.random_rows(height + width, height, width)
    for out_width in (1, 5, 64):
        n_emitters = 3 if height * out_width <= 1 << 16 else 1  # (the reference is a Python loop)
        spec = cc.random_spec(height + width + out_width, [width], n_emitters, out_width)
        check(ctx, spec, [rows], what=f"out_width {out_width}")


def test_device_host_and_reference_agree_and_the_sources_stay(ctx):
    for seed in range(4):
        widths = [5, 2, 9][:1 + seed % 3]
        sources = [cc.random_rows(seed + 7 * s, 1 << (11 - 2 * s), w, density=0.25 * (seed + 1)) for s, w in enumerate(widths)]
        spec = cc.random_spec(seed, widths, 6, 7)
        d_src = [ts.DeviceMatrix.upload(ctx, s) for s in sources]
        d_out, live = ts.collect_rows(ctx, spec, d_src)
        got = d_out.download()
        want, want_live = cc.reference(spec, sources)
        same(got, want, f"seed {seed}: device against the reference")
        host, host_live = collect_rows_host(spec, sources)
        same(got, host, f"seed {seed}: device against the library's host loop")
        assert live == want_live == host_live
        for d, s in zip(d_src, sources):
            same(d.download(), s, "a source after the call")
        again, live_again = ts.collect_rows(ctx, spec, d_src)
        same(again.download(), got, "a second call")
        assert live_again == live


# ------------------------------------------------------------------ 2. densities
N = 1 << 12


def _two_slots(width=4):
    """Two emitters on columns 0 and 1, as a machine with two access slots."""
    spec = CollectSpec([width], 4, pad=[P - 1, 0, 7, 1])
    spec.emit(0, when=col(0), terms=[col(2), ROW, 0, col(0)])
    spec.emit(0, when=col(1), terms=[col(3), ROW, 1, col(1)])
    return spec


def _selected(select0, select1):
    rows = cc.random_rows(11, N, 4)
    quiet, loud = np.array([0, P, 2 * P], dtype=np.uint32), np.array([1, P + 1, 0xFFFFFFFF], dtype=np.uint32)
    pick = np.arange(N) % 3
    rows[:, 0] = np.where(select0, loud[pick], quiet[pick])
    rows[:, 1] = np.where(select1, loud[(pick + 1) % 3], quiet[(pick + 1) % 3])
    return rows


DENSITIES = {
    "nothing": (np.zeros(N, bool), np.zeros(N, bool)),
    "everything": (np.ones(N, bool), np.ones(N, bool)),
    "only the last row's last emitter": (np.zeros(N, bool), np.arange(N) == N - 1),
    "only row 0": (np.arange(N) == 0, np.arange(N) == 0),
    "alternating rows": (np.arange(N) % 2 == 0, np.arange(N) % 2 == 1),
    "whole blocks empty between full ones": ((np.arange(N) // 1024) % 2 == 1, (np.arange(N) // 1024) % 2 == 1),
}


@pytest.mark.parametrize("name", list(DENSITIES))
def test_densities(ctx, name):
    rows = _selected(*DENSITIES[name])
    got, live = check(ctx, _two_slots(), [rows], what=name)
    assert live == int(DENSITIES[name][0].sum() + DENSITIES[name][1].sum())
    if name == "nothing":
        assert got.tolist() == [[P - 1, 0, 7, 1]], "height 1, all pad"
    if name == "everything":
        assert got.shape[0] == 2 * N and (got[:, 1] == np.arange(2 * N) // 2).all() and (got[:, 2] == np.arange(2 * N) % 2).all()


# ------------------------------------------------------------------ 3. the knob changes no word
CASE_ROWS = cc.random_rows(42, N, 6)
CASE_SPEC = cc.random_spec(42, [6], 3, 5)


@pytest.mark.parametrize("block_rows", [1, 3, 64, 255, 1000, 1024])
def test_same_words_for_every_block_rows(ctx, monkeypatch, block_rows):
    """4096 rows: with 1 row per workgroup there are 4096 workgroups and 16 trips of the offsets loop, so the carry is
    crossed; 3 and 255 leave a short last workgroup; 1000 leaves lanes without rows."""
    default, live = check(ctx, CASE_SPEC, [CASE_ROWS], what="default")
    monkeypatch.setenv(KNOB, str(block_rows))
    got, live_knob = collect(ctx, CASE_SPEC, [CASE_ROWS])
    same(got, default, f"{KNOB}={block_rows}")
    assert live_knob == live


@pytest.mark.parametrize("value", ["0", "1025", "-1", "x"])
def test_knob_outside_its_range_is_refused(ctx, monkeypatch, value):
    monkeypatch.setenv(KNOB, value)
    with pytest.raises(TsError, match=r"TS_COLLECT_BLOCK_ROWS must be in \[1, 1024\]"):
        collect(ctx, CASE_SPEC, [CASE_ROWS[:16]])


def test_knob_too_small_for_the_heights_is_refused(ctx, monkeypatch):
    """One launch takes fewer than 2^32 threads, so the job grid and the pad workgroups stay below 2^24 workgroups of 256
    lanes: 2^24 rows with one row per block are refused before any device work, with 2 rows per block they are taken."""
    rows = np.zeros((1 << 24, 1), dtype=np.uint32)
    rows[::1 << 12] = 1
    d = ts.DeviceMatrix.upload(ctx, rows)
    spec = CollectSpec([1], 2).emit(0, when=col(0), terms=[ROW, col(0)])
    monkeypatch.setenv(KNOB, "1")
    with pytest.raises(TsError, match="TS_COLLECT_BLOCK_ROWS is too small for sources of these heights"):
        ts.collect_rows(ctx, spec, [d])
    monkeypatch.setenv(KNOB, "2")
    got, live = ts.collect_rows(ctx, spec, [d])
    assert live == 1 << 12
    want = np.stack([np.arange(0, 1 << 24, 1 << 12, dtype=np.uint32), np.ones(1 << 12, dtype=np.uint32)], axis=1)
    same(got.download(), want)


# ------------------------------------------------------------------ 4. sources
@pytest.mark.parametrize("block_rows", [None, 48])
def test_four_sources_with_interleaved_emitters(ctx, monkeypatch, block_rows):
    """Heights 2^12, 2^6, 1 and 2^10 and four widths; the emitters of the four sources alternate in the spec, so the
    order rule -- source first, then row, then the emitter's place in the spec -- is not the order they are written in.
    A block never straddles two sources: with 48 rows per block every source but the third ends in a short block."""
    if block_rows:
        monkeypatch.setenv(KNOB, str(block_rows))
    heights, widths = [1 << 12, 1 << 6, 1, 1 << 10], [3, 7, 1, 4]
    sources = [cc.random_rows(20 + s, heights[s], widths[s], density=[0.3, 0.9, 1.0, 0.5][s]) for s in range(4)]
    spec = CollectSpec(widths, 4, pad=[1, 2, 3, 4])
    for e in range(12):
        s = (3 * e + 1) % 4  # 1, 0, 3, 2, 1, ...
        spec.emit(s, when=ALWAYS if e % 5 == 0 else col(0), terms=[e, ROW, col(widths[s] - 1), s])
    got, live = check(ctx, spec, sources)
    order = got[:live, [3, 1, 0]].astype(np.int64)  # (source, row, emitter): strictly ascending
    key = (order[:, 0] << 40) + (order[:, 1] << 8) + order[:, 2]
    assert (np.diff(key) > 0).all() and set(order[:, 0].tolist()) == {0, 1, 2, 3}


def test_one_handle_as_two_sources(ctx):
    rows = cc.random_rows(5, 1 << 9, 4)
    spec = CollectSpec([4, 4], 3).emit(1, when=col(0), terms=[col(1), ROW, 1]).emit(0, when=col(0), terms=[col(2), ROW, 0])
    d = ts.DeviceMatrix.upload(ctx, rows)
    d_out, live = ts.collect_rows(ctx, spec, [d, d])
    want, want_live = cc.reference(spec, [rows, rows])
    same(d_out.download(), want)
    assert live == want_live
    same(d.download(), rows, "the source after the call")


# ------------------------------------------------------------------ 5. sixteen emitters
@pytest.mark.parametrize("block_rows", [None, 255, 256])
def test_sixteen_emitters_all_firing(ctx, monkeypatch, block_rows):
    """16 emitters on one source, all firing: a block is capped at 4096 / 16 = 256 rows and the list of a full block
    holds exactly 4096 entries; 255 rows per block leave its last entries unused and the last block short."""
    if block_rows:
        monkeypatch.setenv(KNOB, str(block_rows))
    rows = cc.random_rows(16, 1 << 10, 3)
    rows[:, 0] = np.array([1, P + 1, 0xFFFFFFFF, 5], dtype=np.uint32)[np.arange(1 << 10) % 4]
    spec = CollectSpec([3], 3)
    for e in range(16):
        spec.emit(0, when=col(0) if e % 2 else ALWAYS, terms=[ROW, e, col(1 + e % 2)])
    got, live = check(ctx, spec, [rows])
    assert live == 16 << 10 and got.shape[0] == 16 << 10
    assert (got[:, 0] == np.arange(16 << 10) // 16).all() and (got[:, 1] == np.arange(16 << 10) % 16).all()


# ------------------------------------------------------------------ 6. heights
def test_out_heights_and_the_refusal_returns_every_block(ctx):
    rows = _selected(np.arange(N) % 4 == 0, np.arange(N) % 4 == 2)  # 2048 fire
    spec = _two_slots()
    got, live = check(ctx, spec, [rows], out_height=2048, what="out_height = n_live: no pad row")
    assert live == 2048 and got.shape[0] == 2048
    got, _ = check(ctx, spec, [rows], out_height=4096, what="out_height = 2 n_live")
    assert (got[2048:] == [P - 1, 0, 7, 1]).all()
    odd = rows.copy()
    odd[5, 0] = 1  # 2049 fire
    check(ctx, spec, [odd], out_height=0, what="one more: 4096 rows, 2047 of them pad")
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
        assert st == 1 and own._l.ts_last_error(own.h).decode() == "collect: 2049 rows selected, out_height 2048"
        assert not out.value and n_live.value == 0, "a refused call left a handle"
        assert own.stat(STAT_LIVE_BLOCKS) == live_before, "a refused call kept pool blocks"
        reserved.append(own.stat(STAT_POOL_BYTES))
    # and every further refused call finds all its blocks in the pool: a kept one would have to be reserved anew
    assert reserved[1:] == reserved[:-1], "a refused call kept pool blocks"
    for bad in (3, 1 << 28):
        with pytest.raises(TsError, match="neither 0 nor a power of two"):
            ts.collect_rows(own, spec, [d], bad)
        assert own.stat(STAT_LIVE_BLOCKS) == live_before
    d_out, _ = ts.collect_rows(own, spec, [d])
    assert own.stat(STAT_LIVE_BLOCKS) == live_before + 1, "an accepted call keeps its result and nothing else"
    same(d_out.download(), cc.reference(spec, [odd])[0], "the matrix still collects")


def test_refusals_leave_no_handle(ctx):
    rows = cc.random_rows(4, 16, 4)
    d = ts.DeviceMatrix.upload(ctx, rows)
    good = _two_slots()
    lib, out, live = ctx._l, C.c_void_p(), C.c_uint64()

    def refused(text, spec=good, ctx_h=ctx.h, handles=(d.h,), out_p=C.byref(out), live_p=C.byref(live), sources=True):
        out.value = 12345
        t = spec.tape() if spec is not None else None
        hs = (C.c_void_p * 4)(*handles)
        st = lib.ts_matrix_collect_rows(ctx_h, t.ctypes.data_as(ts._lib.u32p) if t is not None else None,
                                        len(t) if t is not None else 0, hs if sources else None, 0, out_p, live_p)
        assert st == 1 and text in lib.ts_last_error(ctx_h).decode(), lib.ts_last_error(ctx_h)
        assert not out.value, "a refused call left a handle"

    refused("null argument", spec=None)
    refused("null argument", sources=False)
    refused("null argument", handles=(None,))
    refused("null argument", live_p=None)
    assert lib.ts_matrix_collect_rows(ctx.h, good.tape().ctypes.data_as(ts._lib.u32p), len(good.tape()),
                                      (C.c_void_p * 4)(d.h), 0, None, C.byref(live)) == 1
    refused("written for a source 0 of 5 columns, this one has 4", spec=_two_slots(5))
    refused("the selector column is outside the source", spec=CollectSpec([4], 1).emit(0, when=col(4), terms=[1]))
    other = ts.Context(0)
    refused("made on this context", ctx_h=other.h)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 1), ctx)
    consumed = ts.DeviceMatrix.upload(ctx, rows)
    _, consumed_data = pcs.commit([((4, 1), consumed)])
    refused("unconsumed", handles=(consumed.h,))
    same(ts.collect_rows(ctx, good, [d])[0].download(), cc.reference(good, [rows])[0], "the matrix still collects")


# ------------------------------------------------------------------ 7. pool poison
def test_pool_poison_changes_nothing():
    """Every out word -- pad rows included -- every block count and every block offset is written by the kernels before
    it is read: the same matrices on a clean context and on contexts whose pool hands out blocks full of 0x00000001 and
    0xFFFFFFFF (which fill blocks meanwhile: stat 9 is above 0 there)."""
    from tapstark_amd.build import build

    build()
    trio = _poison.make_contexts()
    cases = []
    for seed in (3, 7):
        widths = [5, 3]
        sources = [cc.random_rows(seed + s, 1 << (11 - 3 * s), widths[s], density=0.3) for s in range(2)]
        cases.append((cc.random_spec(seed, widths, 5, 6), sources))
    quiet = np.zeros((1 << 10, 2), dtype=np.uint32)
    cases.append((CollectSpec([2], 3, pad=[9, 8, 7]).emit(0, when=col(0), terms=[1, 2, 3]), [quiet]))

    def run(c):
        out = []
        for spec, sources in cases:
            for out_height in (0, 1 << 14):
                m, live = ts.collect_rows(c, spec, [ts.DeviceMatrix.upload(c, s) for s in sources], out_height)
                out += [m.download(), live]
        return out

    want = []
    for spec, sources in cases:
        for out_height in (0, 1 << 14):
            want += list(cc.reference(spec, sources, out_height))
    _poison.same_everywhere(trio, run, want=want, what="collect")
    assert all(c.stat(_poison.STAT_FILLS) > 0 for c in trio[1:])


# ------------------------------------------------------------------ 8. the memory table of a CPU trace
N_CPU, N_ADDR = 1 << 6, 8
CHALLENGES = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)


def _range_table(ctx, d_table, height):
    index = DeriveBuilder(2)
    index.output(index.row(), 0)
    d_rng = ts.DeviceMatrix.upload(ctx, np.zeros((height, 2), dtype=np.uint32)).derive(index)  # (zeros: no trace)
    fill_memory_range_multiplicities(d_rng, d_table, allow_missing=True)
    return d_rng


def _statement(ctx, cpu):
    """collect -> derive -> sort -> derive -> scan -> derive -> multiplicities: the three resident traces, the compiled
    AIRs and their side data, the collected access matrix as downloaded, n_live."""
    d_cpu = ts.DeviceMatrix.upload(ctx, cpu)
    d_acc, d_table, n_live = memory_cpu_table(ctx, d_cpu)
    acc = d_acc.download()
    d_rng = _range_table(ctx, d_table, 2 * N_CPU)  # timestamps and so clock gaps stay below 2 n
    airs = [MemoryCpuAir(), MemoryTableAir(), BusRangeAir()]
    heights = [N_CPU, acc.shape[0], 2 * N_CPU]
    tabs = [bc.Table(a, np.zeros((h, a.width()), dtype=np.uint32)) for a, h in zip(airs, heights)]
    return [d_cpu, d_table, d_rng], tabs, acc, n_live


def test_memory_cpu_statement_is_proved_without_the_table_leaving_hbm(ctx):
    cpu = generate_memory_cpu_trace(N_CPU, N_ADDR)
    A = MemoryCpuAir
    assert 0 < cpu[:, A.SEL_A].sum() < N_CPU and 0 < cpu[:, A.SEL_B].sum() < N_CPU, "both slots are conditional"
    traces, tabs, acc, n_live = _statement(ctx, cpu)
    host, host_live = collect_rows_host(memory_cpu_collect_spec(), [cpu])
    same(acc, host, "the collected matrix against the host's")
    assert n_live == host_live == int(cpu[:, A.SEL_A].sum() + cpu[:, A.SEL_B].sum())
    table = traces[1].download()
    T = MemoryTableAir
    assert table[:n_live, T.LIVE].all() and not table[n_live:, T.LIVE].any()
    cairs = bc.compiled(ctx, tabs)
    bad, fv, rep = ts.check_multi(None, cairs, traces, [t.pis for t in tabs], [t.logup for t in tabs], CHALLENGES, ctx=ctx)
    assert (bad, fv) == (-1, -1) and rep.balanced
    config = bc.config(ctx, 1)
    proof = ts.prove_multi_bus(config, cairs, ts.BfChallenger(), traces, [t.pis for t in tabs], [t.logup for t in tabs])
    bc.verify(config, tabs, proof)  # raises unless accepted with the bus sum at zero


def test_memory_cpu_one_read_value_changed_is_named(ctx):
    A = MemoryCpuAir
    cpu = generate_memory_cpu_trace(N_CPU, N_ADDR)
    row = int(np.flatnonzero(cpu[:, A.SEL_A])[3])
    cpu[row, A.VAL_A] = (int(cpu[row, A.VAL_A]) + 1) % P
    traces, tabs, _, _ = _statement(ctx, cpu)
    cairs = bc.compiled(ctx, tabs)
    bad, fv, rep = ts.check_multi(None, cairs, traces, [t.pis for t in tabs], [t.logup for t in tabs], CHALLENGES, ctx=ctx)
    assert (bad, fv) == (-1, -1), "every constraint holds: the memory table is filled from the writes"
    assert not rep.balanced and rep.n_unbalanced == 2
    # the CPU sends the changed read, which nobody receives
    assert list(rep.tuple[:rep.n_values]) == [11, int(cpu[row, A.ADDR_A]), 2 * row, int(cpu[row, A.VAL_A]), 0]
    assert tuple(rep.first) == (0, row, 0) and rep.sum == 1


def test_cpp_memory_cpu_resident_example(ctx, tmp_path):
    """examples/memory_cpu_resident.cpp: the access table collected from a CPU trace, the memory table made from it,
    proved and verified; one changed read value named."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "memory_cpu_resident")
    source = os.path.join(ROOT, "examples", "memory_cpu_resident.cpp")
    text = open(source).read()
    # two uploads in the text: the CPU trace -- the only trace -- and a matrix of zeros the range table is derived from
    assert "ts_matrix_collect_rows(" in text and text.count("ts_matrix_upload(") == 2
    assert "ts_matrix_upload(ctx, trace.data()" in text and "ts_matrix_upload(ctx, zeros.data()" in text
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source,
                           "-L", libdir, "-ltapstark_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "32 CPU rows, " in r.stdout and "rows x 5 collected in HBM" in r.stdout
    assert "verify -> 0, bus sum zero" in r.stdout
    assert "constraints hold in every table; 2 tuples out of balance" in r.stdout and "sent (11, " in r.stdout
    assert r.stdout.rstrip().endswith("memory_cpu_resident: as expected")
