"""ts_matrix_scan on the GPU against the exact reference of tests/_scan_cases.py, word for word: heights and widths
around the lane group, the wave and the workgroup, every value of the TS_SCAN_BLOCK_ROWS knob, resets at every boundary,
the edge words, maps composed across workgroups, finals, pool poison, and the read values of a memory table filled
without leaving HBM.  Heights are powers of two: no call makes a matrix of another height (the host loop is tested at
other heights in tests/test_scan_cpu.py)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd._lib import TsError
from tapstark_amd.airs import (BusRangeAir, MemoryAccessAir, MemoryTableAir, fill_memory_range_multiplicities,
                               generate_memory_accesses, generate_memory_table, memory_fill_helper_program,
                               memory_fill_scan, memory_gap_program, memory_table_unfilled_source_program)
from tapstark_amd.derive import DeriveBuilder
from tapstark_amd.scan import ScanSpec, col, running_product, running_sum, scan_rows_host

import _bus_cases as bc
import _poison
import _scan_cases as sc
from _scan_cases import EDGE, P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "TS_SCAN_BLOCK_ROWS"
THREADS = 256  # lanes of a workgroup: a lane owns ceil(block_rows / 256) consecutive rows


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(autouse=True)
def default_knob(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


def scan(ctx, spec, rows, finals=False):
    got = ts.DeviceMatrix.upload(ctx, rows).scan(spec, finals=finals)
    return (got[0].download(), got[1]) if finals else got.download()


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]}: "
                           f"{int(got[tuple(bad[0])]):#x} for {int(want[tuple(bad[0])]):#x}")


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("width", [1, 3, 17])
@pytest.mark.parametrize("height", [1, 2, 64, 128, 256, 512, 1024, 2048, 1 << 12, 1 << 14])
def test_heights_and_widths(ctx, height, width):
    for seed in (height + width, 1000 + height + width):
        spec = sc.random_spec(seed, width)
        rows = sc.random_rows(seed, height, width)
        got, last = scan(ctx, spec, rows, finals=True)
        want, want_last = sc.reference(spec, rows, finals=True)
        same(got, want, f"seed {seed}")
        assert last.tolist() == want_last.tolist(), f"seed {seed}"


def test_eight_scans_device_host_and_reference_agree(ctx):
    for seed in range(6):
        spec = sc.random_spec(seed, 5, n_scans=8)
        rows = sc.random_rows(seed, 1 << 11, 5)
        d_src = ts.DeviceMatrix.upload(ctx, rows)
        got = d_src.scan(spec).download()
        same(got, sc.reference(spec, rows), f"seed {seed}: device against the reference")
        same(got, scan_rows_host(spec, rows), f"seed {seed}: device against the library's host loop")
        same(d_src.download(), rows, "the source after the call")
        same(d_src.scan(spec).download(), got, "a second call")


# ------------------------------------------------------------------ 2. the knob changes no word
CASE_ROWS = sc.random_rows(42, 1 << 12, 6)


def _case_spec():
    """Five random scans, a segmented running product and an exclusive general recurrence appended behind them."""
    spec = sc.random_spec(42, 6, n_scans=5)
    nxt = max(6, max(c["dst"] for c in spec.columns) + 1)
    spec.extend(running_product(0, dst=nxt, reset=1))
    spec.add(nxt + 1, a=col(2), b=col(3), init=P - 1, exclusive=True)
    spec.out_width = 0
    return spec


@pytest.mark.parametrize("block_rows", [1, 3, 64, 255, 1000, 1024])
def test_same_words_for_every_block_rows(ctx, monkeypatch, block_rows):
    """4096 rows: with 1 row per workgroup there are 4096 workgroups and 16 trips of the totals loop, so the carried map
    is crossed; 3 and 255 leave a short last workgroup; 1000 leaves lanes of the last wave without rows."""
    spec, rows = _case_spec(), CASE_ROWS
    default, default_last = scan(ctx, spec, rows, finals=True)
    want, want_last = sc.reference(spec, rows, finals=True)
    same(default, want, "default")
    monkeypatch.setenv(KNOB, str(block_rows))
    got, last = scan(ctx, spec, rows, finals=True)
    same(got, default, f"{KNOB}={block_rows}")
    assert last.tolist() == default_last.tolist() == want_last.tolist()


@pytest.mark.parametrize("value", ["0", "1025", "-1", "x"])
def test_knob_outside_its_range_is_refused(ctx, monkeypatch, value):
    monkeypatch.setenv(KNOB, value)
    with pytest.raises(TsError, match=r"TS_SCAN_BLOCK_ROWS must be in \[1, 1024\]"):
        ts.DeviceMatrix.upload(ctx, CASE_ROWS[:16]).scan(running_sum(0))


# ------------------------------------------------------------------ 3. boundaries
@pytest.mark.parametrize("block_rows", [1024, 600])
def test_resets_at_every_boundary(ctx, monkeypatch, block_rows):
    """Reset rows exactly at, one before and one after every lane-group, wave and workgroup boundary; the inclusive and
    the exclusive form on the same placements, a running sum and a general recurrence."""
    monkeypatch.setenv(KNOB, str(block_rows))
    rpt = -(-block_rows // THREADS)
    height = 1 << 12
    rows = sc.random_rows(block_rows, height, 4)
    for step, off in itertools.product((rpt, 64 * rpt, block_rows), (-1, 0, 1)):
        rows[:, 3] = (np.arange(height) - off) % step == 0
        spec = ScanSpec()
        for k, exclusive in enumerate((False, True)):
            spec.add(4 + 2 * k, a=1, b=col(0), init=7, reset=3, exclusive=exclusive)
            spec.add(5 + 2 * k, a=col(1), b=col(2), init=P - 1, reset=3, exclusive=exclusive)
        same(scan(ctx, spec, rows), sc.reference(spec, rows), f"every {step} rows, offset {off}")


def test_reset_on_every_row_no_row_and_row_0_only(ctx):
    rows = sc.random_rows(3, 1 << 11, 3)
    for where, flags in (("every row", 1), ("no row", 0), ("row 0 only", np.arange(1 << 11) == 0)):
        rows[:, 2] = flags
        spec = running_sum(0, reset=2, dst=3, init=5).extend(running_sum(1, reset=2, dst=4, init=5, exclusive=True))
        same(scan(ctx, spec, rows), sc.reference(spec, rows), where)


# ------------------------------------------------------------------ 4. the edge words
def test_edge_words_in_a_b_and_reset(ctx):
    """Every triple of edge words as (a, b, reset) of one row, each followed by a plain row: p reads as 0 (no reset, a
    zero factor), p + 1 as 1, 0xFFFFFFFF as 268435453; the untouched column keeps 0xFFFFFFFF."""
    triples = list(itertools.product(EDGE, repeat=3))
    rows = np.zeros((1024, 4), dtype=np.uint32)
    rows[0:2 * len(triples):2, :3] = triples
    rows[1::2, :3] = [3, 5, 0]
    rows[:, 3] = 0xFFFFFFFF
    for init in (0, 1, P - 1):
        spec = ScanSpec().add(4, a=col(0), b=col(1), init=init, reset=2).add(2, a=col(0), b=col(1), init=init, reset=2,
                                                                             exclusive=True)
        got = scan(ctx, spec, rows)
        same(got, sc.reference(spec, rows), f"init {init}")
        assert got[:, [2, 4]].max() < P and (got[:, 3] == 0xFFFFFFFF).all() and (got[:, :2] == rows[:, :2]).all()


def test_truncated_result_drops_the_helper_columns(ctx):
    rows = sc.random_rows(9, 512, 7)
    spec = ScanSpec(out_width=5).add(2, a=col(5), b=col(6), reset=4)
    got = scan(ctx, spec, rows)
    assert got.shape == (512, 5)
    same(got, sc.reference(spec, rows))


# ------------------------------------------------------------------ 5. associativity across workgroups
def test_a_zero_in_another_workgroup(ctx):
    rows = np.full((1 << 12, 2), 3, dtype=np.uint32)
    rows[1500, 0] = P  # stored as p, a zero all the same: in the second workgroup, the rows after it in the next two
    got, last = scan(ctx, running_product(0, dst=1), rows, finals=True)
    assert got[1499, 1] == pow(3, 1500, P) and not got[1500:, 1].any() and last.tolist() == [0]
    same(got, sc.reference(running_product(0, dst=1), rows))


def test_all_ones_sum(ctx):
    rows = np.ones((1 << 14, 1), dtype=np.uint32)
    got, last = scan(ctx, running_sum(0, dst=1).extend(running_sum(0, dst=2, exclusive=True)), rows, finals=True)
    assert (got[:, 1] == np.arange(1, (1 << 14) + 1)).all() and (got[:, 2] == np.arange(1 << 14)).all()
    assert last.tolist() == [1 << 14, 1 << 14]


# ------------------------------------------------------------------ 6. finals
def test_finals_against_the_last_row(ctx):
    rows = sc.random_rows(12, 1 << 11, 4)
    spec = ScanSpec().add(4, a=col(0), b=col(1), init=2, reset=3).add(5, a=1, b=col(2)).add(0, a=col(1), b=1, init=1)
    d_src = ts.DeviceMatrix.upload(ctx, rows)
    with_finals, last = d_src.scan(spec, finals=True)
    got = with_finals.download()
    assert last.tolist() == got[-1, [4, 5, 0]].tolist() == sc.reference(spec, rows, finals=True)[1].tolist()
    same(d_src.scan(spec).download(), got, "finals=None gives the same matrix")


# ------------------------------------------------------------------ 7. refusals leave no handle
def test_refusals_leave_no_handle(ctx):
    rows = sc.random_rows(4, 16, 3)
    d = ts.DeviceMatrix.upload(ctx, rows)
    good = ScanSpec().add(3, a=col(0), b=col(1), reset=2)
    lib, out = ctx._l, C.c_void_p()

    def refused(text, spec=good, ctx_h=ctx.h, src_h=d.h, out_p=C.byref(out)):
        out.value = 12345
        assert lib.ts_matrix_scan(ctx_h, C.byref(spec.c_spec()) if spec is not None else None, src_h, out_p, None) == 1
        assert text in lib.ts_last_error(ctx_h).decode(), lib.ts_last_error(ctx_h)
        assert not out.value, "a refused call left a handle"

    refused("null argument", spec=None)
    refused("null argument", src_h=None)
    assert lib.ts_matrix_scan(ctx.h, C.byref(good.c_spec()), d.h, None, None) == 1
    refused("column of a is outside the source", spec=ScanSpec().add(3, a=col(3)))
    refused("column 3 is beyond the source", spec=ScanSpec().add(4))
    bad = good.c_spec()
    bad.struct_size += 8
    out.value = 12345
    assert lib.ts_matrix_scan(ctx.h, C.byref(bad), d.h, C.byref(out), None) == 1 and not out.value
    assert "struct_size" in lib.ts_last_error(ctx.h).decode()
    other = ts.Context(0)
    refused("made on this context", ctx_h=other.h)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 1), ctx)
    consumed = ts.DeviceMatrix.upload(ctx, rows)
    _, consumed_data = pcs.commit([((4, 1), consumed)])
    refused("unconsumed", src_h=consumed.h)
    same(d.scan(good).download(), sc.reference(good, rows), "the matrix still scans")


# ------------------------------------------------------------------ 8. pool poison
def test_pool_poison_changes_nothing():
    """Every out word, every block map and every block state is written by the kernels before it is read: the same
    matrices and last values on a clean context and on contexts whose pool hands out blocks full of 0x00000001 and
    0xFFFFFFFF (which fill blocks meanwhile: stat 9 is above 0 there)."""
    from tapstark_amd.build import build

    build()
    trio = _poison.make_contexts()
    cases = [(sc.random_spec(s, 5), sc.random_rows(s, 1 << 11, 5)) for s in (3, 7)]
    program, fill = memory_fill_helper_program(), memory_fill_scan()
    table = sc.random_rows(8, 256, 8)

    def run(c):
        out = []
        for spec, rows in cases:
            m, last = ts.DeviceMatrix.upload(c, rows).scan(spec, finals=True)
            out += [m.download(), last]
        return out + [ts.DeviceMatrix.upload(c, table).derive(program).scan(fill).download()]

    want = []
    for spec, rows in cases:
        want += list(sc.reference(spec, rows, finals=True))
    from tapstark_amd.derive import derive_rows_host
    want.append(sc.reference(fill, derive_rows_host(program, table)))
    _poison.same_everywhere(trio, run, want=want, what="scan")
    assert all(c.stat(_poison.STAT_FILLS) > 0 for c in trio[1:])


# ------------------------------------------------------------------ 9. the memory fill
N, N_ADDR, N_SELECTED = 1 << 10, 16, 700
CHALLENGES = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)


def resident_filled_table(ctx, acc, n_live, spoil=None):
    """upload accesses -> derive(source, 0 in value on every read) -> sort_rows -> derive(a, b) -> scan -> derive(gap);
    `spoil(matrix)` may change the sorted table before the scan."""
    A = MemoryTableAir
    d_acc = ts.DeviceMatrix.upload(ctx, acc)
    d_sorted = d_acc.derive(memory_table_unfilled_source_program()).sort_rows([A.ADDR, A.CLK], group_keys=1, n_live=n_live,
                                                                             group_start=True)
    if spoil is not None:
        d_sorted = spoil(d_sorted)
    d_table = d_sorted.derive(memory_fill_helper_program()).scan(memory_fill_scan()).derive(memory_gap_program())
    return d_acc, d_table


def checked(ctx, d_acc, d_table):
    index = DeriveBuilder(2)
    index.output(index.row(), 0)
    d_rng = ts.DeviceMatrix.upload(ctx, np.zeros((N, 2), dtype=np.uint32)).derive(index)
    fill_memory_range_multiplicities(d_rng, d_table, allow_missing=True)
    airs = [MemoryAccessAir(), MemoryTableAir(), BusRangeAir()]
    tabs = [bc.Table(a, np.zeros((N, a.width()), dtype=np.uint32)) for a in airs]  # tapes, logups, public values
    cairs = bc.compiled(ctx, tabs)
    return ts.check_multi(None, cairs, [d_acc, d_table, d_rng], [t.pis for t in tabs], [t.logup for t in tabs], CHALLENGES,
                          ctx=ctx)


def test_memory_fill_equals_the_host_generator(ctx):
    acc = generate_memory_accesses(N, N_ADDR)
    assert (acc[:, MemoryAccessAir.IS_WRITE] == 0).sum() > N // 4 and acc[acc[:, 3] == 0, 2].any()
    _, d_table = resident_filled_table(ctx, acc, N)
    same(d_table.download(), generate_memory_table(acc), "the filled resident table against the host generator")


def test_memory_fill_with_dead_rows_balances_the_bus(ctx):
    acc = generate_memory_accesses(N, N_ADDR, 77, n_selected=N_SELECTED)
    d_acc, d_table = resident_filled_table(ctx, acc, N_SELECTED)
    bad, fv, rep = checked(ctx, d_acc, d_table)
    assert (bad, fv) == (-1, -1) and rep.balanced
    live = generate_memory_table(acc)[:N_SELECTED]
    same(d_table.download()[:N_SELECTED], live, "the live rows against the host generator")


def test_memory_fill_one_written_value_changed_is_named(ctx):
    A = MemoryTableAir
    acc = generate_memory_accesses(N, N_ADDR, 77, n_selected=N_SELECTED)
    want = generate_memory_table(acc)
    row = next(r for r in range(N_SELECTED - 1) if want[r, A.IS_WRITE] and not want[r + 1, A.IS_WRITE]
               and not want[r + 1, A.START])  # a write that a read follows

    def spoil(d_sorted):
        bump = DeriveBuilder(8)
        bump.output(bump.col(A.VALUE) + (bump.row() - row).is_zero(), A.VALUE)
        return d_sorted.derive(bump)

    d_acc, d_table = resident_filled_table(ctx, acc, N_SELECTED, spoil)
    got = d_table.download()
    assert got[row, A.VALUE] == (want[row, A.VALUE] + 1) % P and got[row + 1, A.VALUE] == got[row, A.VALUE], \
        "the read after the changed write carries the changed value"
    bad, fv, rep = checked(ctx, d_acc, d_table)
    assert not rep.balanced and rep.n_unbalanced >= 2
    assert list(rep.tuple[:rep.n_values])[0] == 11, "a memory tuple (MEM_TAG first) is named"


def test_cpp_memory_fill_resident_example(ctx, tmp_path):
    """examples/memory_fill_resident.cpp: the read values of the memory table found by ts_matrix_scan, proved and
    verified against the access table."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "memory_fill_resident")
    source = os.path.join(ROOT, "examples", "memory_fill_resident.cpp")
    text = open(source).read()
    assert "ts_matrix_scan(" in text and text.count("ts_matrix_upload(") == 2  # the accesses; a zero matrix
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source,
                           "-L", libdir, "-ltapstark_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify -> 0, bus sum zero" in r.stdout and " reads " in r.stdout
    assert r.stdout.rstrip().endswith("memory_fill_resident: as expected")
