"""ts_matrix_derive on the GPU against the exact reference of tests/_derive_cases.py, word for word: every op on the
planted operand pairs, heights and widths around the 256-row tile, neighbours across wave and workgroup boundaries,
overwritten and appended columns, the limits of the lowering, pool poison, and the memory table built without leaving
HBM.  The kernel gives every workgroup one tile, so there is no tile knob to vary.  Heights are powers of two: no call
makes a matrix of another height (the host evaluator is tested at other heights in tests/test_derive_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd._lib import TsError
from tapstark_amd.airs import (BusRangeAir, MemoryAccessAir, MemoryTableAir, fill_memory_range_multiplicities,
                               generate_memory_accesses, generate_memory_table, memory_gap_program,
                               memory_table_source_program)
from tapstark_amd.derive import DeriveBuilder, derive_check, derive_rows_host

import _bus_cases as bc
import _derive_cases as dc
import _poison
from _derive_cases import ADD, COL, MUL, NEG, P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ROWS = 1 << 14


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def derive(ctx, program, rows):
    return ts.DeviceMatrix.upload(ctx, rows).derive(program).download()


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]}: "
                           f"{int(got[tuple(bad[0])]):#x} for {int(want[tuple(bad[0])]):#x}")


# ------------------------------------------------------------------ 1. every op
def test_every_op_on_planted_pairs(ctx):
    """Columns 0 and 1 hold every ordered pair of the stored operand words; column 2 + k is op k over them."""
    nodes = [(COL, 0, 0), (COL, 0, 1)]
    for op in dc.ALL_OPS:
        nodes.append(dc.parse(dc.op_program(op))[1][2])
    prog = dc.tape(2, nodes, [(2 + k, 2 + k) for k in range(len(dc.ALL_OPS))])
    pairs = dc.planted_pairs()
    for at in range(0, len(pairs), MAX_ROWS):
        rows = pairs[at:at + MAX_ROWS]
        rows = rows[np.arange(1 << (len(rows) - 1).bit_length()) % len(rows)]  # a matrix's height is a power of two
        got, want = derive(ctx, prog, rows), dc.reference(prog, rows)
        for k, op in enumerate(dc.ALL_OPS):
            same(got[:, 2 + k:3 + k], want[:, 2 + k:3 + k], f"op {op}, rows from {at}")
        same(got, want)


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("width", [1, 3, 17])
@pytest.mark.parametrize("height", [1, 2, 64, 128, 256, 512, 1 << 12])
def test_heights_and_widths(ctx, height, width):
    for seed in (height + width, 1000 + height + width):
        prog = dc.random_program(seed, width)
        rows = dc.random_rows(seed, height, width)
        same(derive(ctx, prog, rows), dc.reference(prog, rows), f"seed {seed}")


@pytest.mark.parametrize("height", [2, 64, 128, 256, 512, 1 << 12])
def test_neighbours_across_wave_and_workgroup_boundaries(ctx, height):
    rows = np.zeros((height, 3), dtype=np.uint32)
    rows[:, 1] = np.arange(height)
    b = DeriveBuilder(3)
    b.output(b.next(1) - b.prev(1), 3)
    got = derive(ctx, b, rows)
    want = np.full(height, 2, dtype=np.int64)
    want[0], want[-1] = 1 - (height - 1), 0 - (height - 2)
    assert got[:, 3].tolist() == [int(v) % P for v in want]
    same(got, dc.reference(b.tape(), rows))


def test_an_output_overwrites_a_column_the_program_reads(ctx):
    rows = dc.random_rows(1, 512, 4)
    b = DeriveBuilder(4)
    x = b.col(1)
    b.output(x + 1, 1)             # overwrites column 1 ...
    b.output(b.col(1) * x, 2)      # ... which later reads still see as it was in the source
    b.output(b.next(1) + b.prev(2), 0)
    got = derive(ctx, b, rows)
    same(got, dc.reference(b.tape(), rows))
    c1 = rows[:, 1].astype(np.uint64) % P
    assert got[:, 2].tolist() == (c1 * c1 % P).tolist()
    assert got.shape == rows.shape and (got[:, 3] == rows[:, 3]).all()


@pytest.mark.parametrize("kind", ["appended", "overwriting", "every column"])
def test_appended_and_overwriting_outputs(ctx, kind):
    rows = dc.random_rows(2, 512, 3)
    nodes = [(COL, 0, 0), (COL, 1, 2), (MUL, 0, 1), (NEG, 2, 0), (ADD, 3, 0)]
    outputs = {"appended": [(2, 3), (4, 4)], "overwriting": [(2, 2), (4, 0)],
               "every column": [(2, 0), (3, 1), (4, 2)]}[kind]
    prog = dc.tape(3, nodes, outputs)
    got = derive(ctx, prog, rows)
    assert got.shape[1] == (5 if kind == "appended" else 3)
    same(got, dc.reference(prog, rows), kind)


def test_untouched_columns_keep_non_canonical_words(ctx):
    edge = np.array([P, P + 1, 1 << 31, 0xFFFFFFFF, 0, P - 1], dtype=np.uint32)
    rows = edge[(np.arange(5 * 1024) * 7 % len(edge))].reshape(1024, 5)
    b = DeriveBuilder(5)
    b.output(b.col(0) + b.col(4), 2)
    b.output(b.col(3), 5)
    got = derive(ctx, b, rows)
    assert (got[:, [0, 1, 3, 4]] == rows[:, [0, 1, 3, 4]]).all(), "copied as stored, not reduced"
    assert (got[:, 5] == rows[:, 3] % P).all() and got[:, [2, 5]].max() < P
    same(got, dc.reference(b.tape(), rows))


# ------------------------------------------------------------------ 3. random programs; device == host == reference
def test_random_programs(ctx):
    for seed in range(40):
        prog = dc.random_program(seed, 5)
        rows = dc.random_rows(seed, 1 << 10, 5)
        d_src = ts.DeviceMatrix.upload(ctx, rows)
        got = d_src.derive(prog).download()
        same(got, dc.reference(prog, rows), f"seed {seed}: device against the reference")
        same(got, derive_rows_host(prog, rows), f"seed {seed}: device against the lowered program on the host")
        same(d_src.download(), rows, "the source after the call")
        same(d_src.derive(prog).download(), got, "a second call")


# ------------------------------------------------------------------ 4. the limits of the lowering
def test_48_live_values(ctx):
    prog = dc.sum_of_loads_program(48, width=7)
    assert derive_check(prog, 7)["n_live"] == 48
    rows = dc.random_rows(48, 512, 7)
    same(derive(ctx, prog, rows), dc.reference(prog, rows))
    with pytest.raises(TsError, match="49 values at once, the limit is 48"):
        ts.DeviceMatrix.upload(ctx, rows).derive(dc.sum_of_loads_program(49, width=7))


def test_4096_node_chain(ctx):
    nodes = [(COL, 0, 0), (COL, 2, 1)]
    while len(nodes) < 4096:
        i = len(nodes)
        nodes.append((MUL, i - 1, 0) if i % 3 == 0 else (ADD, i - 1, 1) if i % 3 == 1 else (dc.XOR, i - 1, i - 2))
    prog = dc.tape(2, nodes, [(4095, 2), (2000, 0)])
    assert derive_check(prog, 2)["n_instructions"] == 4096
    rows = dc.random_rows(4096, 512, 2)
    same(derive(ctx, prog, rows), dc.reference(prog, rows))


def test_256_outputs(ctx):
    nodes = [(COL, 0, 0), (COL, 1, 1), (dc.ROW, 0, 0)]
    for k in range(256):
        nodes.append(((ADD, MUL, dc.SUB, dc.XOR)[k % 4], len(nodes) - 1, k % 3))
    # 128 overwrite every other column of the source, 128 are appended; neither group in column order
    outputs = [(3 + k, 254 - 2 * k if k < 128 else 300 + (k * 37) % 128) for k in range(256)]
    prog = dc.tape(300, nodes, outputs)
    assert derive_check(prog, 300) == {"out_width": 428, "n_instructions": 259, "n_live": 4}
    rows = dc.random_rows(256, 128, 300)
    same(derive(ctx, prog, rows), dc.reference(prog, rows))


# ------------------------------------------------------------------ 5. refusals leave no handle
def test_refusals_leave_no_handle(ctx):
    rows = dc.random_rows(4, 16, 3)
    d = ts.DeviceMatrix.upload(ctx, rows)
    good = dc.random_program(4, 3)
    lib, out = ctx._l, C.c_void_p()

    def refused(text, prog=good, ctx_h=ctx.h, src_h=d.h, out_p=C.byref(out)):
        out.value = 12345
        p = prog.ctypes.data_as(_lib.u32p) if prog is not None else None
        assert lib.ts_matrix_derive(ctx_h, p, len(prog) if prog is not None else 0, src_h, out_p) == 1
        assert text in lib.ts_last_error(ctx_h).decode(), lib.ts_last_error(ctx_h)
        assert not out.value, "a refused call left a handle"

    refused("null argument", prog=None)
    refused("null argument", src_h=None)
    assert lib.ts_matrix_derive(ctx.h, good.ctypes.data_as(_lib.u32p), len(good), d.h, None) == 1
    refused("written for a source of 5 columns, this one has 3", prog=dc.random_program(4, 5))
    refused("unknown op", prog=dc.tape(3, [(2, 0, 0)], [(0, 3)]))
    other = ts.Context(0)
    refused("made on this context", ctx_h=other.h)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 1), ctx)
    consumed = ts.DeviceMatrix.upload(ctx, rows)
    _, consumed_data = pcs.commit([((4, 1), consumed)])
    refused("unconsumed", src_h=consumed.h)
    same(d.derive(good).download(), dc.reference(good, rows), "the matrix still derives")


# ------------------------------------------------------------------ 6. pool poison
def test_pool_poison_changes_nothing():
    """Every out word is written by the kernel and none is read from a pool block it did not write: the same matrix on
    a clean context and on contexts whose pool hands out blocks full of 0x00000001 and 0xFFFFFFFF."""
    from tapstark_amd.build import build

    build()
    trio = _poison.make_contexts()
    cases = [(dc.random_program(s, 5), dc.random_rows(s, 1024, 5)) for s in (3, 7)]
    cases.append((memory_gap_program().tape(), dc.random_rows(8, 256, 8)))

    def run(c):
        return [ts.DeviceMatrix.upload(c, rows).derive(prog).download() for prog, rows in cases]

    _poison.same_everywhere(trio, run, want=[dc.reference(prog, rows) for prog, rows in cases], what="derive")


# ------------------------------------------------------------------ 7. the memory table, resident
N, N_ADDR, N_SELECTED = 1 << 8, 16, 200
CHALLENGES = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)


def test_memory_table_resident(ctx):
    """upload accesses -> derive(source) -> sort_rows -> derive(gap); the range table's index column is ROW over a zero
    matrix, its multiplicities are counted in HBM.  The one download is the assertion's."""
    A = MemoryTableAir
    acc = generate_memory_accesses(N, N_ADDR, 77, n_selected=N_SELECTED)
    d_acc = ts.DeviceMatrix.upload(ctx, acc)
    d_sorted = d_acc.derive(memory_table_source_program()).sort_rows([A.ADDR, A.CLK], group_keys=1, n_live=N_SELECTED,
                                                                    group_start=True)
    d_table = d_sorted.derive(memory_gap_program())
    index = DeriveBuilder(2)
    index.output(index.row(), 0)
    d_rng = ts.DeviceMatrix.upload(ctx, np.zeros((N, 2), dtype=np.uint32)).derive(index)
    n_missing, _ = fill_memory_range_multiplicities(d_rng, d_table, allow_missing=True)
    assert n_missing == 0

    table = d_table.download()
    same(table, generate_memory_table(acc), "the resident table against the host generator")

    airs = [MemoryAccessAir(), MemoryTableAir(), BusRangeAir()]
    tabs = [bc.Table(a, np.zeros((N, a.width()), dtype=np.uint32)) for a in airs]  # tapes, logups, public values
    cairs = bc.compiled(ctx, tabs)
    traces = [d_acc, d_table, d_rng]
    bad, fv, rep = ts.check_multi(None, cairs, traces, [t.pis for t in tabs], [t.logup for t in tabs], CHALLENGES, ctx=ctx)
    assert (bad, fv) == (-1, -1) and rep.balanced
    cfg = bc.config(ctx, 1)
    proof = ts.prove_multi_bus(cfg, cairs, ts.BfChallenger(), traces, [t.pis for t in tabs], [t.logup for t in tabs])
    _, bus_sum = bc.verify(cfg, tabs, proof)
    assert not np.asarray(bus_sum).any()


def test_cpp_memory_table_resident_example(ctx, tmp_path):
    """examples/memory_table_resident.cpp: the statement of memory_table.cpp with no download between the upload of the
    accesses and the verified proof."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "memory_table_resident")
    source = os.path.join(ROOT, "examples", "memory_table_resident.cpp")
    text = open(source).read()
    assert "ts_matrix_download" not in text and text.count("ts_matrix_upload(") == 2  # the accesses; a zero matrix
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source,
                           "-L", libdir, "-ltapstark_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify -> 0, bus sum zero" in r.stdout
    assert r.stdout.rstrip().endswith("memory_table_resident: as expected")
