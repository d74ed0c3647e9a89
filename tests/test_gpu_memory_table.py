"""A memory table on the bus, end to end on the GPU: 2^8 accesses over 16 addresses (MemoryAccessAir), the same accesses
sorted by (addr, clk) in HBM with ``DeviceMatrix.sort_rows`` (MemoryTableAir) and a 2^8 range table (BusRangeAir) that
takes every ``gap``.  FRI (1, 3, 2), the small setting of the other multi-table tests."""
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd.airs import (MEM_TAG, BusRangeAir, MemoryAccessAir, MemoryTableAir, fill_memory_gaps,
                               fill_memory_range_multiplicities, generate_memory_accesses, generate_memory_table,
                               memory_table_source)

import _bus_cases as bc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_ADDR, N_SELECTED = 1 << 8, 16, 200
CHALLENGES = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)
A = MemoryTableAir
P = bc.P


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(scope="module")
def statement(ctx):
    """(accesses, sorted table with gap, range trace with its multiplicities), every step that has a device form on the
    device; the table is also checked against the host generator."""
    acc = generate_memory_accesses(N, N_ADDR, 77, n_selected=N_SELECTED)
    src, n_live = memory_table_source(acc)
    d_sorted = ts.DeviceMatrix.upload(ctx, src).sort_rows([A.ADDR, A.CLK], group_keys=1, n_live=n_live,
                                                          group_start=True)
    table = fill_memory_gaps(d_sorted.download())
    assert n_live == N_SELECTED and (table == generate_memory_table(acc)).all()
    return acc, table, range_trace(ctx, table)[0]


def range_trace(ctx, table):
    """The BusRangeAir trace for ``table``, its multiplicities filled in HBM: (trace, n_missing, first miss)."""
    rng = np.zeros((N, 2), dtype=np.uint32)
    rng[:, 0] = np.arange(N)
    d_rng = ts.DeviceMatrix.upload(ctx, rng)
    n_missing, first = fill_memory_range_multiplicities(d_rng, ts.DeviceMatrix.upload(ctx, table), allow_missing=True)
    return d_rng.download(), n_missing, first


def tables_of(acc, table, rng):
    return [bc.Table(MemoryAccessAir(), acc), bc.Table(MemoryTableAir(), table), bc.Table(BusRangeAir(), rng)]


def check_multi(ctx, tables):
    return ts.check_multi(None, bc.compiled(ctx, tables), [t.trace.copy() for t in tables], [t.pis for t in tables],
                          [t.logup for t in tables], CHALLENGES, ctx=ctx)


def test_the_sorted_table_checks_proves_and_verifies(ctx, statement):
    tables = tables_of(*statement)
    bad, fv, rep = check_multi(ctx, tables)
    assert (bad, fv) == (-1, -1) and rep.balanced
    # every selected access sent and received, every live gap sent, and one range row per distinct gap
    table = statement[1]
    assert rep.n_contributions == 3 * N_SELECTED + len(np.unique(table[:N_SELECTED, A.GAP]))
    cfg = bc.config(ctx, 1)
    proof = bc.prove(cfg, bc.compiled(ctx, tables), tables)
    _, bus_sum = bc.verify(cfg, tables, proof)
    assert not np.asarray(bus_sum).any()


def test_a_changed_read_value_is_named(ctx, statement):
    acc, table, rng = statement
    reads = np.flatnonzero((table[:, A.IS_WRITE] == 0) & (table[:, A.LIVE] == 1))
    row = int(reads[len(reads) // 2])
    bad_table = table.copy()
    bad_table[row, A.VALUE] ^= 1
    bad, fv, rep = check_multi(ctx, tables_of(acc, bad_table, rng))
    # the read no longer returns the last value: the constraint of the row before it, whose `next` it is
    assert bad == 1 and fv >> 16 == row - 1
    # and the bus: the access table still sends the true read (table 0 comes first in the report's order), nobody
    # receives it; the changed tuple is received and was never sent
    addr, clk, value = (int(table[row, c]) for c in (A.ADDR, A.CLK, A.VALUE))
    assert not rep.balanced and rep.n_unbalanced == 2
    assert rep.first == (0, clk, 0) and rep.n_values == 5
    assert rep.tuple == [MEM_TAG, addr, clk, value, 0, 0, 0, 0] and rep.sum == 1
    assert [s.count for s in rep.shares] == [1, 0, 0] and rep.shares[0].first == (clk, 0)
    assert acc[clk].tolist() == [addr, clk, value, 0, 1]


def test_two_swapped_neighbours_miss_the_range_table(ctx, statement):
    """Rows i and i + 1 inside one address group swapped, ``gap`` recomputed: on row i + 1 the clock now goes BACK, its
    gap is clk_small - clk_big - 1 = p minus a little, and no range table of 2^8 rows holds that: the range lookup
    misses, once, on that row (rows i and i + 2 step forward and keep small gaps).  The miss is what we assert, not a
    violated constraint: ``gap`` was recomputed, so the gap constraint itself holds -- being sorted is enforced by the
    range check alone."""
    acc, table, _ = statement
    i = int(np.flatnonzero((table[:-2, A.START] == 0) & (table[1:-1, A.START] == 0) & (table[1:-1, A.LIVE] == 1)
                           & (table[2:, A.LIVE] == 1) & (table[2:, A.START] == 0))[3])
    swapped = table.copy()
    swapped[[i, i + 1]] = swapped[[i + 1, i]]
    swapped = fill_memory_gaps(swapped)
    assert swapped[i + 1, A.GAP] == (int(table[i, A.CLK]) - int(table[i + 1, A.CLK]) - 1) % P >= P - N
    _, n_missing, first = range_trace(ctx, swapped)
    assert n_missing == 1 and first == (0, i + 1, 0)


def test_cpp_memory_table_example(ctx, tmp_path):
    """examples/memory_table.cpp: 64 accesses sorted with ts_matrix_sort_rows, three tables proved and verified with a
    zero bus sum; then one read value changed and named by ts_check_multi."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "memory_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "memory_table.cpp"), "-L", libdir, "-ltapstark_hip",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify -> 0, bus sum zero" in r.stdout
    assert "constraint violated in table 1" in r.stdout and "2 tuples out of balance" in r.stdout
    assert "unbalanced: table 0, row" in r.stdout and f"sent ({MEM_TAG}, " in r.stdout
    assert r.stdout.rstrip().endswith("memory_table: as expected")
