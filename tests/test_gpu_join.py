"""ts_matrix_join_rows on the GPU against the exact reference of tests/_join_cases.py, word for word: the case grid of
tests/test_join_cpu.py, several workgroups, result widths below and above a wave's worth of words, every value of the
TS_LOGUP_HASH_BITS knob that changes the chains, a table of 64-fold duplicates, one key on every row, the miss reports,
the refusals that need a device, pool poison, and the ROM statement filled in HBM and proved against its key.

A resident matrix has a power of two of rows (ts_matrix_upload admits no other height), so the grid runs here at the
source heights 1, 4 and 1024 and at tables of 1, 8 and 512 rows of which 1, 5 and 257 are entered (table_rows): the
rows behind them are pad rows that would otherwise match.  Source heights 3, 1000 and 2^12 + 1 cannot exist on the device;
the host loop runs them in tests/test_join_cpu.py.  A workgroup's partial block (fewer rows than lanes) is every source
height below 256 here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd._lib import TsError
from tapstark_amd.airs import (ROM_TAG, BusKeyTableAir, BusTupleSendAir, fill_bus_key_multiplicities,
                               generate_key_table_trace, generate_rom_fetch_trace, generate_rom_key, rom_join_spec,
                               selected_tuples)
from tapstark_amd.join import ALWAYS, HIT, KEEP, TABLE_ROW, JoinSpec, col, join_rows_host

import _join_cases as jc
import _key_cases as kc
import _poison
from _join_cases import P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "TS_LOGUP_HASH_BITS"
STAT_LIVE_BLOCKS = 11  # ts_ctx_stat: pool blocks handed out and not yet given back
TS_ERR_INVALID, TS_ERR_INVARIANT = 1, 5


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(autouse=True)
def default_knob(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]}: "
                           f"{int(got[tuple(bad[0])]):#x} for {int(want[tuple(bad[0])]):#x}")


def join(ctx, spec, src, table):
    d_src = ts.DeviceMatrix.upload(ctx, src)
    d_table = d_src if table is src else ts.DeviceMatrix.upload(ctx, table)
    out, n_missing, first = d_src.join_rows(d_table, spec, allow_missing=True)
    same(d_src.download(), src, "the source is only read")
    return out.download(), n_missing, first


def check(ctx, spec, src, table, what="", want=None):
    got = join(ctx, spec, src, table)
    want = want or jc.reference(spec, src, table)
    assert got[1:] == want[1:], (what, got[1:], want[1:])
    same(got[0], want[0], what)
    return got


# ------------------------------------------------------------------ 1. the grid
GRID = list(jc.grid(src_heights=(1, 4, 1024), table_heights=(1, (8, 5), (512, 257))))


@pytest.mark.parametrize("name,case", GRID, ids=[name for name, _ in GRID])
def test_grid_against_the_reference(ctx, name, case):
    check(ctx, *case, what=name)


@pytest.mark.parametrize("height", [2, 8, 16, 32, 64, 128, 256, 512])
def test_partial_and_full_blocks(ctx, height):
    check(ctx, *jc.case(height, height, 64, 2, 3, flags=TABLE_ROW | HIT, place="appended"), what=f"height {height}")


def _wide(seed, height, width):
    """A result of exactly ``width`` columns."""
    if width == 1:  # the key column is the dst column
        rng = np.random.default_rng(seed)
        table = rng.integers(0, 1 << 32, size=(64, 2), dtype=np.uint32)
        src = table[rng.integers(0, 64, size=height), :1].copy()
        src[rng.random(height) < 0.1] = 3
        return JoinSpec(keys=[(col(0), col(0))], fetch=[(1, 0, 11)]), src, table
    spec, src, table = jc.case(seed, height, 256, 1, 2, flags=TABLE_ROW, place="appended", extra=width - 5)
    return spec, src, table


@pytest.mark.parametrize("width", [1, 5, 70])
@pytest.mark.parametrize("height", [1 << 12, 1 << 13])
def test_several_workgroups_and_result_widths(ctx, height, width):
    spec, src, table = _wide(width, height, width)
    got = check(ctx, spec, src, table, what=f"{height} x {width}")
    assert got[0].shape == (height, width) and 0 < got[1] < height


def test_seventy_columns_with_dst_columns_on_both_sides_of_column_64(ctx):
    rng = np.random.default_rng(9)
    table = rng.integers(0, 1 << 32, size=(128, 4), dtype=np.uint32)
    table[:, 0] = rng.permutation(128)
    src = rng.integers(0, 1 << 32, size=(1 << 10, 72), dtype=np.uint32)
    src[:, 70] = rng.integers(0, 140, size=1 << 10)
    spec = JoinSpec(keys=[(col(70), col(0))], fetch=[(1, 63, 1), (2, 64, 2), (3, 0, 3), (1, 71, 4), (2, 72, 5), (3, 65, 6)],
                    flags=TABLE_ROW | HIT)
    got = check(ctx, spec, src, table)
    assert got[0].shape == (1 << 10, 75)


# ------------------------------------------------------------------ 2. the hash knob, duplicates, one key
@pytest.mark.parametrize("bits", [0, 3, 32])
def test_same_words_for_every_hash_mask(ctx, monkeypatch, bits):
    """0: one chain through every entry; 3: eight chains, those of the last slots wrap past the end; 32: the hash."""
    spec, src, table = jc.case(17, 1 << 10, 1 << 8, 2, 3, flags=TABLE_ROW | HIT, consts=False)
    table[:, :2] = np.random.default_rng(1).integers(0, 1 << 32, size=(256, 2), dtype=np.uint32)  # 256 classes
    src[:, :2] = table[np.random.default_rng(2).integers(0, 256, size=1 << 10), :2]
    src[::7, 0] ^= 1  # misses walk a whole chain
    want = jc.reference(spec, src, table)
    assert 0 < want[1] < 1 << 10
    monkeypatch.setenv(KNOB, str(bits))
    check(ctx, spec, src, table, what=f"{bits} hash bits", want=want)
    chase_spec, m = jc.chase(bits, 1 << 8)
    check(ctx, chase_spec, m, m, what="src is table")


@pytest.mark.parametrize("value", ["33", "-1", "x"])
def test_knob_outside_its_range_is_refused(ctx, monkeypatch, value):
    spec, m = jc.chase(1, 16)
    d = ts.DeviceMatrix.upload(ctx, m)
    before = ctx.stat(STAT_LIVE_BLOCKS)
    monkeypatch.setenv(KNOB, value)
    with pytest.raises(TsError, match="TS_LOGUP_HASH_BITS must be in"):
        d.join_rows(d, spec)
    assert ctx.stat(STAT_LIVE_BLOCKS) == before


def test_every_tuple_64_times_the_lowest_row_wins(ctx):
    rng = np.random.default_rng(11)
    tuples = rng.integers(0, 1 << 32, size=(64, 3), dtype=np.uint32)
    table = np.concatenate([np.repeat(tuples, 64, axis=0), rng.integers(0, 1 << 32, size=(1 << 12, 2), dtype=np.uint32)],
                           axis=1)[rng.permutation(1 << 12)]
    src = np.concatenate([tuples[rng.integers(0, 64, size=1 << 11)], np.zeros((1 << 11, 1), dtype=np.uint32)], axis=1)
    spec = JoinSpec(keys=[(col(q), col(q)) for q in range(3)], fetch=[(3, 3, 0), (4, 4, 0)], flags=TABLE_ROW)
    for _ in range(2):  # the insert race is another one every time
        out, n_missing, _ = check(ctx, spec, src, table)
    assert n_missing == 0
    lowest = {tuple(t): int(np.flatnonzero((table[:, :3] == t).all(axis=1)).min()) for t in tuples.tolist()}
    assert out[:, 5].tolist() == [lowest[tuple(r)] for r in src[:, :3].tolist()]


def test_every_row_on_one_key(ctx):
    spec, src, table = jc.case(23, 1 << 13, 256, 1, 2, flags=TABLE_ROW | HIT, hit=1.0)
    src[:, 0] = table[77, 0]
    src[:, 1] = 1  # every row takes part
    out, n_missing, first = check(ctx, spec, src, table)
    assert (n_missing, first) == (0, None) and len(set(out[:, -2].tolist())) == 1 and out[:, -1].all()


# ------------------------------------------------------------------ 3. misses
def _miss_case(height=1 << 10):
    rng = np.random.default_rng(31)
    table = np.stack([rng.permutation(64) + 500, rng.integers(0, P, size=64)], axis=1).astype(np.uint32)
    src = np.zeros((height, 3), dtype=np.uint32)
    src[:, 0] = table[rng.integers(0, 64, size=height), 0]
    src[:, 1] = 1
    return JoinSpec(keys=[(col(0), col(0))], when=col(1), fetch=[(1, 2, 9)], flags=HIT), src, table


def test_no_miss_one_miss_on_the_last_row_all_miss(ctx):
    spec, src, table = _miss_case()
    assert check(ctx, spec, src, table, "none")[1:] == (0, None)
    one = src.copy()
    one[-1, 0] = 7
    assert check(ctx, spec, one, table, "the last row")[1:] == (1, len(src) - 1)
    every = src.copy()
    every[:, 0] += 1000
    out, n_missing, first = check(ctx, spec, every, table, "all")
    assert (n_missing, first) == (len(src), 0) and (out[:, 2] == 9).all() and not out[:, 3].any()
    # a row that would miss but takes no part is not counted
    quiet = one.copy()
    quiet[-1, 1] = 2 * P
    quiet[5, 0], quiet[5, 1] = 7, 0
    assert check(ctx, spec, quiet, table, "no part")[1:] == (0, None)
    late = src.copy()
    late[[300, 301, 900], 0] = 7  # three waves report; the least row is the answer
    assert check(ctx, spec, late, table, "three")[1:] == (3, 300)


def test_a_miss_without_a_count_is_an_error_that_returns_every_block():
    from tapstark_amd.build import build

    build()
    own = ts.Context(0)  # its pool holds only what this test took and gave back
    spec, src, table = _miss_case()
    src[700, 0] = 7
    d_src, d_table = ts.DeviceMatrix.upload(own, src), ts.DeviceMatrix.upload(own, table)
    s, _keep = spec.c_spec()
    before = own.stat(STAT_LIVE_BLOCKS)
    assert before >= 2, "the source and the table are live blocks"
    for first_p in (True, False):
        out, first = C.c_void_p(12345), C.c_uint64(77)
        st = own._l.ts_matrix_join_rows(own.h, C.byref(s), d_src.h, d_table.h, C.byref(out), None,
                                        C.byref(first) if first_p else None)
        assert st == TS_ERR_INVARIANT
        assert own._l.ts_last_error(own.h).decode() == "join: the key of source row 700 is in no table row (1 such rows)"
        assert not out.value, "a refused call left a handle"
        assert own.stat(STAT_LIVE_BLOCKS) == before, "a refused call kept pool blocks"
    with pytest.raises(TsError, match="source row 700"):
        d_src.join_rows(d_table, spec)
    got, n_missing, first_missing = d_src.join_rows(d_table, spec, allow_missing=True)
    assert (n_missing, first_missing) == (1, 700) and own.stat(STAT_LIVE_BLOCKS) == before + 1
    same(got.download(), jc.reference(spec, src, table)[0], "with a count the result is complete")


# ------------------------------------------------------------------ 4. refusals that need a device
def test_refusals_leave_no_handle(ctx):
    spec, src, table = _miss_case(16)
    d_src, d_table = ts.DeviceMatrix.upload(ctx, src), ts.DeviceMatrix.upload(ctx, table)
    lib, out, n, first = ctx._l, C.c_void_p(), C.c_uint64(), C.c_uint64()
    before = ctx.stat(STAT_LIVE_BLOCKS)

    def refused(text, spec=spec, ctx_h=ctx.h, src_h=d_src.h, table_h=d_table.h, out_p=C.byref(out)):
        out.value = 12345
        s, _keep = spec.c_spec() if spec is not None else (None, None)
        st = lib.ts_matrix_join_rows(ctx_h, C.byref(s) if s is not None else None, src_h, table_h, out_p, C.byref(n),
                                     C.byref(first))
        assert st == TS_ERR_INVALID and text in lib.ts_last_error(ctx_h).decode(), lib.ts_last_error(ctx_h)
        assert (out_p is None or not out.value) and n.value == 0 and first.value == 2 ** 64 - 1
        assert ctx.stat(STAT_LIVE_BLOCKS) == before

    refused("null argument", spec=None)
    refused("null argument", src_h=None)
    refused("null argument", table_h=None)
    refused("null argument", out_p=None)
    refused("the column is outside the source", spec=JoinSpec(keys=[(col(3), col(0))], fetch=[(1, 2, 0)]))
    refused("the column is outside the table", spec=JoinSpec(keys=[(col(0), col(2))], fetch=[(1, 2, 0)]))
    refused("table_rows 65 above the table's height 64", spec=JoinSpec(keys=[(col(0), col(0))], fetch=[(1, 2, 0)], table_rows=65))
    other = ts.Context(0)
    refused("made on this context", ctx_h=other.h)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 1), ctx)
    consumed = ts.DeviceMatrix.upload(ctx, src)
    _, consumed_data = pcs.commit([((4, 1), consumed)])
    before = ctx.stat(STAT_LIVE_BLOCKS)
    refused("the source must be a row-major, unconsumed matrix", src_h=consumed.h)
    refused("the table must be a row-major, unconsumed matrix", table_h=consumed.h)
    check(ctx, spec, src, table, "the matrices still join")


# ------------------------------------------------------------------ 5. pool poison
def test_pool_poison_changes_nothing():
    """Every word of the result, every slot and the miss report are written before they are read: the same matrices on
    a clean context and on contexts whose pool hands out blocks full of 0x00000001 and 0xFFFFFFFF."""
    from tapstark_amd.build import build

    build()
    trio = _poison.make_contexts()
    cases = [jc.case(3, 1 << 11, 256, 2, 3, flags=TABLE_ROW | HIT, place="appended"),
             jc.case(4, 1 << 9, 64, 1, 32, flags=KEEP, place="inside", entered=40),
             jc.case(5, 1 << 6, 4, 3, 0, flags=HIT)]
    spec, src, table = _miss_case()
    cases += [(spec, src, table), (spec, src + np.uint32(1000), table)]  # no miss; every row misses

    def run(c):
        out = []
        for spec, src, table in cases:
            m, n_missing, first = ts.DeviceMatrix.upload(c, src).join_rows(ts.DeviceMatrix.upload(c, table), spec, True)
            out += [m.download(), n_missing, -1 if first is None else first]
        return out

    want = []
    for spec, src, table in cases:
        m, n_missing, first = jc.reference(spec, src, table)
        want += [m, n_missing, -1 if first is None else first]
    _poison.same_everywhere(trio, run, want=want, what="join")
    assert all(c.stat(_poison.STAT_FILLS) > 0 for c in trio[1:])


# ------------------------------------------------------------------ 6. the ROM statement
N_SEND, K, N_ROM = 1 << 6, 2, 1 << 4


def _rom_tables(rom, trace):
    mult = generate_key_table_trace(rom, selected_tuples(trace, 3))
    return [kc.Table(BusTupleSendAir(ROM_TAG, K, 3), trace), kc.Table(BusKeyTableAir(ROM_TAG, 3), mult, key=rom)]


@pytest.mark.parametrize("log_blowup", [1, 2])
def test_rom_statement_filled_in_hbm_is_the_host_s_proof(ctx, log_blowup):
    rom = generate_rom_key(N_ROM, 5)
    unfilled = generate_rom_fetch_trace(N_SEND, K, rom, 6, unfilled=True)
    host = unfilled
    for spec in rom_join_spec(K):
        host, n_missing, _ = jc.reference(spec, host, rom)
        assert n_missing == 0
    same(host, generate_rom_fetch_trace(N_SEND, K, rom, 6), "the reference fills what the generator writes")
    tables = _rom_tables(rom, host)
    cfg = kc.config(ctx, log_blowup)
    cairs = kc.compiled(ctx, tables)
    key = kc.make_key(cfg, tables)
    want = kc.prove(cfg, key, cairs, tables)  # traces filled on the host

    d_trace = ts.DeviceMatrix.upload(ctx, unfilled)  # the only trace upload
    for spec in rom_join_spec(K):
        d_trace, n_missing, first = d_trace.join_rows(key.values(0), spec)
        assert (n_missing, first) == (0, None)
    same(d_trace.download(), host, "the trace filled in HBM")
    d_rom = ts.DeviceMatrix.upload(ctx, np.zeros((N_ROM, 1), dtype=np.uint32))
    assert fill_bus_key_multiplicities(d_rom, key.values(0), [d_trace], n_values=3) == (0, None)
    proof = ts.prove_multi_key(cfg, key, cairs, ts.BfChallenger(), [d_trace, d_rom], [t.pis for t in tables],
                               [t.logup for t in tables])
    assert len(proof.words) == len(want.words) and (proof.words == want.words).all(), "not the host's proof"
    _, bus_sum = kc.verify(cfg, key.root, tables, proof)  # raises unless accepted with the bus sum at zero
    assert not np.asarray(bus_sum).any()
    changed = rom.copy()
    changed[3, 1] = (int(changed[3, 1]) + 1) % 64
    other = ts.MultiKey(cfg, [changed], keep_values=False)
    with pytest.raises(ts.VerificationError):
        kc.verify(cfg, other.root, tables, proof)


def test_rom_pc_outside_the_rom_is_named(ctx):
    rom = generate_rom_key(N_ROM, 5)
    bad = generate_rom_fetch_trace(N_SEND, K, rom, 6, unfilled=True)
    row = int(np.flatnonzero(bad[:, 7] == 1)[4])
    bad[row, 4] = 7
    d, d_rom = ts.DeviceMatrix.upload(ctx, bad), ts.DeviceMatrix.upload(ctx, rom)
    specs = rom_join_spec(K)
    d, n_missing, first = d.join_rows(d_rom, specs[0])
    assert (n_missing, first) == (0, None)
    with pytest.raises(TsError, match=f"source row {row} is in no table row"):
        d.join_rows(d_rom, specs[1])
    _, n_missing, first = d.join_rows(d_rom, specs[1], allow_missing=True)
    assert (n_missing, first) == (1, row)


def test_host_loop_and_device_agree_on_the_rom(ctx):
    rom = generate_rom_key(N_ROM, 8)
    unfilled = generate_rom_fetch_trace(N_SEND, K, rom, 9, unfilled=True)
    spec = rom_join_spec(K)[1]
    same(join(ctx, spec, unfilled, rom)[0], join_rows_host(spec, unfilled, rom)[0])


def test_cpp_rom_fetch_resident_example(ctx, tmp_path):
    """examples/rom_fetch_resident.cpp: the trace filled from the key's values in HBM, proved and verified; one pc
    outside the ROM named."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "rom_fetch_resident")
    source = os.path.join(ROOT, "examples", "rom_fetch_resident.cpp")
    text = open(source).read()
    # four uploads in the text: the ROM, the unfilled trace -- the only trace of the statement --, the zeros of the ROM
    # table's column, and the changed trace of the last step
    assert text.count("ts_matrix_join_rows(ctx") == 3 and text.count("ts_matrix_upload(") == 4
    assert "ts_matrix_upload(ctx, trace.data(), N, W, &unfilled)" in text and "ts_multi_key_values(key, 0, &rom_values)" in text
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source,
                           "-L", libdir, "-ltapstark_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "64 rows x 2 slots, " in r.stdout and ", 128 slots hold what the ROM says" in r.stdout
    assert "0 misses in the fill, TSPF v8 proof of " in r.stdout and "verify -> 0, bus sum zero" in r.stdout
    assert ": 1 miss, first_missing " in r.stdout and "without a count: status 5, join: the key of source row " in r.stdout
    assert r.stdout.rstrip().endswith("rom_fetch_resident: as expected")
