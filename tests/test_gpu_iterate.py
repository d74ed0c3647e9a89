"""The iterate form of ts_matrix_derive on the GPU, word for word against the plain Python loop of
tests/_iterate_cases.py AND against ts_derive_rows_host: heights and widths around the lane and the wave, group layouts
that straddle waves and count blocks, one long group among single rows (divergence inside a wave), group counts around
a wave and a trip of the offsets loop, every value of the TS_ITERATE_BLOCK_ROWS knob, outputs that overwrite what the
program reads, the refusals, pool poison, and a sponge chip filled and proved without its table leaving HBM.  Heights
are powers of two: no call makes a resident matrix of another height (the host loop is tested at other heights in
tests/test_iterate_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd._lib import TsError
from tapstark_amd.iterate import IterateBuilder, iterate_rows_host

import _derive_cases as dc
import _iterate_cases as ic
import _poison
from _field_cases import P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "TS_ITERATE_BLOCK_ROWS"
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


def check(ctx, prog, rows, what="", want=None):
    got = ts.DeviceMatrix.upload(ctx, rows).iterate(prog).download()
    same(got, ic.reference(prog, rows) if want is None else want, f"{what}: device against the reference")
    same(got, iterate_rows_host(prog, rows), f"{what}: device against the library's host loop")
    return got


def grouped(seed, width, lengths, column=0):
    """random rows whose reset column starts groups of the given lengths"""
    starts, height = ic.starts_of_lengths(lengths)
    assert height & (height - 1) == 0, height
    return ic.with_resets(dc.random_rows(seed, height, width), column, starts, seed)


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("width", [1, 3, 17])
@pytest.mark.parametrize("height", [1, 2, 64, 128, 4096])
def test_heights_and_widths(ctx, height, width):
    n = 3 if height == 4096 else 6
    for seed in range(n):
        prog = ic.random_program(1000 * width + seed, width)
        rows = ic.random_rows(height + seed, height, width, ic.parse(prog)[4])
        check(ctx, prog, rows, f"seed {seed}")


LAYOUTS = {
    "every row a start": [1] * 2048,
    "one group of the whole matrix": [1 << 10],
    "equal groups of 64": [64] * 64,
    "equal groups of 65": [65] * 63 + [1],
    "seeded lengths 1..130": ic.padded(np.random.default_rng(130).integers(1, 131, size=60).tolist()),
    "one group of 1000 rows among single rows": [1] * 12 + [1000] + [1] * 12,
    "exactly 64 groups": [4] * 64,
    "exactly 65 groups": [4] * 63 + [2, 2],
    "exactly 4097 groups": [2] * 4095 + [1, 1],
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_group_layouts(ctx, monkeypatch, name):
    """4097 groups with one row per count block: 8192 blocks, so the offsets loop makes 32 trips and the carry is
    crossed; 65 and 4097 groups leave a last workgroup of one lane."""
    if name.endswith("4097 groups"):
        monkeypatch.setenv(KNOB, "1")
    lengths = LAYOUTS[name]
    rows = grouped(len(lengths), 3, lengths)
    assert len(ic.group_starts(rows.tolist(), 0)) == len(lengths)
    for prog in (ic.sponge_like(3, 0), ic.fibonacci(3, 0), ic.op_program(ic.IS_GROUP_LAST), ic.op_program(ic.STEP)):
        check(ctx, prog, rows, name)


def test_no_reset_column_is_one_group(ctx):
    rows = dc.random_rows(8, 512, 2)
    got = check(ctx, ic.fibonacci(2, ic.NO_RESET), rows)
    a, b = 0, 1
    for r in range(512):
        assert (int(got[r, 2]), int(got[r, 3])) == (a, b)
        a, b = b, (a + b) % P


@pytest.mark.parametrize("op", ic.ALL_OPS)
def test_every_op(ctx, op):
    rows = grouped(op, 3, [1, 2, 5, 64, 1, 70, 13, 100])
    check(ctx, ic.op_program(op), rows, f"op {op}")


def test_sixteen_carries_and_carries_no_output_reaches(ctx):
    rows = grouped(16, 2, [7, 1, 90, 30])
    check(ctx, ic.sixteen_carries(2, 0), rows)
    # carry 1 counts the rows and no output reads it; it is still latched on every row
    nodes = [(ic.CARRY, 0, 0), (dc.COL, 0, 1), (dc.ADD, 0, 1), (ic.CARRY, 1, 0), (dc.CONST, 1, 0), (dc.ADD, 3, 4)]
    check(ctx, ic.tape(2, nodes, [(2, 2)], [(2, 0), (5, 9)], 0), rows)


# ------------------------------------------------------------------ 2. the knob changes no word
CASE_ROWS = grouped(42, 6, ic.padded(np.random.default_rng(42).integers(1, 40, size=200).tolist()), column=2)
CASE_PROG = ic.random_program(4, 6)
_case = {}


def case_reference():
    if not _case:
        prog = ic.parse(CASE_PROG)
        _case["prog"] = ic.tape(prog[0], prog[1], prog[2], prog[3], 2)
        _case["want"] = ic.reference(_case["prog"], CASE_ROWS)
    return _case["prog"], _case["want"]


@pytest.mark.parametrize("block_rows", [1, 3, 64, 1024])
def test_same_words_for_every_block_rows(ctx, monkeypatch, block_rows):
    prog, want = case_reference()
    monkeypatch.setenv(KNOB, str(block_rows))
    check(ctx, prog, CASE_ROWS, f"{KNOB}={block_rows}", want=want)


@pytest.mark.parametrize("value", ["0", "1025", "-1", "x"])
def test_knob_outside_its_range_is_refused(ctx, monkeypatch, value):
    monkeypatch.setenv(KNOB, value)
    with pytest.raises(TsError, match=r"TS_ITERATE_BLOCK_ROWS must be in \[1, 1024\]"):
        check(ctx, ic.fibonacci(6, 2), CASE_ROWS[:16])


# ------------------------------------------------------------------ 3. what is written and what is kept
def test_outputs_overwrite_the_reset_column_and_a_column_the_program_reads(ctx):
    rows = grouped(5, 3, [4, 1, 1, 66, 130, 2, 52])
    b = IterateBuilder(3, reset_column=0, max_group_rows=130)
    acc = b.carry(7)
    new = acc * 3 + b.col(1) + b.next(1) + b.prev(0)
    b.set_carry(acc, new)
    b.output(new, 0)             # over the reset column: the groups are still those of the source
    b.output(b.step() + new, 1)  # over a column the program reads, of this row and of the next
    got = check(ctx, b.tape(), rows)
    assert (got[:, 2] == rows[:, 2]).all()


def test_untouched_columns_keep_non_canonical_words(ctx):
    rows = grouped(6, 4, [4] * 32)
    rows[:, 3] = np.array([P, 0xFFFFFFFF, 1 << 31, P + 1, 5], dtype=np.uint64).astype(np.uint32)[np.arange(128) % 5]
    got = check(ctx, ic.sponge_like(4, 0, word=3), rows)
    assert (got[:, :4] == rows).all() and got.shape[1] == 5 and (got[:, 4] < P).all()


def test_the_source_stays_and_a_second_call_gives_the_same_words(ctx):
    rows = grouped(7, 3, [8] * 128)
    d = ts.DeviceMatrix.upload(ctx, rows)
    prog = ic.sponge_like(3, 0, dst=1)
    first = d.iterate(prog).download()
    same(d.download(), rows, "the source after the call")
    same(d.iterate(prog).download(), first, "a second call")
    same(first, ic.reference(prog, rows))


# ------------------------------------------------------------------ 4. refusals
def _refused(own, prog, d, status, text, live_before):
    out = C.c_void_p(12345)
    st = own._l.ts_matrix_derive(own.h, prog.ctypes.data_as(ts._lib.u32p), len(prog), d.h, C.byref(out))
    assert st == status and own._l.ts_last_error(own.h).decode() == text, own._l.ts_last_error(own.h)
    assert not out.value, "a refused call left a handle"
    assert own.stat(STAT_LIVE_BLOCKS) == live_before, "a refused call kept pool blocks"


@pytest.mark.parametrize("block_rows", [None, 1, 100])
def test_the_least_over_long_group_is_named(monkeypatch, block_rows):
    """Three over-long groups: one of 41 rows from row 1000 (it straddles count blocks with the knob at 1 and at its
    default, 1024), a longer one later, and the final group, which no start ends.  The first is named.
    Then only the final one is over-long."""
    from tapstark_amd.build import build

    build()
    if block_rows:
        monkeypatch.setenv(KNOB, str(block_rows))
    lengths = [40] * 25 + [41] + [40] * 10 + [300] + [40] * 5 + [107]
    rows = grouped(3, 3, lengths)
    own = ts.Context(0)
    d = ts.DeviceMatrix.upload(own, rows)
    live_before = own.stat(STAT_LIVE_BLOCKS)
    prog = ic.sponge_like(3, 0, max_group_rows=40)
    text = "iterate: the group that starts at row 1000 has 41 rows, max_group_rows is 40"
    assert ic.longest_refusal(rows.tolist(), 0, 40) == text
    for _ in range(2):
        _refused(own, prog, d, TS_ERR_INVARIANT, text, live_before)
    with pytest.raises(TsError) as e:
        iterate_rows_host(prog, rows)
    assert text in str(e.value)
    rows = grouped(3, 3, [40] * 25 + [24] + [40] * 24 + [64])
    with pytest.raises(TsError, match="iterate: the group that starts at row 1984 has 64 rows, max_group_rows is 40"):
        ts.DeviceMatrix.upload(own, rows).iterate(prog)
    same(ts.DeviceMatrix.upload(own, rows).iterate(ic.sponge_like(3, 0, max_group_rows=64)).download(),
         ic.reference(prog, rows), "max_group_rows = the longest group")


def test_refusals_leave_no_handle(ctx):
    rows = grouped(4, 3, [4] * 4)
    d = ts.DeviceMatrix.upload(ctx, rows)
    good = ic.sponge_like(3, 0)
    lib, out = ctx._l, C.c_void_p()

    def refused(text, prog=good, ctx_h=ctx.h, handle=d.h, n_words=None):
        out.value = 12345
        st = lib.ts_matrix_derive(ctx_h, prog.ctypes.data_as(ts._lib.u32p) if prog is not None else None,
                                  (len(prog) if prog is not None else 0) if n_words is None else n_words, handle,
                                  C.byref(out))
        assert st == TS_ERR_INVALID and text in lib.ts_last_error(ctx_h).decode(), lib.ts_last_error(ctx_h)
        assert not out.value, "a refused call left a handle"

    refused("null argument", prog=None)
    refused("null argument", handle=None)
    refused("iterate: the program is written for a source of 4 columns, this one has 3", prog=ic.sponge_like(4, 0))
    refused("words, the header asks for", n_words=len(good) - 1)
    refused("iterate: reset_column 3 is outside the source", prog=ic.sponge_like(3, 3))
    refused("iterate: max_group_rows is 0", prog=ic.sponge_like(3, 0, max_group_rows=0))
    refused("is above the work limit of 1048576", prog=ic.sponge_like(3, 0, max_group_rows=1 << 20))
    refused("unknown op 40", prog=dc.tape(3, [(ic.CARRY, 0, 0)], [(0, 3)]))
    other = ts.Context(0)
    refused("made on this context", ctx_h=other.h)
    same(d.iterate(good).download(), ic.reference(good, rows), "the matrix still iterates")


# ------------------------------------------------------------------ 5. pool poison
def test_pool_poison_changes_nothing():
    """Every out word, every count, offset, start and the two words the host reads are written by the kernels before
    they are read: the same matrices on a clean context and on contexts whose pool hands out blocks full of 0x00000001
    and 0xFFFFFFFF."""
    from tapstark_amd.build import build

    build()
    trio = _poison.make_contexts()
    cases = []
    for seed in (3, 7):
        prog = ic.random_program(seed, 5)
        cases.append((prog, ic.random_rows(seed, 1 << 11, 5, ic.parse(prog)[4])))
    cases.append((ic.sixteen_carries(2, 1), grouped(9, 2, [1] * 24 + [500] + [2] * 250, column=1)))

    def run(c):
        return [ts.DeviceMatrix.upload(c, rows).iterate(prog).download() for prog, rows in cases]

    _poison.same_everywhere(trio, run, want=[ic.reference(prog, rows) for prog, rows in cases], what="iterate")
    assert all(c.stat(_poison.STAT_FILLS) > 0 for c in trio[1:])


# ------------------------------------------------------------------ 6. a sponge chip filled and proved in HBM
N_CALLS, MAX_LEN = 1 << 5, 12
CHALLENGES = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)


def _sponge_statement(ctx, calls):
    """expand -> iterate -> join: the two resident traces, the tables with their AIRs, n_live."""
    from tapstark_amd.airs import SpongeCallAir, SpongeChipAir, sponge_chip_table, sponge_fetch_digests
    import _bus_cases as bc

    d_calls = ts.DeviceMatrix.upload(ctx, calls)
    d_chip, n_live = sponge_chip_table(ctx, d_calls, max_len=MAX_LEN)
    d_calls = sponge_fetch_digests(d_calls, d_chip)
    airs = [SpongeCallAir(), SpongeChipAir()]
    tabs = [bc.Table(a, np.zeros((h, a.width()), dtype=np.uint32)) for a, h in zip(airs, [len(calls), d_chip.dims()[0]])]
    return [d_calls, d_chip], tabs, n_live


def test_sponge_chip_resident(ctx):
    from tapstark_amd.airs import (SPONGE_IV, SPONGE_TAG, SpongeCallAir, SpongeChipAir, generate_sponge_call_trace,
                                   generate_sponge_chip_trace)
    import _bus_cases as bc

    A, T = SpongeCallAir, SpongeChipAir
    calls = generate_sponge_call_trace(N_CALLS, MAX_LEN, 5, unfilled=True)
    assert 0 < calls[:, A.SEL].sum() < N_CALLS and not calls[:, A.DIGEST].any()
    traces, tabs, n_live = _sponge_statement(ctx, calls)
    chip = traces[1].download()
    same(chip, generate_sponge_chip_trace(calls), "the chip table made in HBM against the host's")
    assert n_live == int(calls[calls[:, A.SEL] == 1][:, A.LEN].sum())
    # every state is the seventh power of its acc, and acc is the state before plus the word
    before = SPONGE_IV
    for first, last, _, word, acc, state in chip.tolist():
        assert acc == ((SPONGE_IV if first else before) + word) % P and state == pow(acc, 7, P)
        before = state
    filled = traces[0].download()
    same(filled, generate_sponge_call_trace(N_CALLS, MAX_LEN, 5), "the digests fetched back by id")
    cairs = bc.compiled(ctx, tabs)
    pis, logups = [t.pis for t in tabs], [t.logup for t in tabs]
    bad, fv, rep = ts.check_multi(None, cairs, traces, pis, logups, CHALLENGES, ctx=ctx)
    assert (bad, fv) == (-1, -1) and rep.balanced
    # one absorbed word changed after the digests were fetched: the chip is refilled, the machine's digest is stale
    # (before the proof, which consumes the traces)
    row = int(np.flatnonzero(chip[:, T.LAST] == 1)[2])
    chip[row, T.WORD] += 1
    d_chip = ts.DeviceMatrix.upload(ctx, chip).iterate(ts.airs.sponge_program(MAX_LEN))
    bad, fv, rep = ts.check_multi(None, cairs, [traces[0], d_chip], pis, logups, CHALLENGES, ctx=ctx)
    assert (bad, fv) == (-1, -1), "every constraint holds: the chip is made from its words"
    assert not rep.balanced and rep.n_unbalanced == 2
    assert rep.tuple[0] == SPONGE_TAG and rep.tuple[1] == chip[row, T.ID]
    config = bc.config(ctx, 3)  # state = acc^7: eight quotient chunks
    proof = ts.prove_multi_bus(config, cairs, ts.BfChallenger(), traces, pis, logups)
    bc.verify(config, tabs, proof)  # raises unless accepted with the bus sum at zero


def test_cpp_sponge_chip_resident_example(ctx, tmp_path):
    """examples/sponge_chip_resident.cpp: the chip table expanded from a call trace, its state column filled by the
    iterate form, the digests fetched back, proved and verified; one changed word named.  No trace comes down."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "sponge_chip_resident")
    source = os.path.join(ROOT, "examples", "sponge_chip_resident.cpp")
    text = open(source).read()
    assert "ts_matrix_download" not in text and text.count("ts_matrix_upload(") == 1
    assert "ts_matrix_expand_rows(" in text and "ts_matrix_join_rows(" in text and "ts::air::Iterate" in text
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source,
                           "-L", libdir, "-ltapstark_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "32 call rows, " in r.stdout and "rows x 6 expanded in HBM" in r.stdout
    assert "verify -> 0, bus sum zero" in r.stdout
    assert "constraints hold in every table; 2 tuples out of balance" in r.stdout and "(19, " in r.stdout
    assert r.stdout.rstrip().endswith("sponge_chip_resident: as expected")
