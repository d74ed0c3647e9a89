"""ts_matrix_expand_rows on the GPU against the exact reference of tests/_expand_cases.py, word for word: source heights
and widths around the lane, the wave and the workgroup, every count pattern (nothing, the identity, one row asking for
2^14 rows among rows asking for nothing, elements that straddle tiles), words that only their reduced value decides,
every value of the TS_EXPAND_BLOCK_ROWS knob, the two late refusals with sums past 32 bits, pool poison, and the chip
table of a span statement made and proved without the trace leaving HBM.  Source heights are powers of two: no call
makes a matrix of another height (the host loop is tested at other heights in tests/test_expand_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd._lib import TsError
from tapstark_amd.airs import (BUS_TAG, BusRangeAir, SpanCallAir, SpanChipAir, fill_span_range_multiplicities,
                               generate_span_call_trace, generate_span_chip_trace, span_chip_table)
from tapstark_amd.derive import DeriveBuilder
from tapstark_amd.expand import ALWAYS, FIRST, J, LAST, REMAINING, ROW, ExpandSpec, col, expand_rows_host, stepped

import _bus_cases as bc
import _expand_cases as xc
import _poison
from _expand_cases import P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "TS_EXPAND_BLOCK_ROWS"
STAT_POOL_BYTES = 3  # ts_ctx_stat: bytes the device pool has reserved, handed out or not
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


def expand(ctx, spec, src, out_height=0):
    got, live = ts.expand_rows(ctx, spec, ts.DeviceMatrix.upload(ctx, src), out_height)
    return got.download(), live


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]}: "
                           f"{int(got[tuple(bad[0])]):#x} for {int(want[tuple(bad[0])]):#x}")


def check(ctx, spec, src, out_height=0, what=""):
    got, live = expand(ctx, spec, src, out_height)
    want, want_live = xc.reference(spec, src, out_height)
    assert live == want_live, what
    same(got, want, what)
    return got, live


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("width", [1, 3, 17])
@pytest.mark.parametrize("height", [1, 2, 64, 256, 1024, 1 << 12, 1 << 14])
def test_heights_and_widths(ctx, height, width):
    src = xc.random_rows(height + width, height, width)
    kinds = set()
    for out_width in (1, 5, 64):
        spec = xc.random_spec(height + width + out_width, width, out_width)
        kinds |= {xc._term(t)[0] for t in spec.terms}
        check(ctx, spec, src, what=f"out_width {out_width}")
    assert kinds == set(range(8)), "every term kind"


def test_device_host_and_reference_agree_and_the_source_stays(ctx):
    for seed in range(4):
        width = [5, 2, 9, 3][seed]
        src = xc.random_rows(seed, 1 << (11 - seed), width, max_count=[7, 1, 40, 3][seed], density=0.25 * (seed + 1))
        spec = xc.random_spec(seed, width, 7, max_count=[7, 1, 40, 3][seed])
        d_src = ts.DeviceMatrix.upload(ctx, src)
        d_out, live = d_src.expand_rows(spec)
        got = d_out.download()
        want, want_live = xc.reference(spec, src)
        same(got, want, f"seed {seed}: device against the reference")
        host, host_live = expand_rows_host(spec, src)
        same(got, host, f"seed {seed}: device against the library's host loop")
        assert live == want_live == host_live
        same(d_src.download(), src, "the source after the call")
        again, live_again = ts.expand_rows(ctx, spec, d_src)
        same(again.download(), got, "a second call")
        assert live_again == live


# ------------------------------------------------------------------ 2. count patterns
N = 1 << 12
BIG = 1 << 14
ROWS = np.arange(N)
PATTERN_SPEC = ExpandSpec(4, 7, count=col(1), when=col(0), max_count=BIG, pad=[P - 1, 0, 7, 1, 2, 3, 4],
                          terms=[ROW, J, REMAINING, FIRST, LAST, stepped(2, 1), col(3)])


def _pattern(counts):
    src = xc.random_rows(11, N, 4)
    src[:, 0] = np.array(xc.LOUD, dtype=np.uint32)[ROWS % 3]
    src[:, 1] = np.asarray(counts, dtype=np.uint32)
    return src


PATTERNS = {
    "all 0": np.zeros(N, int),
    "all 1 (the identity)": np.ones(N, int),
    "only the last row 1": (ROWS == N - 1).astype(int),
    "only the first row 1": (ROWS == 0).astype(int),
    "one row of 2^14 at the first row": np.where(ROWS == 0, BIG, 0),
    "one row of 2^14 at a middle row": np.where(ROWS == 1717, BIG, 0),
    "one row of 2^14 at the last row": np.where(ROWS == N - 1, BIG, 0),
    "alternating 0 and 3": np.where(ROWS % 2 == 1, 3, 0),
    "seeded 0..7": np.random.default_rng(5).integers(0, 8, size=N),
    "whole blocks of nothing between full ones": np.where((ROWS // 1024) % 2 == 1, 2, 0),
}


@pytest.mark.parametrize("name", list(PATTERNS))
def test_count_patterns(ctx, name):
    counts = PATTERNS[name]
    got, live = check(ctx, PATTERN_SPEC, _pattern(counts), what=name)
    assert live == int(counts.sum())
    if name == "all 0":
        assert got.tolist() == [[P - 1, 0, 7, 1, 2, 3, 4]], "height 1, all pad"
    if name.startswith("all 1"):
        assert got.shape[0] == N and (got[:, 0] == ROWS).all() and not got[:, 1].any() and got[:, 3].all() and got[:, 4].all()
    if name.startswith("one row of 2^14"):
        assert got.shape[0] == BIG and len(set(got[:, 0].tolist())) == 1 and (got[:, 1] == np.arange(BIG)).all()


def test_a_constant_count_of_24(ctx):
    src = xc.random_rows(24, N, 3)
    spec = ExpandSpec(3, 4, count=24, when=col(0), max_count=24, terms=[ROW, J, LAST, col(2)])
    got, live = check(ctx, spec, src)
    assert live % 24 == 0 and 0 < live < 24 * N and (got[:live, 1] == np.arange(live) % 24).all()
    check(ctx, ExpandSpec(3, 2, count=24, when=ALWAYS, max_count=24, terms=[ROW, J]), src[:64])


@pytest.mark.parametrize("block_rows", [64, 255])
def test_elements_straddle_tiles(ctx, monkeypatch, block_rows):
    """Counts of knob + 1 and knob - 1 in turn: the first element of a source row falls one output row further into its
    tile with every pair, so tiles begin and end inside elements, at every place."""
    monkeypatch.setenv(KNOB, str(block_rows))
    counts = np.where(ROWS % 2 == 0, block_rows + 1, block_rows - 1)
    spec = ExpandSpec(4, 4, count=col(1), when=ALWAYS, max_count=block_rows + 1, terms=[ROW, J, REMAINING, stepped(2, P - 1)])
    got, live = check(ctx, spec, _pattern(counts)[:N // 4])
    assert live == block_rows * N // 4


# ------------------------------------------------------------------ 3. reduced values
def test_words_decide_mod_p(ctx):
    sel = np.array(xc.QUIET + xc.LOUD + [2, P - 1], dtype=np.uint32)
    cnt = np.array([1, 2, 3, P, P + 3, 2 * P, 2 * P + 1, 0], dtype=np.uint32)
    src = np.stack([sel, cnt, np.arange(8, dtype=np.uint32)], axis=1)
    got, live = check(ctx, ExpandSpec(3, 3, count=col(1), when=col(0), max_count=3, terms=[col(2), col(1), J]), src)
    # rows 0 .. 2 are quiet; p and 2p ask for nothing, p + 3 for 3, 2p + 1 for 1; the copied word stays as stored
    assert live == 4 and got[:4].tolist() == [[4, P + 3, 0], [4, P + 3, 1], [4, P + 3, 2], [6, 2 * P + 1, 0]]
    got, live = check(ctx, ExpandSpec(3, 1, count=col(1), when=ALWAYS, max_count=3, terms=[col(2)]), src)
    assert got[:live, 0].tolist() == [0, 1, 1, 2, 2, 2, 4, 4, 4, 6]


def test_stepped_and_copied_words_at_the_edges(ctx):
    src = np.array([[P - 1], [P], [0xFFFFFFFF], [5]], dtype=np.uint32)
    spec = ExpandSpec(1, 3, count=3, max_count=3, terms=[stepped(0, 1), stepped(0, P - 1), col(0)])
    got, live = check(ctx, spec, src)
    top = (1 << 28) - 3  # 0xFFFFFFFF mod p
    assert live == 12 and got[:9].tolist() == [
        [P - 1, P - 1, P - 1], [0, P - 2, P - 1], [1, P - 3, P - 1],
        [0, 0, P], [1, P - 1, P], [2, P - 2, P],
        [top, top, 0xFFFFFFFF], [top + 1, top - 1, 0xFFFFFFFF], [top + 2, top - 2, 0xFFFFFFFF]]


def test_a_count_of_all_ones_is_over_every_max_count(ctx):
    src = np.ones((8, 1), dtype=np.uint32)
    src[5, 0] = 0xFFFFFFFF
    with pytest.raises(TsError) as e:
        expand(ctx, ExpandSpec(1, 1, count=col(0), max_count=1 << 27, terms=[J]), src)
    assert e.value.code == TS_ERR_INVARIANT, str(e.value)
    assert f"expand: row 5 asks for {(1 << 28) - 3} rows, max_count {1 << 27}" in str(e.value), str(e.value)


# ------------------------------------------------------------------ 4. the knob changes no word
CASE_ROWS = xc.random_rows(42, N, 6)
CASE_SPEC = xc.random_spec(42, 6, 9, kinds=[7, 1, 2, 3, 4, 5, 6, 0, 7])
_case = {}


def case_reference():
    if not _case:
        _case["want"] = xc.reference(CASE_SPEC, CASE_ROWS)
    return _case["want"]


@pytest.mark.parametrize("block_rows", [1, 2, 63, 64, 65, 255, 256, 1024])
def test_same_words_for_every_block_rows(ctx, monkeypatch, block_rows):
    """4096 rows: with 1 row per workgroup there are 4096 blocks and 16 trips of the offsets loop, so the carry is
    crossed, and every output row is a tile of its own; 63, 65 and 255 leave short last blocks and tiles that straddle
    blocks; 2, 63 and 64 keep one row per lane, 65 to 256 cross the wave, 1024 gives a lane four rows."""
    want, want_live = case_reference()
    monkeypatch.setenv(KNOB, str(block_rows))
    got, live = expand(ctx, CASE_SPEC, CASE_ROWS)
    same(got, want, f"{KNOB}={block_rows}")
    assert live == want_live


@pytest.mark.parametrize("value", ["0", "1025", "-1", "x"])
def test_knob_outside_its_range_is_refused(ctx, monkeypatch, value):
    monkeypatch.setenv(KNOB, value)
    with pytest.raises(TsError, match=r"TS_EXPAND_BLOCK_ROWS must be in \[1, 1024\]"):
        expand(ctx, CASE_SPEC, CASE_ROWS[:16])


def test_knob_too_small_for_the_heights_is_refused(ctx, monkeypatch):
    """One launch takes fewer than 2^32 threads, so a grid stays below 2^24 workgroups of 256 lanes: 2^24 source rows
    with one row per block are refused before any device work; 2^12 rows asking for 2^12 each are 2^24 tiles of one
    output row and are refused after the wait, with every block given back; with 2 per block both are taken."""
    src = np.zeros((1 << 24, 1), dtype=np.uint32)
    src[::1 << 12] = 1
    d = ts.DeviceMatrix.upload(ctx, src)
    spec = ExpandSpec(1, 2, count=col(0), max_count=1, terms=[ROW, J])
    tall = np.full((1 << 12, 1), 1 << 12, dtype=np.uint32)
    d_tall = ts.DeviceMatrix.upload(ctx, tall)
    tall_spec = ExpandSpec(1, 1, count=col(0), max_count=1 << 12, terms=[J])
    monkeypatch.setenv(KNOB, "1")
    with pytest.raises(TsError, match="TS_EXPAND_BLOCK_ROWS is too small for a source or a result of this height"):
        ts.expand_rows(ctx, spec, d)
    before = ctx.stat(STAT_LIVE_BLOCKS)
    with pytest.raises(TsError, match="TS_EXPAND_BLOCK_ROWS is too small for a source or a result of this height"):
        ts.expand_rows(ctx, tall_spec, d_tall)
    assert ctx.stat(STAT_LIVE_BLOCKS) == before
    monkeypatch.setenv(KNOB, "2")
    got, live = ts.expand_rows(ctx, spec, d)
    assert live == 1 << 12
    want = np.stack([np.arange(0, 1 << 24, 1 << 12, dtype=np.uint32), np.zeros(1 << 12, dtype=np.uint32)], axis=1)
    same(got.download(), want)
    got, live = ts.expand_rows(ctx, tall_spec, d_tall)
    assert live == 1 << 24 and (got.download()[:, 0] == np.arange(1 << 24) % (1 << 12)).all()


# ------------------------------------------------------------------ 5. heights and the late refusals
def _refused(own, spec, d, out_height, status, text, live_before):
    """A refused call on the context `own`: the status, the whole text, no handle, no rows, every pool block back."""
    t = spec.words()
    out, n_live = C.c_void_p(12345), C.c_uint64(77)
    st = own._l.ts_matrix_expand_rows(own.h, t.ctypes.data_as(ts._lib.u32p), len(t), d.h, out_height, C.byref(out),
                                      C.byref(n_live))
    assert st == status and own._l.ts_last_error(own.h).decode() == text, own._l.ts_last_error(own.h)
    assert not out.value and n_live.value == 0, "a refused call left a handle"
    assert own.stat(STAT_LIVE_BLOCKS) == live_before, "a refused call kept pool blocks"


def test_out_heights_and_the_refusals_return_every_block(ctx):
    counts = np.where(ROWS % 4 == 0, 2, 0)  # 2048 rows asked for
    spec = PATTERN_SPEC
    got, live = check(ctx, spec, _pattern(counts), out_height=2048, what="out_height = n_live: no pad row")
    assert live == 2048 and got.shape[0] == 2048
    got, _ = check(ctx, spec, _pattern(counts), out_height=4096, what="out_height = 2 n_live")
    assert (got[2048:] == spec.pad).all()
    counts[5] = 1  # 2049
    odd = _pattern(counts)
    check(ctx, spec, odd, out_height=0, what="one more: 4096 rows, 2047 of them pad")
    # the refusals after the wait, on a context of its own: its pool holds only what this test took and gave back
    own = ts.Context(0)
    d = ts.DeviceMatrix.upload(own, odd)
    live_before = own.stat(STAT_LIVE_BLOCKS)
    assert live_before >= 1, "the source is a live block"
    reserved = []
    for _ in range(4):
        _refused(own, spec, d, 2048, TS_ERR_INVALID, "expand: 2049 rows asked for, out_height 2048", live_before)
        reserved.append(own.stat(STAT_POOL_BYTES))
    # and every further refused call finds all its blocks in the pool: a kept one would have to be reserved anew
    assert reserved[1:] == reserved[:-1], "a refused call kept pool blocks"
    for bad in (3, 1 << 28):
        with pytest.raises(TsError, match="neither 0 nor a power of two"):
            ts.expand_rows(own, spec, d, bad)
        assert own.stat(STAT_LIVE_BLOCKS) == live_before
    d_out, _ = ts.expand_rows(own, spec, d)
    assert own.stat(STAT_LIVE_BLOCKS) == live_before + 1, "an accepted call keeps its result and nothing else"
    same(d_out.download(), xc.reference(spec, odd)[0], "the matrix still expands")


@pytest.mark.parametrize("block_rows", [None, 1, 100])
def test_the_least_row_over_max_count_is_named(monkeypatch, block_rows):
    """Two offenders, in different blocks and lanes for every knob; the lower one is named with its count, and wins over
    the total, which is over the height as well."""
    from tapstark_amd.build import build

    build()
    if block_rows:
        monkeypatch.setenv(KNOB, str(block_rows))
    counts = np.ones(N, int)
    counts[[1717, 3000]] = [P + 9, 8]  # (9 after reduction)
    counts[1716] = 7
    src = _pattern(counts)
    src[1000, 0] = 0  # takes no part: its count is not looked at
    src[1000, 1] = 100
    own = ts.Context(0)
    d = ts.DeviceMatrix.upload(own, src)
    live_before = own.stat(STAT_LIVE_BLOCKS)
    spec = ExpandSpec(4, 2, count=col(1), when=col(0), max_count=7, terms=[ROW, J])
    for out_height in (0, 1024):
        _refused(own, spec, d, out_height, TS_ERR_INVARIANT, "expand: row 1717 asks for 9 rows, max_count 7", live_before)
    with pytest.raises(ValueError, match="row 1717 asks for 9 rows, max_count 7"):
        xc.reference(spec, src, 1024)
    src[1717, 1] = 1
    with pytest.raises(TsError, match="expand: row 3000 asks for 8 rows, max_count 7"):
        ts.expand_rows(own, spec, ts.DeviceMatrix.upload(own, src))


@pytest.mark.parametrize("rows,each,block_rows", [(64, 1 << 26, 1), (1024, 1 << 22, None)])
def test_a_total_past_32_bits_is_refused_exactly(monkeypatch, rows, each, block_rows):
    """64 rows of 2^26 with one row per block wrap a 32-bit carry across blocks; 1024 rows of 2^22 in one block wrap a
    32-bit position inside the block.  Both ask for 2^32 rows, which a 32-bit sum reads as 0: the call is refused with
    the exact number.  An ordinary error return: nothing is written."""
    from tapstark_amd.build import build

    build()
    if block_rows:
        monkeypatch.setenv(KNOB, str(block_rows))
    own = ts.Context(0)
    d = ts.DeviceMatrix.upload(own, np.full((rows, 1), each, dtype=np.uint32))
    live_before = own.stat(STAT_LIVE_BLOCKS)
    spec = ExpandSpec(1, 1, count=col(0), max_count=1 << 27, terms=[J])
    assert rows * each == 4294967296
    _refused(own, spec, d, 0, TS_ERR_INVALID, "expand: 4294967296 rows asked for, out_height 134217728", live_before)
    _refused(own, spec, d, 1 << 10, TS_ERR_INVALID, "expand: 4294967296 rows asked for, out_height 1024", live_before)


def test_refusals_leave_no_handle(ctx):
    src = xc.random_rows(4, 16, 4)
    d = ts.DeviceMatrix.upload(ctx, src)
    good = ExpandSpec(4, 2, count=col(1), when=col(0), max_count=7, terms=[ROW, J])
    lib, out, live = ctx._l, C.c_void_p(), C.c_uint64()

    def refused(text, spec=good, ctx_h=ctx.h, handle=d.h, out_p=C.byref(out), live_p=C.byref(live)):
        out.value = 12345
        t = spec.words() if spec is not None else None
        st = lib.ts_matrix_expand_rows(ctx_h, t.ctypes.data_as(ts._lib.u32p) if t is not None else None,
                                       len(t) if t is not None else 0, handle, 0, out_p, live_p)
        assert st == 1 and text in lib.ts_last_error(ctx_h).decode(), lib.ts_last_error(ctx_h)
        assert not out.value, "a refused call left a handle"

    refused("null argument", spec=None)
    refused("null argument", handle=None)
    refused("null argument", live_p=None)
    t = good.words()
    assert lib.ts_matrix_expand_rows(ctx.h, t.ctypes.data_as(ts._lib.u32p), len(t), d.h, 0, None, C.byref(live)) == 1
    refused("written for a source of 5 columns, this one has 4",
            spec=ExpandSpec(5, 2, count=col(1), when=col(0), max_count=7, terms=[ROW, J]))
    refused("the count column is outside the source", spec=ExpandSpec(4, 1, count=col(4), max_count=7, terms=[1]))
    other = ts.Context(0)
    refused("made on this context", ctx_h=other.h)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 1), ctx)
    consumed = ts.DeviceMatrix.upload(ctx, src)
    _, consumed_data = pcs.commit([((4, 1), consumed)])
    refused("unconsumed", handle=consumed.h)
    same(ts.expand_rows(ctx, good, d)[0].download(), xc.reference(good, src)[0], "the matrix still expands")


# ------------------------------------------------------------------ 6. pool poison
def test_pool_poison_changes_nothing():
    """Every out word -- pad rows included -- every in-block position, block offset and offender word is written by the
    kernels before it is read: the same matrices on a clean context and on contexts whose pool hands out blocks full of
    0x00000001 and 0xFFFFFFFF (which fill blocks meanwhile: stat 9 is above 0 there)."""
    from tapstark_amd.build import build

    build()
    trio = _poison.make_contexts()
    cases = []
    for seed in (3, 7):
        src = xc.random_rows(seed, 1 << 11, 5, density=0.3)
        cases.append((xc.random_spec(seed, 5, 6), src))
    quiet = np.zeros((1 << 10, 2), dtype=np.uint32)
    cases.append((ExpandSpec(2, 3, count=col(1), when=col(0), max_count=1, pad=[9, 8, 7], terms=[1, 2, 3]), quiet))
    skew = np.zeros((1 << 10, 2), dtype=np.uint32)
    skew[700] = (1, 3000)
    cases.append((ExpandSpec(2, 3, count=col(1), when=col(0), max_count=3000, pad=[9, 8, 7], terms=[ROW, J, LAST]), skew))

    def run(c):
        out = []
        for spec, src in cases:
            for out_height in (0, 1 << 14):
                m, live = ts.expand_rows(c, spec, ts.DeviceMatrix.upload(c, src), out_height)
                out += [m.download(), live]
        return out

    want = []
    for spec, src in cases:
        for out_height in (0, 1 << 14):
            want += list(xc.reference(spec, src, out_height))
    _poison.same_everywhere(trio, run, want=want, what="expand")
    assert all(c.stat(_poison.STAT_FILLS) > 0 for c in trio[1:])


# ------------------------------------------------------------------ 7. the chip table of a span statement
N_CALLS, MAX_LEN, TABLE = 1 << 8, 7, 1 << 6
CHALLENGES = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)


def _range_table(ctx, d_chip, height):
    index = DeriveBuilder(2)
    index.output(index.row(), 0)
    d_rng = ts.DeviceMatrix.upload(ctx, np.zeros((height, 2), dtype=np.uint32)).derive(index)  # (zeros: no trace)
    fill_span_range_multiplicities(d_rng, d_chip, allow_missing=True)
    return d_rng


def _statement(ctx, calls):
    """expand -> derive -> multiplicities: the three resident traces, the tables with their AIRs, n_live."""
    d_calls = ts.DeviceMatrix.upload(ctx, calls)
    d_chip, n_live = span_chip_table(ctx, d_calls, max_len=MAX_LEN)
    d_rng = _range_table(ctx, d_chip, TABLE)
    airs = [SpanCallAir(), SpanChipAir(), BusRangeAir()]
    heights = [len(calls), d_chip.dims()[0], TABLE]
    tabs = [bc.Table(a, np.zeros((h, a.width()), dtype=np.uint32)) for a, h in zip(airs, heights)]
    return [d_calls, d_chip, d_rng], tabs, n_live


def test_span_statement_is_proved_without_the_chip_table_leaving_hbm(ctx):
    calls = generate_span_call_trace(N_CALLS, MAX_LEN, TABLE, 5)
    A, T = SpanCallAir, SpanChipAir
    assert 0 < calls[:, A.SEL].sum() < N_CALLS
    traces, tabs, n_live = _statement(ctx, calls)
    chip = generate_span_chip_trace(calls)
    same(traces[1].download(), chip, "the chip table made in HBM against the host's")
    assert n_live == int(calls[calls[:, A.SEL] == 1][:, A.LEN].sum()) == int(chip[:, T.LIVE].sum())
    rng = traces[2].download()
    counts = np.bincount(chip[:n_live, T.ADDR], minlength=TABLE)
    assert (rng[:, 0] == np.arange(TABLE)).all() and (rng[:, 1] == (P - counts) % P).all()
    cairs = bc.compiled(ctx, tabs)
    pis, logups = [t.pis for t in tabs], [t.logup for t in tabs]
    bad, fv, rep = ts.check_multi(None, cairs, traces, pis, logups, CHALLENGES, ctx=ctx)
    assert (bad, fv) == (-1, -1) and rep.balanced
    config = bc.config(ctx, 1)
    proof = ts.prove_multi_bus(config, cairs, ts.BfChallenger(), traces, pis, logups)
    bc.verify(config, tabs, proof)  # raises unless accepted with the bus sum at zero
    host = ts.prove_multi_bus(config, cairs, ts.BfChallenger(), [calls.copy(), chip.copy(), rng.copy()], pis, logups)
    assert len(proof.words) > 1000 and np.array_equal(proof.words, host.words), "the proof from the host-made tables"


def test_span_past_the_range_table_is_named(ctx):
    A = SpanCallAir
    calls = generate_span_call_trace(N_CALLS, MAX_LEN, TABLE, 5)
    row = int(np.flatnonzero((calls[:, A.SEL] == 1) & (calls[:, A.LEN] >= 2))[3])
    calls[row, A.BASE] = TABLE + 1 - calls[row, A.LEN]  # its last element is address TABLE, the first outside
    traces, tabs, _ = _statement(ctx, calls)
    cairs = bc.compiled(ctx, tabs)
    bad, fv, rep = ts.check_multi(None, cairs, traces, [t.pis for t in tabs], [t.logup for t in tabs], CHALLENGES, ctx=ctx)
    assert (bad, fv) == (-1, -1), "every constraint holds: the chip is made from the calls"
    assert not rep.balanced and rep.n_unbalanced == 1
    assert list(rep.tuple[:rep.n_values]) == [BUS_TAG, TABLE] and rep.sum == 1 and rep.first[0] == 1


def test_cpp_span_chip_resident_example(ctx, tmp_path):
    """examples/span_chip_resident.cpp: the chip table expanded from a call trace, proved and verified; one span
    past the range table named."""
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "span_chip_resident")
    source = os.path.join(ROOT, "examples", "span_chip_resident.cpp")
    text = open(source).read()
    # two uploads in the text: the call trace -- the only trace -- and a matrix of zeros the range table is derived from
    assert "ts_matrix_expand_rows(" in text and text.count("ts_matrix_upload(") == 2
    assert "ts_matrix_upload(ctx, trace.data()" in text and "ts_matrix_upload(ctx, zeros.data()" in text
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source,
                           "-L", libdir, "-ltapstark_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "32 call rows, " in r.stdout and "rows x 8 expanded in HBM" in r.stdout
    assert "verify -> 0, bus sum zero" in r.stdout
    assert "constraints hold in every table; 1 tuple out of balance" in r.stdout and "sent (7, " in r.stdout
    assert r.stdout.rstrip().endswith("span_chip_resident: as expected")
