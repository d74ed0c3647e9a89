"""ts_matrix_sort_rows and ts_matrix_gather_rows on the GPU (csrc/sort.hip): every downloaded matrix is compared word for
word with the numpy reference of tests/_sort_cases.py, and the source is checked unchanged.

Lengths: a sorted length that is no power of two is n_live inside the next power of two with tail rows that would
sort first (tests/_sort_cases.py says why); a power of two is also the whole matrix.

The levels of the count scan: it runs over 256 * workgroups words in tiles of 1024, so it takes its SECOND level from
5 workgroups on and its THIRD from 4097 on; with TS_SORT_BLOCK_ROWS = 1 a workgroup owns one row, so the lengths 4 | 5
and 4096 | 4097 are the last of one level and the first of the next."""
import ctypes as C

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd._lib import TsError

import _poison
import _sort_cases as sc

pytestmark = pytest.mark.gpu
KNOB = "TS_SORT_BLOCK_ROWS"
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099, 8192)
SCAN_LEVEL_EDGES = (4, 5, 4096, 4097)  # at one row per workgroup (see above)


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def run(ctx, src, keys, **kw):
    d = ts.DeviceMatrix.upload(ctx, src)
    out = d.sort_rows(keys, **kw).download()
    assert (d.download() == src).all(), "the source changed"
    return out


def check(ctx, src, keys, what="", **kw):
    got, want = run(ctx, src, keys, **kw), sc.reference(src, keys, **kw)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, not {want.shape}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} words differ, first at (row, column) {bad[0].tolist()}"
    return got


def length_case(length, family="uniform", width=3):
    return sc.tail_case(sc.key_family(family, length), sc.pow2_at_least(length), width)


# ------------------------------------------------------------------ 1. lengths, at every knob value
@pytest.mark.parametrize("block_rows", [1, 4, 64])
@pytest.mark.parametrize("length", LENGTHS)
def test_lengths(ctx, monkeypatch, length, block_rows):
    monkeypatch.setenv(KNOB, str(block_rows))
    src, n_live = length_case(length)
    check(ctx, src, [2], f"length {length}, {block_rows} rows per workgroup", n_live=n_live, source_row=True,
          group_start=True, group_keys=1)


@pytest.mark.parametrize("length", SCAN_LEVEL_EDGES)
def test_scan_level_edges(ctx, monkeypatch, length):
    monkeypatch.setenv(KNOB, "1")
    src, n_live = length_case(length)
    check(ctx, src, [2], f"length {length}, one row per workgroup", n_live=n_live, source_row=True)


def test_default_knob_several_workgroups(ctx, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    src, n_live = length_case((1 << 16) + 1)
    check(ctx, src, [2], "2^16 + 1 rows", n_live=n_live, source_row=True, group_start=True, group_keys=1)


def test_same_matrix_for_every_knob_value(ctx, monkeypatch):
    src, n_live = length_case(1000, "edge_words")
    outs = []
    for value in (None, "1", "3", "64", "255", "256", "257", "2048"):
        if value is None:
            monkeypatch.delenv(KNOB, raising=False)
        else:
            monkeypatch.setenv(KNOB, value)
        outs.append(check(ctx, src, [2], f"knob {value}", n_live=n_live, source_row=True))
    assert all((o == outs[0]).all() for o in outs)


@pytest.mark.parametrize("bad", ["0", "2049", "-1", "x", "1.5"])
def test_invalid_knob_values_are_refused(ctx, monkeypatch, bad):
    monkeypatch.setenv(KNOB, bad)
    with pytest.raises(TsError, match=KNOB):
        run(ctx, sc.matrix(sc.key_family("uniform", 8)), [2])


# ------------------------------------------------------------------ 2. key families
@pytest.mark.parametrize("block_rows", [4, 64, None])
@pytest.mark.parametrize("family", sc.KEY_FAMILIES)
def test_key_families(ctx, monkeypatch, family, block_rows):
    if block_rows is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(block_rows))
    src, n_live = length_case(1000, family)
    got = check(ctx, src, [2], family, n_live=n_live, source_row=True, group_start=True, group_keys=1)
    if family == "all_equal":  # stability: nothing moves
        assert (got[:, 3] == np.arange(src.shape[0])).all()
        assert got[:, 4].sum() == 1


# ------------------------------------------------------------------ 3. several keys, odd columns
@pytest.mark.parametrize("block_rows", [4, None])
@pytest.mark.parametrize("n_keys", [2, 4])
def test_multi_key(ctx, monkeypatch, n_keys, block_rows):
    if block_rows is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(block_rows))
    src, columns = sc.multi_key_case(1 << 10, n_keys)
    for group_keys in (0, 1, n_keys):
        check(ctx, src, columns, f"{n_keys} keys, group_keys {group_keys}", group_keys=group_keys, source_row=True,
              group_start=True)


@pytest.mark.parametrize("width", [1, 3, 17])
def test_key_in_the_last_column(ctx, monkeypatch, width):
    monkeypatch.setenv(KNOB, "64")
    src = sc.matrix(sc.key_family("uniform", 256), width)
    check(ctx, src, [width - 1], f"width {width}", source_row=True, group_start=True, group_keys=1)


# ------------------------------------------------------------------ 4. n_live and the flags
@pytest.mark.parametrize("n_live", [0, 1, 255, 256])
def test_n_live(ctx, monkeypatch, n_live):
    monkeypatch.setenv(KNOB, "64")
    src, _ = sc.tail_case(sc.key_family("uniform", n_live), 256)
    got = check(ctx, src, [2], f"n_live {n_live}", n_live=n_live, source_row=True, group_start=True, group_keys=1)
    assert (got[n_live:, :3] == src[n_live:]).all() and (got[n_live:, 4] == 0).all()


@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("group_keys", [0, 1, 2])
def test_flags(ctx, monkeypatch, flags, group_keys):
    monkeypatch.setenv(KNOB, "64")
    src, columns = sc.multi_key_case(256, 2)
    got = check(ctx, src, columns, f"flags {flags}", group_keys=group_keys, n_live=200, source_row=flags[0],
                group_start=flags[1])
    assert got.shape[1] == src.shape[1] + flags[0] + flags[1]


# ------------------------------------------------------------------ 5. refusals that need a matrix
def test_refusals(ctx):
    src = sc.matrix(sc.key_family("uniform", 16))
    d = ts.DeviceMatrix.upload(ctx, src)
    for what, kw in {"between 1 and 4 keys": dict(keys=[]),
                     "outside the source": dict(keys=[3]),
                     "named twice": dict(keys=[1, 2, 1]),
                     "group_keys": dict(keys=[1], group_keys=2),
                     "n_live": dict(keys=[1], n_live=17)}.items():
        with pytest.raises(TsError, match=what):
            d.sort_rows(**kw)
    with pytest.raises(TsError, match="between 1 and 4 keys"):
        d.sort_rows([0, 1, 2, 0, 1])
    lib = ctx._l
    spec = _lib.SortSpecC(struct_size=C.sizeof(_lib.SortSpecC), n_keys=1, n_live=16)
    out = C.c_void_p()

    def refused(text, spec=spec, ctx_h=ctx.h, src_h=d.h, out_p=C.byref(out)):
        assert lib.ts_matrix_sort_rows(ctx_h, C.byref(spec) if spec is not None else None, src_h, out_p) == 1
        assert text in lib.ts_last_error(ctx_h).decode()
        assert not out.value

    refused("null argument", spec=None)
    refused("null argument", src_h=None)
    refused("null argument", out_p=None)
    refused("struct_size", _lib.SortSpecC(struct_size=8, n_keys=1))
    refused("flag bit", _lib.SortSpecC(struct_size=C.sizeof(_lib.SortSpecC), n_keys=1, flags=4))
    other = ts.Context(0)
    refused("made on this context", ctx_h=other.h)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 2, 1), ctx)
    from tapstark_amd.airs import FibonacciAir, fibonacci_public_values, generate_fibonacci_trace

    consumed = ts.DeviceMatrix.upload(ctx, src)
    _, consumed_data = pcs.commit([((4, 1), consumed)])
    refused("unconsumed", src_h=consumed.h)
    fib = generate_fibonacci_trace(0, 1, 64)
    _, data = pcs.commit([((6, 1), fib)])
    cair = ts.CompiledAir(ctx, ts.air_tape(FibonacciAir(), 3))
    chunk = pcs.quotient_chunks(data, cair, fibonacci_public_values(fib), [1, 2, 3, 4])[0]
    refused("row-major", src_h=chunk.h)
    assert (d.sort_rows([2]).download() == sc.reference(src, [2])).all()  # and the matrix still sorts


# ------------------------------------------------------------------ 6. gather_rows
@pytest.mark.parametrize("index_height", [64, 256, 1024])
def test_gather_rows(ctx, index_height):
    src = _poison.rand_mat(5, 256, 7)
    index = np.random.default_rng(6).integers(0, 256, size=(index_height, 3), dtype=np.uint32)
    index[: index_height // 2, 1] = 9  # repeated indices
    d_src, d_index = ts.DeviceMatrix.upload(ctx, src), ts.DeviceMatrix.upload(ctx, index)
    got = d_src.gather_rows(d_index, column=1).download()
    assert (got == src[index[:, 1]]).all()
    assert (d_src.download() == src).all() and (d_index.download() == index).all()


def test_gather_reorders_a_payload_by_the_source_row_column(ctx):
    keys = sc.matrix(sc.key_family("uniform", 512), 1)
    payload = _poison.rand_mat(8, 512, 20)
    order = ts.DeviceMatrix.upload(ctx, keys).sort_rows([0], source_row=True)
    got = ts.DeviceMatrix.upload(ctx, payload).gather_rows(order, column=1).download()
    assert (got == payload[np.argsort(keys[:, 0], kind="stable")]).all()


def test_gather_refuses_an_index_outside_the_source(ctx):
    src = _poison.rand_mat(5, 64, 2)
    index = np.zeros((128, 1), dtype=np.uint32)
    index[[40, 77, 100], 0] = (64, 1000, 0xFFFFFFFF)
    d_src = ts.DeviceMatrix.upload(ctx, src)
    with pytest.raises(TsError, match="gather: row index 64 at row 40 outside the source"):
        d_src.gather_rows(ts.DeviceMatrix.upload(ctx, index))
    with pytest.raises(TsError, match="index_column"):
        d_src.gather_rows(ts.DeviceMatrix.upload(ctx, index), column=1)


# ------------------------------------------------------------------ 7. the poisoned pool
def test_poisoned_pool(ctx, monkeypatch):
    """The permutation, the carried keys, the count tree and the output come from the pool and are written by the call
    before they are read: the clean context and the two filled ones, first use and recycled blocks, give the
    reference's words, so no poison word reached the output."""
    monkeypatch.setenv(KNOB, "4")
    src, n_live = length_case(1000)
    kw = dict(n_live=n_live, source_row=True, group_start=True, group_keys=1)
    targets = _poison.make_contexts()
    _poison.same_everywhere(targets, lambda c: run(c, src, [2], **kw), want=sc.reference(src, [2], **kw), what="sort")
