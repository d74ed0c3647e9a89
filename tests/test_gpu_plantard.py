"""The Plantard twiddle form on the device (csrc/bb.hpp plant_mul, csrc/ntt_rounds.hpp on the uint2 tables):

  * the DEVICE build of the product and radix_butterflies<4, INV, TOP> on a Plantard table, against plain Python
    integers (tests/_plantard_cases.py).  The field probe runs ONCE per module, as a child process with its own
    time limit; if it fails the fixture fails and nothing starts it again;
  * whole transforms through ts_coset_lde_batch and ts_dft_batch against the CPU oracle, at the smallest heights
    that reach each code path: 2^6 and 2^12 (the strided kernel alone), 2^13 (three passes, run-time plan),
    2^20 (the fixed 256-row plan, the 4096-element contiguous kernels), the extension by one bit on the shifts 31
    and 1 (shift 1: block 0 of the result is the input, copied, and the passes step over it); and the transpose
    with the first inverse round folded in, through a commit of a 2^20 x 16 row-major matrix.

All comparisons are exact.  (The CPU oracle takes about 1.5 s for a 2^20 x 2 extension, so every kind of matrix is
kept at that height.)"""
import functools

import numpy as np
import pytest

import _plantard_cases as pc
import tapstark_amd as ts
from _field_cases import EXTREME_KINDS, extreme_mat

pytestmark = pytest.mark.gpu
P = pc.P


# ------------------------------------------------------------------ the product and the register butterflies
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return pc.run_probe(str(tmp_path_factory.mktemp("plantard_device")), device=True)


def test_device_p_inv64(probe):
    records, _, results = probe
    pc.check_plant_consts(records["plant_consts"][2], results["plant_consts"])


def test_device_plant_const(probe):
    records, _, results = probe
    pc.check_plant_const(records["plant_const"][2], results["plant_const"])


def test_device_plant_mul(probe):
    records, _, results = probe
    pc.check_plant_mul(records["plant_mul"][2], results["plant_mul"])


@pytest.mark.parametrize("name", pc.DEVICE_ONLY)
def test_device_plantard_butterflies(probe, name):
    records, tables, results = probe
    pc.check_bfly(name, records[name][2], tables[name], results[name])


# ------------------------------------------------------------------ whole transforms
@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(scope="module")
def dft(ctx):
    return ts.Radix2Dft(ctx)


def matrix(kind, h, w):
    if kind == "random":
        return np.random.default_rng(2024 + h).integers(0, P, size=(h, w), dtype=np.uint32)
    return extreme_mat(kind, h, w)


@functools.lru_cache(maxsize=2)
def bitrev_index(log_h):
    idx = np.arange(1 << log_h, dtype=np.uint32)
    out = np.zeros_like(idx)
    for b in range(log_h):
        out |= ((idx >> np.uint32(b)) & np.uint32(1)) << np.uint32(log_h - 1 - b)
    return out


def same(a, b):
    return a.shape == b.shape and bool((a == b).all())


@pytest.mark.parametrize("kind", EXTREME_KINDS + ["random"])
@pytest.mark.parametrize("log_n", [6, 12, 13, 20])
def test_transforms_match_the_oracle(ctx, dft, orc, log_n, kind):
    x = matrix(kind, 1 << log_n, 2)
    dm = ts.DeviceMatrix.upload(ctx, x)
    for shift in (31, 1):
        got = dft.coset_lde_batch(dm, 1, shift).download()
        assert same(got, orc.coset_lde_batch(x, 1, shift)), f"coset_lde_batch shift {shift}"
    assert same(dft.dft_batch(dm).download(), orc.dft_batch(x)), "dft_batch"
    assert same(dft.idft_batch(dm).download(), orc.dft_batch(x, inverse=True)), "idft_batch"
    assert same(dm.download(), x), "the input matrix was modified"


def test_commit_with_the_fused_first_round(ctx, orc):
    """Pcs::commit on the trace domain extends on the shift 31, which is no coset of the LDE's own: the transpose
    takes the first inverse round (k_transpose_bitrev_r16) and the contiguous inverse pass starts a round later."""
    x = matrix("random", 1 << 20, 16)
    x[0, :], x[-1, :], x[1, 0] = P - 1, 0, P - 1
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 1, 0), ctx)
    _, data = pcs.commit([((20, 1), x.copy())])
    lde = data.lde(0)
    del data
    assert same(lde, orc.coset_lde_batch(x, 1, 31)[bitrev_index(21)])
