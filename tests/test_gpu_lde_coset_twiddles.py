"""The coset LDE with the coset's factor in the twiddles (csrc/ntt_lde.hip: k_lde_mid, k_lde_fwd_contig).

coset_lde multiplies coefficient k by shift^k / n once and runs the forward passes of coset beta with block
beta's twiddles of the N-point transform (stage base log_blowup, chunk index beta).  Every case compares the
result word for word with the CPU oracle's coset_lde_batch, at the smallest height of each code path:

    2^1, 2^3     single launch; the stage base alone decides the twiddle index
    2^12         the largest single-launch height
    2^13         the first two-pass height: run-time plan with one strided stage
    2^16         run-time plan, several strided rounds
    2^20         the fixed plan
    2^21         the fixed plan on 2^13-element chunks (blowup 2 only)

Blowups 1 (one coset: base stage 0), 2, 4 and 8 (more cosets than a radix-16 group has stages below it); 2 and 4 at
2^20.  Shifts: 31 (no block of the LDE is the input), 1 (block 0 is, and the scale is the constant 1/n), the shift
that makes block 1 of a blowup of 2 the input, and 7 (an ordinary shift with a table).

The second test proves a 2^13 x 3 SynthMulAir at log_blowup 2 with TS_LDE_OWN_COSET 0 and 1 against the oracle's
prove: its two quotient chunks go through the two-matrix launch, whose shifts -- and scale tables -- differ."""
import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd.airs import SynthMulAir, generate_synth_mul_trace

pytestmark = pytest.mark.gpu
P = 0x78000001
G27 = 0x1A427A41
NO_PIS = np.zeros(0, dtype=np.uint32)


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def own_shift_b1(log_n):
    """the shift for which block 1 of a blowup of 2 is the input: w_2n^-1 (test_gpu_lde_own_coset.py own_shift)"""
    w = pow(G27, 1 << (27 - (log_n + 1)), P)
    return pow(w, P - 2, P)


HEIGHTS = [(1, 2), (3, 3), (12, 5), (13, 3), (16, 4), (20, 2), (21, 1)]


def blowups(log_n):
    return (1,) if log_n == 21 else (1, 2) if log_n == 20 else (0, 1, 2, 3)


CASES = [(log_n, w, b) for log_n, w in HEIGHTS for b in blowups(log_n)]
_inputs = {}


def lde_input(ctx, log_n, w):
    """one random matrix per height, uploaded once and left as it is"""
    if log_n not in _inputs:
        x = np.random.default_rng(4200 + log_n).integers(0, P, size=(1 << log_n, w), dtype=np.uint32)
        _inputs[log_n] = (x, ts.DeviceMatrix.upload(ctx, x))
    return _inputs[log_n]


@pytest.mark.parametrize("log_n,w,b", CASES, ids=[f"2p{h}x{w}-b{b}" for h, w, b in CASES])
def test_coset_lde_is_the_oracles(ctx, orc, log_n, w, b):
    dft = ts.Radix2Dft(ctx)
    x, dx = lde_input(ctx, log_n, w)
    for shift in (31, 1, own_shift_b1(log_n), 7):
        got = dft.coset_lde_batch(dx, b, shift).download()
        want = orc.coset_lde_batch(x, b, shift)
        assert got.shape == want.shape == ((1 << log_n) << b, w)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"shift {shift}: {len(bad)} words differ, the first at (row, column) {tuple(bad[0])}"


def test_chunk_pair_with_two_shifts(ctx, orc, monkeypatch):
    air, trace = SynthMulAir(3), generate_synth_mul_trace(1 << 13, 3)
    tape = ts.air_tape(air, 0)
    cfg = (2, 5, 4)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))
    want = orc.prove(orc.FriConfig(*cfg), tape, trace, NO_PIS)
    monkeypatch.setenv("TS_REDUCE_LOW", "0")
    for knob in ("0", "1"):
        monkeypatch.setenv("TS_LDE_OWN_COSET", knob)
        ctx.set_kernel_timing(True)
        try:
            ctx.take_kernel_timings()
            got = ts.prove(config, air, ts.BfChallenger(), trace.copy(), NO_PIS).words
            ran = {k: v[0] for k, v in ctx.take_kernel_timings().items()}
        finally:
            ctx.set_kernel_timing(False)
        # the trace and the chunk pair in ONE launch set (the reduced opening is not extended by LDE here)
        assert sum(v for k, v in ran.items() if "k_lde_mid" in k) == 2, ran
        assert len(got) == len(want) and (got == want).all(), \
            f"TS_LDE_OWN_COSET={knob}: {int((got != want).sum())} proof words differ from the oracle's"
