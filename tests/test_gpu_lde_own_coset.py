"""The block of a coset LDE that is the LDE's own input (csrc/ntt_plan.hpp lde_own_coset; ntt_lde.hip coset_lde,
k_lde_own_copy, the block-skipping k_lde_mid and k_lde_fwd_contig_own).

Where shift * w_N^bitrev_b(beta) = 1, block beta of the LDE holds the input itself.  coset_lde copies it there and
leaves it out of its passes; TS_LDE_OWN_COSET=0 makes it compute every block, as it always did.  Both give the same
words, so every case below compares the two word for word, and the kernel timers show which launches ran.

Small heights are downloaded and compared as arrays.  From 2^20 rows up the standalone LDE's result stays in HBM
and is compared through the Merkle root of the Blake3 MMCS over the matrix as it stands (a digest of every word),
and so is its block beta against the bit-reversed input; committed LDEs are downloaded at every height."""
import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd.airs import (HighDegreeAir, SynthMulAir, generate_high_degree_trace, generate_synth_mul_trace)

pytestmark = pytest.mark.gpu
P = 0x78000001
G27 = 0x1A427A41
NO_PIS = np.zeros(0, dtype=np.uint32)
KNOB = "TS_LDE_OWN_COSET"
COPY = "k_lde_own_copy"


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def rand_mat(seed, h, w):
    return np.random.default_rng(seed).integers(0, P, size=(h, w), dtype=np.uint32)


def bitrev(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2) if bits else 0


def bitrev_perm(bits):
    i = np.arange(1 << bits, dtype=np.int64)
    r = np.zeros_like(i)
    for k in range(bits):
        r |= ((i >> k) & 1) << (bits - 1 - k)
    return r


def own_shift(log_n, b, beta):
    """the shift for which block beta is the input: w_N^(-bitrev_b(beta))"""
    w = pow(G27, 1 << (27 - (log_n + b)), P)
    return pow(w, (P - 1 - bitrev(beta, b)) % (P - 1), P)


def launches(ctx, run):
    """run()'s result and {kernel-timer name: launches}"""
    ctx.set_kernel_timing(True)
    try:
        ctx.take_kernel_timings()
        out = run()
        t = ctx.take_kernel_timings()
    finally:
        ctx.set_kernel_timing(False)
    return out, {k: v[0] for k, v in t.items()}


def root_of(ctx, m):
    """Merkle root over the rows of a device matrix (which is consumed)"""
    return ts.Blake3Mmcs(ctx).commit([m])[0]


# one input per height, shared by every (blowup, beta) of that height.  2^10 and 2^12: the single-launch k_lde_mid;
# 2^13: the first three-pass height, run-time round plan; 2^20: the fixed plan; 2^21 and 2^22: the fixed plan on
# 2^13 and 2^14 chunks, the latter with four chunks per workgroup of the forward pass.
# Widths that are no multiple of four at the small heights, 4 (16 .. 64 MB) at the large ones.
HEIGHTS = [(10, 3), (12, 5), (13, 3), (20, 4), (21, 4), (22, 4)]
_inputs = {}


def lde_input(ctx, log_n, w):
    if log_n not in _inputs:
        x = rand_mat(100 + log_n, 1 << log_n, w)
        _inputs[log_n] = (x, ts.DeviceMatrix.upload(ctx, x))
    return _inputs[log_n]


@pytest.mark.parametrize("log_n,w", HEIGHTS, ids=[f"2p{h}x{w}" for h, w in HEIGHTS])
def test_every_own_block_of_every_plan(ctx, monkeypatch, log_n, w):
    dft = ts.Radix2Dft(ctx)
    x, dx = lde_input(ctx, log_n, w)
    n, big = 1 << log_n, log_n >= 20
    xr = dx.bit_reverse_rows()  # what an own block holds when the result's rows are bit-reversed
    want_block = root_of(ctx, ts.DeviceMatrix.from_device_ptr(ctx, xr.device_ptr(), n, w)) if big else xr.download()
    for b in (1, 2, 3):
        for beta in range(1 << b):
            shift = own_shift(log_n, b, beta)
            res = {}
            for knob in ("0", "1"):
                monkeypatch.setenv(KNOB, knob)
                lde, ran = launches(ctx, lambda: dft.coset_lde_batch(dx, b, shift, bit_reversed=True))
                assert ran.get(COPY, 0) == int(knob), (b, beta, knob, ran)
                assert lde.dims() == (n << b, w)
                block = ts.DeviceMatrix.from_device_ptr(ctx, lde.device_ptr() + 4 * w * beta * n, n, w)
                res[knob] = (root_of(ctx, block), root_of(ctx, lde)) if big else (block.download(), lde.download())
            for k in (0, 1):
                assert (res["1"][k] == res["0"][k]).all(), f"b={b} beta={beta}: the copied block's LDE differs"
            assert (res["1"][0] == want_block).all(), f"b={b} beta={beta}: block beta is not the input"
    assert (dx.download() == x).all()  # the input is left as it was


def test_own_block_lde_is_the_oracles(ctx, orc, monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    dft = ts.Radix2Dft(ctx)
    x = rand_mat(7, 1 << 10, 3)
    for b, beta in ((1, 1), (2, 0), (2, 3), (3, 5)):
        shift = own_shift(10, b, beta)
        assert (dft.coset_lde_batch(x, b, shift).download() == orc.coset_lde_batch(x, b, shift)).all(), (b, beta)
    assert (dft.lde_batch(x, 2).download() == orc.coset_lde_batch(x, 2, 1)).all()


@pytest.mark.parametrize("log_n", [10, 13, 20])
def test_no_own_block_launches_what_it_always_did(ctx, monkeypatch, log_n):
    """shift 31 (the trace commit's): no coset of the LDE is H_n, and the knob changes no launch"""
    dft = ts.Radix2Dft(ctx)
    _, dx = lde_input(ctx, log_n, dict(HEIGHTS)[log_n])
    ran = {}
    dft.coset_lde_batch(dx, 2, 31)  # the context builds and keeps the scale table of a shape on first use
    for knob in ("0", "1"):
        monkeypatch.setenv(KNOB, knob)
        lde, ran[knob] = launches(ctx, lambda: dft.coset_lde_batch(dx, 2, 31, bit_reversed=True))
        del lde
    assert ran["1"] == ran["0"] and COPY not in ran["1"], ran
    if log_n >= 13:
        assert any(k.startswith("k_transpose_bitrev_r16") for k in ran["1"]), ran  # the fused first round stays
    # a blowup of 1 (one coset, which shift 1 makes the input) has nothing to leave out
    monkeypatch.setenv(KNOB, "1")
    _, ran1 = launches(ctx, lambda: dft.coset_lde_batch(dx, 0, 1))
    assert COPY not in ran1, ran1


def chunk_case(name, n):
    if name == "mul5":  # degree 3: two chunks, one pair launch
        return SynthMulAir(5), generate_synth_mul_trace(n, 5), 2
    return HighDegreeAir(5), generate_high_degree_trace(n), 4  # four chunks, a launch set each


@pytest.mark.parametrize("name,log_n", [("mul5", 13), ("mul5", 20), ("deg5", 13), ("deg5", 20)])
def test_quotient_chunk_commit(ctx, monkeypatch, name, log_n):
    """The quotient chunks, column-major as the quotient kernel leaves them, committed on their own domains
    31 w_{n qd}^c.  The LDE shift of chunk c is w_{n qd}^-c = w_N^-(c << (b - lqd)), so block
    bitrev_b(c << (b - lqd)) of its LDE is the chunk: blocks 0 and 1 for the two chunks of the flagship."""
    air, trace, qd = chunk_case(name, 1 << log_n)
    b = 2
    n = 1 << log_n
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0))
    assert 1 << cair.log_quotient_degree == qd
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(b, 4, 8), ctx)
    _, tdata = pcs.commit([((log_n, 1), trace)])
    g = pow(G27, 1 << (27 - (log_n + cair.log_quotient_degree)), P)
    shifts = [31 * pow(g, c, P) % P for c in range(qd)]
    alpha = rand_mat(5, 1, 4)[0]
    got = {}
    for knob in ("0", "1"):
        monkeypatch.setenv(KNOB, knob)
        chunks = pcs.quotient_chunks(tdata, cair, NO_PIS, alpha)
        vals = [c.download() for c in chunks] if knob == "1" else None
        (root, data), ran = launches(ctx, lambda: pcs.commit([((log_n, s), c) for s, c in zip(shifts, chunks)]))
        mids = sum(v for k, v in ran.items() if "k_lde_mid" in k)
        assert mids == (1 if qd == 2 else qd), ran  # two chunks: the pair launch
        assert ran.get(COPY, 0) == (mids if knob == "1" else 0), ran
        got[knob] = (root, [data.lde(c) for c in range(qd)], vals)
    assert (got["1"][0] == got["0"][0]).all(), "commitment differs"
    for c in range(qd):
        on, off = got["1"][1][c], got["0"][1][c]
        assert on.shape == (n << b, 4) and (on == off).all(), f"chunk {c}: {int((on != off).sum())} LDE words differ"
        beta = bitrev(c << (b - cair.log_quotient_degree), b)
        own = on[beta * n:(beta + 1) * n]  # row t of a block: the chunk's row bitrev(t)
        assert (own == got["1"][2][c][bitrev_perm(log_n)]).all(), f"chunk {c}: block {beta} is not the chunk"


@pytest.mark.parametrize("log_n", [6, 10, 13])
def test_whole_proofs(ctx, orc, monkeypatch, log_n):
    """The flagship's AIR: the chunk pair and the reduced opening each copy one block, and the proof is the
    proof without the copies and the oracle's."""
    monkeypatch.setenv("TS_REDUCE_LOW", "1")
    air, trace = SynthMulAir(64), generate_synth_mul_trace(1 << log_n)
    tape = ts.air_tape(air, 0)
    cfg = (2, 5, 4)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))
    proofs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv(KNOB, knob)
        proofs[knob], ran = launches(ctx, lambda: ts.prove(config, air, ts.BfChallenger(), trace.copy(), NO_PIS))
        assert ran.get(COPY, 0) == (2 if knob == "1" else 0), ran
    on, off = proofs["1"].words, proofs["0"].words
    assert len(on) == len(off) and (on == off).all(), f"{int((on != off).sum())} proof words differ"
    want = orc.prove(orc.FriConfig(*cfg), tape, trace, NO_PIS)
    assert len(on) == len(want) and (on == want).all()
    ts.verify(config, air, ts.BfChallenger(), proofs["1"], NO_PIS)
