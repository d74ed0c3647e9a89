"""GPU tests of the on-device TwoAdicSubgroupDft (ts_dft_batch, ts_coset_lde_batch,
ts_matrix_bit_reverse_rows), Pcs::get_evaluations_on_domain kept on the device and ts_matrix_device_ptr.
Everything is bit-exact against the CPU oracle (oracle/dft.c): no tolerances.

Shapes: every height at which the plan changes -- one kernel (n <= 4096), the first contiguous + strided
plan (2^13), the fixed 256-row strided plan on 2^12 / 2^13 / 2^14-element chunks (2^20 is covered by its
siblings 2^21 and 2^22, which share its kernel) and a generic strided plan in between (2^17) -- times widths
below the 32-column tile, with a remainder, and a multiple of it."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import tapstark_amd as ts
from _field_cases import EXTREME_KINDS, extreme_mat
from tapstark_amd._lib import TsError

pytestmark = pytest.mark.gpu
P = 0x78000001
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

SHAPES = [(lg, w) for lg in (0, 1, 2, 5, 9, 12, 13, 17) for w in (1, 3, 33, 64)] + \
         [(lg, w) for lg in (21, 22) for w in (1, 3)]
SHAPE_IDS = [f"2^{lg}x{w}" for lg, w in SHAPES]
ADDED_BITS = (0, 1, 2, 4)


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


@pytest.fixture(scope="module")
def dft(ctx):
    return ts.Radix2Dft(ctx)


def rand_mat(seed, h, w):
    """Seeded canonical values, some forced to 0 and to p - 1."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, P, size=(h, w), dtype=np.uint32)
    flat = m.reshape(-1)
    k = max(1, flat.size // 16)
    flat[rng.integers(0, flat.size, size=k)] = 0
    flat[rng.integers(0, flat.size, size=k)] = P - 1
    if flat.size >= 2:
        flat[0], flat[-1] = 0, P - 1
    return m


def rand_shift(seed):
    return int(np.random.default_rng(seed).integers(2, P))


def powers(s, n):
    """[s^k mod p for k < n], exact integer arithmetic (products of two values < 2^31 fit 64 bits)."""
    pw = np.ones(n, dtype=np.uint64)
    k, sk = 1, s % P  # sk = s^k
    while k < n:
        pw[k:2 * k] = pw[:k] * np.uint64(sk) % np.uint64(P)
        sk, k = sk * sk % P, 2 * k
    return pw


def scale_rows(m, pw):
    return ((m.astype(np.uint64) * pw[:, None]) % np.uint64(P)).astype(np.uint32)


@functools.lru_cache(maxsize=4)
def bitrev_index(log_h):
    idx = np.arange(1 << log_h, dtype=np.uint32)
    out = np.zeros_like(idx)
    for b in range(log_h):
        out |= ((idx >> np.uint32(b)) & np.uint32(1)) << np.uint32(log_h - 1 - b)
    return out


def oracle_bit_reverse_rows(orc, m):
    m = np.ascontiguousarray(m, dtype=np.uint32).copy()
    orc.lib().ts_or_bit_reverse_rows(m.ctypes.data_as(orc.u32p), C.c_size_t(m.shape[0]), C.c_size_t(m.shape[1]))
    return m


def same(a, b):
    return a.shape == b.shape and bool((a == b).all())


# ------------------------------------------------------------------ dft / idft / coset forms
@pytest.mark.parametrize("log_n,w", SHAPES, ids=SHAPE_IDS)
def test_dft_batch_matches_oracle(ctx, dft, orc, log_n, w):
    check_dft_batch(ctx, dft, orc, log_n, w, rand_mat(1000 + 64 * log_n + w, 1 << log_n, w))


@pytest.mark.parametrize("kind", EXTREME_KINDS)
@pytest.mark.parametrize("log_n,w", [(0, 1), (1, 3), (2, 3), (5, 33)], ids=["2^0x1", "2^1x3", "2^2x3", "2^5x33"])
def test_dft_batch_extreme_matrices(ctx, dft, orc, log_n, w, kind):
    check_dft_batch(ctx, dft, orc, log_n, w, extreme_mat(kind, 1 << log_n, w))


def check_dft_batch(ctx, dft, orc, log_n, w, x):
    n = 1 << log_n
    dm = ts.DeviceMatrix.upload(ctx, x)

    def unchanged():
        assert same(dm.download(), x), "the input matrix was modified"

    want_f, want_i = orc.dft_batch(x), orc.dft_batch(x, inverse=True)
    if log_n <= 8:
        assert same(want_f, orc.naive_dft(x)) and same(want_i, orc.naive_dft(x, inverse=True))
    f = dft.dft_batch(dm)
    assert f.dims() == (n, w)
    assert same(f.download(), want_f), "dft_batch"
    unchanged()
    assert same(dft.idft_batch(dm).download(), want_i), "idft_batch"
    unchanged()
    back = dft.idft_batch(f)
    assert same(back.download(), x), "idft(dft(x)) != x"
    assert same(f.download(), want_f)
    # coset forms: coset_dft(x, s)[k] = sum_j (x_j s^j) w^(jk); coset_idft(y, s)_k = idft(y)_k s^-k
    for shift in (31, rand_shift(77 + log_n)):
        got = dft.coset_dft_batch(dm, shift).download()
        assert same(got, orc.dft_batch(scale_rows(x, powers(shift, n)))), f"coset_dft_batch shift {shift}"
        unchanged()
        got = dft.coset_idft_batch(dm, shift).download()
        assert same(got, scale_rows(want_i, powers(pow(shift, P - 2, P), n))), f"coset_idft_batch shift {shift}"
        unchanged()
    # bit_reverse_rows
    assert same(dm.bit_reverse_rows().download(), oracle_bit_reverse_rows(orc, x))
    unchanged()


# ------------------------------------------------------------------ coset LDE
@pytest.mark.parametrize("shift_kind", ["one", "generator", "random"])
@pytest.mark.parametrize("log_n,w", SHAPES, ids=SHAPE_IDS)
def test_coset_lde_batch_matches_oracle_and_commit(ctx, dft, orc, log_n, w, shift_kind):
    n = 1 << log_n
    shift = {"one": 1, "generator": 31, "random": rand_shift(500 + log_n)}[shift_kind]
    x = rand_mat(3000 + 64 * log_n + w, n, w)
    dm = ts.DeviceMatrix.upload(ctx, x)
    # Row j of coset_lde_batch(x, b, s) is p(s w_{n 2^b}^j), p the interpolant of x over H_n, and
    # w_{n 2^b} = w_{16 n}^(2^(4-b)): the result for b < 4 is every 2^(4-b)-th row of the one for b = 4.  The
    # tall shapes take the oracle's b = 4 result once and slice it; the others ask the oracle for every b
    # (which also checks the slicing rule itself).
    want4 = orc.coset_lde_batch(x, 4, shift)
    for b in ADDED_BITS:
        want = want4[:: 1 << (4 - b)]
        if log_n <= 13:
            direct = orc.coset_lde_batch(x, b, shift)
            assert same(direct, want), "oracle: slicing rule"
        got = dft.coset_lde_batch(dm, b, shift)
        assert got.dims() == (n << b, w)
        assert same(got.download(), want), f"coset_lde_batch added_bits {b} shift {shift}"
        del got
        got_br = dft.coset_lde_batch(dm, b, shift, bit_reversed=True).download()
        if b >= 1:
            # two_adic_pcs.rs:235-239: commit extends on shift = generator / domain.shift and bit-reverses
            domain_shift = 31 * pow(shift, P - 2, P) % P
            pcs = ts.TwoAdicFriPcs(ts.FriConfig(b, 1, 0), ctx)
            _, data = pcs.commit([((log_n, domain_shift), x)])
            lde = data.lde(0)
            del data
            assert same(got_br, lde), f"bit_reversed LDE != ts_pcs_data_lde of the commit, added_bits {b}"
            if log_n + b <= 20:
                assert same(got_br, want[bitrev_index(log_n + b)])
        else:
            assert same(got_br, want[bitrev_index(log_n + b)]), "bit_reversed, added_bits 0"
        assert same(dm.download(), x), "the input matrix was modified"
    if shift == 1:
        assert same(dft.lde_batch(dm, 1).download(), want4[::8])


# ------------------------------------------------------------------ evaluations on domain
def test_evaluations_on_domain_mixed_heights(ctx, orc):
    mats = [rand_mat(41, 1 << 9, 33), rand_mat(42, 1 << 5, 3)]
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(1, 1, 0), ctx)
    _, data = pcs.commit([((9, 1), mats[0].copy()), ((5, 1), mats[1].copy())])
    for idx, (h, w) in enumerate(data.dims):
        lde = data.lde(idx)
        assert lde.shape == (h, w)
        log_h = h.bit_length() - 1
        for log_size in range(log_h + 1):
            got = pcs.get_evaluations_on_domain(data, idx, log_size)
            assert got.dims() == (1 << log_size, w)
            want = lde[: 1 << log_size][bitrev_index(log_size)]
            assert same(got.download(), want), (idx, log_size)
        # the domain of the trace itself: evaluations on 31 * H_n (two_adic_pcs.rs:247-258)
        n_log = log_h - 1
        want = orc.coset_lde_batch(mats[idx], 0, 31)
        assert same(pcs.get_evaluations_on_domain(data, idx, n_log).download(), want)
        with pytest.raises(TsError) as ei:
            pcs.get_evaluations_on_domain(data, idx, log_h + 1)
        assert ei.value.code == 1
    for bad in (2, 0xFFFFFFFF):
        with pytest.raises(TsError) as ei:
            pcs.get_evaluations_on_domain(data, bad, 0)
        assert ei.value.code == 1


# ------------------------------------------------------------------ device-only pipeline
def test_device_only_pipeline_then_a_proof(ctx, dft, orc):
    from tapstark_amd.airs import SynthMulAir, generate_synth_mul_trace

    x = rand_mat(7, 1 << 13, 5)
    lde = dft.coset_lde_batch(ts.DeviceMatrix.upload(ctx, x), 1, 31)
    ptr = lde.device_ptr()
    assert ptr != 0 and ptr == lde.device_ptr()
    copy = ts.DeviceMatrix.from_device_ptr(ctx, ptr, 1 << 14, 5)
    del lde
    assert same(copy.download(), orc.coset_lde_batch(x, 1, 31))
    # the new launches leave the context's pool and twiddle caches sound: a proof still has its fixture digest
    golden = json.load(open(os.path.join(GOLDEN, "oracle_fixtures.json")))
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 28, 8), ctx))
    proof = ts.prove(config, SynthMulAir(64), ts.BfChallenger(), generate_synth_mul_trace(1 << 10), [])
    assert orc.blake3(proof.words.tobytes()).hex() == golden["synthmul64_2pow10_proof_blake3"]


def test_matrices_made_on_the_device(ctx, dft, orc):
    """Quotient chunks are column-major inside the library: the transforms and the pointer see their
    row-major values."""
    from tapstark_amd.airs import FibonacciAir, fibonacci_public_values, generate_fibonacci_trace

    trace = generate_fibonacci_trace(0, 1, 1 << 7)
    pis = fibonacci_public_values(trace)
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(2, 1, 0), ctx)
    _, data = pcs.commit([((7, 1), trace)])
    air = ts.CompiledAir(ctx, ts.air_tape(FibonacciAir(), len(pis)))
    chunk = pcs.quotient_chunks(data, air, pis, [3, 1, 4, 1])[0]
    vals = chunk.download()
    assert same(dft.dft_batch(chunk).download(), orc.dft_batch(vals))
    assert same(chunk.bit_reverse_rows().download(), oracle_bit_reverse_rows(orc, vals))
    assert same(chunk.download(), vals)
    copy = ts.DeviceMatrix.from_device_ptr(ctx, chunk.device_ptr(), *vals.shape)
    assert same(copy.download(), vals) and same(chunk.download(), vals)


# ------------------------------------------------------------------ refusals
def test_error_paths(ctx, dft):
    x = rand_mat(9, 1 << 12, 2)
    dm = ts.DeviceMatrix.upload(ctx, x)
    for shift in (0, P, 0xFFFFFFFF):
        for call in (lambda: dft.coset_dft_batch(dm, shift), lambda: dft.coset_idft_batch(dm, shift),
                     lambda: dft.coset_lde_batch(dm, 1, shift)):
            with pytest.raises(TsError) as ei:
                call()
            assert ei.value.code == 1 and "shift" in str(ei.value)
    # a result taller than the tallest LDE ts_pcs_commit makes (2^27 rows)
    for added_bits in (16, 27, 40, 0xFFFFFFFF):
        with pytest.raises(TsError) as ei:
            dft.coset_lde_batch(dm, added_bits, 31)
        assert ei.value.code == 1
    assert dft.coset_lde_batch(dm, 0, 31).dims() == (1 << 12, 2)
    # a height that is no power of two cannot become a matrix at all: upload and from-device refuse it
    with pytest.raises(TsError) as ei:
        ts.DeviceMatrix.from_device_ptr(ctx, dm.device_ptr(), 3 << 10, 2)
    assert ei.value.code == 1
    with pytest.raises(TsError) as ei:
        ts.DeviceMatrix.upload(ctx, x[: 3 << 10])
    assert ei.value.code == 1
    assert (dm.download() == x).all()


# ------------------------------------------------------------------ partial transpose tiles
# 2^7 x 65: full 64-row tiles with one full and one partial column tile; 2^3 x 1: below one row tile.  (No call
# of the C ABI can hand a transpose a height that is no power of two: matrices, LDEs and taptree inputs all
# refuse one, test_error_paths above and taptree.cpp's log2_strict.)
@pytest.mark.parametrize("log_n,w", [(7, 65), (3, 1)], ids=["2^7x65", "2^3x1"])
def test_partial_tile_transposes_match_oracle(ctx, dft, orc, log_n, w):
    x = rand_mat(9000 + 64 * log_n + w, 1 << log_n, w)
    dm = ts.DeviceMatrix.upload(ctx, x)
    assert same(dm.bit_reverse_rows().download(), oracle_bit_reverse_rows(orc, x)), "bit_reverse_rows"
    assert same(dft.dft_batch(dm).download(), orc.dft_batch(x)), "dft_batch"
    assert same(dft.idft_batch(dm).download(), orc.dft_batch(x, inverse=True)), "idft_batch"
    assert same(dm.download(), x), "the input matrix was modified"


# ------------------------------------------------------------------ kernel-timer names
# bench.py and the profile tools find the NTT kernels by their timer names.  The names below are those of the
# commit before the pass plan got one owner (ntt_plan.hpp) for the same calls, character for character as its
# launch macros spelled them.
NTT_STEMS = ("k_intt_contig", "k_lde_mid", "k_lde_fwd_contig", "k_dft_", "k_transpose")
LDE_TIMER_NAMES = {
    (12, 3): ["k_lde_mid<0>", "k_transpose_bitrev", "k_transpose_unbitrev"],
    (13, 3): ["(k_intt_contig<12, true>)", "k_lde_fwd_contig<12>", "k_lde_mid<0>", "k_transpose_bitrev_r16",
              "k_transpose_unbitrev"],
    (20, 1): ["(k_intt_contig<12, true>)", "k_lde_fwd_contig<12>", "k_lde_mid<1>", "k_transpose_bitrev_r16",
              "k_transpose_unbitrev"],
    (21, 1): ["(k_intt_contig<13, true>)", "(k_lde_mid<1, 8192, 512, 13>)", "k_lde_fwd_contig<13>",
              "k_transpose_bitrev_r16", "k_transpose_unbitrev"],
    (22, 1): ["(k_intt_contig<14, true>)", "(k_lde_fwd_contig<14, 4>)", "(k_lde_mid<1, 8192, 512, 14>)",
              "k_transpose_bitrev_r16", "k_transpose_unbitrev"],
}
# a Fibonacci proof at 2^13, log_blowup 1: the trace (two columns: a partial transpose tile) and its quotient chunk
FIB_TIMER_NAMES = ["(k_intt_contig<12, true>)", "k_intt_contig<12>", "k_lde_fwd_contig<12>", "k_lde_mid<0>",
                   "k_transpose_bitrev_r16"]


def test_kernel_timer_names(ctx, dft):
    from tapstark_amd.airs import FibonacciAir, fibonacci_public_values, generate_fibonacci_trace

    def ntt_names():
        return sorted(k for k in ctx.take_kernel_timings() if k.lstrip("(").startswith(NTT_STEMS))

    mats = {shape: ts.DeviceMatrix.upload(ctx, rand_mat(sum(shape), 1 << shape[0], shape[1])) for shape in LDE_TIMER_NAMES}
    trace = generate_fibonacci_trace(0, 1, 1 << 13)
    pis = fibonacci_public_values(trace)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(1, 4, 0), ctx))
    ctx.set_kernel_timing(True)
    try:
        ctx.take_kernel_timings()
        for shape, want in LDE_TIMER_NAMES.items():
            dft.coset_lde_batch(mats[shape], 1, 31)
            assert ntt_names() == sorted(want), shape
        ts.prove(config, FibonacciAir(), ts.BfChallenger(), trace, pis)
        assert ntt_names() == sorted(FIB_TIMER_NAMES)
    finally:
        ctx.set_kernel_timing(False)
