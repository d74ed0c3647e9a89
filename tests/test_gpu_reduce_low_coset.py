"""The reduced opening on the low coset, extended by the coset LDE (csrc/open.hip k_reduce_low, k_ef_interleave;
prover.cpp open_reduce_slab), against the one-pass kernel over every LDE row (k_reduce_fused).

Both compute the same field elements, so for every case the proof with TS_REDUCE_LOW=1 is, word for word, the proof
with TS_REDUCE_LOW=0 and the oracle's, and the verifiers accept it.  The kernel timers show which path ran: the
cases are small (the policy would send all of them down the old path), so it is the knob that is under test, and
the shapes are the ones where the new launches change form: fewer rows than a workgroup, the one-launch LDE plans,
both sides of the 4096-row boundary between the single strided pass and the two-pass plan, widths that are no
multiple of the 8-column batch, one, two and four quotient chunks, blowups 2, 4 and 8.  Sharded slabs and proofs
with a preprocessed key keep the old kernels whatever the knob says."""
import threading

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd.airs import (FibonacciAir, HighDegreeAir, SelectorAir, SynthExtAir, SynthMulAir,
                               fibonacci_public_values, generate_fibonacci_trace, generate_high_degree_trace,
                               generate_selector_preprocessed, generate_selector_trace, generate_synth_ext_trace,
                               generate_synth_mul_trace)

pytestmark = pytest.mark.gpu
NO_PIS = np.zeros(0, dtype=np.uint32)


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


def make_case(name, n):
    """(air, trace, public values, quotient chunks)"""
    if name == "fib":  # w = 2
        tr = generate_fibonacci_trace(0, 1, n)
        return FibonacciAir(), tr, fibonacci_public_values(tr), 1
    if name == "mul5":  # a width that is no multiple of 4
        return SynthMulAir(5), generate_synth_mul_trace(n, 5), NO_PIS, 2
    if name == "mul64":  # the flagship's AIR
        return SynthMulAir(64), generate_synth_mul_trace(n), NO_PIS, 2
    if name == "ext163":
        return SynthExtAir(163), generate_synth_ext_trace(n, 163), NO_PIS, 1
    if name == "deg5":  # a^4 b: four quotient chunks
        return HighDegreeAir(5), generate_high_degree_trace(n), NO_PIS, 4
    raise ValueError(name)


def reduce_kernels(ctx, run):
    """run()'s result and the launch counts of the reduce kernels and of the interleave"""
    ctx.set_kernel_timing(True)
    try:
        ctx.take_kernel_timings()
        out = run()
        t = ctx.take_kernel_timings()
    finally:
        ctx.set_kernel_timing(False)
    return out, {k: v[0] for k, v in t.items() if k.startswith(("k_reduce", "k_ef_interleave"))}


# air, log_n, log_blowup: every log_n of {3, 6, 10, 12, 13} and every blowup of {1, 2, 3} for each AIR
# (SynthExt-163 up to 2^10 rows; four chunks need log_blowup >= 2)
CASES = [
    ("fib", 3, 1), ("fib", 6, 2), ("fib", 10, 3), ("fib", 12, 2), ("fib", 13, 1),
    ("mul5", 3, 2), ("mul5", 6, 3), ("mul5", 10, 1), ("mul5", 12, 2), ("mul5", 13, 3),
    ("mul64", 3, 3), ("mul64", 6, 1), ("mul64", 10, 2), ("mul64", 12, 3), ("mul64", 13, 2),
    ("ext163", 3, 2), ("ext163", 6, 3), ("ext163", 10, 1),
    ("deg5", 3, 2), ("deg5", 6, 3), ("deg5", 10, 2), ("deg5", 12, 3), ("deg5", 13, 2),
]


@pytest.mark.parametrize("name,log_n,log_blowup", CASES, ids=[f"{c[0]}-2p{c[1]}-b{c[2]}" for c in CASES])
def test_low_coset_proof_is_the_full_reduce_proof_and_the_oracles(ctx, orc, monkeypatch, name, log_n, log_blowup):
    air, trace, pis, qd = make_case(name, 1 << log_n)
    tape = ts.air_tape(air, len(pis))
    cair = ts.CompiledAir(ctx, tape)
    assert 1 << cair.log_quotient_degree == qd
    cfg = (log_blowup, 5, 4)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))
    proofs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("TS_REDUCE_LOW", knob)
        proofs[knob], ran = reduce_kernels(ctx, lambda: ts.prove(config, cair, ts.BfChallenger(), trace.copy(), pis))
        want_ran = {"k_reduce_low": 1, "k_ef_interleave": 1} if knob == "1" else {"k_reduce_fused": 1}
        assert ran == want_ran, (knob, ran)
    full, low = proofs["0"].words, proofs["1"].words
    assert len(low) == len(full) and (low == full).all(), f"{int((low != full).sum())} proof words differ"
    ocfg = orc.FriConfig(*cfg)
    want = orc.prove(ocfg, tape, trace, pis)
    assert len(low) == len(want) and (low == want).all(), f"{int((low != want).sum())} words differ from the oracle"
    assert orc.verify(ocfg, tape, low, pis) == 0
    ts.verify(config, air, ts.BfChallenger(), proofs["1"], pis)


def test_unset_knob_follows_the_width_policy(ctx, monkeypatch):
    """Narrow proofs are bound by their launches and keep the one-pass kernel; from the crossover width up
    (profiles/reduce_low_coset_crossover.txt) the low coset is reduced and extended."""
    monkeypatch.delenv("TS_REDUCE_LOW", raising=False)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 5, 4), ctx))
    for name, want in (("fib", {"k_reduce_fused": 1}), ("mul64", {"k_reduce_low": 1, "k_ef_interleave": 1})):
        air, trace, pis, _ = make_case(name, 1 << 6)
        proof, ran = reduce_kernels(ctx, lambda: ts.prove(config, air, ts.BfChallenger(), trace.copy(), pis))
        assert ran == want, (name, ran)
        ts.verify(config, air, ts.BfChallenger(), proof, pis)


def test_preprocessed_key_keeps_the_one_pass_kernel(ctx, monkeypatch):
    n = 1 << 10
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 5, 4), ctx))
    prep = generate_selector_preprocessed(n)
    key = ts.PreprocessedKey(config, prep)
    cair = ts.CompiledAir(ctx, ts.air_tape(SelectorAir(), 2, 3))
    trace, pis = generate_selector_trace(prep)
    proofs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("TS_REDUCE_LOW", knob)
        proofs[knob], ran = reduce_kernels(ctx, lambda: ts.prove(config, cair, ts.BfChallenger(), trace.copy(), pis,
                                                                 preprocessed=key))
        assert ran == {"k_reduce_fused_pre": 1}, (knob, ran)
    assert len(proofs["1"].words) == len(proofs["0"].words) and (proofs["1"].words == proofs["0"].words).all()
    ts.verify(config, cair, ts.BfChallenger(), proofs["1"], pis, preprocessed_root=key.root)


def test_sharded_slabs_keep_the_one_pass_kernel(ctx, orc, monkeypatch):
    """prove_sharded over two thread-ranks (two cosets each): every rank reduces its slab with k_reduce_fused, and
    the proof is the single-GPU proof -- itself made on the low coset -- and the oracle's."""
    from tapstark_amd.comm import LocalCommGroup

    monkeypatch.setenv("TS_REDUCE_LOW", "1")
    G, log_n, cfg = 2, 10, (2, 5, 4)
    air, trace, pis, _ = make_case("mul64", 1 << log_n)
    n = trace.shape[0]
    tape = ts.air_tape(air, 0)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))
    single, ran = reduce_kernels(ctx, lambda: ts.prove(config, air, ts.BfChallenger(), trace.copy(), pis))
    assert ran == {"k_reduce_low": 1, "k_ef_interleave": 1}, ran
    group = LocalCommGroup(G)
    proofs, rans, errors = [None] * G, [None] * G, [None] * G

    def rank_main(r):
        try:
            c = ts.Context(0)
            conf = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), c))
            rows = np.ascontiguousarray(trace[r * n // G:(r + 1) * n // G])
            p, rans[r] = reduce_kernels(c, lambda: ts.prove_sharded(conf, ts.CompiledAir(c, tape), ts.BfChallenger(),
                                                                    rows, pis, group.comm(r), 4))
            proofs[r] = p.words
        except BaseException as e:  # noqa: BLE001
            errors[r] = e

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank is stuck in a collective"
    for r in range(G):
        assert errors[r] is None, f"rank {r}: {errors[r]!r}"
        assert rans[r] == {"k_reduce_fused": 1}, (r, rans[r])
        assert len(proofs[r]) == len(single.words) and (proofs[r] == single.words).all(), f"rank {r}: proof differs"
    want = orc.prove(orc.FriConfig(*cfg), tape, trace, pis)
    assert len(want) == len(single.words) and (want == single.words).all()
    assert orc.verify(orc.FriConfig(*cfg), tape, proofs[0], pis) == 0
