"""AIRs with preprocessed columns on the GPU: the quotient kernels over two committed matrices, check_constraints
over two matrices, whole TSPF v3 proofs against a commit-once key, the rejections, the one-pass opening and the
statuses.  The reference's AIR language has such columns (uni-stark/src/symbolic_builder.rs:68-99,144-148) but
its prove / verify pass width 0 (prover.rs:46, verifier.rs:40), so exactness comes from two equalities:

* the quotient of an AIR with P preprocessed and W main columns is, row by row, the quotient of the joined AIR
  over hstack(preprocessed, main), which the oracle and the existing ts_quotient_chunks compute;
* a whole proof is the composition of oracle-tested ABI stages -- ts_pcs_commit, ts_pcs_open over any rounds x
  matrices x points (fri/src/two_adic_pcs.rs:260-419), the host challenger -- around that quotient.

The CPU half is tests/test_air_prep_cpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib, taptree as tt
from tapstark_amd.airs import (SelectorAir, SynthMulAir, generate_random_air_trace, generate_selector_preprocessed,
                               generate_selector_trace, generate_synth_mul_trace, random_air_case, splitmix64_stream)
from tapstark_amd.comm import LocalCommGroup
from _prep_airs import join_tape, next_row_loads, prep_width, split_tape

pytestmark = pytest.mark.gpu
P = 0x78000001
G27 = 0x1A427A41
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_UNSUPPORTED = 1, 4
SEEDS = [s for s in range(36) if random_air_case(s)[0].width() >= 2]
VALID_SEEDS = [s for s in SEEDS if s % 3 == 0]
SEGMENT_SEEDS = [0, 6, 9, 12, 21, 27]
TALL_SEED = next(s for s in VALID_SEEDS if random_air_case(s)[0].valid)  # proved again at n = 2^10
WAIT_JIT_INSTR = 3000  # larger programs stay on the interpreter in the specialised pass, as in test_gpu_air_fuzz.py


@pytest.fixture(scope="module")
def ctx():
    from tapstark_amd.build import build

    build()
    return ts.default_context()


class Case:
    """A random AIR split into P preprocessed and W main columns, with its inputs and the oracle's quotient of the
    joined AIR (computed once, shared, never modified)."""

    def __init__(self, orc, seed):
        self.seed = seed
        air, self.log_n = random_air_case(seed)
        self.air, self.valid = air, air.valid
        n, w = 1 << self.log_n, air.width()
        self.pw = prep_width(seed, w)
        self.v1 = ts.air_tape(air, air.n_public)
        self.v2 = split_tape(self.v1, self.pw)
        if air.valid:
            joined, self.pis, _ = generate_random_air_trace(air, n)
        else:
            joined = splitmix64_stream(seed + 1, n * w).reshape(n, w).astype(np.uint32)
            self.pis = splitmix64_stream(seed + 2, max(air.n_public, 1))[:air.n_public].astype(np.uint32)
        self.joined = np.ascontiguousarray(joined, dtype=np.uint32)
        self.prep = np.ascontiguousarray(self.joined[:, :self.pw])
        self.main = np.ascontiguousarray(self.joined[:, self.pw:])
        self.lqd = orc.log_quotient_degree(self.v1)
        self.b = max(self.lqd, 1)
        self.alpha = splitmix64_stream(seed + 3, 4).astype(np.uint32)
        lde = orc.commit_lde(self.joined, 1, self.b)
        self.want = orc.split_quotient(orc.quotient_values(self.v1, lde, self.log_n, self.b, self.pis, self.alpha),
                                       self.log_n, self.lqd)
        self.want.setflags(write=False)


@pytest.fixture(scope="module")
def cases(orc):
    return {s: Case(orc, s) for s in SEEDS}


def _compile(ctx, tape, monkeypatch, jit: bool, **kw):
    with monkeypatch.context() as m:
        if not jit:
            m.setenv("TS_NO_JIT", "1")
        m.setenv("TS_JIT_MAX_INSTR", str(WAIT_JIT_INSTR))
        return ts.CompiledAir(ctx, tape, **kw)


def _commit(pcs, log_n, m):
    return pcs.commit([((log_n, 1), m.copy())])


def _chunks_pre(ctx, case, cair):
    pcs = ts.TwoAdicFriPcs(ts.FriConfig(case.b, 3, 2), ctx)
    _, key = _commit(pcs, case.log_n, case.prep)
    _, data = _commit(pcs, case.log_n, case.main)
    return [ch.download() for ch in pcs.quotient_chunks(data, cair, case.pis, case.alpha, preprocessed=key)]


def _same(got, want, what):
    assert len(got) == want.shape[0], what
    for c, g in enumerate(got):
        assert (g == want[c]).all(), f"{what}: chunk {c}: {int((g != want[c]).sum())} words differ"


# ------------------------------------------------------------------ A. quotient kernels
def test_case_set_has_the_edges(cases):
    """P = 1 and W = 1; P > W; an AIR whose only next-row reads are preprocessed; lqd 0 and lqd 3."""
    progs = {s: ts.CompiledAir(None, c.v2).program() for s, c in cases.items()}
    assert any(c.pw == 1 and c.main.shape[1] == 1 for c in cases.values())
    assert any(c.pw > c.main.shape[1] for c in cases.values())
    assert any(next_row_loads(progs[s])[0] and not next_row_loads(progs[s])[1] for s in cases)
    assert any(c.lqd == 0 for c in cases.values()) and any(c.lqd == 3 for c in cases.values())
    assert max(c.log_n for c in cases.values()) == 6 and min(c.log_n for c in cases.values()) == 1
    assert len(cases) >= 33


@pytest.mark.parametrize("chunk", range(12))
@pytest.mark.parametrize("jit", [False, True], ids=["interp", "jit"])
def test_quotient_over_two_matrices(ctx, cases, monkeypatch, jit, chunk):
    """== the oracle's quotient of the joined AIR, and == ts_quotient_chunks of the version-1 AIR on the unsplit
    trace, through the interpreter (k_quotient_pre) and through the specialised kernel."""
    n_jit, seeds = 0, SEEDS[chunk::12]
    for seed in seeds:
        case = cases[seed]
        cair = _compile(ctx, case.v2, monkeypatch, jit)
        assert cair.preprocessed_width == case.pw and cair.log_quotient_degree == case.lqd
        if jit and not cair.is_jit:  # above the synchronous budget: joined, or (above this run's) left alone
            state, _ = cair.jit_wait()
            assert state == (3 if len(cair.program()["code"]) <= WAIT_JIT_INSTR else 0), seed
        assert cair.is_jit == (jit and len(cair.program()["code"]) <= WAIT_JIT_INSTR), seed
        n_jit += int(cair.is_jit)
        got = _chunks_pre(ctx, case, cair)
        _same(got, case.want, f"seed {seed} vs oracle")
        v1 = _compile(ctx, case.v1, monkeypatch, False)
        pcs = ts.TwoAdicFriPcs(ts.FriConfig(case.b, 3, 2), ctx)
        _, data = _commit(pcs, case.log_n, case.joined)
        ref = [ch.download() for ch in pcs.quotient_chunks(data, v1, case.pis, case.alpha)]
        for c, (g, r) in enumerate(zip(got, ref)):
            assert (g == r).all(), f"seed {seed} vs ts_quotient_chunks: chunk {c}"
    assert n_jit >= (len(seeds) - 1 if jit else 0)  # (one program of the set is above this run's budget)


@pytest.mark.parametrize("seed", SEGMENT_SEEDS)
def test_quotient_segmented(ctx, cases, monkeypatch, seed):
    case = cases[seed]
    cair = _compile(ctx, case.v2, monkeypatch, True, segment_instr=16)
    assert len(cair.segment_plan()["segments"]) > 1
    state, _ = cair.jit_wait()
    assert state == 3 and cair.is_jit, f"segmented specialisation failed (state {state})"
    _same(_chunks_pre(ctx, case, cair), case.want, f"seed {seed} segmented")


_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import tapstark_amd as ts
from oracle import oracle_py as orc
import test_gpu_preprocessed as T
orc.build()
case = T.Case(orc, int(sys.argv[2]))
ctx = ts.default_context()
cair = ts.CompiledAir(ctx, case.v2)
assert not cair.is_jit
got = T._chunks_pre(ctx, case, cair)
ok = len(got) == case.want.shape[0] and all((g == case.want[c]).all() for c, g in enumerate(got))
print("CHILD", "same" if ok else "DIFFERENT", cair.program()["n_regs"])
"""


def test_quotient_global_slab_interpreter(ctx):
    """TS_INTERP_LDS_MAX_REGS=4: the register file goes to the global slab (k_quotient_pre<64, true>); in a child
    process of its own, with the knob in its environment from the start."""
    env = dict(os.environ, TS_NO_JIT="1", TS_INTERP_LDS_MAX_REGS="4")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, "3"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    word = [l for l in r.stdout.splitlines() if l.startswith("CHILD")][0].split()
    assert word[1] == "same" and int(word[2]) > 4, r.stdout


# ------------------------------------------------------------------ B. check_constraints
def test_check_constraints_over_two_matrices(ctx, orc, cases, monkeypatch, global_slab=False):
    for seed in VALID_SEEDS:
        case = cases[seed]
        cair = _compile(ctx, case.v2, monkeypatch, False)
        if global_slab:  # read at every launch: the register file goes to the global slab from here on
            monkeypatch.setenv("TS_INTERP_LDS_MAX_REGS", "1")
            assert cair.program()["n_regs"] > 1
        joined_tape = join_tape(case.v2)
        assert (joined_tape == case.v1).all()
        n = 1 << case.log_n
        assert ts.check_constraints(cair, case.main, case.pis, ctx, preprocessed=case.prep) == -1 == \
            orc.check_constraints(joined_tape, case.joined, case.pis), seed
        bad_main = case.main.copy()
        bad_main[(seed * 7) % n, seed % bad_main.shape[1]] ^= 1
        assert ts.check_constraints(cair, bad_main, case.pis, ctx, preprocessed=case.prep) == \
            orc.check_constraints(joined_tape, np.hstack([case.prep, bad_main]), case.pis), seed
        bad_prep = case.prep.copy()
        bad_prep[(seed * 5) % n, seed % case.pw] ^= 1
        assert ts.check_constraints(cair, case.main, case.pis, ctx, preprocessed=bad_prep) == \
            orc.check_constraints(joined_tape, np.hstack([bad_prep, case.main]), case.pis), seed


def test_check_constraints_over_two_matrices_global_slab(ctx, orc, cases, monkeypatch):
    """The same through k_check_constraints_pre<64, true>: one 64-lane tile mostly inactive (n = 2) and exactly full
    (n = 2^6) among the seeded cases, then n = 2^10, sixteen tiles, which they do not reach: a valid trace, and a
    cell changed in the last tile but one."""
    assert {1, 6} <= {cases[s].log_n for s in VALID_SEEDS}
    test_check_constraints_over_two_matrices(ctx, orc, cases, monkeypatch, global_slab=True)
    case = cases[TALL_SEED]
    n, r = 1 << 10, (1 << 10) - 70
    joined, pis, _ = generate_random_air_trace(case.air, n)
    joined = np.ascontiguousarray(joined, dtype=np.uint32)
    cair = _compile(ctx, case.v2, monkeypatch, False)
    check = lambda m: ts.check_constraints(cair, np.ascontiguousarray(m[:, case.pw:]), pis, ctx,
                                           preprocessed=np.ascontiguousarray(m[:, :case.pw]))
    assert check(joined) == -1 == orc.check_constraints(case.v1, joined, pis)
    late = []
    for col in (0, joined.shape[1] - 1):  # a preprocessed cell, a main cell
        bad = joined.copy()
        bad[r, col] ^= 1
        late.append(orc.check_constraints(case.v1, bad, pis))
        assert check(bad) == late[-1], col
    assert max(late) >> 16 >= r - 1


# ------------------------------------------------------------------ C. whole proofs
def _mul_base(z, k):
    return np.array([int(x) * k % P for x in z], dtype=np.uint32)


def _staged_proof(pcs, cair, key, trace, pis, chal):
    """The proof of ts_prove_pre built from public stage calls: (trace root, quotient root, opened values in v3
    order, FriProof words); `chal` ends in the prover's final state."""
    n = trace.shape[0]
    log_n, lqd = n.bit_length() - 1, cair.log_quotient_degree
    chal.observe_commitment(key.root)
    root_t, data_t = pcs.commit([((log_n, 1), trace.copy())])
    chal.observe_commitment(root_t)
    alpha = chal.sample()
    chunks = pcs.quotient_chunks(data_t, cair, pis, alpha, preprocessed=key)
    g = pow(G27, 1 << (27 - (log_n + lqd)), P) if log_n + lqd else 1
    root_q, data_q = pcs.commit([((log_n, 31 * pow(g, c, P) % P), ch) for c, ch in enumerate(chunks)])
    chal.observe_commitment(root_q)
    zeta = chal.sample()
    zeta_next = _mul_base(zeta, pow(G27, 1 << (27 - log_n), P))
    opened, fri = pcs.open([(key.data, [[zeta, zeta_next]]), (data_t, [[zeta, zeta_next]]),
                            (data_q, [[zeta]] * len(chunks))], chal)
    flat = np.concatenate([v for rnd in opened for m in rnd for v in m])
    return root_t, root_q, flat, fri


def _check_whole_proof(ctx, cair, prep, trace, pis, cfg):
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), ctx))
    key = ts.PreprocessedKey(config, prep)
    staged_chal, chal = ts.BfChallenger(), ts.BfChallenger()
    root_t, root_q, opened, fri = _staged_proof(config.pcs, cair, key, trace, pis, staged_chal)
    proof = ts.prove(config, cair, chal, trace.copy(), pis, preprocessed=key)
    pw, w, qd = prep.shape[1], trace.shape[1], 1 << cair.log_quotient_degree
    n_open = 4 * (2 * pw + 2 * w + 4 * qd)
    words = proof.words
    assert list(words[:6]) == [0x46505354, 3, trace.shape[0].bit_length() - 1, w, qd, pw]
    assert (words[6:14] == root_t).all() and (words[14:22] == root_q).all()
    assert (words[22:22 + n_open].reshape(-1, 4) == opened).all(), "opened values differ"
    assert len(words) - 22 - n_open == len(fri) and (words[22 + n_open:] == fri).all(), "FriProof words differ"
    assert (chal.state() == staged_chal.state()).all(), "final challenger state differs"
    assert (proof.preprocessed_local == opened[:pw]).all() and (proof.preprocessed_next == opened[pw:2 * pw]).all()
    assert (proof.trace_local == opened[2 * pw:2 * pw + w]).all()
    assert all(len(q.input_proof) == 3 for q in proof.query_proofs)
    return config, key, proof


@pytest.mark.parametrize("log_n,b", [(3, 1), (6, 2), (9, 3), (12, 2)])
def test_selector_air_whole_proof(ctx, log_n, b):
    air = SelectorAir()
    prep = generate_selector_preprocessed(1 << log_n)
    trace, pis = generate_selector_trace(prep)
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 2, 3))
    config, key, proof = _check_whole_proof(ctx, cair, prep, trace, pis, (b, 3, 2))
    ts.verify(config, cair, ts.BfChallenger(), proof, pis, preprocessed_root=key.root)
    ts.verify(config, air, ts.BfChallenger(), proof, pis, preprocessed_root=key.root)  # host-only AIR from the class


@pytest.mark.parametrize("seed", VALID_SEEDS)
def test_random_air_whole_proof(ctx, cases, monkeypatch, seed):
    case = cases[seed]
    cair = _compile(ctx, case.v2, monkeypatch, True)
    config, key, proof = _check_whole_proof(ctx, cair, case.prep, case.main, case.pis, (case.b, 3, 2))
    ts.verify(config, ts.CompiledAir(None, case.v2), ts.BfChallenger(), proof, case.pis, preprocessed_root=key.root)


def test_one_key_serves_two_proofs(ctx):
    air, n = SelectorAir(), 64
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), ctx))
    prep = generate_selector_preprocessed(n)
    key = ts.PreprocessedKey(config, prep)
    top = [key.data.digests(l).copy() for l in (key.data.log_height, key.data.log_height - 1, 0)]
    lde = key.data.lde(0).copy()
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 2, 3))
    proofs = []
    for a0, b0 in ((3, 5), (1234567, P - 2)):
        trace, pis = generate_selector_trace(prep, a0, b0)
        proof = ts.prove(config, cair, ts.BfChallenger(), trace, pis, preprocessed=key)
        ts.verify(config, cair, ts.BfChallenger(), proof, pis, preprocessed_root=key.root)
        proofs.append(proof.words)
    assert not (len(proofs[0]) == len(proofs[1]) and (proofs[0] == proofs[1]).all())
    for l, want in zip((key.data.log_height, key.data.log_height - 1, 0), top):
        assert (key.data.digests(l) == want).all()
    assert (key.data.digests(key.data.log_height)[0] == key.root).all() and (key.data.lde(0) == lde).all()


def test_prove_pre_without_preprocessed_columns_is_prove(ctx, orc):
    """An AIR with preprocessed_width 0: ts_prove_pre with a null key is ts_prove but for the v3 header, and
    ts_verify_pre with a null root accepts it; so are the other two _pre calls with a null argument."""
    air = SynthMulAir(6)
    trace = generate_synth_mul_trace(32, 6)
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 0))
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(1, 3, 2), ctx))
    v1 = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), []).words
    l, cfg = _lib.lib(), config.pcs.fri._c()
    out = np.zeros(len(v1) + 64, dtype=np.uint32)
    n_words = C.c_size_t()
    chal, m = ts.BfChallenger(), ts.DeviceMatrix.upload(ctx, trace)
    ctx.check(l.ts_prove_pre(ctx.h, C.byref(cfg), cair.h, chal.h, None, m.h, None, 0, out.ctypes.data_as(_lib.u32p),
                             len(out), C.byref(n_words)))
    v3 = out[:n_words.value]
    assert list(v3[:6]) == [v1[0], 3, v1[2], v1[3], v1[4], 0] and (v3[6:] == v1[5:]).all()
    verdict, vchal = C.c_int(-1), ts.BfChallenger()
    assert l.ts_verify_pre(C.byref(cfg), cair.h, vchal.h, None, v3.ctypes.data_as(_lib.u32p), len(v3), None, 0,
                           C.byref(verdict)) == 0 and verdict.value == 0
    pcs = config.pcs
    _, data = _commit(pcs, 5, trace)
    alpha = splitmix64_stream(5, 4).astype(np.uint32)
    a = [c.download() for c in pcs.quotient_chunks(data, cair, [], alpha)]
    outp = (C.c_void_p * 2)()
    ctx.check(l.ts_quotient_chunks_pre(ctx.h, None, data.h, 1, cair.h, None, 0, alpha.ctypes.data_as(_lib.u32p), outp))
    b = [ts.DeviceMatrix(ctx, C.c_void_p(outp[c])).download() for c in range(2)]
    assert all((x == y).all() for x, y in zip(a, b))
    viol, tm = C.c_int64(7), ts.DeviceMatrix.upload(ctx, trace)
    ctx.check(l.ts_check_constraints_pre(ctx.h, cair.h, None, tm.h, None, 0, C.byref(viol)))
    assert viol.value == ts.check_constraints(cair, trace, [], ctx) == -1


# ------------------------------------------------------------------ D. rejections
@pytest.fixture(scope="module")
def selector_proof(ctx):
    air, n = SelectorAir(), 64
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), ctx))
    prep = generate_selector_preprocessed(n)
    key = ts.PreprocessedKey(config, prep)
    cair = ts.CompiledAir(ctx, ts.air_tape(air, 2, 3))
    trace, pis = generate_selector_trace(prep)
    proof = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), pis, preprocessed=key)
    ts.verify(config, cair, ts.BfChallenger(), proof, pis, preprocessed_root=key.root)
    return config, cair, key, prep, trace, pis, proof.words.copy()


def _rejected(config, cair, words, pis, root):
    with pytest.raises(ts.VerificationError) as e:
        ts.verify(config, cair, ts.BfChallenger(), words, pis, preprocessed_root=root)
    assert e.value.code != 0


def test_rejections(ctx, orc, selector_proof):
    config, cair, key, prep, trace, pis, words = selector_proof
    other_prep = prep.copy()
    other_prep[5, 1] ^= 1
    other = ts.PreprocessedKey(config, other_prep)
    assert not (other.root == key.root).all()
    _rejected(config, cair, words, pis, other.root)  # another key's root
    for k in (22, 22 + 4 * 3 + 5):  # a word of preprocessed_local, of preprocessed_next
        bad = words.copy()
        bad[k] = (int(bad[k]) + 1) % P
        _rejected(config, cair, bad, pis, key.root)
    bad = words.copy()
    bad[5] = 2  # the header's preprocessed_width
    _rejected(config, cair, bad, pis, key.root)
    # a main trace made for another sel column than the key's: proved all the same (as a release build of the
    # reference would), rejected by the verifier, and check_constraints names the oracle's first violating row
    flipped = prep.copy()
    flipped[:, 0] ^= 1
    wrong_trace, wrong_pis = generate_selector_trace(flipped)
    proof = ts.prove(config, cair, ts.BfChallenger(), wrong_trace.copy(), wrong_pis, preprocessed=key)
    assert proof.words[1] == 3
    _rejected(config, cair, proof.words, wrong_pis, key.root)
    got = ts.check_constraints(cair, wrong_trace, wrong_pis, ctx, preprocessed=prep)
    joined = join_tape(ts.air_tape(SelectorAir(), 2, 3))
    assert got == orc.check_constraints(joined, np.hstack([prep, wrong_trace]), wrong_pis) and got >= 0


# ------------------------------------------------------------------ E. one-pass opening
OPEN_KERNELS = ("k_bary_weights", "k_bary_dots", "k_bary_finish", "k_reduce")


def _open_launches(ctx, run):
    ctx.set_kernel_timing(True)
    try:
        ctx.take_kernel_timings()
        run()
        t = ctx.take_kernel_timings()
    finally:
        ctx.set_kernel_timing(False)
    return {k: v[0] for k, v in t.items() if k.lstrip("(").startswith(OPEN_KERNELS)}, t


def test_opening_is_one_pass(ctx):
    n = 1 << 10
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), ctx))
    prep = generate_selector_preprocessed(n)
    key = ts.PreprocessedKey(config, prep)
    cair = ts.CompiledAir(ctx, ts.air_tape(SelectorAir(), 2, 3))
    trace, pis = generate_selector_trace(prep)
    plain_air = ts.CompiledAir(ctx, ts.air_tape(SynthMulAir(3), 0))  # the same W = 3, qd = 2, no key
    assert plain_air.log_quotient_degree == cair.log_quotient_degree
    plain_trace = generate_synth_mul_trace(n, 3)
    pre, all_pre = _open_launches(ctx, lambda: ts.prove(config, cair, ts.BfChallenger(), trace.copy(), pis,
                                                        preprocessed=key))
    plain, _ = _open_launches(ctx, lambda: ts.prove(config, plain_air, ts.BfChallenger(), plain_trace.copy(), []))
    assert pre.get("k_reduce_fused_pre") == 1 and "k_reduce_fused" not in pre, pre
    assert plain.get("k_reduce_fused") == 1, plain
    assert not any(k.startswith("k_reduce<") or k.startswith("(k_reduce<") for k in all_pre), all_pre
    assert any(k.startswith("k_quotient") for k in all_pre)
    # the opening of three rounds costs one more launch than that of two: the key's barycentric dot products
    assert sum(pre.values()) == sum(plain.values()) + 1, (pre, plain)
    dots = lambda d: sum(v for k, v in d.items() if "k_bary_dots" in k)
    assert dots(pre) == dots(plain) + 1, (pre, plain)


# ------------------------------------------------------------------ F. statuses
def _raises(code, f, needle=None):
    with pytest.raises(_lib.TsError) as e:
        f()
    assert e.value.code == code, (e.value.code, str(e.value))
    assert str(e.value), "no text in ts_last_error"
    if needle:
        assert needle in str(e.value), str(e.value)


def _prove_ok(ctx, config, cair, key, trace, pis):
    proof = ts.prove(config, cair, ts.BfChallenger(), trace.copy(), pis, preprocessed=key)
    ts.verify(config, cair, ts.BfChallenger(), proof, pis, preprocessed_root=key.root)


def test_invalid_keys(ctx, selector_proof):
    config, cair, key, prep, trace, pis, _ = selector_proof
    pcs, n = config.pcs, len(prep)

    class K:  # what prove() and quotient_chunks() take: .data
        def __init__(self, data):
            self.data = data

    taller = K(pcs.commit([((7, 1), generate_selector_preprocessed(2 * n))])[1])
    narrower = K(pcs.commit([((6, 1), prep[:, :2].copy())])[1])
    two = K(pcs.commit([((6, 1), prep.copy()), ((6, 1), prep.copy())])[1])
    other_ctx = ts.Context(ctx.device)
    foreign = ts.PreprocessedKey(ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), other_ctx)), prep)
    _, data = _commit(pcs, 6, trace)
    alpha = splitmix64_stream(1, 4).astype(np.uint32)
    for what, bad in (("height", taller), ("width", narrower), ("matrix count", two), ("context", foreign)):
        m = ts.DeviceMatrix.upload(ctx, trace)
        _raises(TS_ERR_INVALID, lambda: ts.prove(config, cair, ts.BfChallenger(), m, pis, preprocessed=bad))
        assert m.dims() == trace.shape and (m.download() == trace).all(), what  # refused before the trace is taken
        _raises(TS_ERR_INVALID, lambda: pcs.quotient_chunks(data, cair, pis, alpha, preprocessed=bad))
        _prove_ok(ctx, config, cair, key, trace, pis)
    # null arguments, and a key for an AIR that has no preprocessed columns
    l, cfg = _lib.lib(), pcs.fri._c()
    out, n_words = np.zeros(16, dtype=np.uint32), C.c_size_t()
    m = ts.DeviceMatrix.upload(ctx, trace)
    p32 = lambda a: a.ctypes.data_as(_lib.u32p)
    args = [ctx.h, C.byref(cfg), cair.h, ts.BfChallenger(), key.data.h, m.h, p32(pis), 2, p32(out), len(out),
            C.byref(n_words)]
    for k in (2, 3, 4, 5, 8, 10):
        a = [x.h if isinstance(x, ts.BfChallenger) else x for x in args]
        a[k] = None
        assert l.ts_prove_pre(*a) == TS_ERR_INVALID and l.ts_last_error(ctx.h), k
    plain = ts.CompiledAir(ctx, ts.air_tape(SynthMulAir(3), 0))
    _raises(TS_ERR_INVALID, lambda: ts.prove(config, plain, ts.BfChallenger(), generate_synth_mul_trace(64, 3), [],
                                             preprocessed=key))
    _raises(TS_ERR_INVALID, lambda: ts.check_constraints(cair, trace, pis, ctx, preprocessed=prep[:32].copy()))
    _raises(TS_ERR_INVALID, lambda: ts.check_constraints(cair, trace, pis, ctx, preprocessed=prep[:, :2].copy()))
    _prove_ok(ctx, config, cair, key, trace, pis)


def test_calls_without_a_key_refuse_the_air(ctx, selector_proof):
    config, cair, key, prep, trace, pis, words = selector_proof
    pcs = config.pcs
    _, data = _commit(pcs, 6, trace)
    alpha = splitmix64_stream(1, 4).astype(np.uint32)
    host_config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(2, 3, 2), None, host_only=True))
    locks = tt.make_lock_table(3, 3, 2, 6, lambda ci, q, s, u: tt.winternitz_lock_script(bytes([ci, q, s % 251]), u))
    group = LocalCommGroup(1)
    up = lambda: ts.DeviceMatrix.upload(ctx, trace)
    calls = {
        "ts_prove": lambda: ts.prove(config, cair, ts.BfChallenger(), up(), pis),
        "ts_quotient_chunks": lambda: pcs.quotient_chunks(data, cair, pis, alpha),
        "ts_check_constraints": lambda: ts.check_constraints(cair, trace, pis, ctx),
        "ts_prove_stream": lambda: ts.prove_stream([(config, cair)], [up()], [0], pis),
        "ts_prove_batch": lambda: ts.prove_batch([(config, cair)], [up()], [0], pis),
        "ts_prove_sharded": lambda: ts.prove_sharded(config, cair, ts.BfChallenger(), up(), pis, group.comm(0)),
        "ts_prove_tap": lambda: tt.prove_tap(config, cair, ts.BfChallenger(), up(), pis, locks),
        "ts_prove_tap_sharded": lambda: tt.prove_tap(config, cair, ts.BfChallenger(), up(), pis, locks,
                                                     comm=group.comm(0)),
    }
    for name, f in calls.items():
        _raises(TS_ERR_UNSUPPORTED, f, "ts_prove_pre")
        _prove_ok(ctx, config, cair, key, trace, pis)
    # ts_prove_batch: in the item's own status
    res = ts.prove_batch([(config, cair)], [up(), up()], [0, 0], pis, check=False)
    assert list(res.status) == [TS_ERR_UNSUPPORTED] * 2 and all("ts_prove_pre" in e for e in res.errors)
    # the host-only ones
    with pytest.raises(_lib.TsError) as e:
        ts.verify(host_config, cair, ts.BfChallenger(), words, pis)
    assert e.value.code == TS_ERR_UNSUPPORTED and "ts_prove_pre" in str(e.value)
    with pytest.raises(_lib.TsError) as e:
        tt.verify_tap(host_config, cair, ts.BfChallenger(), words, pis, locks)
    assert e.value.code == TS_ERR_UNSUPPORTED
    with pytest.raises(_lib.TsError) as e:
        ts.Proof(words).to_postcard()
    assert e.value.code == TS_ERR_UNSUPPORTED
    _prove_ok(ctx, config, cair, key, trace, pis)
