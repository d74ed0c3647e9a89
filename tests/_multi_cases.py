"""The statements of tests/test_gpu_multi.py and tests/test_multi_cpu.py: several plain AIR tables of mixed heights
for ``ts_prove_multi``, the Python staging that pins a multi proof to calls the oracle already checks, and the
writer of the fixture tests/golden/multi_proof_small.json.

A table is (air, trace, public values).  The AIRs come from tapstark_amd.airs: FibonacciAir (quotient degree 1),
SynthMulAir (2), HighDegreeAir(5) and RandomAir seeds 90 / 93 (4).  Cases are named as the issue names them."""
import json
import os

import numpy as np

import tapstark_amd as ts
from tapstark_amd.airs import (FibonacciAir, HighDegreeAir, SynthMulAir, fibonacci_public_values,
                               generate_fibonacci_trace, generate_high_degree_trace, generate_random_air_trace,
                               generate_synth_mul_trace, random_air_case)

P = 0x78000001
G27 = 0x1A427A41  # generator of the 2^27 subgroup
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_proof_small.json")
FRI_QUERIES, FRI_POW = 3, 2  # FRI (b, 3, 2) throughout


class Table:
    def __init__(self, air, trace, pis):
        self.air = air
        self.trace = np.ascontiguousarray(trace, dtype=np.uint32)
        self.pis = np.asarray(pis, dtype=np.uint32)
        self.tape = ts.air_tape(air, len(self.pis))
        self.lqd = ts.get_log_quotient_degree(air, len(self.pis))
        self.trace.setflags(write=False)

    @property
    def log_n(self):
        return self.trace.shape[0].bit_length() - 1


def fib(log_n, a=0, b=1):
    t = generate_fibonacci_trace(a, b, 1 << log_n)
    return Table(FibonacciAir(), t, fibonacci_public_values(t))


def mul(log_n, width):
    return Table(SynthMulAir(width), generate_synth_mul_trace(1 << log_n, width), [])


def high(log_n):
    return Table(HighDegreeAir(5), generate_high_degree_trace(1 << log_n), [])


def rnd(seed, log_n):
    air, _ = random_air_case(seed)
    trace, pis, _ = generate_random_air_trace(air, 1 << log_n)
    return Table(air, trace, pis)


def _build(name):
    if name == "a":  # two traces and their chunks in one class; the dot kernel's 64-column tile plus a tail
        return [fib(5), mul(5, 72)]
    if name == "b":  # unsorted, a class repeats, a class is missing between the two heights, the tallest not first
        return [fib(3), mul(6, 6), fib(3, 2, 5)]
    if name == "c":  # LDE above the FRI round threshold: k_leaf_tree rounds; shorter inputs join 6 and 12 rounds later
        return [mul(16, 8), fib(10), high(10), fib(4)]
    if name == "d_equal":  # quotient degrees 1, 2, 4 at one height
        return [fib(6), mul(6, 6), rnd(93, 6)]
    if name == "d_mixed":  # the same three degrees at three heights
        return [fib(4), mul(6, 9), rnd(90, 8)]
    if name == "e":  # full job tables: 64 + 64 matrices
        return [fib(3, k, k + 1) for k in range(64)]
    if name == "t1_fib":
        return [fib(3)]
    if name == "t1_mul":
        return [mul(10, 8)]
    raise KeyError(name)


CASE_NAMES = ("a", "b", "c", "d_equal", "d_mixed", "e")
_cache = {}


def case(name, log_blowup=2):
    """The tables of a case whose quotient degree fits the blowup (built once per name, never modified)."""
    if name not in _cache:
        _cache[name] = _build(name)
    return [t for t in _cache[name] if t.lqd <= log_blowup]


def config(ctx, log_blowup):
    return ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(log_blowup, FRI_QUERIES, FRI_POW), ctx))


def compiled(ctx, tables):
    """One CompiledAir per distinct tape (the 64 Fibonacci tables of case e share one)."""
    by_tape, out = {}, []
    for t in tables:
        key = np.asarray(t.tape).tobytes()
        if key not in by_tape:
            by_tape[key] = ts.CompiledAir(ctx, t.tape)
        out.append(by_tape[key])
    return out


def prove(config_, cairs, tables, chal=None):
    return ts.prove_multi(config_, cairs, chal or ts.BfChallenger(), [t.trace.copy() for t in tables],
                          [t.pis for t in tables])


def _mul_base(z, k):
    return np.array([int(x) * k % P for x in z], dtype=np.uint32)


def staged_proof(pcs, cairs, tables, chal):
    """The proof of ts_prove_multi from public stage calls: (trace root, quotient root, opened values (k, 4),
    FriProof words); `chal` ends in the prover's final state.  The chunks of a table come from that table's trace
    COMMITTED ALONE, so that the batch's LDE is pinned to the single-table one."""
    chal.observe(len(tables))
    for t in tables:
        chal.observe(t.log_n)
    root_t, data_t = pcs.commit([((t.log_n, 1), t.trace.copy()) for t in tables])
    chal.observe_commitment(root_t)
    alpha = chal.sample()
    entries = []
    for t, cair in zip(tables, cairs):
        _, alone = pcs.commit([((t.log_n, 1), t.trace.copy())])
        chunks = pcs.quotient_chunks(alone, cair, t.pis, alpha)
        g = pow(G27, 1 << (27 - (t.log_n + t.lqd)), P) if t.log_n + t.lqd else 1
        entries += [((t.log_n, 31 * pow(g, c, P) % P), m) for c, m in enumerate(chunks)]
    root_q, data_q = pcs.commit(entries)
    chal.observe_commitment(root_q)
    zeta = chal.sample()
    points = [[zeta, _mul_base(zeta, pow(G27, 1 << (27 - t.log_n), P))] for t in tables]
    opened, fri = pcs.open([(data_t, points), (data_q, [[zeta]] * len(entries))], chal)
    flat = np.concatenate([v for rnd_ in opened for m in rnd_ for v in m])
    return root_t, root_q, flat, fri


def header_words(tables):
    out = [0x46505354, 6, len(tables)]
    for t in tables:
        out += [t.log_n, t.trace.shape[1], 1 << t.lqd]
    return out


def regions(tables):
    """Word ranges of a v6 proof of `tables`: name -> (first, end)."""
    T = len(tables)
    o = 3 + 3 * T
    r = {"header": (0, 3), "tables": (3, o), "trace_root": (o, o + 8), "quotient_root": (o + 8, o + 16)}
    o += 16
    r["trace_values"] = []
    for t in tables:
        w = t.trace.shape[1]
        r["trace_values"].append((o, o + 8 * w))
        o += 8 * w
    r["chunk_values"] = []
    for t in tables:
        r["chunk_values"].append((o, o + 16 * (1 << t.lqd)))
        o += 16 * (1 << t.lqd)
    r["fri"] = (o, None)
    return r


def length_fields(words, first):
    """Indices of the count and length words of the FriProof that starts at words[first]: R, Q, then per query the
    batch count, per batch the matrix count, every row width and the path length, per round the path length."""
    at, o = [first], first
    R = int(words[o])
    o += 1 + 8 * R
    at.append(o)
    Q = int(words[o])
    o += 1
    for _ in range(Q):
        at.append(o)
        nb = int(words[o])
        o += 1
        for _ in range(nb):
            at.append(o)
            nm = int(words[o])
            o += 1
            for _ in range(nm):
                at.append(o)
                o += 1 + int(words[o])
            at.append(o)
            o += 1 + 8 * int(words[o])
        for _ in range(R):
            o += 8
            at.append(o)
            o += 1 + 8 * int(words[o])
    assert o + 5 == len(words)
    return at


def write_golden(ctx=None):
    """Writes tests/golden/multi_proof_small.json on a machine with a GPU: case b at log_blowup 1, FRI (1, 3, 2)
    -- the proof words of ts_prove_multi, the three tapes and the public values.  The fixture is this library's
    own output (the oracle has no multi-table prover); tests/test_gpu_multi.py checks that a fresh proof still
    equals it, tests/test_multi_cpu.py verifies and corrupts it without a GPU.

        python -c "import sys; sys.path[:0] = ['.', 'tests']; import _multi_cases as m; m.write_golden()"
    """
    ctx = ctx or ts.default_context()
    tables = case("b", 1)
    cfg = config(ctx, 1)
    proof = prove(cfg, compiled(ctx, tables), tables)
    ts.verify_multi(cfg, [ts.CompiledAir(None, t.tape) for t in tables], ts.BfChallenger(), proof,
                    [t.pis for t in tables])
    doc = {"case": "b", "fri": [1, FRI_QUERIES, FRI_POW], "tapes": [[int(x) for x in t.tape] for t in tables],
           "public_values": [[int(x) for x in t.pis] for t in tables], "proof": [int(x) for x in proof.words]}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    return doc


def load_golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    return (doc, [np.array(t, dtype=np.uint32) for t in doc["tapes"]],
            [np.array(p, dtype=np.uint32) for p in doc["public_values"]], np.array(doc["proof"], dtype=np.uint32))
