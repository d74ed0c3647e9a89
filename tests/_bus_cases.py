"""The statements of tests/test_gpu_multi_bus.py and tests/test_multi_bus_cpu.py: tables of mixed heights tied by a
LogUp bus for ``ts_prove_multi_bus``, the Python staging that pins such a proof to public stage calls, and the
writer of the fixture tests/golden/multi_bus_proof_small.json.

A table is (air, trace, public values, LogUp or None).  Senders (BusSendAir(k)) put (BUS_TAG, value) on the bus,
one range table (BusRangeAir) takes every value off as often as it was sent; plain tables (FibonacciAir,
SynthMulAir) sit beside them.  Sender values are drawn below the range table's height, so every case balances."""
import json
import os

import numpy as np

import tapstark_amd as ts
from tapstark_amd.air import aux_dims
from tapstark_amd.airs import (BusRangeAir, BusSendAir, FibonacciAir, SynthMulAir, fibonacci_public_values,
                               generate_bus_range_trace, generate_bus_send_trace, generate_fibonacci_trace,
                               generate_synth_mul_trace)

P = 0x78000001
G27 = 0x1A427A41  # generator of the 2^27 subgroup
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_bus_proof_small.json")
FRI_QUERIES, FRI_POW = 3, 2  # FRI (b, 3, 2) throughout


class Table:
    def __init__(self, air, trace, pis=()):
        self.air = air
        self.trace = np.ascontiguousarray(trace, dtype=np.uint32)
        self.pis = np.asarray(pis, dtype=np.uint32)
        self.tape = ts.air_tape(air, len(self.pis), 0, *aux_dims(air))
        self.logup = getattr(air, "logup", None)
        self.aux_width = self.logup.aux_width if self.logup is not None else 0
        self.lqd = ts.CompiledAir(None, self.tape).log_quotient_degree
        self.trace.setflags(write=False)

    @property
    def log_n(self):
        return self.trace.shape[0].bit_length() - 1


def send(k, log_n, table_log_n, seed):
    return Table(BusSendAir(k), generate_bus_send_trace(1 << log_n, k, 1 << table_log_n, seed))


def rng(log_n, senders):
    return Table(BusRangeAir(), generate_bus_range_trace(1 << log_n, [s.trace for s in senders]))


def fib(log_n):
    t = generate_fibonacci_trace(0, 1, 1 << log_n)
    return Table(FibonacciAir(), t, fibonacci_public_values(t))


def mul(log_n, width):
    return Table(SynthMulAir(width), generate_synth_mul_trace(1 << log_n, width))


def _build(name):
    if name == "a":  # one class
        s = send(1, 5, 5, 11)
        return [s, rng(5, [s])]
    if name == "b":  # the receiver shorter than a sender; a plain table inside (the aux batch skips a table, a class
        # has traces and no aux matrix); K = 5 crosses the batch of four denominators and ends on an odd group; 2 rows
        s2, s5, s1 = send(2, 6, 3, 21), send(5, 3, 3, 22), send(1, 1, 3, 24)  # (seed 24: one of the two rows sends)
        return [rng(3, [s2, s5, s1]), fib(4), s2, s5, s1]
    if name == "c":  # several builder workgroups per table at the default block rows
        s = send(2, 12, 8, 31)
        return [s, rng(8, [s]), mul(10, 8)]
    if name == "e":  # 64 chunks; 32 + 32 + 64 jobs in one class
        ss = [send(1, 3, 3, 40 + k) for k in range(31)]
        return ss + [rng(3, ss)]
    if name == "t1":  # one table that balances alone: every selector is 0
        t = generate_bus_send_trace(1 << 4, 2, 1 << 4, 51).copy()
        t[:, 1::2] = 0
        return [Table(BusSendAir(2), t)]
    if name == "unbalanced":  # case a with one sent value outside the table
        s, r = case("a")
        t = s.trace.copy()
        t[3] = (1 << 5, 1)
        bad = Table(BusSendAir(1), t)
        return [bad, rng(5, [bad])]
    raise KeyError(name)


CASE_NAMES = ("a", "b", "c", "e")
_cache = {}


def case(name):
    """The tables of a case (built once per name, never modified).  Every bus AIR has constraint degree 3 and every
    plain one at most that, so each case fits log_blowup 1 and 2."""
    if name not in _cache:
        _cache[name] = _build(name)
    return list(_cache[name])


def config(ctx, log_blowup):
    return ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(log_blowup, FRI_QUERIES, FRI_POW), ctx))


def compiled(ctx, tables):
    """One CompiledAir per distinct tape (the 31 senders of case e share one)."""
    by_tape, out = {}, []
    for t in tables:
        key = np.asarray(t.tape).tobytes()
        if key not in by_tape:
            by_tape[key] = ts.CompiledAir(ctx, t.tape)
        out.append(by_tape[key])
    return out


def prove(config_, cairs, tables, chal=None):
    return ts.prove_multi_bus(config_, cairs, chal or ts.BfChallenger(), [t.trace.copy() for t in tables],
                              [t.pis for t in tables], [t.logup for t in tables])


def verify(config_, tables, proof, check_bus=True):
    return ts.verify_multi_bus(config_, [ts.CompiledAir(None, t.tape) for t in tables], ts.BfChallenger(), proof,
                               [t.pis for t in tables], check_bus=check_bus)


def _mul_base(z, k):
    return np.array([int(x) * k % P for x in z], dtype=np.uint32)


def staged_proof(pcs, cairs, tables, chal):
    """The proof of ts_prove_multi_bus from public stage calls: (trace root, aux root, exposed (A, 4), quotient root,
    opened values (k, 4), FriProof words); `chal` ends in the prover's final state.  The aux matrix of a table comes
    from the SINGLE-table builder, and its chunks from its trace and its aux matrix each COMMITTED ALONE."""
    ctx = pcs.ctx
    chal.observe(len(tables))
    for t in tables:
        chal.observe(t.log_n)
    root_t, data_t = pcs.commit([((t.log_n, 1), t.trace.copy()) for t in tables])
    chal.observe_commitment(root_t)
    ch = np.concatenate([chal.sample(), chal.sample()]).astype(np.uint32)
    auxs, exposed = {}, {}
    for k, t in enumerate(tables):
        if t.logup is not None:
            m, ex = t.logup.build(ts.DeviceMatrix.upload(ctx, t.trace.copy()), ch)
            auxs[k], exposed[k] = m.download(), np.asarray(ex, dtype=np.uint32)
    root_a, data_a = pcs.commit([((tables[k].log_n, 1), auxs[k].copy()) for k in auxs])
    chal.observe_commitment(root_a)
    for k in auxs:
        for e in exposed[k]:
            chal.observe(int(e))
    alpha = chal.sample()
    entries = []
    for k, (t, cair) in enumerate(zip(tables, cairs)):
        _, alone = pcs.commit([((t.log_n, 1), t.trace.copy())])
        if k in auxs:
            _, alone_a = pcs.commit([((t.log_n, 1), auxs[k].copy())])
            chunks = pcs.quotient_chunks(alone, cair, t.pis, alpha, aux=alone_a, challenges=ch, exposed=exposed[k])
        else:
            chunks = pcs.quotient_chunks(alone, cair, t.pis, alpha)
        g = pow(G27, 1 << (27 - (t.log_n + t.lqd)), P) if t.log_n + t.lqd else 1
        entries += [((t.log_n, 31 * pow(g, c, P) % P), m) for c, m in enumerate(chunks)]
    root_q, data_q = pcs.commit(entries)
    chal.observe_commitment(root_q)
    zeta = chal.sample()
    points = [[zeta, _mul_base(zeta, pow(G27, 1 << (27 - t.log_n), P))] for t in tables]
    opened, fri = pcs.open([(data_a, [points[k] for k in auxs]), (data_t, points),
                            (data_q, [[zeta]] * len(entries))], chal)
    flat = np.concatenate([v for rnd_ in opened for m in rnd_ for v in m])
    ex = np.array([exposed[k] for k in auxs], dtype=np.uint32).reshape(-1, 4)
    return root_t, root_a, ex, root_q, flat, fri


def header_words(tables):
    out = [0x46505354, 7, len(tables)]
    for t in tables:
        out += [t.log_n, t.trace.shape[1], 1 << t.lqd, t.aux_width, 4 if t.aux_width else 0]
    return out


def regions(tables):
    """Word ranges of a v7 proof of `tables`: name -> (first, end), or a list of them per table."""
    T = len(tables)
    A = sum(1 for t in tables if t.aux_width)
    o = 3 + 5 * T
    r = {"header": (0, 3), "tables": (3, o), "trace_root": (o, o + 8), "aux_root": (o + 8, o + 16),
         "exposed": (o + 16, o + 16 + 4 * A)}
    o += 16 + 4 * A
    r["quotient_root"] = (o, o + 8)
    o += 8
    r["opened"] = o
    for name, width in (("aux_values", lambda t: 8 * t.aux_width), ("trace_values", lambda t: 8 * t.trace.shape[1]),
                        ("chunk_values", lambda t: 16 * (1 << t.lqd))):
        r[name] = []
        for t in tables:
            r[name].append((o, o + width(t)))
            o += width(t)
    r["fri"] = (o, None)
    return r


def write_golden(ctx=None):
    """Writes tests/golden/multi_bus_proof_small.json on a machine with a GPU: case b at log_blowup 1, FRI (1, 3, 2)
    -- the proof words of ts_prove_multi_bus, the five tapes and the public values.  The fixture is this library's
    own output; tests/test_gpu_multi_bus.py checks that a fresh proof still equals it, tests/test_multi_bus_cpu.py
    verifies and corrupts it without a GPU.

        python -c "import sys; sys.path[:0] = ['.', 'tests']; import _bus_cases as m; m.write_golden()"
    """
    ctx = ctx or ts.default_context()
    tables = case("b")
    cfg = config(ctx, 1)
    proof = prove(cfg, compiled(ctx, tables), tables)
    _, bus_sum = verify(cfg, tables, proof)
    assert not bus_sum.any()
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
