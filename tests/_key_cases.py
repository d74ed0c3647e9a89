"""The statements of tests/test_gpu_multi_key.py and tests/test_multi_key_cpu.py: tables of mixed heights on a LogUp
bus whose receiving tables are FIXED -- preprocessed columns in a commit-once key -- for ``ts_prove_multi_key``, the
Python staging that pins such a proof to public stage calls, and the writer of the fixture
tests/golden/multi_key_proof_small.json.

A table is (air, trace, public values, LogUp or None, key matrix or None).  The i-th table with a key matrix reads
matrix i of the case's key.  Senders (BusSendAir, BusTupleSendAir) draw their tuples from the key table they look
up, so every case balances by construction."""
import json
import os

import numpy as np

import tapstark_amd as ts
from tapstark_amd.air import aux_dims
from tapstark_amd.airs import (BUS_TAG, BusKeyTableAir, BusSendAir, BusTupleSendAir, FibonacciAir, SelectorAir,
                               TableLookupAir, fibonacci_public_values, generate_bus_send_trace,
                               generate_fibonacci_trace, generate_key_table_trace, generate_lookup_table,
                               generate_range_key, generate_selector_preprocessed, generate_selector_trace,
                               generate_table_lookup_trace, generate_xor_key, generate_xor_send_trace, selected_tuples)

P = 0x78000001
G27 = 0x1A427A41  # generator of the 2^27 subgroup
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_key_proof_small.json")
FRI_QUERIES, FRI_POW = 3, 2  # FRI (b, 3, 2) throughout
XOR_TAG = 11                 # the second bus: (XOR_TAG, a, b, a xor b) never meets (BUS_TAG, value) in a denominator


class Table:
    def __init__(self, air, trace, pis=(), key=None):
        self.air = air
        self.trace = np.ascontiguousarray(trace, dtype=np.uint32)
        self.pis = np.asarray(pis, dtype=np.uint32)
        self.key = None if key is None else np.ascontiguousarray(key, dtype=np.uint32)
        self.prep_width = 0 if key is None else self.key.shape[1]
        self.tape = ts.air_tape(air, len(self.pis), self.prep_width, *aux_dims(air))
        self.logup = getattr(air, "logup", None)
        self.aux_width = self.logup.aux_width if self.logup is not None else 0
        self.lqd = ts.CompiledAir(None, self.tape).log_quotient_degree
        self.trace.setflags(write=False)
        if self.key is not None:
            self.key.setflags(write=False)

    @property
    def log_n(self):
        return self.trace.shape[0].bit_length() - 1


def send(k, log_n, table_log_n, seed):
    return Table(BusSendAir(k), generate_bus_send_trace(1 << log_n, k, 1 << table_log_n, seed))


def xsend(k, log_n, bits, seed):
    return Table(BusTupleSendAir(XOR_TAG, k, 3), generate_xor_send_trace(1 << log_n, k, bits, seed))


def range_key(log_n, senders):
    key = generate_range_key(1 << log_n)
    sent = np.concatenate([selected_tuples(s.trace, 1) for s in senders])
    return Table(BusKeyTableAir(BUS_TAG, 1), generate_key_table_trace(key, sent), key=key)


def xor_key(bits, senders):
    key = generate_xor_key(bits)
    sent = np.concatenate([selected_tuples(s.trace, 3) for s in senders])
    return Table(BusKeyTableAir(XOR_TAG, 3), generate_key_table_trace(key, sent), key=key)


def fib(log_n):
    t = generate_fibonacci_trace(0, 1, 1 << log_n)
    return Table(FibonacciAir(), t, fibonacci_public_values(t))


def selector(log_n):
    prep = generate_selector_preprocessed(1 << log_n)
    t, pis = generate_selector_trace(prep)
    return Table(SelectorAir(), t, pis, key=prep)


def _build(name):
    if name == "ka":  # one class
        s = send(1, 5, 5, 11)
        return [s, range_key(5, [s])]
    if name == "kb":  # key matrices of two heights and two widths; every table kind (plain, key-only, aux-only, key and
        # aux); two buses told apart by tag; a receiver shorter than a sender; a sender of two rows
        s2, s5 = send(2, 6, 3, 21), send(5, 3, 3, 22)
        x = generate_xor_send_trace(2, 1, 2, 24).copy()
        x[:, 3] = (1, 0)  # one of the two rows sends
        x1 = Table(BusTupleSendAir(XOR_TAG, 1, 3), x)
        return [range_key(3, [s2, s5]), fib(4), selector(3), s2, s5, xor_key(2, [x1]), x1]
    if name == "kc":  # several builder workgroups per table at the default block rows
        s, x = send(2, 12, 8, 31), xsend(2, 10, 4, 32)
        return [s, range_key(8, [s]), x, xor_key(4, [x])]
    if name == "ke":  # 64 key + 64 aux + 64 trace + 64 chunk jobs in ONE class: 64 tables of one chunk each.  A key
        # table's multiplicity column is free, so table 2i puts its rows ON the bus (+m) and table 2i+1 takes them off
        key = generate_range_key(8)
        out = []
        for i in range(32):
            m = (np.arange(8, dtype=np.uint32) * (i + 1) + i) % 5 + (1 if i == 0 else 0)
            out.append(Table(BusKeyTableAir(BUS_TAG, 1), m.reshape(8, 1), key=key))
            out.append(Table(BusKeyTableAir(BUS_TAG, 1), ((P - m) % P).reshape(8, 1), key=key))
        return out
    if name == "k0":  # no aux table: the challenge phase is skipped whole
        return [selector(3), fib(4)]
    if name == "kt1":  # one TableLookupAir table that balances alone
        return [Table(TableLookupAir(), generate_table_lookup_trace(1 << 4), key=generate_lookup_table(1 << 4))]
    if name == "unbalanced":  # case ka with one sent value outside the table
        s, r = case("ka")
        t = s.trace.copy()
        t[3] = (1 << 5, 1)
        bad = Table(BusSendAir(1), t)
        return [bad, range_key(5, [bad])]
    raise KeyError(name)


CASE_NAMES = ("ka", "kb", "kc", "ke", "k0")
_cache = {}


def case(name):
    """The tables of a case (built once per name, never modified).  Every AIR has constraint degree at most 3, so each
    case fits log_blowup 1 and 2; a BusKeyTableAir and a BusTupleSendAir(k = 1) have degree 2: one chunk."""
    if name not in _cache:
        _cache[name] = _build(name)
    return list(_cache[name])


def config(ctx, log_blowup):
    return ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(log_blowup, FRI_QUERIES, FRI_POW), ctx))


def compiled(ctx, tables):
    """One CompiledAir per distinct tape."""
    by_tape, out = {}, []
    for t in tables:
        key = np.asarray(t.tape).tobytes()
        if key not in by_tape:
            by_tape[key] = ts.CompiledAir(ctx, t.tape)
        out.append(by_tape[key])
    return out


def key_matrices(tables):
    return [t.key for t in tables if t.key is not None]


def make_key(config_, tables, keep_values=True):
    return ts.MultiKey(config_, [m.copy() for m in key_matrices(tables)], keep_values=keep_values)


def prove(config_, key, cairs, tables, chal=None):
    return ts.prove_multi_key(config_, key, cairs, chal or ts.BfChallenger(), [t.trace.copy() for t in tables],
                              [t.pis for t in tables], [t.logup for t in tables])


def verify(config_, key_root, tables, proof, check_bus=True):
    return ts.verify_multi_key(config_, key_root, [ts.CompiledAir(None, t.tape) for t in tables], ts.BfChallenger(),
                               proof, [t.pis for t in tables], check_bus=check_bus)


def _mul_base(z, k):
    return np.array([int(x) * k % P for x in z], dtype=np.uint32)


def staged_proof(pcs, cairs, tables, chal):
    """The proof of ts_prove_multi_key from public stage calls: (key root, trace root, aux root or None, exposed (A, 4),
    quotient root, opened values (k, 4), FriProof words); `chal` ends in the prover's final state.  The key root is
    ts_pcs_commit's of the key list; the aux matrix of a table comes from the SINGLE-table builder
    (ts_logup_aux_build_pre where the table has a key matrix), and its chunks from its key matrix, its aux matrix and
    its trace each COMMITTED ALONE."""
    ctx = pcs.ctx
    chal.observe(len(tables))
    for t in tables:
        chal.observe(t.log_n)
    keyed = [k for k, t in enumerate(tables) if t.key is not None]
    root_k, data_k = pcs.commit([((tables[k].log_n, 1), tables[k].key.copy()) for k in keyed])
    chal.observe_commitment(root_k)
    root_t, data_t = pcs.commit([((t.log_n, 1), t.trace.copy()) for t in tables])
    chal.observe_commitment(root_t)
    auxs, exposed, ch, root_a, data_a = {}, {}, None, None, None
    if any(t.logup is not None for t in tables):
        ch = np.concatenate([chal.sample(), chal.sample()]).astype(np.uint32)
        for k, t in enumerate(tables):
            if t.logup is not None:
                pre = ts.DeviceMatrix.upload(ctx, t.key.copy()) if t.key is not None else None
                m, ex = t.logup.build(ts.DeviceMatrix.upload(ctx, t.trace.copy()), ch, preprocessed=pre)
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
        kw = {}
        if t.key is not None:
            kw["preprocessed"] = pcs.commit([((t.log_n, 1), t.key.copy())])[1]
        if k in auxs:
            kw.update(aux=pcs.commit([((t.log_n, 1), auxs[k].copy())])[1], challenges=ch, exposed=exposed[k])
        chunks = pcs.quotient_chunks(alone, cair, t.pis, alpha, **kw)
        g = pow(G27, 1 << (27 - (t.log_n + t.lqd)), P) if t.log_n + t.lqd else 1
        entries += [((t.log_n, 31 * pow(g, c, P) % P), m) for c, m in enumerate(chunks)]
    root_q, data_q = pcs.commit(entries)
    chal.observe_commitment(root_q)
    zeta = chal.sample()
    points = [[zeta, _mul_base(zeta, pow(G27, 1 << (27 - t.log_n), P))] for t in tables]
    rounds = [(data_k, [points[k] for k in keyed])]
    if auxs:
        rounds.append((data_a, [points[k] for k in auxs]))
    rounds += [(data_t, points), (data_q, [[zeta]] * len(entries))]
    opened, fri = pcs.open(rounds, chal)
    flat = np.concatenate([v for rnd_ in opened for m in rnd_ for v in m])
    ex = np.array([exposed[k] for k in auxs], dtype=np.uint32).reshape(-1, 4)
    return root_k, root_t, root_a, ex, root_q, flat, fri


def header_words(tables):
    out = [0x46505354, 8, len(tables)]
    for t in tables:
        out += [t.log_n, t.trace.shape[1], 1 << t.lqd, t.aux_width, 4 if t.aux_width else 0, t.prep_width]
    return out


def regions(tables):
    """Word ranges of a v8 proof of `tables`: name -> (first, end), or a list of them per table.  Without an aux
    table the aux root and the exposed words are empty ranges."""
    T = len(tables)
    A = sum(1 for t in tables if t.aux_width)
    o = 3 + 6 * T
    r = {"header": (0, 3), "tables": (3, o), "trace_root": (o, o + 8)}
    o += 8
    r["aux_root"] = (o, o + (8 if A else 0))
    o += 8 if A else 0
    r["exposed"] = (o, o + 4 * A)
    o += 4 * A
    r["quotient_root"] = (o, o + 8)
    o += 8
    r["opened"] = o
    for name, width in (("key_values", lambda t: 8 * t.prep_width), ("aux_values", lambda t: 8 * t.aux_width),
                        ("trace_values", lambda t: 8 * t.trace.shape[1]), ("chunk_values", lambda t: 16 * (1 << t.lqd))):
        r[name] = []
        for t in tables:
            r[name].append((o, o + width(t)))
            o += width(t)
    r["fri"] = (o, None)
    return r


def write_golden(ctx=None):
    """Writes tests/golden/multi_key_proof_small.json on a machine with a GPU: case kb at log_blowup 1, FRI (1, 3, 2)
    -- the proof words of ts_prove_multi_key, the key root, the tapes and the public values.  The fixture is this
    library's own output; tests/test_gpu_multi_key.py checks that a fresh proof still equals it,
    tests/test_multi_key_cpu.py verifies and corrupts it without a GPU.

        python -c "import sys; sys.path[:0] = ['.', 'tests']; import _key_cases as m; m.write_golden()"
    """
    ctx = ctx or ts.default_context()
    tables = case("kb")
    cfg = config(ctx, 1)
    key = make_key(cfg, tables)
    proof = prove(cfg, key, compiled(ctx, tables), tables)
    _, bus_sum = verify(cfg, key.root, tables, proof)
    assert not bus_sum.any()
    doc = {"case": "kb", "fri": [1, FRI_QUERIES, FRI_POW], "key_root": [int(x) for x in key.root],
           "tapes": [[int(x) for x in t.tape] for t in tables],
           "public_values": [[int(x) for x in t.pis] for t in tables], "proof": [int(x) for x in proof.words]}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    return doc


def load_golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    return (doc, [np.array(t, dtype=np.uint32) for t in doc["tapes"]],
            [np.array(p, dtype=np.uint32) for p in doc["public_values"]], np.array(doc["proof"], dtype=np.uint32),
            np.array(doc["key_root"], dtype=np.uint32))
