"""The statements of tests/test_gpu_single_golden.py and tests/test_single_cpu.py: one single-table proof of each
wire format that has a key or an aux source (TSPF v1, v3, v4, v5), the four ts_verify* entry points as one call,
and the writer of the fixture tests/golden/single_proofs_small.json.

    fib       FibonacciAir                       ts_prove          v1
    selector  SelectorAir + PreprocessedKey      ts_prove_pre      v3
    range     RangeLookupAir + its LogUp source  ts_prove_aux      v4
    table     TableLookupAir + key + source      ts_prove_pre_aux  v5

Every case has the smallest height the suite proves its AIR at (two rows), log_blowup 1 and FRI (1, 3, 2)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.air import aux_dims
from tapstark_amd.airs import (FibonacciAir, RangeLookupAir, SelectorAir, TableLookupAir, fibonacci_public_values,
                               generate_fibonacci_trace, generate_lookup_table, generate_range_lookup_trace,
                               generate_selector_preprocessed, generate_selector_trace, generate_table_lookup_trace)

P = 0x78000001
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "single_proofs_small.json")
FRI = (1, 3, 2)
LOG_N = 1
CASE_NAMES = ("fib", "selector", "range", "table")
VERSION = {"fib": 1, "selector": 3, "range": 4, "table": 5}
ENTRIES = ("ts_verify", "ts_verify_pre", "ts_verify_aux", "ts_verify_pre_aux")
OWN_ENTRY = dict(zip(CASE_NAMES, ENTRIES))
# fixed stage inputs of the quotient and check_constraints records: alpha, then gamma and beta
ALPHA = np.array([11, 22, 33, 44], dtype=np.uint32)
CHALLENGES = np.array([5, 6, 7, 8, 9, 10, 11, 12], dtype=np.uint32)


class Statement:
    """(air, tape, trace, public values, preprocessed matrix or None, LogUp or None) of a case; arrays read-only."""

    def __init__(self, name, log_n=LOG_N):
        n = 1 << log_n
        self.name, self.log_n, self.prep, self.logup = name, log_n, None, None
        if name == "fib":
            self.air = FibonacciAir()
            self.trace = generate_fibonacci_trace(0, 1, n)
            self.pis = fibonacci_public_values(self.trace)
            self.tape = ts.air_tape(self.air, 3)
        elif name == "selector":
            self.air = SelectorAir()
            self.prep = generate_selector_preprocessed(n)
            self.trace, self.pis = generate_selector_trace(self.prep)
            self.tape = ts.air_tape(self.air, 2, 3)
        elif name == "range":
            self.air, self.logup = RangeLookupAir(), RangeLookupAir.logup
            self.trace, self.pis = generate_range_lookup_trace(n), np.zeros(0, dtype=np.uint32)
            self.tape = ts.air_tape(self.air, 0, 0, *aux_dims(self.air))
        elif name == "table":
            self.air, self.logup = TableLookupAir(), TableLookupAir.logup
            self.prep = generate_lookup_table(n)
            self.trace, self.pis = generate_table_lookup_trace(n), np.zeros(0, dtype=np.uint32)
            self.tape = ts.air_tape(self.air, 0, 1, *aux_dims(self.air))
        else:
            raise KeyError(name)
        self.trace = np.ascontiguousarray(self.trace, dtype=np.uint32)
        self.pis = np.asarray(self.pis, dtype=np.uint32)
        for a in (self.trace, self.pis, self.prep):
            if a is not None:
                a.setflags(write=False)


class Lane:
    """A statement on one context: config, compiled AIR, key and aux source."""

    def __init__(self, ctx, st):
        self.ctx, self.st = ctx, st
        self.config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*FRI), ctx))
        self.cair = ts.CompiledAir(ctx, st.tape)
        self.key = None if st.prep is None else ts.PreprocessedKey(self.config, st.prep.copy(), keep_values=True)

    def source(self):
        if self.st.logup is None:
            return None
        return self.st.logup.aux_source_with(self.key.values) if self.key is not None else self.st.logup.aux_source

    def prove(self):
        return ts.prove(self.config, self.cair, ts.BfChallenger(), self.st.trace.copy(), self.st.pis,
                        preprocessed=self.key, aux=self.source()).words

    def stages(self):
        """(sha256 of the quotient chunks' words for ALPHA and CHALLENGES, check_constraints of the trace,
        check_constraints of the trace with one word of its last row changed)."""
        st, pcs, ctx = self.st, self.config.pcs, self.ctx
        aux = ch = ex = aux_data = None
        if st.logup is not None:
            ch = CHALLENGES
            m, ex = st.logup.build(ts.DeviceMatrix.upload(ctx, st.trace), ch,
                                   self.key.values if self.key is not None else None)
            aux = m.download()
            _, aux_data = pcs.commit([((st.log_n, 1), aux.copy())])
        _, data = pcs.commit([((st.log_n, 1), st.trace.copy())])
        chunks = pcs.quotient_chunks(data, self.cair, st.pis, ALPHA, preprocessed=self.key, aux=aux_data,
                                     challenges=ch, exposed=ex)
        digest = hashlib.sha256(b"".join(c.download().astype("<u4").tobytes() for c in chunks)).hexdigest()
        bad = st.trace.copy()
        bad[-1, 0] = (int(bad[-1, 0]) + 1) % P
        check = [ts.check_constraints(self.cair, t, st.pis, ctx, preprocessed=st.prep, aux=aux, challenges=ch,
                                      exposed=ex) for t in (st.trace.copy(), bad)]
        return digest, check[0], check[1]


def prove_batch(lanes):
    """The four statements through ts_prove_batch_lookup, one lane each: (v5 words, exposed words) per case."""
    res = ts.prove_batch_lookup([(ln.config, ln.cair) for ln in lanes], [ln.st.trace.copy() for ln in lanes],
                                list(range(len(lanes))), public_values=[ln.st.pis for ln in lanes],
                                keys=[ln.key for ln in lanes], logups=[ln.st.logup for ln in lanes])
    return [(res.proofs[i].words, res.exposed[i]) for i in range(len(lanes))]


def launch_counts(lane):
    """kernel name -> launches of one proof of the lane's statement."""
    lane.prove()  # specialisation and pool growth stay out of the count
    lane.ctx.set_kernel_timing(True)
    lane.ctx.take_kernel_timings()
    lane.prove()
    out = {k: n for k, (n, _) in lane.ctx.take_kernel_timings().items()}
    lane.ctx.set_kernel_timing(False)
    return out


# ------------------------------------------------------------------ the verify family (host only)
def _ptr(a):
    return a.ctypes.data_as(_lib.u32p) if a is not None and len(a) else None


def verify_call(entry, tape, words, pis, root=None, cap_exposed=None, null_exposed=False):
    """One ts_verify* call on a fresh challenger: (status, verdict, text, exposed words).  `root` and the exposed
    buffer go to the entry points that take them; `cap_exposed` defaults to the AIR's count.  The text is that of
    ts_last_error(NULL), "" on TS_OK."""
    l = _lib.lib()
    cair = ts.CompiledAir(None, tape)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    pis = np.ascontiguousarray(pis, dtype=np.uint32)
    root = None if root is None else np.ascontiguousarray(root, dtype=np.uint32)
    cfg, chal, verdict = ts.FriConfig(*FRI)._c(), ts.BfChallenger(), C.c_int(-1)
    exposed = np.zeros(max(cair.n_exposed, 1), dtype=np.uint32)
    cap = cair.n_exposed if cap_exposed is None else cap_exposed
    args = [C.byref(cfg), cair.h, chal.h]
    if entry in ("ts_verify_pre", "ts_verify_pre_aux"):
        args.append(_ptr(root))
    args += [_ptr(words), len(words), _ptr(pis), len(pis)]
    if entry in ("ts_verify_aux", "ts_verify_pre_aux"):
        args += [None if null_exposed or not cair.n_exposed else _ptr(exposed), cap]
    rc = getattr(l, entry)(*args, C.byref(verdict))
    text = (l.ts_last_error(None) or b"").decode() if rc else ""
    return int(rc), int(verdict.value), text, exposed[:cair.n_exposed] if rc == 0 and verdict.value == 0 else None


def verify_matrix(doc):
    """case -> entry -> [status, verdict, text]: every golden proof at every entry point, with its own AIR and, where
    the AIR has preprocessed columns, its key root."""
    return {name: {e: list(verify_call(e, c["tape"], c["proof"], c["public_values"], c["key_root"])[:3])
                   for e in ENTRIES} for name, c in doc["cases"].items()}


def refusal_variants(name, c):
    """(label, arguments of verify_call) of the refused forms of a golden at its own entry point: truncated, a changed
    header word 5 to 8, a null root, a short or null buffer for the exposed words."""
    words, base = np.array(c["proof"], dtype=np.uint32), (c["tape"],)
    out = [("truncated by one", (*base, words[:-1], c["public_values"], c["key_root"]), {}),
           ("truncated to six words", (*base, words[:6], c["public_values"], c["key_root"]), {})]
    for k in (5, 6, 7, 8):
        w = words.copy()
        w[k] ^= 1
        out.append((f"header word {k} changed", (*base, w, c["public_values"], c["key_root"]), {}))
    if c["key_root"] is not None:
        out.append(("null root", (*base, words, c["public_values"], None), {}))
    if len(c["exposed"]):
        out.append(("short exposed_out", (*base, words, c["public_values"], c["key_root"]),
                    {"cap_exposed": len(c["exposed"]) - 1}))
        out.append(("null exposed_out", (*base, words, c["public_values"], c["key_root"]), {"null_exposed": True}))
    return out


def refusals(doc):
    return {name: {label: list(verify_call(OWN_ENTRY[name], *args, **kw)[:3])
                   for label, args, kw in refusal_variants(name, c)} for name, c in doc["cases"].items()}


def write_golden(ctxs=None):
    """Writes tests/golden/single_proofs_small.json on a machine with a GPU.  Per case: the tape, the public values,
    the key root, the exposed words and the proof words of its own prove call; the v5 proof and exposed words of the
    same statement through ts_prove_batch_lookup; the digest of its quotient chunks and its two check_constraints
    results.  Then, host only, what every ts_verify* entry point answers to every proof and to its refused forms.
    The fixture is this library's own output, tied to the oracle by the v1 case (orc.prove gives the same words).

        python -c "import sys; sys.path[:0] = ['.', 'tests']; import _single_cases as s; s.write_golden()"
    """
    from oracle import oracle_py as orc

    ctxs = ctxs or [ts.default_context()] + [ts.Context(0) for _ in range(3)]
    lanes = [Lane(ctx, Statement(name)) for ctx, name in zip(ctxs, CASE_NAMES)]
    doc = {"fri": list(FRI), "log_n": LOG_N, "cases": {}}
    batch = prove_batch(lanes)
    for ln, (b_words, b_exposed) in zip(lanes, batch):
        st = ln.st
        words = ln.prove()
        root = None if ln.key is None else [int(x) for x in ln.key.root]
        exposed = ts.verify(ln.config, ts.CompiledAir(None, st.tape), ts.BfChallenger(), words, st.pis,
                            preprocessed_root=root)
        assert int(words[1]) == VERSION[st.name] and int(b_words[1]) == 5
        digest, check, check_bad = ln.stages()
        assert check == -1 and check_bad >= 0
        doc["cases"][st.name] = {
            "version": VERSION[st.name], "tape": [int(x) for x in st.tape], "public_values": [int(x) for x in st.pis],
            "key_root": root, "exposed": [int(x) for x in (exposed if exposed is not None else [])],
            "proof": [int(x) for x in words], "batch_proof": [int(x) for x in b_words],
            "batch_exposed": [int(x) for x in b_exposed], "chunks_sha256": digest, "check": check,
            "check_bad": check_bad}
    doc["verify"] = verify_matrix(doc)
    doc["refusals"] = refusals(doc)
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    fib = lanes[0].st
    want = orc.prove(orc.FriConfig(*FRI), fib.tape, fib.trace, fib.pis)
    assert np.array_equal(want, np.array(doc["cases"]["fib"]["proof"], dtype=np.uint32)), "v1 differs from the oracle"
    assert all(c["check"] == -1 and c["check_bad"] >= 0 for c in doc["cases"].values())
    return doc


_doc = None


def load_golden():
    global _doc
    if _doc is None:
        with open(GOLDEN) as f:
            _doc = json.load(f)
    return _doc
