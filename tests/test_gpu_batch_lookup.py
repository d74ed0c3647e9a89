"""ts_prove_batch_lookup on the GPU: AIRs with a preprocessed key, challenge-phase columns or both in batch lanes.
The call adds no kernel: per item it is ts_prove_pre_aux driven by a lane thread, so every check here is an
EQUALITY, word for word, with the solo call on the same context -- proof words, exposed words, final challenger
state, digest -- and the solo path itself is what test_gpu_pre_aux.py, test_gpu_aux.py and test_gpu_preprocessed.py
tie to the oracle.  Heights 2^3 and 2^10, FRI (1, 3, 2) and (2, 3, 2), as the solo whole-proof tests use."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.air import LogUp, aux_dims
from tapstark_amd.airs import (FibonacciAir, RangeLookupAir, SelectorAir, TableLookupAir, fibonacci_public_values,
                               generate_fibonacci_trace, generate_lookup_table, generate_range_lookup_trace,
                               generate_selector_preprocessed, generate_selector_trace, generate_table_lookup_trace)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _aux_airs  # noqa: E402,F401  (imported unchanged: the maps the solo tests rest on)
import _pre_aux_airs  # noqa: E402,F401
from _digests import hexd  # noqa: E402
from _poison import make_contexts  # noqa: E402

pytestmark = pytest.mark.gpu
P = 0x78000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_ERR_INVALID, TS_ERR_UNSUPPORTED, TS_ERR_INVARIANT, TS_ERR_BUFFER = 1, 4, 5, 6
SHAPES = [(3, 1), (3, 2), (10, 1), (10, 2)]  # (log_n, log_blowup)
NO_MISS = 2**64 - 1


class WideRangeAir(RangeLookupAir):
    """RangeLookupAir with a spare fourth main column: the width of a quotient chunk, the one column-major matrix
    the ABI makes."""

    def width(self) -> int:
        return 4


class Lane:
    """One lane: its context, (StarkConfig, CompiledAir), key, LogUp and a trace generator."""

    def __init__(self, ctx, kind, log_n, b):
        self.ctx, self.kind, self.n = ctx, kind, 1 << log_n
        self.config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(b, 3, 2), ctx))
        self.key = self.logup = None
        n = self.n
        if kind == "table":
            self.air = TableLookupAir()
            self.key = ts.PreprocessedKey(self.config, generate_lookup_table(n), keep_values=True)
            self.logup = self.air.logup
            tape = ts.air_tape(self.air, 0, 1, *aux_dims(self.air))
        elif kind in ("range", "wide"):
            self.air = RangeLookupAir() if kind == "range" else WideRangeAir()
            self.logup = self.air.logup
            tape = ts.air_tape(self.air, 0, 0, *aux_dims(self.air))
        elif kind == "selector":
            self.air = SelectorAir()
            self.prep = generate_selector_preprocessed(n)
            self.key = ts.PreprocessedKey(self.config, self.prep)
            tape = ts.air_tape(self.air, 2, 3)
        else:
            self.air = FibonacciAir()
            tape = ts.air_tape(self.air, 3)
        self.cair = ts.CompiledAir(ctx, tape)
        self.pair = (self.config, self.cair)

    def statement(self, seed):
        """(trace, public values) of this lane's AIR, different for every seed."""
        n = self.n
        if self.kind == "table":
            return generate_table_lookup_trace(n, seed=1000 + seed), []
        if self.kind == "range":
            return generate_range_lookup_trace(n, seed=2000 + seed), []
        if self.kind == "wide":
            return np.hstack([generate_range_lookup_trace(n, seed=2500 + seed),
                              np.full((n, 1), seed, dtype=np.uint32)]), []
        if self.kind == "selector":
            return generate_selector_trace(self.prep, a0=3 + seed, b0=5 + 2 * seed)
        t = generate_fibonacci_trace(seed, 2 * seed + 1, n)
        return t, fibonacci_public_values(t)

    def source(self):
        if self.logup is None:
            return None
        return self.logup.aux_source_with(self.key.values) if self.key is not None else self.logup.aux_source

    def solo(self, trace, pis, chal):
        """The solo reference on this lane's context: (v5 words, exposed words, final challenger state).
        ts.prove(config, cair, clone, trace, pis, preprocessed=key, aux=source) on one clone of `chal`, and
        ts_prove_pre_aux itself on another.  For an AIR with both widths ts.prove IS that call; for the others it is
        ts_prove_aux / ts_prove_pre / ts_prove, whose proofs differ from ts_prove_pre_aux's in the header words alone
        (include/tapstark.h), so their words are compared behind the header."""
        c1, c2 = chal.clone(), chal.clone()
        source = self.source()
        via_prove = ts.prove(self.config, self.cair, c1, np.array(trace), pis, preprocessed=self.key, aux=source).words
        failure = []
        from tapstark_amd.stark import _aux_callback
        cb = _aux_callback(self.ctx, self.cair, source, failure) if source is not None else _lib.AUX_FN()
        out, n_words = np.zeros(len(via_prove) + 64, dtype=np.uint32), C.c_size_t()
        m = ts.DeviceMatrix.upload(self.ctx, np.array(trace))
        p = np.ascontiguousarray(pis, dtype=np.uint32)
        cfg = self.config.pcs.fri._c()
        rc = self.ctx._l.ts_prove_pre_aux(self.ctx.h, C.byref(cfg), self.cair.h, c2.h,
                                          self.key.data.h if self.key is not None else None, m.h,
                                          p.ctypes.data_as(_lib.u32p) if len(p) else None, len(p), cb, None,
                                          out.ctypes.data_as(_lib.u32p), len(out), C.byref(n_words))
        assert rc == 0 and not failure, (rc, failure)
        v5 = out[:n_words.value].copy()
        head = {1: 5, 3: 6, 4: 8, 5: 9}[int(via_prove[1])]
        assert int(v5[1]) == 5 and len(v5) - 9 == len(via_prove) - head and (v5[9:] == via_prove[head:]).all(), \
            f"{self.kind}: ts_prove_pre_aux and ts.prove differ behind the header"
        assert (c1.state() == c2.state()).all()
        return v5, self.verify(v5, pis, chal), c2.state()

    def verify(self, words, pis, chal=None):
        """Accepted by the verifier against the key's root; returns the exposed words."""
        root = self.key.root if self.key is not None else None
        c = chal.clone() if chal is not None else ts.BfChallenger()
        if root is not None and self.logup is not None:
            return ts.verify(self.config, self.cair, c, words, pis, preprocessed_root=root)
        return ts.verify_pre_aux(self.config, self.cair, c, words, pis, preprocessed_root=root)


@pytest.fixture(scope="module")
def ctxs():
    from tapstark_amd.build import build

    build()
    return [ts.default_context()] + [ts.Context(0) for _ in range(3)]


def _chal(i):
    c = ts.BfChallenger()
    c.observe(100 + i)
    return c


def _same(proof, want):
    return proof is not None and len(proof.words) == len(want) and bool((proof.words == want).all())


def _batch(lanes, traces, lane_of, pis, chals, **kw):
    return ts.prove_batch_lookup([ln.pair for ln in lanes], traces, lane_of, public_values=pis, challengers=chals,
                                 keys=[ln.key for ln in lanes], logups=[ln.logup for ln in lanes], **kw)


def _check_items(orc, lanes, lane_of, stmts, chals, res):
    for i, (trace, pis) in enumerate(stmts):
        ln = lanes[lane_of[i]]
        want, exposed, state = ln.solo(trace, pis, chals[i])
        assert res.status[i] == 0, (i, res.errors[i])
        assert _same(res.proofs[i], want), f"item {i} ({ln.kind}): proof differs from the solo call"
        assert int(res.proofs[i].words[1]) == 5
        assert len(res.exposed[i]) == ln.cair.n_exposed and (res.exposed[i] == exposed).all(), f"item {i}: exposed"
        assert (res.final_states[i] == state).all(), f"item {i}: final challenger state"
        assert hexd(res.digests[i]) == orc.blake3(want.tobytes()).hex(), f"item {i}: digest"
        got = ln.verify(res.proofs[i].words, pis, chals[i])
        if ln.logup is not None:
            assert (got == exposed).all()
            ln.logup.verify(got)
        assert res.n_missing[i] == 0 and res.first_missing[i] == NO_MISS


# ------------------------------------------------------------------ 1. equality with the solo call, mixed lanes
@pytest.mark.parametrize("log_n,b", SHAPES)
@pytest.mark.parametrize("with_fib", [False, True])
def test_mixed_lanes_equal_the_solo_call(ctxs, orc, log_n, b, with_fib):
    kinds = ["table", "range", "selector"] + (["fib"] if with_fib else [])
    lanes = [Lane(ctxs[k], kind, log_n, b) for k, kind in enumerate(kinds)]
    lane_of = [i % len(lanes) for i in range(8)]
    stmts = [lanes[lane_of[i]].statement(i) for i in range(8)]
    chals = [_chal(i) for i in range(8)]
    before = [c.state() for c in chals]
    # device traces and host arrays, alternating per lane visit
    traces = [ts.DeviceMatrix.upload(lanes[lane_of[i]].ctx, t) if (i // len(lanes)) % 2 == 0 else t.copy()
              for i, (t, _) in enumerate(stmts)]
    res = _batch(lanes, traces, lane_of, [p for _, p in stmts], chals, digests=True, gate_ms=0.2)
    assert res.rc == 0
    assert all((c.state() == s).all() for c, s in zip(chals, before)), "a caller's challenger changed"
    starts = np.sort(res.start_ms)
    assert (np.diff(starts) >= 0.2 - 1e-9).all(), "two proofs started within the gate"
    _check_items(orc, lanes, lane_of, stmts, chals, res)
    for i, t in enumerate(traces):  # device traces are consumed
        if isinstance(t, ts.DeviceMatrix):
            with pytest.raises(_lib.TsError):
                t.download()


# ------------------------------------------------------------------ 2. in-lane fills
def _fill_case(ctxs_, log_n, b):
    """Two lanes (TableLookupAir with a key, RangeLookupAir without), each with a host-array item and a
    device-trace item whose multiplicity column is zeroed and filled in the lane.  Returns per item the proof
    words, exposed words and final state, and the solo references of the traces filled first."""
    lanes = [Lane(ctxs_[0], "table", log_n, b), Lane(ctxs_[1], "range", log_n, b)]
    cols = [1, 2]  # the multiplicity column of each AIR
    lane_of = [0, 1, 0, 1]
    full = [lanes[lane_of[i]].statement(40 + i)[0] for i in range(4)]
    zeroed = []
    for i, t in enumerate(full):
        z = t.copy()
        z[:, cols[lane_of[i]]] = 0
        zeroed.append(z)
    chals = [_chal(50 + i) for i in range(4)]
    traces = [zeroed[0], zeroed[1], ts.DeviceMatrix.upload(lanes[0].ctx, zeroed[2]),
              ts.DeviceMatrix.upload(lanes[1].ctx, zeroed[3])]
    res = _batch(lanes, traces, lane_of, None, chals, fills=[[ln.logup.mult_spec(1)] for ln in lanes])
    want = []
    for i in range(4):
        ln = lanes[lane_of[i]]
        m = ts.DeviceMatrix.upload(ln.ctx, zeroed[i])
        assert ln.logup.fill_multiplicities(m, 1, preprocessed=ln.key.values if ln.key else None) == (0, NO_MISS)
        filled = m.download()
        assert (filled == full[i]).all(), "LogUp.fill_multiplicities does not rebuild the generator's column"
        want.append(ln.solo(filled, [], chals[i]))
    return lanes, res, want


@pytest.mark.parametrize("log_n,b", SHAPES)
def test_in_lane_fills_equal_the_solo_proof_of_the_filled_trace(ctxs, log_n, b):
    lanes, res, want = _fill_case(ctxs, log_n, b)
    assert res.rc == 0
    for i, (words, exposed, state) in enumerate(want):
        assert _same(res.proofs[i], words), f"item {i}: differs from the solo proof of the filled trace"
        assert (res.exposed[i] == exposed).all() and not res.exposed[i].any(), f"item {i}: the sum is not zero"
        assert (res.final_states[i] == state).all()
        assert res.n_missing[i] == 0 and res.first_missing[i] == NO_MISS


# ------------------------------------------------------------------ 3. one key, many items
@pytest.mark.parametrize("log_n,b", [(3, 2), (10, 1)])
def test_one_key_serves_many_items(ctxs, orc, log_n, b):
    ln = Lane(ctxs[0], "table", log_n, b)
    first_stmt, first_chal = ln.statement(70), _chal(70)
    earlier = ln.solo(*first_stmt, first_chal)[0]
    root = ln.key.root.copy()
    lde = ln.key.data.lde(0).copy()
    values = ln.key.values.download().copy()
    stmts = [ln.statement(71 + i) for i in range(6)]
    chals = [_chal(71 + i) for i in range(6)]
    res = _batch([ln], [t.copy() for t, _ in stmts], [0] * 6, None, chals, digests=True)
    _check_items(orc, [ln], [0] * 6, stmts, chals, res)
    assert len({res.proofs[i].words.tobytes() for i in range(6)}) == 6
    assert (ln.key.root == root).all() and (ln.key.data.lde(0) == lde).all()
    assert (ln.key.values.download() == values).all()
    again = ln.solo(*first_stmt, first_chal)[0]
    assert len(again) == len(earlier) and (again == earlier).all()


# ------------------------------------------------------------------ 4. data errors stay in their item
def test_data_errors_stay_in_their_item(ctxs):
    """[a value outside the table under a fill, a good item, a zero denominator, a good item] on one lane.  The
    challenges of a proof come out of the transcript, so a zero denominator cannot be arranged through a spec: the
    middle item's source is a callback that runs the builder with gamma = -(a table value), as
    test_logup_zero_denominator_through_a_table_value builds one, and hands back the builder's status."""
    n = 1 << 10
    ln = Lane(ctxs[0], "table", 10, 2)
    outside_row = 9
    bad = generate_table_lookup_trace(n, seed=81, outside_row=outside_row)
    stmts = [bad, ln.statement(82)[0], ln.statement(83)[0], ln.statement(84)[0]]
    zeroed = [t.copy() for t in stmts]
    for z in zeroed:
        z[:, 1] = 0
    chals = [_chal(80 + i) for i in range(4)]
    # what the solo calls say
    m = ts.DeviceMatrix.upload(ln.ctx, zeroed[0])
    miss = ln.logup.fill_multiplicities(m, 1, preprocessed=ln.key.values, allow_missing=True)
    assert miss == (1, outside_row)
    with pytest.raises(_lib.TsError) as e:
        ln.logup.fill_multiplicities(ts.DeviceMatrix.upload(ln.ctx, zeroed[0]), 1, preprocessed=ln.key.values)
    miss_text = str(e.value).split(": ", 1)[1]
    assert e.value.code == TS_ERR_INVARIANT and "is in no table row" in miss_text
    target = 37
    forced = np.zeros(8, dtype=np.uint32)
    forced[0] = P - target
    forced[4:] = (5, 6, 7, 8)
    with pytest.raises(_lib.TsError) as e:
        ln.logup.build(ts.DeviceMatrix.upload(ln.ctx, stmts[2]), forced, preprocessed=ln.key.values)
    zero_text = str(e.value).split(": ", 1)[1]
    rows = np.flatnonzero(stmts[2][:target + 1, 0] == target)
    where = f"row {rows[0]}, interaction 0" if len(rows) else f"row {target}, interaction 1"
    assert e.value.code == TS_ERR_INVARIANT and "zero denominator" in zero_text and where in zero_text

    l = _lib.lib()
    spec_keep = ln.logup._spec_c()

    def zero_denominator(_user, ctx_h, trace_h, _challenges, _n, aux_out, exposed_out):
        return l.ts_logup_aux_build_pre(ctx_h, C.byref(spec_keep[0]), ln.key.values.h, trace_h,
                                        forced.ctypes.data_as(_lib.u32p), aux_out, exposed_out)

    cb = _lib.AUX_FN(zero_denominator)

    def edit(items, lanes_c):
        items[2].logup = None
        items[2].aux_fn = C.cast(cb, C.c_void_p)

    res = _batch([ln], [zeroed[0], zeroed[1], ts.DeviceMatrix.upload(ln.ctx, zeroed[2]), zeroed[3]], [0] * 4, None,
                 chals, fills=[[ln.logup.mult_spec(1)]], check=False, _edit_items=edit)
    assert list(res.status) == [TS_ERR_INVARIANT, 0, TS_ERR_INVARIANT, 0] and res.rc == TS_ERR_INVARIANT
    assert (int(res.n_missing[0]), int(res.first_missing[0])) == miss
    assert all(res.n_missing[i] == 0 and res.first_missing[i] == NO_MISS for i in (1, 2, 3))
    # the lane's context holds the text of its LAST failure; item 0's is checked in a call of its own below
    assert zero_text in res.errors[2] and "aux callback" in res.errors[2]
    assert res.proofs[0] is None and res.proofs[2] is None
    for i in (1, 3):
        want, exposed, state = ln.solo(stmts[i], [], chals[i])
        assert _same(res.proofs[i], want), f"item {i}: the item after a data error differs from its solo proof"
        assert (res.exposed[i] == exposed).all() and (res.final_states[i] == state).all()
    res = _batch([ln], [zeroed[0], zeroed[1]], [0, 0], None, chals[:2], fills=[[ln.logup.mult_spec(1)]], check=False)
    assert list(res.status) == [TS_ERR_INVARIANT, 0] and miss_text in res.errors[0]
    assert (int(res.n_missing[0]), int(res.first_missing[0])) == miss
    assert _same(res.proofs[1], ln.solo(stmts[1], [], chals[1])[0])


# ------------------------------------------------------------------ 5. item refusals
def test_item_refusals(ctxs):
    log_n, b = 3, 2
    n = 1 << log_n
    table, rng, wide = Lane(ctxs[0], "table", log_n, b), Lane(ctxs[1], "range", log_n, b), Lane(ctxs[2], "wide", log_n, b)
    bare = Lane(ctxs[3], "table", log_n, b)  # a TableLookupAir lane whose key kept no values
    bare.key = ts.PreprocessedKey(bare.config, generate_lookup_table(n))
    lanes = [table, rng, wide, bare]
    tall = ts.PreprocessedKey(table.config, generate_lookup_table(2 * n), keep_values=True)
    three = LogUp([(("const", 1), [("col", 0)]), (("col", 2), [("col", 1)]), (("const", 1), [("col", 1)])])
    assert three.aux_width == 12 != rng.cair.aux_width
    three_keep = three._spec_c()
    noop = _lib.AUX_FN(lambda user, c, t, ch, k, aux_out, exposed_out: 0)
    # a column-major matrix of WideRangeAir's width: a quotient chunk of a Fibonacci trace
    fib = Lane(ctxs[2], "fib", log_n, b)
    ft, fp = fib.statement(1)
    _, data = fib.config.pcs.commit([(fib.config.pcs.natural_domain_for_degree(n), ft)])
    chunk = fib.config.pcs.quotient_chunks(data, fib.cair, fp, [1, 2, 3, 4])[0]
    assert chunk.dims() == (n, 4)

    stmt = lambda ln, s: ln.statement(s)[0]
    dev = lambda ln, s: ts.DeviceMatrix.upload(ln.ctx, stmt(ln, s))
    traces = [
        dev(bare, 0),    # 0: a kind-2 spec on a lane without key_values
        dev(rng, 1),     # 1: both aux sources
        dev(rng, 2),     # 2: none for an aux AIR
        dev(rng, 3),     # 3: a spec whose aux width is not the AIR's
        dev(table, 4),   # 4: a key of another height (this lane's key is swapped for `tall` below)
        chunk,           # 5: a column-major device trace for an aux AIR
        stmt(rng, 6),    # 6: a proof buffer one word short
        stmt(rng, 7),    # 7: good
        stmt(wide, 8),   # 8: good
    ]
    lane_of = [3, 1, 1, 1, 0, 2, 1, 1, 2]
    chals = [_chal(90 + i) for i in range(9)]
    need = len(rng.solo(stmt(rng, 6), [], chals[6])[0])

    def edit(items, lanes_c):
        items[1].aux_fn = C.cast(noop, C.c_void_p)
        items[2].logup = None
        items[3].logup = C.pointer(three_keep[0])
        lanes_c[0].key = tall.data.h
        lanes_c[0].key_values = tall.values.h
        items[6].cap_words = need - 1

    res = _batch(lanes, traces, lane_of, None, chals, check=False, _edit_items=edit)
    assert list(res.status) == [TS_ERR_INVALID] * 6 + [TS_ERR_BUFFER, 0, 0], (list(res.status), res.errors)
    assert res.rc == TS_ERR_INVALID and res.n_words[6] == need
    for i in range(6):  # nothing was consumed
        assert traces[i].dims() == ((n, 4) if i == 5 else stmt(lanes[lane_of[i]], i).shape), i
    assert (traces[0].download() == stmt(bare, 0)).all()
    for i, ln, s in ((7, rng, 7), (8, wide, 8)):
        assert _same(res.proofs[i], ln.solo(stmt(ln, s), [], chals[i])[0]), i
    # each refusal alone, for its text (a lane's context keeps the last one only)
    needles = ["key_values", "exactly one of logup / aux_fn", "exactly one of logup / aux_fn", "aux width", "height",
               "row-major"]
    for i in range(6):
        only = lambda items, lanes_c, i=i: (edit(items, lanes_c), [setattr(items[k], "lane", 99)
                                                                   for k in range(9) if k != i])
        r = _batch(lanes, traces, lane_of, None, chals, check=False, _edit_items=only)
        assert r.status[i] == TS_ERR_INVALID and needles[i] in r.errors[i], (i, r.errors[i])


# ------------------------------------------------------------------ 6. ts_prove_batch is unchanged
def test_prove_batch_is_unchanged(ctxs):
    table, fib = Lane(ctxs[0], "table", 10, 2), Lane(ctxs[1], "fib", 10, 2)
    res = ts.prove_batch([table.pair], [table.statement(1)[0]], [0], [], check=False)
    assert list(res.status) == [TS_ERR_UNSUPPORTED] and "ts_prove_aux" in res.errors[0]
    rng = Lane(ctxs[2], "range", 10, 2)
    res = ts.prove_batch([rng.pair], [rng.statement(1)[0]], [0], [], check=False)
    assert list(res.status) == [TS_ERR_UNSUPPORTED]
    stmts = [fib.statement(i) for i in range(3)]
    chals = [_chal(i) for i in range(3)]
    res = ts.prove_batch([fib.pair], [t.copy() for t, _ in stmts], [0] * 3, [p for _, p in stmts], chals)
    for i, (t, p) in enumerate(stmts):
        c = chals[i].clone()
        direct = ts.prove(fib.config, fib.cair, c, t.copy(), p)
        assert int(direct.words[1]) == 1 and _same(res.proofs[i], direct.words)
        assert (res.final_states[i] == c.state()).all()


# ------------------------------------------------------------------ 7. nothing reads unwritten HBM
def _poison_run(lane_ctxs, log_n, b):
    """Case 1's TableLookupAir lane and case 2, as one list of arrays."""
    ln = Lane(lane_ctxs[0], "table", log_n, b)
    stmts = [ln.statement(i) for i in range(3)]
    chals = [_chal(i) for i in range(3)]
    traces = [stmts[0][0].copy(), ts.DeviceMatrix.upload(ln.ctx, stmts[1][0]), stmts[2][0].copy()]
    res = _batch([ln], traces, [0] * 3, None, chals, digests=True)
    out = [r.words for r in res.proofs] + list(res.exposed) + [res.final_states, res.digests]
    _, fres, _ = _fill_case(lane_ctxs, log_n, b)
    return out + [r.words for r in fres.proofs] + list(fres.exposed) + [fres.final_states]


@pytest.mark.parametrize("log_n,b", [(3, 1), (10, 2)])
def test_nothing_reads_unwritten_hbm(log_n, b):
    from tapstark_amd.build import build

    build()
    results = []
    for word, lane_ctxs in zip(("clean", "0x00000001", "0xFFFFFFFF"), make_contexts(2)):
        before = sum(c.stat(9) for c in lane_ctxs)
        results.append(_poison_run(lane_ctxs, log_n, b))
        filled = sum(c.stat(9) for c in lane_ctxs) - before
        assert (filled == 0) if word == "clean" else (filled > 0), (word, filled)
    for word, got in zip(("0x00000001", "0xFFFFFFFF"), results[1:]):
        assert len(got) == len(results[0])
        for k, (g, w) in enumerate(zip(got, results[0])):
            assert g.shape == w.shape and (g == w).all(), f"{word}: array {k} differs from the clean context's"


# ------------------------------------------------------------------ 8. the C++ example
def test_cpp_example(ctxs, tmp_path):
    libdir = os.path.join(ROOT, "tap-stark_amd", "lib")
    exe = str(tmp_path / "prove_batch_lookup")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "prove_batch_lookup.cpp"), "-L", libdir, "-ltapstark_hip",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    r = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every proof verified" in r.stdout and "every lookup sum is zero" in r.stdout
