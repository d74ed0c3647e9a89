"""What a commit-once key is worth at the headline shape, in one process on one box:

    python tools/time_preprocessed.py [LOG_N [PROOFS_PER_LANE [OUT.json]]]   (default 20 6 profiles/preprocessed_prove.json)

SynthMulAir-64's constraints (tap-stark_amd/airs.py) over a 2^LOG_N-row trace, FRI (log_blowup 2, 28 queries, 8
proof-of-work bits), the lanes and start gate of bench.py's headline: 4 lanes (one context and one host thread
each), no two proofs starting within a quarter of one proof's solo time.  Two legs, each with its own warm-up:

    (a) main64         ts_prove, all 64 columns in the main trace: today's way, the yardstick
    (b) key16_main48   ts_prove_pre, the first 16 of the SAME 64 columns in a preprocessed key committed once per
                       context OUTSIDE the timed region, the other 48 in the trace

The traces are device-resident and copied device to device before every proof (a proof consumes its trace), as
in tools/time_ingest.py's resident leg.  Leg (b) extends and hashes 48 columns instead of 64 and runs the same
quotient and opening work (plus one more barycentric-dot launch, one more Merkle path per query).  Both proofs
are verified once, outside the timed region.  ms per proof and the box's clock and power over each leg go to
OUT.json.  No threshold: the figures are reported as they come."""
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import tapstark_amd as ts
from tapstark_amd.air import BaseAir
from tapstark_amd.airs import SynthMulAir, generate_synth_mul_trace
from tapstark_amd.benchutil import GpuSamplerProcess

W, PW, LANES, CFG = 64, 16, 4, (2, 28, 8)


class SynthMulSplitAir(BaseAir):
    """SynthMulAir(W) with its first PW columns read from the preprocessed matrix: the same constraints, in the
    same order, over hstack(preprocessed, main)."""

    def width(self) -> int:
        return W - PW

    def preprocessed_width(self) -> int:
        return PW

    def eval(self, builder) -> None:
        prep, main = builder.preprocessed(), builder.main()
        reps = W // 3

        def col(off, j):
            return prep.row_slice(off)[j] if j < PW else main.row_slice(off)[j - PW]

        for i in range(reps):
            a, b, c = col(0, 3 * i), col(0, 3 * i + 1), col(0, 3 * i + 2)
            builder.assert_zero(a * a * b - c)
            builder.when_first_row().assert_eq(a * a + 1, b)
            builder.when_transition().assert_eq(a + reps, col(1, 3 * i))


def main():
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    per_lane = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "preprocessed_prove.json")
    n = 1 << log_n
    joined = generate_synth_mul_trace(n, W)
    prep, main_cols = np.ascontiguousarray(joined[:, :PW]), np.ascontiguousarray(joined[:, PW:])
    ctxs = [ts.default_context()] + [ts.Context(0) for _ in range(LANES - 1)]
    confs = [ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), c)) for c in ctxs]
    tape_a, tape_b = ts.air_tape(SynthMulAir(W), 0), ts.air_tape(SynthMulSplitAir(), 0, PW)
    airs_a = [ts.CompiledAir(c, tape_a) for c in ctxs]
    airs_b = [ts.CompiledAir(c, tape_b) for c in ctxs]
    assert all(a.is_jit for a in airs_a + airs_b), "the specialised quotient kernel is what the headline runs"
    k = min(n, 1 << 10)
    assert ts.check_constraints(airs_b[0], main_cols[:k], [], ctxs[0], preprocessed=prep[:k]) == -1
    keys = [ts.PreprocessedKey(conf, prep) for conf in confs]  # once per context, outside the timed region

    gate = {"ms": 0.0, "last": -1e18, "lock": threading.Lock()}

    def start_gate():
        if gate["ms"] <= 0:
            return
        with gate["lock"]:
            while True:
                wait = gate["last"] + gate["ms"] * 1e-3 - time.perf_counter()
                if wait <= 0:
                    break
                time.sleep(min(wait, 2e-4))
            gate["last"] = time.perf_counter()

    pool = ThreadPoolExecutor(max_workers=LANES)

    def run_leg(prove_on):
        """prove_on(lane) -> Proof: one proof on that lane, its trace copied from the resident one first."""
        last = [None] * LANES

        def job(l):
            for _ in range(per_lane):
                start_gate()
                last[l] = prove_on(l)

        def sync():
            for c in ctxs:
                c.synchronize()

        gate["ms"] = 0.0
        list(pool.map(job, range(LANES)))  # warm-up: pool blocks, tables
        sync()
        t0 = time.perf_counter()
        prove_on(0)
        solo = 1e3 * (time.perf_counter() - t0)
        gate["ms"] = 0.25 * solo
        sampler = GpuSamplerProcess(0, 0.01)
        t0 = time.perf_counter()
        list(pool.map(job, range(LANES)))
        sync()
        t1 = time.perf_counter()
        sampler.stop()
        steps = per_lane * LANES
        return last[0], {"ms_per_proof": round(1e3 * (t1 - t0) / steps, 4), "proofs": steps,
                         "solo_ms": round(solo, 4), "start_gate_ms": round(gate["ms"], 4),
                         "box": sampler.window(t0, t1)}

    def resident_copy(l, m, width):
        return ts.DeviceMatrix.from_device_ptr(ctxs[l], m.device_ptr(), n, width)

    full = [ts.DeviceMatrix.upload(c, joined) for c in ctxs]
    proof_a, leg_a = run_leg(lambda l: ts.prove(confs[l], airs_a[l], ts.BfChallenger(), resident_copy(l, full[l], W), []))
    ts.verify(confs[0], airs_a[0], ts.BfChallenger(), proof_a, [])
    del full
    rest = [ts.DeviceMatrix.upload(c, main_cols) for c in ctxs]
    proof_b, leg_b = run_leg(lambda l: ts.prove(confs[l], airs_b[l], ts.BfChallenger(),
                                                resident_copy(l, rest[l], W - PW), [], preprocessed=keys[l]))
    ts.verify(confs[0], airs_b[0], ts.BfChallenger(), proof_b, [], preprocessed_root=keys[0].root)
    leg_a["proof_words"], leg_b["proof_words"] = int(len(proof_a.words)), int(len(proof_b.words))

    out = {"workload": f"SynthMulAir-64's constraints, 2^{log_n} rows, FRI {CFG}, {LANES} lanes, device-resident traces",
           "legs": {"a_main64_ts_prove": leg_a, f"b_key{PW}_main{W - PW}_ts_prove_pre": leg_b},
           "yardstick": "a_main64_ts_prove",
           "b_over_a": round(leg_b["ms_per_proof"] / leg_a["ms_per_proof"], 4),
           "key": f"{PW} columns committed once per context, outside the timed region"}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
