"""ts_prove_batch against ts_prove_stream on one box: ms/proof of the same config-3 workload (2^20 x 64
SynthMul, log_blowup 2, 28 queries, 8 PoW bits) on 4 lanes with the start gate bench.py uses (a quarter
of one proof's solo time), in alternating windows of 20 proofs each:

  stream        ts_prove_stream, device-born traces (what bench.py times)
  batch         ts_prove_batch, device-born traces, no digests
  batch+digest  ts_prove_batch, device-born traces, Blake3 of every proof on the lane threads
  batch+pinned  ts_prove_batch, traces uploaded from page-locked host memory on each lane's stream

Every window is bracketed by a device sync of every lane; trace generation is outside the timed region.
Evidence for INTEGRATION.md, not a gate:  python tools/batch_vs_stream.py [--windows 3] [--proofs 20] [--out f.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tapstark_amd as ts  # noqa: E402
from tapstark_amd.airs import SynthMulAir  # noqa: E402

LOG_N, WIDTH, CFG, LANES = 20, 64, (2, 28, 8), 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--proofs", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tapstark_amd.build import build

    build()
    n, K = 1 << LOG_N, args.proofs
    ctxs = [ts.Context(0) for _ in range(LANES)]
    tape = ts.air_tape(SynthMulAir(WIDTH), 0)
    lanes = [(ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), c)), ts.CompiledAir(c, tape)) for c in ctxs]
    lane_of = [i % LANES for i in range(K)]

    def sync():
        for c in ctxs:
            c.synchronize()

    # solo time of one proof (after a warm-up) -> the gate, as bench.py sets it
    conf, air = lanes[0]
    solo = []
    for _ in range(4):
        m = ts.DeviceMatrix.synth_mul(ctxs[0], n, WIDTH)
        sync()
        t0 = time.perf_counter()
        ts.prove(conf, air, ts.BfChallenger(), m, [])
        solo.append(1e3 * (time.perf_counter() - t0))
    single_ms = float(np.median(solo[1:]))
    gate_ms = 0.25 * single_ms

    pinned = []
    for l in range(LANES):  # read-only during a call: one buffer per lane serves all of its items
        p = ts.PinnedHostMatrix(n, WIDTH)
        p.array[:] = ts.DeviceMatrix.synth_mul(ctxs[l], n, WIDTH).download()
        pinned.append(p)

    def device_traces():
        mats = [ts.DeviceMatrix.synth_mul(ctxs[lane_of[i]], n, WIDTH) for i in range(K)]
        sync()
        return mats

    def run(mode):
        traces = [pinned[lane_of[i]] for i in range(K)] if mode == "batch+pinned" else device_traces()
        t0 = time.perf_counter()
        if mode == "stream":
            _, st, wl = ts.prove_stream(lanes, traces, lane_of, [], gate_ms=gate_ms)
        else:
            r = ts.prove_batch(lanes, traces, lane_of, public_values=[], gate_ms=gate_ms,
                               digests=(mode == "batch+digest"))
            st, wl = r.start_ms, r.wall_ms
        sync()
        # beside the whole call: the span the library's own clock covers (first start to last end), which
        # leaves out the binding's work before and after the call
        span[mode].append(float(np.max(st + wl) - np.min(st)) / K)
        return 1e3 * (time.perf_counter() - t0) / K

    modes = ["stream", "batch", "batch+digest", "batch+pinned"]
    span = {m: [] for m in modes}
    run("stream")  # warm-up of the lanes' pools and graphs
    run("batch+pinned")
    per = {m: [] for m in modes}
    span = {m: [] for m in modes}  # the warm-up calls do not count
    for w in range(args.windows):
        order = modes if w % 2 == 0 else modes[::-1]  # alternate, so no mode always follows the same one
        for m in order:
            per[m].append(run(m))
    med = {m: float(np.median(v)) for m, v in per.items()}
    out = {"workload": f"config3 2^{LOG_N}x{WIDTH} SynthMul, {LANES} lanes, {K} proofs per window",
           "single_ms": round(single_ms, 3), "gate_ms": round(gate_ms, 3),
           "ms_per_proof": {m: [round(x, 3) for x in v] for m, v in per.items()},
           "median_ms_per_proof": {m: round(v, 3) for m, v in med.items()},
           "library_span_ms_per_proof": {m: [round(x, 3) for x in v] for m, v in span.items()},
           "batch_vs_stream": round(med["batch"] / med["stream"], 4),
           "digest_cost": round(med["batch+digest"] / med["batch"] - 1, 4),
           "pinned_vs_device": round(med["batch+pinned"] / med["batch"], 4)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
