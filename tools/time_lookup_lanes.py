"""What batch lanes give a lookup AIR, in one process on one box:

    python tools/time_lookup_lanes.py [LOG_N [REPS [OUT.json]]]      (default 20 20 profiles/lookup_lanes.json)

TableLookupAir-shaped work (tools/time_table_lookup.py's MultiTableLookupAir: the table in a preprocessed key, L
lookups against it) at 2^LOG_N rows, K = 2 and K = 8 interactions, FRI (log_blowup 2, 28 queries, 8 proof-of-work
bits), device-resident traces copied device to device before every proof, keys committed outside the timed region.
Per K, alternated inside every repetition so that all legs see the same box:

    solo            ts_prove_pre_aux through the Python aux callback, one context, one proof at a time: the yardstick
                    (the parent of ts_prove_batch_lookup cannot run a lookup AIR in lanes at all)
    lanes           ts_prove_batch_lookup, 4 lanes, a window of PROOFS proofs, the LogUp spec run by the library, the
                    start gate at a quarter of the solo time (the headline's gate)
    lanes+fill      the same with the multiplicity columns handed over zeroed and filled in the lane
    mul solo, mul lanes   ts_prove and ts_prove_batch of SynthMulAir over as many columns as main + aux: what the
                    lanes give a plain AIR of that size, to read the lookup AIR's gain against

Median over REPS repetitions of the window's ms per proof (host clock around the call, every lane synchronised before
and after); the per-proof wall times inside the lanes are kept.  No ratio is fixed in advance: the figures are
written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.air import aux_dims  # noqa: E402
from tapstark_amd.airs import SynthMulAir  # noqa: E402
from time_table_lookup import CFG, MultiTableLookupAir, lookup_columns  # noqa: E402

LANES, PROOFS = 4, 20


def main():
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "lookup_lanes.json")
    from tapstark_amd.build import build

    build()
    n = 1 << log_n
    ctxs = [ts.Context(0) for _ in range(LANES)]
    configs = [ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), c)) for c in ctxs]
    table = np.arange(n, dtype=np.uint32).reshape(n, 1)
    lane_of = [i % LANES for i in range(PROOFS)]
    med = lambda v: round(float(np.median(v)), 4)

    def sync():
        for c in ctxs:
            c.synchronize()

    legs = {}
    for lookups in (1, 4):
        air = MultiTableLookupAir(lookups)
        K, w, aw = 2 * lookups, air.width(), air.aux_width
        tape = ts.air_tape(air, 0, 1, *aux_dims(air))
        cairs = [ts.CompiledAir(c, tape) for c in ctxs]
        lanes = list(zip(configs, cairs))
        keys = [ts.PreprocessedKey(conf, table, keep_values=True) for conf in configs]  # outside the timed region
        values, mults = lookup_columns(n, lookups)
        full = np.ascontiguousarray(np.hstack([values, mults]))
        zeroed = np.ascontiguousarray(np.hstack([values, np.zeros_like(mults)]))
        res_full = [ts.DeviceMatrix.upload(c, full) for c in ctxs]
        res_zero = [ts.DeviceMatrix.upload(c, zeroed) for c in ctxs]
        fills = [air.logup.mult_spec(2 * i + 1, [2 * i]) for i in range(lookups)]
        mw = w + aw
        mul_tape = ts.air_tape(SynthMulAir(mw), 0)
        mul_lanes = [(conf, ts.CompiledAir(c, mul_tape)) for conf, c in zip(configs, ctxs)]

        def copies(resident, width=w):
            out = [ts.DeviceMatrix.from_device_ptr(ctxs[lane_of[i]], resident[lane_of[i]].device_ptr(), n, width)
                   for i in range(PROOFS)]
            sync()
            return out

        source = air.logup.aux_source_with(keys[0].values)

        def solo():
            traces = [ts.DeviceMatrix.from_device_ptr(ctxs[0], res_full[0].device_ptr(), n, w) for _ in range(PROOFS)]
            sync()
            per = []
            for t in traces:
                t0 = time.perf_counter()
                ts.prove(configs[0], cairs[0], ts.BfChallenger(), t, [], preprocessed=keys[0], aux=source)
                per.append(1e3 * (time.perf_counter() - t0))
            return per

        def mul_solo():
            traces = [ts.DeviceMatrix.synth_mul(ctxs[0], n, mw) for _ in range(PROOFS)]
            sync()
            per = []
            for t in traces:
                t0 = time.perf_counter()
                ts.prove(configs[0], mul_lanes[0][1], ts.BfChallenger(), t, [])
                per.append(1e3 * (time.perf_counter() - t0))
            return per

        def window(call):
            """(ms per proof by the host clock, the library's per-proof wall times, its span per proof)"""
            t0 = time.perf_counter()
            r = call()
            sync()
            ms = 1e3 * (time.perf_counter() - t0) / PROOFS
            return ms, [round(float(x), 4) for x in r.wall_ms], float(np.max(r.start_ms + r.wall_ms) -
                                                                       np.min(r.start_ms)) / PROOFS

        def lookup_window(resident, gate_ms, with_fills):
            traces = copies(resident)
            return window(lambda: ts.prove_batch_lookup(lanes, traces, lane_of, keys=keys, logups=[air.logup] * LANES,
                                                        fills=[fills] * LANES if with_fills else None, gate_ms=gate_ms))

        def mul_window(gate_ms):
            traces = [ts.DeviceMatrix.synth_mul(ctxs[lane_of[i]], n, mw) for i in range(PROOFS)]
            sync()
            return window(lambda: ts.prove_batch(mul_lanes, traces, lane_of, public_values=[], gate_ms=gate_ms))

        # warm-up (pools, twiddles, specialisations), one verified proof of each lookup leg, and the gates
        solo_ms, mul_solo_ms = med(solo()[1:]), med(mul_solo()[1:])
        gate, mul_gate = 0.25 * solo_ms, 0.25 * mul_solo_ms
        for resident, with_fills in ((res_full, False), (res_zero, True)):
            r = ts.prove_batch_lookup(lanes, copies(resident), lane_of, keys=keys, logups=[air.logup] * LANES,
                                      fills=[fills] * LANES if with_fills else None, gate_ms=gate)
            got = ts.verify(configs[0], cairs[0], ts.BfChallenger(), r.proofs[-1], [], preprocessed_root=keys[0].root)
            air.logup.verify(got)
        mul_window(mul_gate)

        rec = {k: [] for k in ("solo", "lanes", "lanes_fill", "mul_solo", "mul_lanes")}
        walls = {k: [] for k in ("solo", "lanes", "lanes_fill", "mul_lanes")}
        spans = {k: [] for k in ("lanes", "lanes_fill", "mul_lanes")}
        for _ in range(reps):
            per = solo()
            rec["solo"].append(float(np.median(per)))
            walls["solo"].append([round(x, 4) for x in per])
            for name, f in (("lanes", lambda: lookup_window(res_full, gate, False)),
                            ("lanes_fill", lambda: lookup_window(res_zero, gate, True)),
                            ("mul_lanes", lambda: mul_window(mul_gate))):
                ms, wl, span = f()
                rec[name].append(ms)
                walls[name].append(wl)
                spans[name].append(span)
            rec["mul_solo"].append(float(np.median(mul_solo())))
        m = {k: med(v) for k, v in rec.items()}
        legs[f"K{K}"] = {
            "interactions": K, "main_width": w, "preprocessed_width": 1, "aux_width": aw, "synth_mul_width": mw,
            "gate_ms": round(gate, 4), "mul_gate_ms": round(mul_gate, 4),
            "solo_ms": m["solo"], "lanes_ms_per_proof": m["lanes"], "lanes_fill_ms_per_proof": m["lanes_fill"],
            "mul_solo_ms": m["mul_solo"], "mul_lanes_ms_per_proof": m["mul_lanes"],
            "lanes_over_solo": round(m["lanes"] / m["solo"], 4),
            "lanes_fill_over_solo": round(m["lanes_fill"] / m["solo"], 4),
            "mul_lanes_over_mul_solo": round(m["mul_lanes"] / m["mul_solo"], 4),
            "library_span_ms_per_proof": {k: med(v) for k, v in spans.items()},
            "median_wall_inside_a_lane_ms": {k: med([x for wl in v for x in wl]) for k, v in walls.items()},
            "per_rep_ms_per_proof": {k: [round(x, 4) for x in v] for k, v in rec.items()},
            "per_proof_wall_ms": walls,
        }
        del res_full, res_zero, keys, cairs, lanes, mul_lanes
    out = {"workload": f"TableLookupAir-shaped, 2^{log_n} rows, FRI {CFG}, {LANES} lanes, windows of {PROOFS} proofs, "
                       f"legs alternated, median of {reps} repetitions",
           "legs": legs,
           "notes": "keys committed outside the timed region; traces device-resident, copied device to device outside "
                    "the timed region; solo = ts_prove_pre_aux through the Python aux callback on one context; the gate "
                    "is a quarter of the leg's own solo time; per_proof_wall_ms of a lanes leg is the library's own "
                    "clock around each proof inside its lane"}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    slim = {k: {kk: vv for kk, vv in v.items() if kk not in ("per_proof_wall_ms", "per_rep_ms_per_proof")}
            for k, v in legs.items()}
    print(json.dumps(slim))


if __name__ == "__main__":
    main()
