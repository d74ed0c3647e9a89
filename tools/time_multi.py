"""What one multi-table proof costs against its two yardsticks, in one process on one context:

    python tools/time_multi.py [REPS [OUT.json]]      (default 20 profiles/prove_multi.json)

SynthMulAir-16 tables, FRI (log_blowup 2, 28 queries, 8 proof-of-work bits), traces generated in HBM outside the timed
region.  Two shapes: heights (2^20, 2^18, 2^16, 2^14) and four tables of 2^18.  Three legs, alternated inside every
repetition so that all of them see the same box:

    multi           ts_prove_multi, the one-pass-per-height-class opening (csrc/open_multi.hip)
    multi_generic   ts_prove_multi with TS_MULTI_OPEN_GENERIC=1: the same proof through TwoAdicFriPcs::open
    four            four ts_prove calls, one per table: the sum of their times and of their proof words

The yardsticks are the generic leg and the four-proof leg of the same run.  Median over REPS repetitions of the host
clock around the call (the context synchronised before and after).  The stage times ("compute opened values ...",
"reduce rows") of the two multi legs come from ts_ctx_take_timings in extra repetitions of their own, because stage
timing waits for an event per stage.  No ratio is fixed in advance: the figures are written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.airs import SynthMulAir  # noqa: E402

CFG = (2, 28, 8)
WIDTH = 16
SHAPES = {"mixed_20_18_16_14": (20, 18, 16, 14), "equal_4x18": (18, 18, 18, 18)}
KNOB = "TS_MULTI_OPEN_GENERIC"
STAGES = ("compute opened values with Lagrange interpolation", "reduce rows")


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "prove_multi.json")
    from tapstark_amd.build import build

    build()
    ctx = ts.Context(0)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), ctx))
    air = ts.CompiledAir(ctx, ts.air_tape(SynthMulAir(WIDTH), 0))
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731

    def traces(logs):
        out = [ts.DeviceMatrix.synth_mul(ctx, 1 << ln, WIDTH) for ln in logs]
        ctx.synchronize()
        return out

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), r

    def multi(logs, generic):
        if generic:
            os.environ[KNOB] = "1"
        else:
            os.environ.pop(KNOB, None)
        try:
            tr = traces(logs)
            return timed(lambda: ts.prove_multi(config, [air] * len(logs), ts.BfChallenger(), tr, [[]] * len(logs)))
        finally:
            os.environ.pop(KNOB, None)

    def four(logs):
        tr = traces(logs)
        return timed(lambda: [ts.prove(config, air, ts.BfChallenger(), t, []) for t in tr])

    def stages(logs, generic):
        ctx.take_timings()
        ctx.set_timing(True)
        try:
            multi(logs, generic)
            got = ctx.take_timings()
        finally:
            ctx.set_timing(False)
        return {s: round(sum(ms for name, ms in got if name == s), 4) for s in STAGES}

    out = {}
    for name, logs in SHAPES.items():
        # warm-up (pools, twiddles, the specialisation) and the equality of the two multi legs
        _, a = multi(logs, False)
        _, b = multi(logs, True)
        assert len(a.words) == len(b.words) and (a.words == b.words).all(), "the two opening paths disagree"
        ts.verify_multi(config, [air] * len(logs), ts.BfChallenger(), a, [[]] * len(logs))
        _, singles = four(logs)
        rec = {"multi": [], "multi_generic": [], "four": []}
        for _ in range(reps):
            rec["multi"].append(multi(logs, False)[0])
            rec["multi_generic"].append(multi(logs, True)[0])
            rec["four"].append(four(logs)[0])
        st = {"multi": [stages(logs, False) for _ in range(5)], "multi_generic": [stages(logs, True) for _ in range(5)]}
        m = {k: med(v) for k, v in rec.items()}
        words_four = int(sum(len(p.words) for p in singles))
        out[name] = {
            "log_heights": list(logs), "width": WIDTH,
            "ms_per_statement": m,
            "multi_over_generic": round(m["multi"] / m["multi_generic"], 4),
            "multi_over_four": round(m["multi"] / m["four"], 4),
            "proof_words": {"multi": int(len(a.words)), "four": words_four,
                            "multi_over_four": round(len(a.words) / words_four, 4)},
            "stage_ms": {leg: {s: med([r[s] for r in runs]) for s in STAGES} for leg, runs in st.items()},
            "per_rep_ms": {k: [round(x, 4) for x in v] for k, v in rec.items()},
        }
    doc = {"workload": f"SynthMulAir-{WIDTH} tables, FRI {CFG}, one context, legs alternated, median of {reps} "
                       "repetitions; stage times from 5 repetitions with stage timing on",
           "shapes": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "per_rep_ms"} for k, v in out.items()}))


if __name__ == "__main__":
    main()
