"""What a multi-table proof with a LogUp bus costs against its yardsticks, in one process on one context:

    python tools/time_multi_bus.py [REPS [OUT.json]]      (default 20 profiles/multi_bus.json)

BusSendAir / BusRangeAir tables (tap-stark_amd/airs.py), FRI (log_blowup 2, 28 queries, 8 proof-of-work bits), traces
uploaded outside the timed region.  Two shapes: senders of 2^20 (k = 5) and 2^18 (k = 2) rows with range tables of
2^16 and 2^14 rows; three senders (k = 2) and a range table, all of 2^18 rows.  Legs, alternated inside every
repetition (in an order that rotates from one repetition to the next) so that all of them see the same box:

    bus             ts_prove_multi_bus
    bus_per_table   the same with TS_MULTI_LOGUP_PER_TABLE=1: one ts_logup_aux_build per table
    bus_generic     the same with TS_MULTI_OPEN_GENERIC=1: the opening through TwoAdicFriPcs::open
    separate        one ts_prove_aux per table (no statement across the tables): the sum of times and of proof words
    build_multi     ts_logup_aux_build_multi alone on the resident traces, fixed challenges
    build_loop      one ts_logup_aux_build per table on the same traces
    fill_bus        ts_logup_multiplicities_bus: the range tables' columns from the resident senders
    fill_host       the same through the host: download the senders, numpy.bincount, upload the range tables

Median over REPS repetitions of the host clock around the call (the context synchronised before and after); the
whole measurement is repeated three times and every median is given with the spread (max - min) of the three, so
that "faster" can mean "by more than the spread".  No ratio is fixed in advance: the figures are written as they
come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.air import aux_dims, logup_build_multi, logup_multiplicities_bus  # noqa: E402
from tapstark_amd.airs import (BusRangeAir, BusSendAir, generate_bus_range_trace,  # noqa: E402
                               generate_bus_send_trace)

CFG = (2, 28, 8)
P = 0x78000001
# per shape: senders (k, log rows, log of the range table they draw from), range tables (log rows)
SHAPES = {"mixed_20_18_16_14": ([(5, 20, 16), (2, 18, 14)], [16, 14]),
          "equal_4x18": ([(2, 18, 18), (2, 18, 18), (2, 18, 18)], [18])}
LOGUP_KNOB, OPEN_KNOB = "TS_MULTI_LOGUP_PER_TABLE", "TS_MULTI_OPEN_GENERIC"
REPEATS = 3


def statement(shape):
    """(airs, host traces, senders per range table) of a shape; every case balances."""
    senders, ranges = SHAPES[shape]
    airs, traces, by_range = [], [], {r: [] for r in ranges}
    for i, (k, log_n, log_t) in enumerate(senders):
        airs.append(BusSendAir(k))
        traces.append(generate_bus_send_trace(1 << log_n, k, 1 << log_t, 100 + i))
        by_range[log_t].append(len(traces) - 1)
    for r in ranges:
        airs.append(BusRangeAir())
        traces.append(generate_bus_range_trace(1 << r, [traces[i] for i in by_range[r]]))
    return airs, traces, [by_range[r] for r in ranges]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "multi_bus.json")
    from tapstark_amd.build import build

    build()
    ctx = ts.Context(0)
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), ctx))
    med = lambda v: float(np.median(v))  # noqa: E731

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = fn()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), r

    out = {}
    for name in SHAPES:
        airs, host, by_range = statement(name)
        T, n_send = len(airs), len(SHAPES[name][0])
        cairs = [ts.CompiledAir(ctx, ts.air_tape(a, 0, 0, *aux_dims(a))) for a in airs]
        logups = [a.logup for a in airs]
        challenges = (np.arange(1, 9, dtype=np.uint64) * 0x1234567 % P).astype(np.uint32)

        def upload():
            m = [ts.DeviceMatrix.upload(ctx, t) for t in host]
            ctx.synchronize()
            return m

        def bus(knob=None):
            for k in (LOGUP_KNOB, OPEN_KNOB):
                os.environ.pop(k, None)
            if knob:
                os.environ[knob] = "1"
            try:
                tr = upload()
                return timed(lambda: ts.prove_multi_bus(config, cairs, ts.BfChallenger(), tr, [[]] * T, logups))
            finally:
                os.environ.pop(knob or LOGUP_KNOB, None)

        def separate():
            tr = upload()
            return timed(lambda: [ts.prove(config, cairs[t], ts.BfChallenger(), tr[t], [], aux=logups[t].aux_source)
                                  for t in range(T)])

        resident = upload()

        def fill_bus():
            def run():
                for ri, senders in enumerate(by_range):
                    lookers = [(resident[i], [[("col", 2 * j)] for j in range(airs[i].k)],
                                [("col", 2 * j + 1) for j in range(airs[i].k)]) for i in senders]
                    logup_multiplicities_bus(resident[n_send + ri], [("col", 0)], lookers, out_column=1, negate=1)
            return timed(run)

        def fill_host():
            def run():
                for ri, senders in enumerate(by_range):
                    n = host[n_send + ri].shape[0]
                    got = [resident[i].download() for i in senders]
                    resident[n_send + ri] = ts.DeviceMatrix.upload(ctx, generate_bus_range_trace(n, got))
            return timed(run)

        legs = {
            "bus": lambda: bus(), "bus_per_table": lambda: bus(LOGUP_KNOB), "bus_generic": lambda: bus(OPEN_KNOB),
            "separate": separate,
            "build_multi": lambda: timed(lambda: logup_build_multi(logups, resident, challenges)),
            "build_loop": lambda: timed(lambda: [lg.build(m, challenges) for lg, m in zip(logups, resident)]),
            "fill_bus": fill_bus, "fill_host": fill_host,
        }
        # warm-up (pools, twiddles, the specialisations) and the equalities the legs rest on
        _, a = bus()
        _, b = bus(LOGUP_KNOB)
        _, c = bus(OPEN_KNOB)
        assert all(len(a.words) == len(x.words) and (a.words == x.words).all() for x in (b, c)), "the legs disagree"
        ts.verify_multi_bus(config, [ts.CompiledAir(None, ts.air_tape(x, 0, 0, *aux_dims(x))) for x in airs],
                            ts.BfChallenger(), a, [[]] * T)
        _, singles = separate()
        fill_bus()
        assert all((resident[n_send + ri].download() == host[n_send + ri]).all() for ri in range(len(by_range)))
        fill_host()
        assert all((resident[n_send + ri].download() == host[n_send + ri]).all() for ri in range(len(by_range)))
        for leg in ("build_multi", "build_loop"):
            legs[leg]()
        medians = {k: [] for k in legs}
        for _ in range(REPEATS):
            rec = {k: [] for k in legs}
            order = list(legs)
            for i in range(reps):  # the order rotates: no leg always follows the same neighbour (an idle gap, a host leg)
                for k in order[i % len(order):] + order[:i % len(order)]:
                    rec[k].append(legs[k]()[0])
            for k, v in rec.items():
                medians[k].append(med(v))
        ms = {k: {"median_ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4),
                  "medians_ms": [round(x, 4) for x in v]} for k, v in medians.items()}
        words_sep = int(sum(len(p.words) for p in singles))
        out[name] = {
            "tables": [{"air": type(x).__name__, "k": getattr(x, "k", None), "rows_log2": int(t.shape[0]).bit_length() - 1,
                        "width": int(t.shape[1]), "aux_width": x.aux_width} for x, t in zip(airs, host)],
            "ms": ms,
            "proof_words": {"bus": int(len(a.words)), "separate": words_sep,
                            "bus_over_separate": round(len(a.words) / words_sep, 4)},
        }
    doc = {"workload": f"BusSendAir / BusRangeAir tables, FRI {CFG}, one context, legs alternated; per leg the median of "
                       f"{reps} repetitions, measured {REPEATS} times: median_ms is the median of the {REPEATS} medians, "
                       "spread_ms their max - min",
           "shapes": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {"ms": {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()},
                          "proof_words": v["proof_words"]} for k, v in out.items()}))


if __name__ == "__main__":
    main()
