"""What the exact bus check costs against its neighbours, in one process on one context:

    python tools/time_bus_check.py [REPS [OUT.json]]      (default 20 profiles/bus_check.json)

The two bus statements of tools/time_multi_bus.py (BusSendAir / BusRangeAir, tap-stark_amd/airs.py), traces resident:
senders of 2^20 (k = 5) and 2^18 (k = 2) rows with range tables of 2^16 and 2^14 rows; three senders (k = 2) and a
range table, all of 2^18 rows.  Legs, alternated inside every repetition in an order that rotates from one repetition
to the next:

    bus_check    ts_bus_check over all tables
    build_multi  ts_logup_aux_build_multi on the same traces, fixed challenges (what a proof spends on the same rows)
    fill_bus     ts_logup_multiplicities_bus: the range tables' columns from the resident senders
    host         the host route to the same verdict: download every trace, pack (tag, value) into 64-bit words,
                 numpy.unique and numpy.bincount of the multiplicities per tuple, sums mod p

and the input that is hardest on the atomics, timed alone: `all_equal_2^20`, 2^20 rows that all send ONE tuple against
one row that takes it off 2^20 times (every probe and every add of the insert launch goes to one slot).  The library
holds one form of the insert kernel, with the wave-level combine; the same leg on the two earlier forms (one add per
contribution; the add combined alone) is kept in profiles/bus_check_combine_experiment.json.

Median over REPS repetitions of the host clock around the call (the context synchronised before and after); the whole
measurement is repeated three times and every median is given with the spread (max - min) of the three.  No ratio is
fixed in advance: the figures are written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.air import logup_build_multi, logup_multiplicities_bus  # noqa: E402
from tapstark_amd.airs import (BUS_TAG, BusRangeAir, BusSendAir, generate_bus_range_trace,  # noqa: E402
                               generate_bus_send_trace)

P = 0x78000001
SHAPES = {"mixed_20_18_16_14": ([(5, 20, 16), (2, 18, 14)], [16, 14]),
          "equal_4x18": ([(2, 18, 18), (2, 18, 18), (2, 18, 18)], [18])}
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


def host_unbalanced(logups, traces) -> int:
    """The number of unbalanced tuples from downloaded traces, for LogUps whose tuples are (constant, column)."""
    keys, weights = [], []
    for lg, t in zip(logups, traces):
        for (mk, mv), vals in lg.interactions:
            (k0, tag), (k1, col) = vals
            assert (mk, k0, k1) == (1, 0, 1)
            w = t[:, mv].astype(np.int64) % P
            live = w != 0
            keys.append((np.uint64(tag) << np.uint64(32)) | t[live, col].astype(np.uint64))
            weights.append(w[live])
    keys, weights = np.concatenate(keys), np.concatenate(weights)
    _, inverse = np.unique(keys, return_inverse=True)
    sums = np.bincount(inverse, weights=weights.astype(np.float64))  # below 2^53: exact
    return int(np.count_nonzero(sums.astype(np.int64) % P))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "bus_check.json")
    from tapstark_amd.build import build

    build()
    ctx = ts.Context(0)
    med = lambda v: float(np.median(v))  # noqa: E731

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = fn()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), r

    def measure(legs):
        medians = {k: [] for k in legs}
        for _ in range(REPEATS):
            rec = {k: [] for k in legs}
            order = list(legs)
            for i in range(reps):  # the order rotates: no leg always follows the same neighbour
                for k in order[i % len(order):] + order[:i % len(order)]:
                    rec[k].append(legs[k]()[0])
            for k, v in rec.items():
                medians[k].append(med(v))
        return {k: {"median_ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4),
                    "medians_ms": [round(x, 4) for x in v]} for k, v in medians.items()}

    challenges = (np.arange(1, 9, dtype=np.uint64) * 0x1234567 % P).astype(np.uint32)
    out = {}
    for name in SHAPES:
        airs, host, by_range = statement(name)
        n_send = len(SHAPES[name][0])
        logups = [a.logup for a in airs]
        resident = [ts.DeviceMatrix.upload(ctx, t) for t in host]

        def fill_bus():
            def run():
                for ri, senders in enumerate(by_range):
                    lookers = [(resident[i], [[("col", 2 * j)] for j in range(airs[i].k)],
                                [("col", 2 * j + 1) for j in range(airs[i].k)]) for i in senders]
                    logup_multiplicities_bus(resident[n_send + ri], [("col", 0)], lookers, out_column=1, negate=1)
            return timed(run)

        legs = {
            "bus_check": lambda: timed(lambda: ts.bus_check(logups, resident)),
            "build_multi": lambda: timed(lambda: logup_build_multi(logups, resident, challenges)),
            "fill_bus": fill_bus,
            "host": lambda: timed(lambda: host_unbalanced(logups, [m.download() for m in resident])),
        }
        # warm-up, and the equalities the legs rest on
        _, rep = legs["bus_check"]()
        assert rep.balanced, rep
        assert legs["host"]()[1] == 0
        legs["build_multi"]()
        fill_bus()
        assert all((resident[n_send + ri].download() == host[n_send + ri]).all() for ri in range(len(by_range)))
        out[name] = {
            "tables": [{"air": type(x).__name__, "k": getattr(x, "k", None), "rows_log2": int(t.shape[0]).bit_length() - 1,
                        "width": int(t.shape[1])} for x, t in zip(airs, host)],
            "n_contributions": rep.n_contributions, "n_tuples": rep.n_tuples,
            "possible_contributions": int(sum(t.shape[0] * len(lg.interactions) for t, lg in zip(host, logups))),
            "ms": measure(legs),
        }
        del resident

    # every contribution on one tuple
    n = 1 << 20
    send = np.empty((n, 2), dtype=np.uint32)
    send[:, 0], send[:, 1] = 33, 1
    recv = np.array([[33, (P - n) % P]], dtype=np.uint32)
    spec = ts.LogUp([(("col", 1), [("const", BUS_TAG), ("col", 0)])])
    mats = [ts.DeviceMatrix.upload(ctx, send), ts.DeviceMatrix.upload(ctx, recv)]
    leg = {"bus_check": lambda: timed(lambda: ts.bus_check([spec, spec], mats))}
    _, rep = leg["bus_check"]()
    assert rep.balanced and rep.n_tuples == 1 and rep.n_contributions == n + 1, rep
    out["all_equal_2^20"] = {"n_contributions": rep.n_contributions, "n_tuples": rep.n_tuples, "ms": measure(leg),
                             "wave_combine": "built in (the only form); earlier forms: "
                                             "profiles/bus_check_combine_experiment.json"}

    doc = {"workload": "ts_bus_check on resident BusSendAir / BusRangeAir traces, one context, legs alternated; per leg "
                       f"the median of {reps} repetitions, measured {REPEATS} times: median_ms is the median of the "
                       f"{REPEATS} medians, spread_ms their max - min",
           "shapes": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()} for k, v in out.items()}))


if __name__ == "__main__":
    main()
