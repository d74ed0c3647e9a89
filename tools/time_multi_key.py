"""What a multi-table proof against a commit-once key costs against its yardsticks, in one process on one context:

    python tools/time_multi_key.py [REPS [OUT.json]]      (default 20 profiles/multi_key.json)

FRI (log_blowup 2, 28 queries, 8 proof-of-work bits), traces uploaded and the key committed outside the timed region.
Two statements:

    range   the mixed-height shape of tools/time_multi_bus.py with its two range tables moved into a key: BusSendAir
            senders of 2^20 (k = 5) and 2^18 (k = 2) rows, BusKeyTableAir tables over key matrices 0 .. 2^16 - 1 and
            0 .. 2^14 - 1
    xor     a BusTupleSendAir sender of 2^20 rows against the 8-bit xor table (a, b, a xor b), a key matrix of 2^16 rows

Legs, alternated inside every repetition (in an order drawn afresh for every repetition, so that no leg always
follows the same neighbour -- the host leg leaves the GPU idle for tens of ms and the leg behind it pays for that) so
that all of them see the same box:

    key             ts_prove_multi_key
    key_per_table   the same with TS_MULTI_LOGUP_PER_TABLE=1: one ts_logup_aux_build(_pre) per table
    key_generic     the same with TS_MULTI_OPEN_GENERIC=1: the opening through TwoAdicFriPcs::open
    bus             the same statement through ts_prove_multi_bus, the tables as main columns pinned by BusRangeAir
                    (range only: the xor table has no such form) -- the yardstick
    build_multi_pre ts_logup_aux_build_multi_pre alone on the resident traces and the key's values, fixed challenges
    build_loop      one ts_logup_aux_build / ts_logup_aux_build_pre per table on the same matrices
    fill_pre        ts_logup_multiplicities_bus_pre: the tables' multiplicity columns from the resident senders
    fill_host       the same through the host: download the senders, numpy.bincount, upload the columns

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
from tapstark_amd.airs import (BUS_TAG, BusKeyTableAir, BusRangeAir, BusSendAir, BusTupleSendAir,  # noqa: E402
                               generate_bus_range_trace, generate_bus_send_trace, generate_range_key, generate_xor_key,
                               generate_xor_send_trace)

CFG = (2, 28, 8)
P = 0x78000001
XOR_TAG = 11
LOGUP_KNOB, OPEN_KNOB = "TS_MULTI_LOGUP_PER_TABLE", "TS_MULTI_OPEN_GENERIC"
REPEATS = 3


def _mult(counts):
    return ((P - counts % P) % P).astype(np.uint32).reshape(-1, 1)


def statement(name):
    """(airs, host traces, key matrix or None per table, fills) with fills = [(table index, n_values, sender
    indices)]; the bus twin (airs, traces) of the range statement, or None.  Every statement balances."""
    if name == "range":
        senders = [(5, 20, 16), (2, 18, 14)]
        airs = [BusSendAir(k) for k, _, _ in senders]
        traces = [generate_bus_send_trace(1 << n, k, 1 << t, 100 + i) for i, (k, n, t) in enumerate(senders)]
        bus_airs, bus_traces = list(airs), list(traces)
        keys, fills = [None, None], []
        for i, (_, _, t) in enumerate(senders):
            twin = generate_bus_range_trace(1 << t, [traces[i]])
            airs.append(BusKeyTableAir(BUS_TAG, 1))
            traces.append(np.ascontiguousarray(twin[:, 1:2]))
            keys.append(generate_range_key(1 << t))
            fills.append((len(airs) - 1, 1, [i]))
            bus_airs.append(BusRangeAir())
            bus_traces.append(twin)
        return airs, traces, keys, fills, (bus_airs, bus_traces)
    x = generate_xor_send_trace(1 << 20, 1, 8, 200)
    sent = x[x[:, 3] == 1]
    counts = np.bincount(sent[:, 0].astype(np.int64) * 256 + sent[:, 1], minlength=1 << 16)
    return ([BusTupleSendAir(XOR_TAG, 1, 3), BusKeyTableAir(XOR_TAG, 3)], [x, _mult(counts)],
            [None, generate_xor_key(8)], [(1, 3, [0])], None)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "multi_key.json")
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
    for name in ("range", "xor"):
        airs, host, keys, fills, twin = statement(name)
        T = len(airs)
        tape = lambda a, pw: ts.air_tape(a, 0, pw, *aux_dims(a))  # noqa: E731
        widths = [0 if k is None else k.shape[1] for k in keys]
        cairs = [ts.CompiledAir(ctx, tape(a, pw)) for a, pw in zip(airs, widths)]
        logups = [a.logup for a in airs]
        key = ts.MultiKey(config, [k.copy() for k in keys if k is not None])
        key_of = {}
        for t, k in enumerate(keys):
            if k is not None:
                key_of[t] = len(key_of)
        pre = [key.values(key_of[t]) if t in key_of else None for t in range(T)]
        challenges = (np.arange(1, 9, dtype=np.uint64) * 0x1234567 % P).astype(np.uint32)

        def upload(traces=host):
            m = [ts.DeviceMatrix.upload(ctx, t) for t in traces]
            ctx.synchronize()
            return m

        def with_knob(knob, fn):
            for k in (LOGUP_KNOB, OPEN_KNOB):
                os.environ.pop(k, None)
            if knob:
                os.environ[knob] = "1"
            try:
                return fn()
            finally:
                os.environ.pop(knob or LOGUP_KNOB, None)

        def prove_key(knob=None):
            def run():
                tr = upload()
                return timed(lambda: ts.prove_multi_key(config, key, cairs, ts.BfChallenger(), tr, [[]] * T, logups))
            return with_knob(knob, run)

        legs = {"key": lambda: prove_key(), "key_per_table": lambda: prove_key(LOGUP_KNOB),
                "key_generic": lambda: prove_key(OPEN_KNOB)}
        if twin:
            bus_airs, bus_host = twin
            bus_cairs = [ts.CompiledAir(ctx, tape(a, 0)) for a in bus_airs]
            bus_logups = [a.logup for a in bus_airs]

            def prove_bus():
                def run():
                    tr = upload(bus_host)
                    return timed(lambda: ts.prove_multi_bus(config, bus_cairs, ts.BfChallenger(), tr, [[]] * T, bus_logups))
                return with_knob(None, run)
            legs["bus"] = prove_bus

        resident = upload()

        def lookers_of(n_values, senders):
            s = n_values + 1
            out_ = []
            for i in senders:
                k = host[i].shape[1] // s
                out_.append((resident[i], [[("col", s * j + q) for q in range(n_values)] for j in range(k)],
                             [("col", s * j + n_values) for j in range(k)]))
            return out_

        def fill_pre():
            def run():
                for t, nv, senders in fills:
                    logup_multiplicities_bus(resident[t], [("prep", q) for q in range(nv)], lookers_of(nv, senders),
                                             out_column=0, negate=1, table_preprocessed=pre[t])
            return timed(run)

        def fill_host():
            def run():
                for t, nv, senders in fills:
                    counts = np.zeros(host[t].shape[0], dtype=np.int64)
                    for i in senders:
                        g = resident[i].download().reshape(host[i].shape[0], -1, nv + 1)
                        sel = g[g[:, :, nv] == 1].astype(np.int64)
                        idx = sel[:, 0] if nv == 1 else sel[:, 0] * 256 + sel[:, 1]  # the row of the tuple in its table
                        counts += np.bincount(idx, minlength=len(counts))
                    resident[t] = ts.DeviceMatrix.upload(ctx, _mult(counts))
            return timed(run)

        legs.update({
            "build_multi_pre": lambda: timed(lambda: logup_build_multi(logups, resident, challenges, preprocessed=pre)),
            "build_loop": lambda: timed(lambda: [lg.build(m, challenges, preprocessed=p)
                                                 for lg, m, p in zip(logups, resident, pre)]),
            "fill_pre": fill_pre, "fill_host": fill_host,
        })
        # warm-up (pools, twiddles, the specialisations) and the equalities the legs rest on
        _, a = prove_key()
        _, b = prove_key(LOGUP_KNOB)
        _, c = prove_key(OPEN_KNOB)
        assert all(len(a.words) == len(x.words) and (a.words == x.words).all() for x in (b, c)), "the legs disagree"
        _, s = ts.verify_multi_key(config, key.root, [ts.CompiledAir(None, tape(x, pw)) for x, pw in zip(airs, widths)],
                                   ts.BfChallenger(), a, [[]] * T)
        assert not s.any()
        words = {"key": int(len(a.words))}
        if twin:
            _, v7 = legs["bus"]()
            words["bus"] = int(len(v7.words))
        for fill in (fill_pre, fill_host):
            fill()
            assert all((resident[t].download() == host[t]).all() for t, _, _ in fills)
        for leg in ("build_multi_pre", "build_loop"):
            legs[leg]()
        medians = {k: [] for k in legs}
        for rep in range(REPEATS):
            rec = {k: [] for k in legs}
            for i in range(reps):  # a fresh order every repetition: a rotation would keep every leg behind the same
                # neighbour, and the leg behind fill_host (tens of ms with the GPU idle) then measures the idle gap
                for k in np.random.RandomState(1000 * rep + i).permutation(list(legs)):
                    rec[k].append(legs[k]()[0])
            for k, v in rec.items():
                medians[k].append(med(v))
        ms = {k: {"median_ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4),
                  "medians_ms": [round(x, 4) for x in v]} for k, v in medians.items()}
        out[name] = {
            "tables": [{"air": type(x).__name__, "rows_log2": int(t.shape[0]).bit_length() - 1, "width": int(t.shape[1]),
                        "aux_width": x.aux_width, "preprocessed_width": pw} for x, t, pw in zip(airs, host, widths)],
            "ms": ms, "proof_words": words,
        }
    doc = {"workload": f"key tables on the bus, FRI {CFG}, one context, the key committed outside the timed region, legs "
                       f"alternated in a fresh random order per repetition; per leg the median of {reps} repetitions, measured {REPEATS} times: median_ms is the "
                       f"median of the {REPEATS} medians, spread_ms their max - min",
           "statements": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {"ms": {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()},
                          "proof_words": v["proof_words"]} for k, v in out.items()}))


if __name__ == "__main__":
    main()
