"""What fetching table columns by key into a resident trace costs against its neighbours, in one process on one context:

    python tools/time_join.py [REPS [OUT.json]]      (default 20 profiles/join.json)

2^20 resident source rows.  Cases, each with its own four legs:

    t10, t16, t20   one key word against tables of 2^10, 2^16 and 2^20 rows, 2 columns fetched into a width-8 source;
                    every row takes part and finds its key
    key3            a 3-word key against a table of 2^16 rows, 8 columns fetched into a width-24 source
    half            t16 with a `when` column that fires on half of the rows
    onekey          t16 with the same key on every row

    join       ts_matrix_join_rows
    copy       a device-to-device copy of a matrix of the RESULT's size (ts_matrix_from_device): the bytes a join cannot
               avoid writing
    mult       ts_logup_multiplicities_bus over the same keys (weight: the `when` term): the same insert and probe
               without the fetch, with an add per row and a write pass over the table instead
    host       the host route a caller has today: download the source, sort the table's keys, np.searchsorted, index,
               upload (the library's own sequential loop, ts_join_rows_host, is a reference and no yardstick)

Legs are alternated inside every repetition in an order drawn anew (seeded) for every repetition.  Median over REPS
repetitions of the host clock around the call (the context synchronised before and after, so the call's own wait is
inside; every device leg runs once untimed just before, so that the timed call starts on a busy GPU whichever leg came
before it); the whole measurement is repeated three times and every median is given with the spread (max - min) of the
three.  Then, in a pass of its own, HIP events around the two kernels.  No time is fixed in advance: the figures are
written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.air import logup_multiplicities_bus  # noqa: E402
from tapstark_amd.join import ALWAYS, JoinSpec, col  # noqa: E402

P = 0x78000001
LOG_N = 20
REPEATS = 3


def make_case(seed, log_table, n_keys, n_fetch, src_width, when=False, one_key=False):
    """(spec, source, table): the table's columns are keys, fetched values, one spare column (the multiplicity leg
    writes it); key words are below 2^20 so that the host route can pack a tuple into one 64-bit word."""
    r = np.random.default_rng(seed)
    n, m = 1 << LOG_N, 1 << log_table
    table = r.integers(0, P, size=(m, n_keys + n_fetch + 1), dtype=np.uint32)
    table[:, 0] = r.permutation(1 << 20)[:m]  # distinct: every tuple is a class of one
    table[:, 1:n_keys] = r.integers(0, 1 << 20, size=(m, n_keys - 1))
    src = r.integers(0, P, size=(n, src_width), dtype=np.uint32)
    src[:, :n_keys] = table[np.full(n, 77) if one_key else r.integers(0, m, size=n), :n_keys]
    when_col = src_width - 1
    src[:, when_col] = r.integers(0, 2, size=n)
    dst = list(range(n_keys, n_keys + n_fetch))
    spec = JoinSpec(keys=[(col(q), col(q)) for q in range(n_keys)], when=col(when_col) if when else ALWAYS,
                    fetch=[(n_keys + f, dst[f], 0) for f in range(n_fetch)])
    return spec, src, table


def pack(keys):
    out = np.zeros(len(keys), dtype=np.uint64)
    for q in range(keys.shape[1]):
        out = (out << np.uint64(20)) | keys[:, q].astype(np.uint64)
    return out


def host_route(ctx, spec, d_src, table):
    """download, sort the table's keys, search, index, upload"""
    src = d_src.download()
    n_keys = len(spec.keys)
    tkeys, skeys = pack(table[:, :n_keys]), pack(src[:, :n_keys])
    order = np.argsort(tkeys, kind="stable")
    rows = order[np.searchsorted(tkeys[order], skeys)]  # (every key is in the table)
    out = src.copy()
    part = slice(None) if spec.when == ALWAYS else src[:, spec.when[1]] % P != 0
    tcols, dcols = [f[0] for f in spec.fetch], [f[1] for f in spec.fetch]
    out[:, dcols] = 0
    out[part, dcols[0]:dcols[-1] + 1] = table[rows[part], tcols[0]:tcols[-1] + 1]
    return ts.DeviceMatrix.upload(ctx, out)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "join.json")
    from tapstark_amd.build import build

    build()
    ctx = ts.Context(0)
    med = lambda v: float(np.median(v))  # noqa: E731

    def timed(fn, warm=True):
        # the same call once untimed first: a timed call then starts on a GPU that was busy a moment ago, as it is for a
        # trace born in HBM, whichever leg ran before it (tools/time_collect.py)
        if warm:
            fn()
        ctx.synchronize()
        t0 = time.perf_counter()
        r = fn()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), r

    shuffle = np.random.default_rng(99)

    def measure(legs):
        medians = {k: [] for k in legs}
        for _ in range(REPEATS):
            rec = {k: [] for k in legs}
            for i in range(reps):
                for k in shuffle.permutation(list(legs)):
                    rec[k].append(legs[k]()[0])
            for k, v in rec.items():
                medians[k].append(med(v))
        return {k: {"median_ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4),
                    "medians_ms": [round(x, 4) for x in v]} for k, v in medians.items()}

    cases = {
        "t10": make_case(1, 10, 1, 2, 8),
        "t16": make_case(2, 16, 1, 2, 8),
        "t20": make_case(3, 20, 1, 2, 8),
        "key3": make_case(4, 16, 3, 8, 24),
        "half": make_case(5, 16, 1, 2, 8, when=True),
        "onekey": make_case(6, 16, 1, 2, 8, one_key=True),
    }
    out = {}
    for name, (spec, src, table) in cases.items():
        d_src, d_table = ts.DeviceMatrix.upload(ctx, src), ts.DeviceMatrix.upload(ctx, table)
        result, n_missing, _ = d_src.join_rows(d_table, spec)
        height, width = result.dims()
        n_keys, spare = len(spec.keys), table.shape[1] - 1
        looker = [(d_src, [[("col", q) for q in range(n_keys)]],
                   [("const", 1) if spec.when == ALWAYS else ("col", spec.when[1])])]
        legs = {
            "join": lambda: timed(lambda: d_src.join_rows(d_table, spec)[0]),
            "copy": lambda: timed(lambda: ts.DeviceMatrix.from_device_ptr(ctx, result.device_ptr(), height, width)),
            "mult": lambda: timed(lambda: logup_multiplicities_bus(d_table, [("col", q) for q in range(n_keys)], looker,
                                                                   out_column=spare, negate=0)),
            "host": lambda: timed(lambda: host_route(ctx, spec, d_src, table), warm=False),
        }
        # warm-up, and the equalities the comparison rests on
        want = legs["host"]()[1].download()
        assert (legs["join"]()[1].download() == want).all(), name
        assert (legs["copy"]()[1].download() == want).all(), name
        assert legs["mult"]()[1] == (0, None), name
        ms = measure(legs)
        # the two kernels one by one, in a pass of its own after the timed legs: HIP events around every launch
        ctx.synchronize()
        ctx.take_kernel_timings()
        ctx.set_kernel_timing(True)
        for _ in range(reps):
            d_src.join_rows(d_table, spec)
        ctx.synchronize()
        kernels = {k: round(total / count, 4) for k, (count, total) in ctx.take_kernel_timings().items()
                   if k.startswith("k_join")}
        ctx.set_kernel_timing(False)
        out[name] = {"kernel_mean_ms": kernels, "source_rows_log2": LOG_N, "src_width": int(src.shape[1]),
                     "table_rows_log2": int(table.shape[0]).bit_length() - 1, "table_width": int(table.shape[1]),
                     "n_keys": n_keys, "n_fetch": len(spec.fetch), "out_width": int(width),
                     "bytes_of_the_result": int(4 * height * width), "ms": ms,
                     "join_over_copy": round(ms["join"]["median_ms"] / ms["copy"]["median_ms"], 2),
                     "join_over_mult": round(ms["join"]["median_ms"] / ms["mult"]["median_ms"], 2),
                     "host_over_join": round(ms["host"]["median_ms"] / ms["join"]["median_ms"], 1)}
        print(name, out[name]["ms"]["join"], out[name]["kernel_mean_ms"], file=sys.stderr, flush=True)
        del d_src, d_table, result

    # the one host wait: a synchronisation of an idle context costs what the wait alone costs at least
    ctx.synchronize()
    waits = []
    for _ in range(200):
        t0 = time.perf_counter()
        ctx.synchronize()
        waits.append(1e3 * (time.perf_counter() - t0))
    doc = {"workload": f"ts_matrix_join_rows on 2^{LOG_N} resident source rows, one context, legs alternated; per leg the "
                       f"median of {reps} repetitions, measured {REPEATS} times: median_ms is the median of the "
                       f"{REPEATS} medians, spread_ms their max - min",
           "idle_synchronize_ms": round(med(waits), 4),
           "unmeasured": ["other source heights and widths", "8-word keys", "32 fetched columns", "2^27 rows",
                          "rows that miss", "hardware counters of the kernels"],
           "cases": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {"kernels": v["kernel_mean_ms"], **{leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()}}
                      for k, v in out.items()}))


if __name__ == "__main__":
    main()
