"""What expanding the rows of a resident trace by a per-row count costs against its neighbours, in one process on one
context:

    python tools/time_expand.py [REPS [OUT.json]]      (default 20 profiles/expand.json)

2^20 resident source rows of width 8, (id, base, len, sel, d0 .. d3), into an output of width 8: (id, base, len, j,
first, last, d0, base + j).  Cases, each with its own three legs:

    ones        every row asks for 1: 2^20 rows out, the identity in height
    seeded      seeded counts 0 .. 7 on every row: about 3.5 * 2^20 rows out
    precompile  a constant 24 on 2^16 selected rows, the others take no part: 24 * 2^16 rows out
    skew        one row asks for 2^22, all others for 0: 2^22 rows out of one source row
    half        `when` selects half of the rows, seeded counts 0 .. 7 on them

    expand      ts_matrix_expand_rows with out_height 0
    copy        a device-to-device copy of a matrix of the OUTPUT's size (ts_matrix_from_device): the bytes an expansion
                cannot avoid writing
    host        the host route a caller has today: download, np.repeat of the rows by their counts, index ramps for j,
                first, last and the address, pad to a power of two, upload
                (the library's own sequential loop, ts_expand_rows_host, is a reference and no yardstick)

Legs are alternated inside every repetition in an order drawn anew (seeded) for every repetition.  Median over REPS
repetitions of the host clock around the call (the context synchronised before and after, so the call's own wait is
inside; every device leg runs once untimed just before, so that the timed call starts on a busy GPU whichever leg came
before it); the whole measurement is repeated three times and every median is given with the spread (max - min) of the
three.  Per case also ns per output row, so that the skew case can be set against the seeded one.  No time is fixed in
advance: the figures are written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.expand import ALWAYS, FIRST, J, LAST, ExpandSpec, col, stepped  # noqa: E402

P = 0x78000001
LOG_N = 20
REPEATS = 3
ID, BASE, LEN, SEL, D0 = 0, 1, 2, 3, 4
TERMS = [col(ID), col(BASE), col(LEN), J, FIRST, LAST, col(D0), stepped(BASE, 1)]


def source(n, counts, selected):
    r = np.random.default_rng(1234)
    host = r.integers(0, P, size=(n, 8), dtype=np.uint32)
    host[:, ID] = np.arange(n)
    host[:, BASE] = r.integers(0, 1 << 24, size=n)
    host[:, LEN] = counts
    host[:, SEL] = selected
    return host


def spec_for(count, when, max_count):
    return ExpandSpec(8, 8, count=count, when=when, max_count=max_count, terms=TERMS)


def host_route(ctx, resident, constant):
    """The spec on the host: np.repeat and index ramps, padded, uploaded."""
    rows = resident.download()
    n = rows.shape[0]
    takes = rows[:, SEL] % P != 0
    cnt = np.where(takes, constant if constant else rows[:, LEN] % P, 0).astype(np.int64)
    n_live = int(cnt.sum())
    r = np.repeat(np.arange(n), cnt)
    j = np.arange(n_live) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    height = 1
    while height < n_live:
        height *= 2
    out = np.zeros((height, 8), dtype=np.uint32)
    live = out[:n_live]
    live[:, :3] = rows[r, :3]
    live[:, 3] = j
    live[:, 4] = j == 0
    live[:, 5] = j == cnt[r] - 1
    live[:, 6] = rows[r, D0]
    live[:, 7] = (rows[r, BASE].astype(np.int64) % P + j) % P
    return ts.DeviceMatrix.upload(ctx, out)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "expand.json")
    from tapstark_amd.build import build

    build()
    ctx = ts.Context(0)
    med = lambda v: float(np.median(v))  # noqa: E731

    def timed(fn, warm=True):
        # the same call once untimed first: a timed call then starts on a GPU that was busy a moment ago, as it is for a
        # trace born in HBM, whichever leg ran before it (tools/time_sort.py)
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

    n = 1 << LOG_N
    r = np.random.default_rng(77)
    seeded = r.integers(0, 8, size=n)
    rows = np.arange(n)
    cases = {
        "ones": (spec_for(col(LEN), ALWAYS, 1), source(n, 1, 1), 0),
        "seeded": (spec_for(col(LEN), ALWAYS, 7), source(n, seeded, 1), 0),
        "precompile": (spec_for(24, col(SEL), 24), source(n, seeded, rows % 16 == 5), 24),
        "skew": (spec_for(col(LEN), ALWAYS, 1 << 22), source(n, np.where(rows == n // 3, 1 << 22, 0), 1), 0),
        "half": (spec_for(col(LEN), col(SEL), 7), source(n, seeded, r.integers(0, 2, size=n)), 0),
    }
    out = {}
    for name, (spec, host, constant) in cases.items():
        resident = ts.DeviceMatrix.upload(ctx, host)
        result, n_live = ts.expand_rows(ctx, spec, resident)
        height, width = result.dims()
        legs = {
            "expand": lambda: timed(lambda: ts.expand_rows(ctx, spec, resident)[0]),
            "copy": lambda: timed(lambda: ts.DeviceMatrix.from_device_ptr(ctx, result.device_ptr(), height, width)),
            "host": lambda: timed(lambda: host_route(ctx, resident, constant), warm=False),
        }
        # warm-up, and the equalities the comparison rests on
        want = legs["host"]()[1].download()
        assert (legs["expand"]()[1].download() == want).all(), name
        assert (legs["copy"]()[1].download() == want).all(), name
        ms = measure(legs)
        # the three kernels one by one, in a pass of its own after the timed legs: HIP events around every launch
        ctx.synchronize()
        ctx.take_kernel_timings()
        ctx.set_kernel_timing(True)
        for _ in range(reps):
            ts.expand_rows(ctx, spec, resident)
        ctx.synchronize()
        kernels = {k: round(total / count, 4) for k, (count, total) in ctx.take_kernel_timings().items()
                   if k.startswith("k_expand")}
        ctx.set_kernel_timing(False)
        out[name] = {"kernel_mean_ms": kernels, "source_rows_log2": LOG_N, "src_width": 8, "n_live": int(n_live),
                     "out_height": int(height), "out_width": int(width), "bytes_of_the_result": int(4 * height * width),
                     "bytes_of_the_source": int(4 * host.size), "ms": ms,
                     "expand_ns_per_output_row": round(1e6 * ms["expand"]["median_ms"] / max(n_live, 1), 4),
                     "write_kernel_ns_per_output_row": round(1e6 * kernels.get("k_expand_write", 0.0) / max(n_live, 1), 4),
                     "expand_over_copy": round(ms["expand"]["median_ms"] / ms["copy"]["median_ms"], 2),
                     "host_over_expand": round(ms["host"]["median_ms"] / ms["expand"]["median_ms"], 1)}
        del resident, result

    # the one host wait: a synchronisation of an idle context costs what the wait alone costs at least
    ctx.synchronize()
    waits = []
    for _ in range(200):
        t0 = time.perf_counter()
        ctx.synchronize()
        waits.append(1e3 * (time.perf_counter() - t0))
    doc = {"workload": f"ts_matrix_expand_rows on 2^{LOG_N} resident source rows of width 8 into width 8, one context, legs "
                       f"alternated; per leg the median of {reps} repetitions, measured {REPEATS} times: median_ms is the "
                       f"median of the {REPEATS} medians, spread_ms their max - min",
           "idle_synchronize_ms": round(med(waits), 4),
           "skew_against_seeded": {
               "skew_ns_per_output_row": out["skew"]["expand_ns_per_output_row"],
               "seeded_ns_per_output_row": out["seeded"]["expand_ns_per_output_row"],
               "skew_write_kernel_ns_per_output_row": out["skew"]["write_kernel_ns_per_output_row"],
               "seeded_write_kernel_ns_per_output_row": out["seeded"]["write_kernel_ns_per_output_row"]},
           "unmeasured": ["sources and outputs of other widths and heights", "out_height given instead of 0",
                          "hardware counters of the kernels"],
           "cases": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()} for k, v in out.items()}))
    print(json.dumps(doc["skew_against_seeded"]))


if __name__ == "__main__":
    main()
