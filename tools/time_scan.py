"""What scanning columns of a resident trace costs against its neighbours, in one process on one context:

    python tools/time_scan.py [REPS [OUT.json]]      (default 20 profiles/scan.json)

2^20 resident rows of widths 4 and 16.  Column 0 holds uniform field elements, column 1 an `a` = 1 - flag (a quarter of
the rows are flagged), column 2 a `b` = flag * value, column 3 a group-start bit (a group every 64 rows on average, each
starting with a flagged row); wider matrices carry uniform columns behind them.  Legs, alternated inside every
repetition in an order drawn anew (seeded) for every repetition:

    sum        ts_matrix_scan: one running sum of column 0, written over it
    carry      ts_matrix_scan: one segmented "carry the last flagged value": y = a y' + b from columns 1 and 2, started
               over at every group start, written over column 2 (the two helper columns are in the source already: the
               ts_matrix_derive call that makes them is tools/time_derive.py's subject)
    four       ts_matrix_scan: four scans in one call -- the two above, a running product of column 0 and an exclusive
               segmented sum of column 2, the last two appended (width + 2 columns out)
    copy       a device-to-device copy of a matrix of the OUTPUT's size (ts_matrix_from_device): the bytes a scan cannot
               avoid; copy_wide is the same for the output of `four`
    host_sum   the host route a caller has today for the running sum: download, np.cumsum mod p, upload
    host_carry the same for carry: download, np.maximum.accumulate over the flagged row numbers, index, upload
               (numpy cannot vectorise a product or a general recurrence, so `four` has no host leg; the library's own
               sequential loop, ts_scan_rows_host, is a reference and no yardstick)

Median over REPS repetitions of the host clock around the call (the context synchronised before and after, so a wait of
the call's own would be inside; every device leg runs once untimed just before, so that the timed call starts on a busy
GPU whichever leg came before it); the whole measurement is repeated three times and every median is given with the
spread (max - min) of the three.  No time is fixed in advance: the figures are written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.scan import ScanSpec, col, running_product, running_sum  # noqa: E402

P = 0x78000001
LOG_N = 20
REPEATS = 3


def source(n, width):
    r = np.random.default_rng(1234 + width)
    host = r.integers(0, P, size=(n, width), dtype=np.uint32)
    start = r.integers(0, 64, n) == 0
    start[0] = True
    flag = (r.integers(0, 4, n) == 0) | start
    host[:, 1] = 1 - flag
    host[:, 2] = np.where(flag, host[:, 2], 0)
    host[:, 3] = start
    return host


def carry_spec():
    return ScanSpec().add(2, a=col(1), b=col(2), init=0, reset=3)


def four_spec(width):
    spec = running_sum(0).extend(carry_spec()).extend(running_product(0, dst=width))
    return spec.extend(running_sum(2, reset=3, dst=width + 1, exclusive=True))


def host_sum(ctx, resident):
    rows = resident.download()
    rows[:, 0] = np.cumsum(rows[:, 0].astype(np.uint64)) % np.uint64(P)  # 2^20 words below 2^31: no overflow
    return ts.DeviceMatrix.upload(ctx, rows)


def host_carry(ctx, resident):
    rows = resident.download()
    flagged = rows[:, 1] == 0  # every group starts with a flagged row, so the flags alone say where a value comes from
    last = np.maximum.accumulate(np.where(flagged, np.arange(rows.shape[0]), 0))
    rows[:, 2] = rows[last, 2]
    return ts.DeviceMatrix.upload(ctx, rows)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "scan.json")
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
    out = {}
    for width in (4, 16):
        resident = ts.DeviceMatrix.upload(ctx, source(n, width))
        s_sum, s_carry, s_four = running_sum(0), carry_spec(), four_spec(width)
        narrow, wide = resident.scan(s_sum), resident.scan(s_four)

        legs = {
            "sum": lambda: timed(lambda: resident.scan(s_sum)),
            "carry": lambda: timed(lambda: resident.scan(s_carry)),
            "four": lambda: timed(lambda: resident.scan(s_four)),
            "copy": lambda: timed(lambda: ts.DeviceMatrix.from_device_ptr(ctx, narrow.device_ptr(), n, width)),
            "copy_wide": lambda: timed(lambda: ts.DeviceMatrix.from_device_ptr(ctx, wide.device_ptr(), n, width + 2)),
            "host_sum": lambda: timed(lambda: host_sum(ctx, resident), warm=False),
            "host_carry": lambda: timed(lambda: host_carry(ctx, resident), warm=False),
        }
        # warm-up, and the equalities the comparison rests on
        want_sum, want_carry = legs["host_sum"]()[1].download(), legs["host_carry"]()[1].download()
        assert (legs["sum"]()[1].download() == want_sum).all(), "sum"
        assert (legs["carry"]()[1].download() == want_carry).all(), "carry"
        four = legs["four"]()[1].download()
        assert (four[:, 0] == want_sum[:, 0]).all() and (four[:, 2] == want_carry[:, 2]).all(), "four"
        assert (legs["copy"]()[1].download() == want_sum).all() and (legs["copy_wide"]()[1].download() == four).all()
        out[f"width {width}"] = {"rows_log2": LOG_N, "src_width": width, "out_width": {"sum": width, "carry": width,
                                                                                      "four": width + 2},
                                 "bytes_of_the_result": {"narrow": int(4 * n * width), "wide": int(4 * n * (width + 2))},
                                 "ms": measure(legs)}
        del resident, narrow, wide

    doc = {"workload": f"ts_matrix_scan on a resident 2^{LOG_N}-row matrix, one context, legs alternated; per leg the "
                       f"median of {reps} repetitions, measured {REPEATS} times: median_ms is the median of the "
                       f"{REPEATS} medians, spread_ms their max - min",
           "cases": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()} for k, v in out.items()}))


if __name__ == "__main__":
    main()
