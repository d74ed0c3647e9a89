"""What sorting the rows of a resident trace costs against its neighbours, in one process on one context:

    python tools/time_sort.py [REPS [OUT.json]]      (default 20 profiles/sort_rows.json)

2^20 resident rows, widths 4 and 16, four key variants:

    uniform     one key column uniform in [0, p)                (4 digit passes, the top byte nearly trivial)
    addr16      one key column of 16-bit values                 (2 passes of 4: the upper bytes are skipped)
    all_equal   every key word equal                            (no pass at all: histogram, gather)
    addr_clk    two keys: 16 addresses, then the clock 0 .. n-1 (1 + 3 passes: a memory table)

Legs, alternated inside every repetition in an order drawn anew (seeded) for every repetition:

    sort   ts_matrix_sort_rows with source-row and group-start columns
    copy   a device-to-device copy of the same matrix (ts_matrix_from_device): the floor of the bytes that move
    host   the host route, what a caller did before: download, stable np.lexsort, index, upload

(profiles/sort_rows_keys_experiment.json is this tool's output from the time the library held two forms of the passes
behind a knob: `sort_carry`, the key word carried beside the row -- the form that stayed -- and `sort_reread`, the key
word re-read from the matrix through the permutation in every pass.)

Median over REPS repetitions of the host clock around the call (the context synchronised before and after, so the
call's own wait -- the histogram copy back -- is inside; every device leg runs once untimed just before, so that the
timed call starts on a busy GPU whichever leg came before it); the whole measurement is repeated three times and every
median is given with the spread (max - min) of the three.  No ratio is fixed in advance: the figures are written as
they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402

P = 0x78000001
LOG_N = 20
WIDTHS = (4, 16)
REPEATS = 3


def case(variant: str, width: int):
    """(host matrix, key columns) of a variant."""
    n = 1 << LOG_N
    r = np.random.default_rng(1234)
    m = r.integers(0, P, size=(n, width), dtype=np.uint32)
    keys = [0]
    if variant == "addr16":
        m[:, 0] = r.integers(0, 1 << 16, n, dtype=np.uint32)
    elif variant == "all_equal":
        m[:, 0] = 0x12345678
    elif variant == "addr_clk":
        m[:, 0] = r.integers(0, 16, n, dtype=np.uint32)
        m[:, 1] = np.arange(n, dtype=np.uint32)
        keys = [0, 1]
    elif variant != "uniform":
        raise KeyError(variant)
    return m, keys


def host_route(ctx, resident, keys):
    host = resident.download()
    order = np.lexsort([host[:, k] for k in reversed(keys)])
    return ts.DeviceMatrix.upload(ctx, np.ascontiguousarray(host[order]))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "sort_rows.json")
    from tapstark_amd.build import build

    build()
    ctx = ts.Context(0)
    med = lambda v: float(np.median(v))  # noqa: E731

    def timed(fn, warm=True):
        # the same call once untimed first: a timed call then starts on a GPU that was busy a moment ago, as it is
        # for a trace born in HBM, whichever leg ran before it (the leg behind `host` otherwise starts on a GPU that
        # idled for a tenth of a second: 0.03 to 0.07 ms on a 0.1 ms call, measured on two legs running the same code)
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
                # a seeded shuffle per repetition, not a rotation: a rotation keeps every leg behind the same neighbour
                for k in shuffle.permutation(list(legs)):
                    rec[k].append(legs[k]()[0])
            for k, v in rec.items():
                medians[k].append(med(v))
        return {k: {"median_ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4),
                    "medians_ms": [round(x, 4) for x in v]} for k, v in medians.items()}

    out = {}
    for width in WIDTHS:
        for variant in ("uniform", "addr16", "all_equal", "addr_clk"):
            host, keys = case(variant, width)
            resident = ts.DeviceMatrix.upload(ctx, host)
            n = host.shape[0]

            legs = {
                "sort": lambda: timed(lambda: resident.sort_rows(keys, group_keys=1, source_row=True, group_start=True)),
                "copy": lambda: timed(lambda: ts.DeviceMatrix.from_device_ptr(ctx, resident.device_ptr(), n, width)),
                "host": lambda: timed(lambda: host_route(ctx, resident, keys), warm=False),
            }
            # warm-up, and the equality the comparison rests on
            want = legs["host"]()[1].download()
            assert (legs["sort"]()[1].download()[:, :width] == want).all(), (variant, width)
            assert (legs["copy"]()[1].download() == host).all()
            out[f"{variant}_w{width}"] = {"rows_log2": LOG_N, "width": width, "keys": keys,
                                          "matrix_bytes": int(host.nbytes), "ms": measure(legs)}
            del resident

    doc = {"workload": f"ts_matrix_sort_rows on a resident 2^{LOG_N}-row matrix (source-row and group-start columns "
                       "appended), one context, legs alternated; per leg the median of "
                       f"{reps} repetitions, measured {REPEATS} times: median_ms is the median of the {REPEATS} "
                       "medians, spread_ms their max - min",
           "cases": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()} for k, v in out.items()}))


if __name__ == "__main__":
    main()
