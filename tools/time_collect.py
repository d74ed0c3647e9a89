"""What collecting the selected rows of a resident trace costs against its neighbours, in one process on one context:

    python tools/time_collect.py [REPS [OUT.json]]      (default 20 profiles/collect.json)

2^20 resident source rows.  The width-10 source is a machine trace with two access slots per row, (clk, ts_a, addr_a,
val_a, sel_a, ts_b, addr_b, val_b, wr_b, sel_b), and the spec is airs.memory_cpu_collect_spec: two emitters, out_width
5.  Cases, each with its own three legs:

    half       each selector fires on 49 % of the rows: about 2^20 rows out, padded to 2^20
    all        both selectors fire on every row: 2^21 rows out, no pad row
    none       no selector fires: one pad row out -- what the two passes over the selector columns and the wait cost
    sources    the `half` trace as two sources of 2^19 rows, the same two emitters on each (four in the spec): the words of
               `half` again
    slots      8 emitters on a width-24 source (8 slots of (addr, value, sel), 12 % selected each): about 2^20 rows out

    collect    ts_matrix_collect_rows with out_height 0
    copy       a device-to-device copy of a matrix of the OUTPUT's size (ts_matrix_from_device): the bytes a collect cannot
               avoid writing
    host       the host route a caller has today: download, one boolean mask over the (rows, slots) grid of reshaped
               tuples -- numpy's row-major order is the order rule -- pad to a power of two, upload
               (the library's own sequential loop, ts_collect_rows_host, is a reference and no yardstick)

Legs are alternated inside every repetition in an order drawn anew (seeded) for every repetition.  Median over REPS
repetitions of the host clock around the call (the context synchronised before and after, so the call's own wait is
inside; every device leg runs once untimed just before, so that the timed call starts on a busy GPU whichever leg came
before it); the whole measurement is repeated three times and every median is given with the spread (max - min) of the
three.  No time is fixed in advance: the figures are written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.airs import MemoryCpuAir, memory_cpu_collect_spec  # noqa: E402
from tapstark_amd.collect import ROW, CollectSpec, col  # noqa: E402

P = 0x78000001
LOG_N = 20
REPEATS = 3
A = MemoryCpuAir


def cpu_source(n, density):
    r = np.random.default_rng(1234)
    host = r.integers(0, P, size=(n, A.WIDTH), dtype=np.uint32)
    host[:, A.CLK] = np.arange(n)
    host[:, A.TS_A], host[:, A.TS_B] = 2 * np.arange(n), 2 * np.arange(n) + 1
    host[:, A.SEL_A], host[:, A.SEL_B] = r.random(n) < density, r.random(n) < density
    host[:, A.WR_B] = r.integers(0, 2, n)
    return host


def two_sources_spec():
    spec = CollectSpec([A.WIDTH, A.WIDTH], 5)
    for s in range(2):
        spec.emit(s, when=col(A.SEL_A), terms=[col(A.ADDR_A), col(A.TS_A), col(A.VAL_A), 0, 1])
        spec.emit(s, when=col(A.SEL_B), terms=[col(A.ADDR_B), col(A.TS_B), col(A.VAL_B), col(A.WR_B), 1])
    return spec


def slots_source(n, density):
    r = np.random.default_rng(4321)
    host = r.integers(0, P, size=(n, 24), dtype=np.uint32)
    host[:, 2::3] = r.random((n, 8)) < density
    return host


def slots_spec():
    spec = CollectSpec([24], 5)
    for e in range(8):
        spec.emit(0, when=col(3 * e + 2), terms=[col(3 * e), ROW, col(3 * e + 1), e, 1])
    return spec


def padded(rows):
    height = 1
    while height < len(rows):
        height *= 2
    out = np.zeros((height, rows.shape[1]), dtype=np.uint32)
    out[:len(rows)] = rows
    return out


def host_cpu(ctx, residents):
    """The two-slot spec on the host: one (rows, 2, 5) grid of reshaped tuples per source, masked, stacked."""
    parts = []
    for m in residents:
        rows = m.download()
        grid = np.zeros((rows.shape[0], 2, 5), dtype=np.uint32)
        grid[:, 0, :3] = rows[:, [A.ADDR_A, A.TS_A, A.VAL_A]]
        grid[:, 1, :4] = rows[:, [A.ADDR_B, A.TS_B, A.VAL_B, A.WR_B]]
        grid[:, :, 4] = 1
        parts.append(grid[rows[:, [A.SEL_A, A.SEL_B]] % P != 0])
    return ts.DeviceMatrix.upload(ctx, padded(np.concatenate(parts)))


def host_slots(ctx, residents):
    rows = residents[0].download()
    n = rows.shape[0]
    grid = np.zeros((n, 8, 5), dtype=np.uint32)
    grid[:, :, 0], grid[:, :, 2] = rows[:, 0::3], rows[:, 1::3]
    grid[:, :, 1] = np.arange(n, dtype=np.uint32)[:, None]
    grid[:, :, 3] = np.arange(8, dtype=np.uint32)[None, :]
    grid[:, :, 4] = 1
    return ts.DeviceMatrix.upload(ctx, padded(grid[rows[:, 2::3] % P != 0]))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "collect.json")
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
    half = cpu_source(n, 0.49)
    cases = {
        "half": (memory_cpu_collect_spec(), [half], host_cpu),
        "all": (memory_cpu_collect_spec(), [cpu_source(n, 2.0)], host_cpu),
        "none": (memory_cpu_collect_spec(), [cpu_source(n, -1.0)], host_cpu),
        "sources": (two_sources_spec(), [half[:n // 2], half[n // 2:]], host_cpu),
        "slots": (slots_spec(), [slots_source(n, 0.12)], host_slots),
    }
    out = {}
    for name, (spec, sources, host_route) in cases.items():
        residents = [ts.DeviceMatrix.upload(ctx, s) for s in sources]
        result, n_live = ts.collect_rows(ctx, spec, residents)
        height, width = result.dims()
        legs = {
            "collect": lambda: timed(lambda: ts.collect_rows(ctx, spec, residents)[0]),
            "copy": lambda: timed(lambda: ts.DeviceMatrix.from_device_ptr(ctx, result.device_ptr(), height, width)),
            "host": lambda: timed(lambda: host_route(ctx, residents), warm=False),
        }
        # warm-up, and the equalities the comparison rests on
        want = legs["host"]()[1].download()
        assert (legs["collect"]()[1].download() == want).all(), name
        assert (legs["copy"]()[1].download() == want).all(), name
        ms = measure(legs)
        # the three kernels one by one, in a pass of its own after the timed legs: HIP events around every launch
        ctx.synchronize()
        ctx.take_kernel_timings()
        ctx.set_kernel_timing(True)
        for _ in range(reps):
            ts.collect_rows(ctx, spec, residents)
        ctx.synchronize()
        kernels = {k: round(total / count, 4) for k, (count, total) in ctx.take_kernel_timings().items()
                   if k.startswith("k_collect")}
        ctx.set_kernel_timing(False)
        out[name] = {"kernel_mean_ms": kernels, "source_rows_log2": LOG_N, "src_widths": [int(s.shape[1]) for s in sources],
                     "n_emitters": len(spec.emitters), "n_live": int(n_live), "out_height": int(height),
                     "out_width": int(width), "bytes_of_the_result": int(4 * height * width),
                     "bytes_of_the_sources": int(sum(4 * s.size for s in sources)), "ms": ms,
                     "collect_over_copy": round(ms["collect"]["median_ms"] / ms["copy"]["median_ms"], 2),
                     "host_over_collect": round(ms["host"]["median_ms"] / ms["collect"]["median_ms"], 1)}
        del residents, result

    # the one host wait: a synchronisation of an idle context costs what the wait alone costs at least
    ctx.synchronize()
    waits = []
    for _ in range(200):
        t0 = time.perf_counter()
        ctx.synchronize()
        waits.append(1e3 * (time.perf_counter() - t0))
    doc = {"workload": f"ts_matrix_collect_rows on 2^{LOG_N} resident source rows, one context, legs alternated; per leg the "
                       f"median of {reps} repetitions, measured {REPEATS} times: median_ms is the median of the "
                       f"{REPEATS} medians, spread_ms their max - min",
           "idle_synchronize_ms": round(med(waits), 4),
           "unmeasured": ["sources of other widths and heights", "out_height given instead of 0", "sixteen emitters",
                          "hardware counters of the kernels"],
           "cases": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()} for k, v in out.items()}))


if __name__ == "__main__":
    main()
