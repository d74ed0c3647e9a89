"""What grouping the rows of a resident trace by key costs against its neighbours, in one process on one context:

    python tools/time_group.py [REPS [OUT.json]]      (default 20 profiles/group.json)

2^20 resident source rows of width 8.  With one key (column 0) the spec gives (first(0), last(1), COUNT, total(2)) per
group.  Cases, each with its own legs:

    distinct   every row a group of its own: 2^20 groups, no wave is uniform in the accumulate pass
    random     2^16 random addresses: 2^16 groups of about 16 rows, scattered
    sorted     the same rows sorted by key: whole waves go to one group, the combined path
    one        all rows one group: one slot under all inserts, one record under all adds
    half       `random` with a selector that fires on half the rows
    wide       a 3-word key (2^16 tuples) with 8 aggregates (sums, minima, maxima)

    group      ts_matrix_collect_rows with the TGRP tape, out_height 0
    copy       a device-to-device copy of the SOURCE (ts_matrix_from_device): the bytes a group call must read, written
               once more
    host       the host route a caller had before: download, np.lexsort and reduceat over the sorted keys, groups put back
               in order of first appearance, pad to a power of two, upload
    composed   on `sorted` only, the device route available before: sort (group starts), derive (group ends), scan (the
               count and the sum down each group), collect (the rows where a group ends)

Legs are alternated inside every repetition in an order drawn anew (seeded) for every repetition.  Median over REPS
repetitions of the host clock around the call (the context synchronised before and after, so the call's own wait is
inside; every device leg runs once untimed just before); the whole measurement is repeated three times and every median
is given with the spread (max - min) of the three.  The device result is compared with group_rows_host once per case
before anything is timed.  No time is fixed in advance: the figures are written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.collect import ALWAYS, CollectSpec, col  # noqa: E402
from tapstark_amd.derive import DeriveBuilder  # noqa: E402
from tapstark_amd.group import COUNT, GroupSpec, first, greatest, group_rows_host, last, least, total  # noqa: E402
from tapstark_amd.scan import ScanSpec  # noqa: E402
from tapstark_amd.scan import col as scol  # noqa: E402

P = 0x78000001
LOG_N = 20
WIDTH = 8
REPEATS = 3
SEL = 7  # the selector column of `half`


def source(keys, seed=1234):
    r = np.random.default_rng(seed)
    host = r.integers(0, P, size=(len(keys), WIDTH), dtype=np.uint32)
    host[:, 0] = keys
    host[:, SEL] = r.integers(0, 2, size=len(keys))
    return host


def one_key_spec(when=ALWAYS):
    return GroupSpec(WIDTH, 4, [col(0)], when=when, terms=[first(0), last(1), COUNT, total(2)])


def wide_spec():
    terms = [first(0), first(1), first(2), COUNT] + [[total, least, greatest][a % 3](3 + a % 4) for a in range(8)]
    return GroupSpec(WIDTH, len(terms), [col(0), col(1), col(2)], terms=terms)


def padded(rows):
    height = 1
    while height < len(rows):
        height *= 2
    out = np.zeros((height, rows.shape[1]), dtype=np.uint32)
    out[:len(rows)] = rows
    return out


def host_route(ctx, resident, spec):
    """np.lexsort (stable) over the key columns of the rows that take part, reduceat per term, first appearance order."""
    rows = resident.download()
    t = spec.tape()
    n_keys = int(t[4])
    at = np.arange(rows.shape[0])
    if t[5] == 1:
        at = at[rows[:, int(t[6])] % P != 0]
    key_cols = [int(t[8 + 2 * q]) for q in range(n_keys)]
    order = at[np.lexsort([rows[at, c] for c in reversed(key_cols)])] if len(at) else at
    if len(order) == 0:
        return ts.DeviceMatrix.upload(ctx, np.zeros((1, spec.out_width), dtype=np.uint32))
    keys = rows[order][:, key_cols]
    starts = np.flatnonzero(np.concatenate([[True], (keys[1:] != keys[:-1]).any(axis=1)]))
    ends = np.concatenate([starts[1:], [len(order)]]) - 1
    terms = t[7 + 2 * n_keys + spec.out_width:].reshape(-1, 2)
    out = np.zeros((len(starts), spec.out_width), dtype=np.uint32)
    for c, (kind, value) in enumerate(terms.tolist()):
        if kind == 0:
            out[:, c] = value
        elif kind == 1:
            out[:, c] = rows[order[starts], value]
        elif kind == 2:
            out[:, c] = rows[order[ends], value]
        elif kind == 5:
            out[:, c] = ends - starts + 1
        else:
            words = (rows[order, value] % P).astype(np.uint64)
            fn = {6: np.add, 7: np.minimum, 8: np.maximum}[kind]
            out[:, c] = fn.reduceat(words, starts) % P
    return ts.DeviceMatrix.upload(ctx, padded(out[np.argsort(order[starts], kind="stable")]))


def composed_route(ctx, resident):
    """sort -> derive -> scan -> collect for the one-key spec: what the parent offers, on sorted input only."""
    d = resident.sort_rows([0], group_keys=1, group_start=True)  # column 8: a group starts
    ends = DeriveBuilder(WIDTH + 1)
    ends.output(ends.is_last_row() + (1 - ends.is_last_row()) * ends.next(WIDTH), WIDTH + 1)  # 9: a group ends
    ends.output(ends.constant(0), WIDTH + 2)
    ends.output(ends.constant(0), WIDTH + 3)
    d = d.derive(ends)
    d = d.scan(ScanSpec().add(WIDTH + 2, a=1, b=1, init=0, reset=WIDTH).add(WIDTH + 3, a=1, b=scol(2), init=0, reset=WIDTH))
    spec = CollectSpec([WIDTH + 4], 4).emit(0, when=col(WIDTH + 1), terms=[col(0), col(1), col(WIDTH + 2), col(WIDTH + 3)])
    return ts.collect_rows(ctx, spec, [d])[0]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "group.json")
    from tapstark_amd.build import build

    build()
    ctx = ts.Context(0)
    med = lambda v: float(np.median(v))  # noqa: E731

    def timed(fn, warm=True):
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
    addresses = r.integers(0, 1 << 16, size=n).astype(np.uint32)
    rand = source(addresses)
    wide = source(addresses & 0xFF)
    wide[:, 1], wide[:, 2] = (addresses >> 8) & 0xF, addresses >> 12
    cases = {
        "distinct": (one_key_spec(), source(r.permutation(n).astype(np.uint32))),
        "random": (one_key_spec(), rand),
        "sorted": (one_key_spec(), rand[np.argsort(rand[:, 0], kind="stable")]),
        "one": (one_key_spec(), source(np.full(n, 5, dtype=np.uint32))),
        "half": (one_key_spec(when=col(SEL)), rand),
        "wide": (wide_spec(), wide),
    }
    out = {}
    for name, (spec, host) in cases.items():
        resident = ts.DeviceMatrix.upload(ctx, host)
        result, n_live = ts.group_rows(ctx, spec, resident)
        height, width = result.dims()
        want, want_live = group_rows_host(spec, host)
        assert n_live == want_live and (result.download() == want).all(), name
        legs = {
            "group": lambda: timed(lambda: ts.group_rows(ctx, spec, resident)[0]),
            "copy": lambda: timed(lambda: ts.DeviceMatrix.from_device_ptr(ctx, resident.device_ptr(), n, WIDTH)),
            "host": lambda: timed(lambda: host_route(ctx, resident, spec), warm=False),
        }
        assert (legs["host"]()[1].download() == want).all(), name
        if name == "sorted":
            legs["composed"] = lambda: timed(lambda: composed_route(ctx, resident))
            got = legs["composed"]()[1].download()
            assert (got[:n_live] == want[:n_live]).all() and not got[n_live:].any(), name
        ms = measure(legs)
        # the kernels one by one, in a pass of its own after the timed legs: HIP events around every launch
        ctx.synchronize()
        ctx.take_kernel_timings()
        ctx.set_kernel_timing(True)
        for _ in range(reps):
            ts.group_rows(ctx, spec, resident)
        ctx.synchronize()
        kernels = {k: round(total_ms / count, 4) for k, (count, total_ms) in ctx.take_kernel_timings().items()
                   if k.startswith("k_group") or k == "k_collect_offsets"}
        ctx.set_kernel_timing(False)
        out[name] = {"kernel_mean_ms": kernels, "source_rows_log2": LOG_N, "src_width": WIDTH, "n_keys": len(spec.keys),
                     "n_groups": int(n_live), "out_height": int(height), "out_width": int(width),
                     "bytes_of_the_source": int(4 * host.size), "ms": ms,
                     "group_over_copy": round(ms["group"]["median_ms"] / ms["copy"]["median_ms"], 2),
                     "host_over_group": round(ms["host"]["median_ms"] / ms["group"]["median_ms"], 1)}
        if "composed" in ms:
            out[name]["composed_over_group"] = round(ms["composed"]["median_ms"] / ms["group"]["median_ms"], 2)
        del resident, result

    ctx.synchronize()
    waits = []
    for _ in range(200):
        t0 = time.perf_counter()
        ctx.synchronize()
        waits.append(1e3 * (time.perf_counter() - t0))
    doc = {"workload": f"the TGRP tape of ts_matrix_collect_rows on 2^{LOG_N} resident source rows of width {WIDTH}, one "
                       f"context, legs alternated; per leg the median of {reps} repetitions, measured {REPEATS} times: "
                       f"median_ms is the median of the {REPEATS} medians, spread_ms their max - min",
           "idle_synchronize_ms": round(med(waits), 4),
           "unmeasured": ["sources of other widths and heights", "out_height given instead of 0", "sixteen aggregates",
                          "hardware counters of the kernels", "the composed route on unsorted input (it has none)"],
           "cases": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()} for k, v in out.items()}))
    print(json.dumps({k: v["kernel_mean_ms"] for k, v in out.items()}))


if __name__ == "__main__":
    main()
