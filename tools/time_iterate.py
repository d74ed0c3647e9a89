"""What walking a row program with carried state down the groups of a resident trace costs against its neighbours, in
one process on one context:

    python tools/time_iterate.py [REPS [OUT.json]]      (default 20 profiles/iterate.json)

2^20 resident rows of width 6, (first, last, id, word, acc, state), the sponge chip's table: acc = (the IV on a group's
first row, else the state of the row before) + word, state = acc^7, one carry.  Cases, each with its own legs:

    sponge      equal groups of 64 rows: 2^14 groups
    seeded      seeded group lengths 1 .. 128
    single      every row its own group; beside it `derive`: ts_matrix_derive of the same nodes with the constant IV for
                the carry, the yardstick for what the walk adds to the interpreter
    mixed       a 16-carry, 200-node program of field and integer ops over equal groups of 64
    cap         one group of max_group_rows = TS_ITERATE_MAX_WORK / (the length of the lowered list) rows among
                single-row groups: what one lane runs at the work limit

    iterate     the iterate form of ts_matrix_derive
    copy        a device-to-device copy of a matrix of the output's size (ts_matrix_from_device)
    host        the host route a caller has today: download, a numpy loop over the steps vectorised across the groups,
                upload (the library's own loop, ts_derive_rows_host, is a reference and no yardstick)

Legs are alternated inside every repetition in an order drawn anew (seeded) for every repetition.  Median over REPS
repetitions of the host clock around the call (the context synchronised before and after, so the call's own wait is
inside; every device leg runs once untimed just before); the whole measurement is repeated three times and every median
is given with the spread (max - min) of the three.  The host leg of the cap case makes 2^17 numpy steps and is timed
twice per measurement instead of REPS times.  Then the four kernels one by one, HIP events around every launch, in a
pass of its own.  No time is fixed in advance: the figures are written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd.derive import ADD, AND, BITS, COL, CONST, MUL, SUB, XOR, DeriveBuilder  # noqa: E402
from tapstark_amd.iterate import CARRY, MAX_WORK, STEP, IterateBuilder, iterate_check  # noqa: E402

P = 0x78000001
LOG_N = 20
REPEATS = 3
FIRST, LAST, ID, WORD, ACC, STATE = range(6)
IV = 0x5EED


def sponge(max_group_rows):
    b = IterateBuilder(6, reset_column=FIRST, max_group_rows=max_group_rows)
    state = b.carry(IV)
    acc = state + b.col(WORD)
    a2 = acc * acc
    a4 = a2 * a2
    new = a4 * a2 * acc
    b.set_carry(state, new)
    b.output(acc, ACC)
    b.output(new, STATE)
    return b


def sponge_row_local():
    """the sponge's nodes with the constant IV for the carry: what a TDER program makes of the same row"""
    b = DeriveBuilder(6)
    acc = b.constant(IV) + b.col(WORD)
    a2 = acc * acc
    a4 = a2 * a2
    b.output(acc, ACC)
    b.output(a4 * a2 * acc, STATE)
    return b


def mixed(max_group_rows):
    """16 carries, 200 nodes: every carry is mixed with its neighbour and the row's word by field and integer ops"""
    b = IterateBuilder(6, reset_column=FIRST, max_group_rows=max_group_rows)
    carries = [b.carry(k + 1) for k in range(16)]
    v = list(carries)
    word, step = b.col(WORD), b.step()
    k = 0
    while len(b.nodes) < 199:
        other = v[(k + 1) % 16]
        kind = len(b.nodes) % 6
        if kind == 0:
            v[k] = v[k] * other
        elif kind == 1:
            v[k] = v[k] + word
        elif kind == 2:
            v[k] = v[k] ^ other
        elif kind == 3:
            v[k] = v[k].bits(3, 20) + other
        elif kind == 4:
            v[k] = (v[k] & other) - step
        else:
            v[k] = v[k] * v[k]
        k = (k + 1) % 16
    for c, x in zip(carries, v):
        b.set_carry(c, x)
    b.output(v[0] + v[8], ACC)
    b.output(v[15], STATE)
    return b


def table(n, lengths):
    """(n, 6) rows whose `first` column starts groups of the given lengths (their sum is n)"""
    r = np.random.default_rng(1234)
    starts = np.cumsum(lengths) - lengths
    host = np.zeros((n, 6), dtype=np.uint32)
    host[starts, FIRST] = 1
    host[starts + lengths - 1, LAST] = 1
    host[:, ID] = np.repeat(np.arange(len(lengths)), lengths)
    host[:, WORD] = r.integers(0, P, size=n, dtype=np.uint32)
    return host, starts, lengths


def host_route(ctx, resident, builder, starts, lengths):
    """download, one numpy pass per step over every group that has such a row, upload"""
    rows = resident.download()
    out = rows.copy()
    p = np.uint64(P)
    order = np.argsort(-lengths, kind="stable")  # the groups that reach step t are a prefix
    s, ln = starts[order], lengths[order]
    state = [np.full(len(s), init, dtype=np.uint64) for _, init in builder.carries]
    for t in range(int(ln[0])):
        m = int(np.searchsorted(-ln, -t, side="left"))  # groups with length > t
        at = s[:m] + t
        v = []
        for op, a, b in builder.nodes:
            if op == CONST:
                x = np.full(m, a, dtype=np.uint64)
            elif op == COL:
                x = rows[at, b].astype(np.uint64) % p
            elif op == CARRY:
                x = state[a][:m]
            elif op == STEP:
                x = np.full(m, t, dtype=np.uint64)
            elif op == ADD:
                x = (v[a] + v[b]) % p
            elif op == SUB:
                x = (v[a] + p - v[b]) % p
            elif op == MUL:
                x = v[a] * v[b] % p
            elif op == XOR:
                x = (v[a] ^ v[b]) % p
            elif op == AND:
                x = v[a] & v[b]
            elif op == BITS:
                x = (v[a] >> np.uint64(b & 255)) & np.uint64((1 << (b >> 8)) - 1)
            else:
                raise AssertionError(op)
            v.append(x)
        for k, (node, _) in enumerate(builder.carries):
            state[k] = v[node]
        for node, dst in builder.outputs:
            out[at, dst] = v[node].astype(np.uint32)
    return ts.DeviceMatrix.upload(ctx, out)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "iterate.json")
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

    def measure(legs, few=()):
        medians = {k: [] for k in legs}
        for _ in range(REPEATS):
            rec = {k: [] for k in legs}
            for i in range(reps):
                for k in shuffle.permutation(list(legs)):
                    if k in few and i >= 2:
                        continue
                    rec[k].append(legs[k]()[0])
            for k, v in rec.items():
                medians[k].append(med(v))
        return {k: {"median_ms": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4),
                    "medians_ms": [round(x, 4) for x in v]} for k, v in medians.items()}

    n = 1 << LOG_N
    r = np.random.default_rng(77)
    seeded = r.integers(1, 129, size=n // 32)
    seeded = seeded[np.cumsum(seeded) <= n]
    seeded = np.concatenate([seeded, np.ones(n - int(seeded.sum()), dtype=seeded.dtype)])
    list_length = iterate_check(sponge(1), 6)["n_instructions"] + 1  # the nodes kept (both stores ride on theirs), one latch
    cap_rows = MAX_WORK // list_length
    cap_lengths = np.ones(n - cap_rows + 1, dtype=np.int64)
    cap_lengths[(n - cap_rows) // 3] = cap_rows
    cases = {
        "sponge": (sponge(64), np.full(n // 64, 64, dtype=np.int64)),
        "seeded": (sponge(128), seeded.astype(np.int64)),
        "single": (sponge(1), np.ones(n, dtype=np.int64)),
        "mixed": (mixed(64), np.full(n // 64, 64, dtype=np.int64)),
        "cap": (sponge(cap_rows), cap_lengths),
    }
    out = {}
    for name, (builder, lengths) in cases.items():
        host, starts, lengths = table(n, lengths)
        resident = ts.DeviceMatrix.upload(ctx, host)
        result = resident.iterate(builder)
        height, width = result.dims()
        legs = {
            "iterate": lambda: timed(lambda: resident.iterate(builder)),
            "copy": lambda: timed(lambda: ts.DeviceMatrix.from_device_ptr(ctx, result.device_ptr(), height, width)),
            "host": lambda: timed(lambda: host_route(ctx, resident, builder, starts, lengths), warm=False),
        }
        if name == "single":
            local = sponge_row_local()
            legs["derive"] = lambda: timed(lambda: resident.derive(local))
            assert (legs["derive"]()[1].download() == result.download()).all(), "the row-local program on single rows"
        # warm-up, and the equalities the comparison rests on
        want = legs["host"]()[1].download()
        assert (legs["iterate"]()[1].download() == want).all(), name
        assert (legs["copy"]()[1].download() == want).all(), name
        ms = measure(legs, few=("host",) if name == "cap" else ())
        # the four kernels one by one, in a pass of its own after the timed legs: HIP events around every launch
        ctx.synchronize()
        ctx.take_kernel_timings()
        ctx.set_kernel_timing(True)
        for _ in range(reps):
            resident.iterate(builder)
        ctx.synchronize()
        kernels = {k: round(total / count, 4) for k, (count, total) in ctx.take_kernel_timings().items()
                   if k.startswith("k_iterate")}
        ctx.set_kernel_timing(False)
        info = iterate_check(builder, 6)
        out[name] = {"kernel_mean_ms": kernels, "rows_log2": LOG_N, "width": int(width), "n_groups": int(len(lengths)),
                     "longest_group": int(lengths.max()), "n_nodes": len(builder.nodes), "n_carries": len(builder.carries),
                     "n_instructions": info["n_instructions"], "n_live": info["n_live"],
                     "bytes_of_the_result": int(4 * height * width), "ms": ms,
                     "iterate_ns_per_row": round(1e6 * ms["iterate"]["median_ms"] / n, 4),
                     "walk_kernel_ns_per_row_and_instruction":
                         round(1e6 * kernels.get("k_iterate_walk", 0.0) / n / (info["n_instructions"] + len(builder.carries)), 4),
                     "iterate_over_copy": round(ms["iterate"]["median_ms"] / ms["copy"]["median_ms"], 2),
                     "host_over_iterate": round(ms["host"]["median_ms"] / ms["iterate"]["median_ms"], 1)}
        if name == "single":
            out[name]["iterate_over_derive"] = round(ms["iterate"]["median_ms"] / ms["derive"]["median_ms"], 2)
        if name == "cap":
            out[name]["max_group_rows"] = int(cap_rows)
            out[name]["work"] = int(cap_rows * list_length)
        del resident, result

    ctx.synchronize()
    waits = []
    for _ in range(200):
        t0 = time.perf_counter()
        ctx.synchronize()
        waits.append(1e3 * (time.perf_counter() - t0))
    doc = {"workload": f"the iterate form of ts_matrix_derive on 2^{LOG_N} resident rows of width 6, one context, legs "
                       f"alternated; per leg the median of {reps} repetitions, measured {REPEATS} times: median_ms is the "
                       f"median of the {REPEATS} medians, spread_ms their max - min (the host leg of the cap case: 2 "
                       f"repetitions per measurement)",
           "idle_synchronize_ms": round(med(waits), 4),
           "walk_at_the_work_limit_ms": out["cap"]["kernel_mean_ms"].get("k_iterate_walk"),
           "unmeasured": ["other heights and widths", "hardware counters of the kernels",
                          "row tiles staged in LDS instead of lanes streaming down rows a group apart"],
           "cases": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()} for k, v in out.items()}))
    print(json.dumps({k: v["kernel_mean_ms"] for k, v in out.items()}))


if __name__ == "__main__":
    main()
