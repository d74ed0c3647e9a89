"""What deriving columns of a resident trace costs against its neighbours, in one process on one context:

    python tools/time_derive.py [REPS [OUT.json]]      (default 20 profiles/derive.json)

2^20 resident rows, four row programs:

    gap      airs.memory_gap_program: width 8, column 6 overwritten (20 nodes, two reads of the previous row)
    limbs    width 4 -> 6: one column split into a 16-bit and a 15-bit limb
    inv      width 4 -> 5: the field inverse of one column (41 Montgomery products per row)
    mixed    width 16 -> 18: 40 nodes of every kind over several columns and both neighbours, one column overwritten

Legs, alternated inside every repetition in an order drawn anew (seeded) for every repetition:

    derive   ts_matrix_derive
    copy     a device-to-device copy of a matrix of the OUTPUT's size (ts_matrix_from_device): the bytes a derive cannot
             avoid -- it reads the source once and writes the result once
    host     the host route, what a caller did before: download, the same nodes in numpy, upload

Median over REPS repetitions of the host clock around the call (the context synchronised before and after, so a wait of
the call's own would be inside; every device leg runs once untimed just before, so that the timed call starts on a busy
GPU whichever leg came before it); the whole measurement is repeated three times and every median is given with the
spread (max - min) of the three.  No ratio is fixed in advance: the figures are written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tapstark_amd as ts  # noqa: E402
from tapstark_amd import derive as dv  # noqa: E402
from tapstark_amd.airs import memory_gap_program  # noqa: E402

P = 0x78000001
LOG_N = 20
REPEATS = 3


def limbs_program():
    b = dv.DeriveBuilder(4)
    x = b.col(2)
    b.output(x.bits(0, 16), 4)
    b.output(x.bits(16, 15), 5)
    return b


def inv_program():
    b = dv.DeriveBuilder(4)
    b.output(b.col(1).inv(), 4)
    return b


def mixed_program():
    """40 nodes over width 16: two comparisons, an is-zero witness pair, a xor with a limb, selectors and neighbours"""
    b = dv.DeriveBuilder(16)
    a, c, d = b.col(0), b.col(5), b.next(9)
    diff = a - b.prev(0)
    nz = diff.inv() * diff                                  # 1 where the column changed
    b.output(nz, 16)
    lt = c.lt(d) * (1 - b.is_last_row()) + b.is_first_row() * 7
    x = (c.bits(0, 16) ^ d.bits(0, 16)) + (c.bits(16, 15) & d.bits(16, 15)) * 65536
    acc = lt * x + nz * (b.col(12) - b.row()) - (-b.col(15)) * b.col(3)
    b.output(acc + acc.is_zero(), 17)
    b.output(a + c * d, 2)
    assert len(b.nodes) == 40, len(b.nodes)
    return b


def numpy_nodes(tape, rows):
    """the program's outputs over host rows, one vectorised numpy expression per node: the host route's arithmetic"""
    t = [int(w) for w in tape]
    width, n_nodes, n_out = t[2], t[3], t[4]
    p, h = np.uint64(P), rows.shape[0]
    r = np.arange(h, dtype=np.uint64)
    v = []
    for i in range(n_nodes):
        op, a, b = t[5 + 3 * i: 8 + 3 * i]
        if op == dv.CONST:
            x = np.full(h, a, dtype=np.uint64)
        elif op == dv.COL:
            col = rows[:, b].astype(np.uint64) % p
            x = col if a == 0 else np.roll(col, -1 if a == 1 else 1)
        elif op == dv.IS_FIRST_ROW:
            x = (r == 0).astype(np.uint64)
        elif op == dv.IS_LAST_ROW:
            x = (r == h - 1).astype(np.uint64)
        elif op == dv.IS_TRANSITION:
            x = (r != h - 1).astype(np.uint64)
        elif op == dv.ROW:
            x = r
        elif op == dv.ADD:
            x = (v[a] + v[b]) % p
        elif op == dv.SUB:
            x = (v[a] + p - v[b]) % p
        elif op == dv.NEG:
            x = (p - v[a]) % p
        elif op == dv.MUL:
            x = v[a] * v[b] % p
        elif op == dv.INV:
            x, base, e = np.ones(h, dtype=np.uint64), v[a], P - 2
            while e:
                if e & 1:
                    x = x * base % p
                base = base * base % p
                e >>= 1
            x = np.where(v[a] == 0, np.uint64(0), x)
        elif op == dv.IS_ZERO:
            x = (v[a] == 0).astype(np.uint64)
        elif op == dv.LT:
            x = (v[a] < v[b]).astype(np.uint64)
        elif op == dv.BITS:
            x = (v[a] >> np.uint64(b & 255)) & np.uint64((1 << (b >> 8)) - 1)
        elif op == dv.AND:
            x = (v[a] & v[b]) % p
        elif op == dv.XOR:
            x = (v[a] ^ v[b]) % p
        else:
            raise KeyError(op)
        v.append(x)
    outs = [tuple(t[5 + 3 * n_nodes + 2 * k: 7 + 3 * n_nodes + 2 * k]) for k in range(n_out)]
    out = np.zeros((h, max([width] + [d + 1 for _, d in outs])), dtype=np.uint32)
    out[:, :width] = rows
    for n, d in outs:
        out[:, d] = v[n].astype(np.uint32)
    return out


def host_route(ctx, resident, tape):
    return ts.DeviceMatrix.upload(ctx, numpy_nodes(tape, resident.download()))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "derive.json")
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
    for name, builder in (("gap", memory_gap_program()), ("limbs", limbs_program()), ("inv", inv_program()),
                          ("mixed", mixed_program())):
        tape = builder.tape()
        width = builder.src_width
        info = dv.derive_check(tape, width)
        r = np.random.default_rng(1234)
        host = r.integers(0, P, size=(n, width), dtype=np.uint32)
        if name == "gap":  # a table-like matrix: boolean live and start columns
            host[:, 4] = 1
            host[:, 7] = r.integers(0, 2, n, dtype=np.uint32)
        resident = ts.DeviceMatrix.upload(ctx, host)
        derived = resident.derive(tape)
        out_width = info["out_width"]

        legs = {
            "derive": lambda: timed(lambda: resident.derive(tape)),
            "copy": lambda: timed(lambda: ts.DeviceMatrix.from_device_ptr(ctx, derived.device_ptr(), n, out_width)),
            "host": lambda: timed(lambda: host_route(ctx, resident, tape), warm=False),
        }
        # warm-up, and the equality the comparison rests on
        want = legs["host"]()[1].download()
        assert (legs["derive"]()[1].download() == want).all(), name
        assert (legs["copy"]()[1].download() == want).all()
        out[name] = {"rows_log2": LOG_N, "src_width": width, **info,
                     "bytes_read_and_written": int(4 * n * (width + out_width)), "ms": measure(legs)}
        del resident, derived

    doc = {"workload": f"ts_matrix_derive on a resident 2^{LOG_N}-row matrix, one context, legs alternated; per leg the "
                       f"median of {reps} repetitions, measured {REPEATS} times: median_ms is the median of the "
                       f"{REPEATS} medians, spread_ms their max - min",
           "cases": out}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {leg: (m["median_ms"], m["spread_ms"]) for leg, m in v["ms"].items()} for k, v in out.items()}))


if __name__ == "__main__":
    main()
