"""What filling a LogUp multiplicity column costs at a user's size, in one process on one box:

    python tools/time_logup_mult.py [LOG_N [REPS [OUT.json]]]      (default 20 20 profiles/logup_multiplicities.json)

ts_logup_multiplicities over 2^LOG_N resident rows, one context, the median of REPS calls, each timed by the host
clock around a call that ends in its own synchronise.  Legs:

    range_uniform, range_byte, range_all_equal
             one lookup of weight 1 against the range table 0 .. n-1 (RangeLookupAir's columns); the values are
             uniform over the table, byte-valued (256 distinct) or all equal: one add per destination, thousands, all
    xor4     four lookups of (a, b, a xor b) against the table of all pairs of two LOG_N/2-bit operands

Every leg comes with the per-kernel times of one more call and beside two yardsticks of the same run:

    aux_build   ts_logup_aux_build per call on the same trace: a pass over the same cells
    host        what a caller does without the call: download the value columns, count on the CPU (np.bincount; for
                xor4 a packed-key np.bincount, and once the dictionary join a general table needs), upload the column

The filled column is compared with the host's outside the timed regions.  No ratio is fixed in advance."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import tapstark_amd as ts
from tapstark_amd.air import LogUp
from tapstark_amd.airs import RangeLookupAir, splitmix64_stream

P = 0x78000001


def median_ms(f, reps):
    f()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        times.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(times)), 4), round(min(times), 4)


def device_leg(ctx, logup, table, resident, preprocessed, want_column, out_column, reps, ch):
    fill = lambda: logup.fill_multiplicities(resident, table, preprocessed=preprocessed)
    assert fill() == (0, 2 ** 64 - 1)
    assert (resident.download()[:, out_column] == want_column).all(), "the filled column is not the host's"
    med, best = median_ms(fill, reps)
    ctx.set_kernel_timing(True)
    fill()
    kernels = {k: round(ms, 4) for k, (count, ms) in ctx.take_kernel_timings().items() if k.startswith("k_mult")}
    ctx.set_kernel_timing(False)
    leg = {"fill_ms": med, "fill_min_ms": best, "kernels_ms": kernels}
    build = lambda: logup.build(resident, ch, preprocessed=preprocessed)
    leg["aux_build_ms"], leg["aux_build_min_ms"] = median_ms(build, reps)
    return leg


def main():
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "logup_multiplicities.json")
    n = 1 << log_n
    ctx = ts.default_context()
    ch = (splitmix64_stream(5, 8) % np.uint64(P)).astype(np.uint32)
    host_reps = max(3, reps // 4)
    legs = {}

    # ---- one lookup against the range table
    uniform = (splitmix64_stream(11, n) % np.uint64(n)).astype(np.int64)
    for name, values in (("range_uniform", uniform), ("range_byte", uniform % 256),
                         ("range_all_equal", np.full(n, 77 % n, dtype=np.int64))):
        want = ((P - np.bincount(values, minlength=n)) % P).astype(np.uint32)
        trace = np.zeros((n, 3), dtype=np.uint32)
        trace[:, 0], trace[:, 1] = values, np.arange(n)
        resident = ts.DeviceMatrix.upload(ctx, trace)
        leg = device_leg(ctx, RangeLookupAir.logup, 1, resident, None, want, 2, reps, ch)
        value_columns = ts.DeviceMatrix.upload(ctx, trace[:, :1])

        def host():
            v = value_columns.download()[:, 0]
            column = ((P - np.bincount(v, minlength=n)) % P).astype(np.uint32)
            ts.DeviceMatrix.upload(ctx, column.reshape(n, 1))
            ctx.synchronize()

        leg["host_download_bincount_upload_ms"], leg["host_min_ms"] = median_ms(host, host_reps)
        leg.update(lookups=1, n_values=1, distinct_destinations=int(len(np.unique(values))))
        legs[name] = leg
        del resident, value_columns

    # ---- four lookups of (a, b, a xor b): table columns 0 1 2, lookups 3 .. 14, the multiplicity column 15
    half = log_n // 2
    if 2 * half == log_n:
        t = np.arange(n, dtype=np.int64)
        trace = np.zeros((n, 16), dtype=np.uint32)
        trace[:, 0], trace[:, 1] = t >> half, t & ((1 << half) - 1)
        trace[:, 2] = trace[:, 0] ^ trace[:, 1]
        its = [(("col", 15), [("col", 0), ("col", 1), ("col", 2)])]
        counts = np.zeros(n, dtype=np.int64)
        for l in range(4):
            a = (splitmix64_stream(21 + l, n) % np.uint64(1 << half)).astype(np.int64)
            b = (splitmix64_stream(31 + l, n) % np.uint64(1 << half)).astype(np.int64)
            c = 3 + 3 * l
            trace[:, c], trace[:, c + 1], trace[:, c + 2] = a, b, a ^ b
            its.append((("const", 1), [("col", c), ("col", c + 1), ("col", c + 2)]))
            counts += np.bincount((a << half) | b, minlength=n)
        want = ((P - counts) % P).astype(np.uint32)
        logup = LogUp(its)
        resident = ts.DeviceMatrix.upload(ctx, trace)
        leg = device_leg(ctx, logup, 0, resident, None, want, 15, reps, ch)
        value_columns = ts.DeviceMatrix.upload(ctx, trace[:, 3:15])
        table_rows = [tuple(r) for r in trace[:, :3].tolist()]

        def host_packed():
            v = value_columns.download().astype(np.int64)
            got = np.zeros(n, dtype=np.int64)
            for l in range(4):  # (the third word is checked, not trusted: a xor b must be the table's)
                assert ((v[:, 3 * l] ^ v[:, 3 * l + 1]) == v[:, 3 * l + 2]).all()
                got += np.bincount((v[:, 3 * l] << half) | v[:, 3 * l + 1], minlength=n)
            ts.DeviceMatrix.upload(ctx, ((P - got) % P).astype(np.uint32).reshape(n, 1))
            ctx.synchronize()

        def host_dictionary():
            v = value_columns.download().tolist()
            row_of = {}
            for i, tup in enumerate(table_rows):
                row_of.setdefault(tup, i)
            got = [0] * n
            for row in v:
                for l in range(4):
                    got[row_of[(row[3 * l], row[3 * l + 1], row[3 * l + 2])]] += 1
            column = ((P - np.asarray(got, dtype=np.int64)) % P).astype(np.uint32)
            assert (column == want).all()
            ts.DeviceMatrix.upload(ctx, column.reshape(n, 1))
            ctx.synchronize()

        leg["host_download_packed_bincount_upload_ms"], leg["host_min_ms"] = median_ms(host_packed, host_reps)
        t0 = time.perf_counter()
        host_dictionary()
        leg["host_download_dictionary_join_upload_ms_one_run"] = round(1e3 * (time.perf_counter() - t0), 1)
        leg.update(lookups=4, n_values=3, distinct_destinations=int(np.count_nonzero(counts)))
        legs["xor4"] = leg

    out = {"workload": f"ts_logup_multiplicities, 2^{log_n} rows, one context, median of {reps} calls "
                       f"(host yardsticks: {host_reps})",
           "legs": legs,
           "notes": "fill_ms and aux_build_ms include the call's own synchronise and its 32-byte copy back; "
                    "kernels_ms are HIP event times of one further call; host times include the download of the "
                    "value columns and the upload of the one column"}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
