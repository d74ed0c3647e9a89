"""Times the standalone transforms against the project's own LDE, in one process:

    python tools/time_dft.py [LOG_N [WIDTH [REPS [OUT.json]]]]          (default 20 64 20, no file)

ts_dft_batch (forward, inverse, coset forward) and ts_coset_lde_batch (added_bits 1) on a resident
2^LOG_N x WIDTH matrix in a sustained loop, mean milliseconds per call from HIP events on the context's
stream, beside ts_bench_stage(stage 0, LOG_N, WIDTH, log_blowup 1) -- the coset LDE's three NTT passes without
its transposes.  That LDE does one inverse and two forward transforms of this size, so a forward DFT that
takes longer than it does more than three times its arithmetic.  A second loop with per-kernel events
gives the split.  Prints one JSON line and, if OUT.json is given, writes it there too (the other tools' output
directory on the GPU box is the place for it)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tapstark_amd as ts
from tapstark_amd.airs import splitmix64_stream

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
w = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ctx = ts.default_context()
dft = ts.Radix2Dft(ctx)
stream = torch.cuda.ExternalStream(ctx.stream)
dm = ts.DeviceMatrix.upload(ctx, splitmix64_stream(7, (1 << log_n) * w).reshape(1 << log_n, w))

calls = {
    "dft_batch": lambda: dft.dft_batch(dm),
    "idft_batch": lambda: dft.idft_batch(dm),
    "coset_dft_batch_shift31": lambda: dft.coset_dft_batch(dm, 31),
    "coset_lde_batch_bits1_shift31": lambda: dft.coset_lde_batch(dm, 1, 31),
    "coset_lde_batch_bits1_shift31_bit_reversed": lambda: dft.coset_lde_batch(dm, 1, 31, bit_reversed=True),
}


def timed(fn):
    fn()  # tables, first touch, pool blocks
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()  # the result goes back to the context's pool at once; the stream keeps the order
    e1.record(stream)
    ctx.synchronize()
    return e0.elapsed_time(e1) / reps


out = {"log_n": log_n, "width": w, "reps": reps, "ms_per_call": {k: round(timed(f), 4) for k, f in calls.items()}}
out["lde_stage0_log_blowup1_ms"] = round(ctx.bench_stage(0, log_n, w, 1, reps), 4)
out["dft_over_lde"] = round(out["ms_per_call"]["dft_batch"] / out["lde_stage0_log_blowup1_ms"], 3)
ctx.set_kernel_timing(True)
kernels = {}
for name in ("dft_batch", "idft_batch"):
    for _ in range(reps):
        calls[name]()
    kernels[name] = {k: round(ms / reps, 4) for k, (cnt, ms) in sorted(ctx.take_kernel_timings().items())}
ctx.set_kernel_timing(False)
out["kernel_ms_per_call"] = kernels
if len(sys.argv) > 4:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    json.dump(out, open(sys.argv[4], "w"), indent=1)
print(json.dumps(out))
