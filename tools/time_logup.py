"""What the challenge phase costs at a user's size, in one process on one box:

    python tools/time_logup.py [LOG_N [REPS [OUT.json]]]      (default 20 20 profiles/logup_aux.json)

RangeLookupAir-shaped work over 2^LOG_N rows, FRI (log_blowup 2, 28 queries, 8 proof-of-work bits), for K = 2
(one lookup: value, table, multiplicity) and K = 8 (four lookups against one table: four value columns, the table,
four multiplicity columns).  Per K:

    build    ts_logup_aux_build alone in a sustained loop (each call ends in its own device synchronise), beside
             the bytes it must move: the referenced trace columns read, the aux matrix written
    lde, hash   the coset LDE and the Merkle hashing of a matrix of the aux matrix's shape alone (ts_bench_stage 0
             and 1), the two stages the same proof spends on the aux matrix after it is built
    prove_aux   ts_prove_aux, solo: one context, one proof at a time, the host clock around a call that ends
             synchronised -- the lanes-free solo timing of the headline
    prove    ts_prove of SynthMulAir over as many columns as main + aux together (constraint degree 3, as LogUp's):
             the yardstick, timed the same way and alternated with prove_aux

Traces are device-resident and copied device to device before every proof (a proof consumes its trace).  One proof
of each kind is verified outside the timed region.  No ratio is fixed in advance; the figures are written as
they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import tapstark_amd as ts
from tapstark_amd.air import BaseAir, LogUp, aux_dims
from tapstark_amd.airs import SynthMulAir, splitmix64_stream

P = 0x78000001
CFG = (2, 28, 8)


class MultiLookupAir(BaseAir):
    """L lookups against one table: columns value_0..value_{L-1}, table, mult_0..mult_{L-1}; 2 L interactions
    (+1, value_i), (mult_i, table).  L = 1 is RangeLookupAir but for the column order."""

    def __init__(self, lookups: int):
        self.L = lookups
        its = []
        for i in range(lookups):
            its += [(("const", 1), [("col", i)]), (("col", lookups + 1 + i), [("col", lookups)])]
        self.logup = LogUp(its)
        self.aux_width, self.n_challenges, self.n_exposed = self.logup.aux_width, 2, 4

    def width(self) -> int:
        return 2 * self.L + 1

    def eval(self, builder) -> None:
        local, nxt = builder.main().row_slice(0), builder.main().row_slice(1)
        builder.when_first_row().assert_zero(local[self.L])
        builder.when_transition().assert_eq(nxt[self.L], local[self.L] + 1)
        self.logup.eval(builder)


def lookup_trace(n: int, lookups: int) -> np.ndarray:
    out = np.empty((n, 2 * lookups + 1), dtype=np.uint32)
    out[:, lookups] = np.arange(n)
    for i in range(lookups):
        values = (splitmix64_stream(11 + i, n) % np.uint64(n)).astype(np.int64)
        out[:, i] = values
        out[:, lookups + 1 + i] = (P - np.bincount(values, minlength=n)) % P
    return out


def timed(f, reps, sync):
    f()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    sync()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "logup_aux.json")
    n = 1 << log_n
    ctx = ts.default_context()
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), ctx))
    ch = (splitmix64_stream(5, 8) % np.uint64(P)).astype(np.uint32)
    legs = {}
    for lookups in (1, 4):
        air = MultiLookupAir(lookups)
        K, w, aw = 2 * lookups, air.width(), air.aux_width
        cair = ts.CompiledAir(ctx, ts.air_tape(air, 0, 0, *aux_dims(air)))
        host = lookup_trace(n, lookups)
        resident = ts.DeviceMatrix.upload(ctx, host)
        copy = lambda m, width: ts.DeviceMatrix.from_device_ptr(ctx, m.device_ptr(), n, width)
        aux, S = air.logup.build(resident, ch)
        assert not S.any()
        k = min(n, 1 << 12)
        small = lookup_trace(k, lookups)
        a_small, s_small = air.logup.build(ts.DeviceMatrix.upload(ctx, small), ch)
        assert ts.check_constraints(cair, small, [], ctx, aux=a_small, challenges=ch, exposed=s_small) == -1
        del aux, a_small
        build_ms = timed(lambda: air.logup.build(resident, ch), reps, ctx.synchronize)
        moved = 4 * n * (w + aw)  # every trace column is referenced; the aux matrix is written once more by the scan
        lde_ms = ctx.bench_stage(0, log_n, aw, CFG[0], reps)
        hash_ms = ctx.bench_stage(1, log_n, aw, CFG[0], reps)
        # the yardstick: the same total column count, constraint degree 3
        yw = w + aw
        yair = ts.CompiledAir(ctx, ts.air_tape(SynthMulAir(yw), 0))
        assert yair.max_constraint_degree == cair.max_constraint_degree == 3
        ytrace = ts.DeviceMatrix.synth_mul(ctx, n, yw)
        prove_aux = lambda: ts.prove(config, cair, ts.BfChallenger(), copy(resident, w), [], aux=air.logup.aux_source)
        prove = lambda: ts.prove(config, yair, ts.BfChallenger(), copy(ytrace, yw), [])
        pa, py = prove_aux(), prove()
        air.logup.verify(ts.verify(config, cair, ts.BfChallenger(), pa, []))
        ts.verify(config, yair, ts.BfChallenger(), py, [])
        ctx.synchronize()
        t_aux, t_y = [], []
        for _ in range(reps):  # alternated: both see the same box
            t0 = time.perf_counter()
            prove_aux()
            t1 = time.perf_counter()
            prove()
            t2 = time.perf_counter()
            t_aux.append(1e3 * (t1 - t0))
            t_y.append(1e3 * (t2 - t1))
        med = lambda v: round(float(np.median(v)), 4)
        legs[f"K{K}"] = {
            "interactions": K, "main_width": w, "aux_width": aw,
            "build_ms": round(build_ms, 4), "build_bytes": moved,
            "build_GBps": round(moved / build_ms / 1e6, 2),
            "aux_lde_ms": round(lde_ms, 4), "aux_hash_ms": round(hash_ms, 4),
            "prove_aux_solo_ms": med(t_aux), "prove_aux_min_ms": round(min(t_aux), 4),
            "yardstick": f"ts_prove of SynthMulAir({yw})", "prove_solo_ms": med(t_y),
            "prove_min_ms": round(min(t_y), 4), "prove_aux_over_prove": round(med(t_aux) / med(t_y), 4),
            "proof_words": int(len(pa.words)), "yardstick_proof_words": int(len(py.words)),
        }
        del resident, ytrace
    out = {"workload": f"RangeLookupAir-shaped, 2^{log_n} rows, FRI {CFG}, one context, solo proofs, {reps} repetitions",
           "legs": legs,
           "notes": "build_ms includes the call's own synchronise and its 32-byte copy back; build_bytes = 4 n "
                    "(main width + aux width)"}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
