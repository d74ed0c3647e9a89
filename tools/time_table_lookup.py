"""What a lookup against a FIXED table costs beside today's shape, in one process on one box:

    python tools/time_table_lookup.py [LOG_N [REPS [OUT.json]]]      (default 20 20 profiles/table_lookup.json)

2^LOG_N rows, FRI (log_blowup 2, 28 queries, 8 proof-of-work bits), for K = 2 (one lookup) and K = 8 (four lookups
against one table).  Per K:

    prove_pre_aux   ts_prove_pre_aux of the TableLookupAir shape: value and multiplicity columns in the main trace,
                    the table in a preprocessed key committed OUTSIDE the timed region, LogUp built with
                    ts_logup_aux_build_pre from a row-major device copy of the table
    prove_aux       the yardstick, from the same run: ts_prove_aux of the RangeLookupAir shape, the table as a main
                    column the prover fills in (and two constraints that make it the row index)
    build_pre, build   ts_logup_aux_build_pre and ts_logup_aux_build alone in a sustained loop (each call ends in
                    its own device synchronise), beside the bytes each must move

Solo proofs (one context, one proof at a time, the host clock around a call that ends synchronised), the two kinds
alternated so that both see the same box, median of REPS.  Traces are device-resident and copied device to device
before every proof (a proof consumes its trace).  One proof of each kind is verified outside the timed region.  No
ratio is fixed in advance; the figures are written as they come."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import tapstark_amd as ts
from tapstark_amd.air import BaseAir, LogUp, aux_dims
from tapstark_amd.airs import splitmix64_stream

P = 0x78000001
CFG = (2, 28, 8)


class MultiTableLookupAir(BaseAir):
    """L lookups against one table in the key: main columns value_0..value_{L-1}, mult_0..mult_{L-1}, one
    preprocessed column; 2 L interactions (+1, value_i), (mult_i, table).  L = 1 is TableLookupAir."""

    preprocessed_width = 1

    def __init__(self, lookups: int):
        self.L = lookups
        its = []
        for i in range(lookups):
            its += [(("const", 1), [("col", i)]), (("col", lookups + i), [("prep", 0)])]
        self.logup = LogUp(its)
        self.aux_width, self.n_challenges, self.n_exposed = self.logup.aux_width, 2, 4

    def width(self) -> int:
        return 2 * self.L

    def eval(self, builder) -> None:
        self.logup.eval(builder)


class MultiRangeLookupAir(BaseAir):
    """The same lookups with the table as a main column (tools/time_logup.py MultiLookupAir): columns
    value_0..value_{L-1}, table, mult_0..mult_{L-1}."""

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


def lookup_columns(n: int, lookups: int):
    """(values (n, L), multiplicities (n, L)) against the table 0 .. n-1."""
    values = np.empty((n, lookups), dtype=np.uint32)
    mults = np.empty((n, lookups), dtype=np.uint32)
    for i in range(lookups):
        v = (splitmix64_stream(11 + i, n) % np.uint64(n)).astype(np.int64)
        values[:, i] = v
        mults[:, i] = (P - np.bincount(v, minlength=n)) % P
    return values, mults


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
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "table_lookup.json")
    n = 1 << log_n
    ctx = ts.default_context()
    config = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), ctx))
    ch = (splitmix64_stream(5, 8) % np.uint64(P)).astype(np.uint32)
    table = np.arange(n, dtype=np.uint32).reshape(n, 1)
    legs = {}
    for lookups in (1, 4):
        tair, rair = MultiTableLookupAir(lookups), MultiRangeLookupAir(lookups)
        K, aw = 2 * lookups, tair.aux_width
        tc = ts.CompiledAir(ctx, ts.air_tape(tair, 0, 1, *aux_dims(tair)))
        rc = ts.CompiledAir(ctx, ts.air_tape(rair, 0, 0, *aux_dims(rair)))
        assert tc.max_constraint_degree == rc.max_constraint_degree == 3
        values, mults = lookup_columns(n, lookups)
        t_host = np.ascontiguousarray(np.hstack([values, mults]))
        r_host = np.ascontiguousarray(np.hstack([values, table, mults]))
        t_res, r_res = ts.DeviceMatrix.upload(ctx, t_host), ts.DeviceMatrix.upload(ctx, r_host)
        copy = lambda m, width: ts.DeviceMatrix.from_device_ptr(ctx, m.device_ptr(), n, width)
        key = ts.PreprocessedKey(config, table, keep_values=True)  # the commit: outside the timed region
        source = tair.logup.aux_source_with(key.values)
        # both builders give a sum of zero, and the same sum columns
        aux_t, S_t = tair.logup.build(t_res, ch, preprocessed=key.values)
        aux_r, S_r = rair.logup.build(r_res, ch)
        assert not S_t.any() and not S_r.any()
        del aux_t, aux_r
        build_pre_ms = timed(lambda: tair.logup.build(t_res, ch, preprocessed=key.values), reps, ctx.synchronize)
        build_ms = timed(lambda: rair.logup.build(r_res, ch), reps, ctx.synchronize)
        # every referenced column is read once, the aux matrix written and its sum column rewritten by the scan
        moved_pre, moved = 4 * n * (tair.width() + 1 + aw), 4 * n * (rair.width() + aw)
        prove_t = lambda: ts.prove(config, tc, ts.BfChallenger(), copy(t_res, tair.width()), [], preprocessed=key,
                                   aux=source)
        prove_r = lambda: ts.prove(config, rc, ts.BfChallenger(), copy(r_res, rair.width()), [],
                                   aux=rair.logup.aux_source)
        pt, pr = prove_t(), prove_r()
        tair.logup.verify(ts.verify(config, tc, ts.BfChallenger(), pt, [], preprocessed_root=key.root))
        rair.logup.verify(ts.verify(config, rc, ts.BfChallenger(), pr, []))
        ctx.synchronize()
        t_t, t_r = [], []
        for _ in range(reps):  # alternated: both see the same box
            t0 = time.perf_counter()
            prove_t()
            t1 = time.perf_counter()
            prove_r()
            t2 = time.perf_counter()
            t_t.append(1e3 * (t1 - t0))
            t_r.append(1e3 * (t2 - t1))
        med = lambda v: round(float(np.median(v)), 4)
        legs[f"K{K}"] = {
            "interactions": K, "main_width": tair.width(), "preprocessed_width": 1, "aux_width": aw,
            "yardstick_main_width": rair.width(),
            "prove_pre_aux_solo_ms": med(t_t), "prove_pre_aux_min_ms": round(min(t_t), 4),
            "yardstick": "ts_prove_aux, the table as a main column", "prove_aux_solo_ms": med(t_r),
            "prove_aux_min_ms": round(min(t_r), 4), "prove_pre_aux_over_prove_aux": round(med(t_t) / med(t_r), 4),
            "build_pre_ms": round(build_pre_ms, 4), "build_pre_bytes": moved_pre,
            "build_pre_GBps": round(moved_pre / build_pre_ms / 1e6, 2),
            "build_ms": round(build_ms, 4), "build_bytes": moved, "build_GBps": round(moved / build_ms / 1e6, 2),
            "proof_words": int(len(pt.words)), "yardstick_proof_words": int(len(pr.words)),
        }
        del t_res, r_res, key
    out = {"workload": f"TableLookupAir-shaped, 2^{log_n} rows, FRI {CFG}, one context, solo proofs alternated, "
                       f"median of {reps}",
           "legs": legs,
           "notes": "the key's commit (LDE and leaf hashing of the table) is outside the timed region; build_*_ms "
                    "include the call's own synchronise and its 32-byte copy back; *_bytes = 4 n (columns read + "
                    "aux width)"}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
