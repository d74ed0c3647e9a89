"""What packed / Montgomery ingest is worth at the headline shape, in one process on one box:

    python tools/time_ingest.py [LOG_N [PROOFS_PER_LANE [OUT.json]]]     (default 20 6 profiles/ingest_headline.json)

A 2^LOG_N x 64 trace goes up from page-locked host memory inside the timed region on 4 lanes (one context and
one host thread each, a start gate of a quarter of one proof's solo time), every upload followed by its proof,
as bench.py's h2d_inclusive leg does.  The legs differ only in the form the SAME values cross the link in:

    (a) u32      canonical words through ts_matrix_upload_async: today's path, the yardstick
    (b) monty32  Montgomery words through ts_matrix_upload_packed_async
    (c) u16      every column 2 bytes
    (d) u8       every column 1 byte
    (e) mixed    16 x u32 + 16 x u16 + 32 x u8 in one row (128 bytes instead of 256)

and a device-resident leg (no upload) for the floor.  The values have to fit a byte, so the AIR is ByteMulAir-64
below: SynthMulAir's triples a * a * b = c with a < 4, b < 16 drawn per row -- the same constraint degree,
quotient degree and width as the headline's SynthMulAir-64, hence the same kernels and proof size.  All legs
prove the same trace, so every proof must have the same Blake3 digest: asserted.  ms per proof, GB/s of link
traffic and the box's clock and power over each leg go to OUT.json.

NOT measured here: the host's own canonical-to-Montgomery pass that leg (b) removes (a Plonky3 host's
`as_canonical_u32` map over the trace and its temporary) -- there is no such host in this repository."""
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import tapstark_amd as ts
from tapstark_amd.air import BaseAir
from tapstark_amd.airs import splitmix64_stream
from tapstark_amd.benchutil import GpuSamplerProcess

P = 0x78000001
W, LANES, CFG = 64, 4, (2, 28, 8)


class ByteMulAir(BaseAir):
    """21 triples (a, b, c) with a * a * b - c = 0 (degree 3, as SynthMulAir) and one free column."""

    def width(self) -> int:
        return W

    def eval(self, builder) -> None:
        local = builder.main().row_slice(0)
        for i in range(W // 3):
            a, b, c = local[3 * i], local[3 * i + 1], local[3 * i + 2]
            builder.assert_zero(a * a * b - c)


def byte_mul_trace(n: int) -> np.ndarray:
    rnd = splitmix64_stream(0x1291, n * W).reshape(n, W).astype(np.uint64)
    t = np.zeros((n, W), dtype=np.uint32)
    for i in range(W // 3):
        a, b = rnd[:, 3 * i] % 4, rnd[:, 3 * i + 1] % 16
        t[:, 3 * i], t[:, 3 * i + 1], t[:, 3 * i + 2] = a, b, a * a * b  # at most 9 * 15 = 135
    t[:, W - 1] = rnd[:, W - 1] % 256
    return t


def to_monty32(values: np.ndarray) -> np.ndarray:
    return ((values.astype(np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)  # values < 2^8


def main():
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    per_lane = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "ingest_headline.json")
    n = 1 << log_n
    trace = byte_mul_trace(n)
    assert int(trace.max()) < 256
    tape = ts.air_tape(ByteMulAir(), 0)
    ctxs = [ts.default_context()] + [ts.Context(0) for _ in range(LANES - 1)]
    lanes = [(c, ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*CFG), c)), ts.CompiledAir(c, tape)) for c in ctxs]
    assert ts.check_constraints(ByteMulAir(), trace[: 1 << 10], [], ctxs[0]) == -1

    legs = {
        "a_u32": (None, trace),
        "b_monty32": (ts.TraceFormat("monty32"), to_monty32(trace)),
        "c_u16": (ts.TraceFormat("u16"), trace),
        "d_u8": (ts.TraceFormat("u8"), trace),
        "e_mixed_16u32_16u16_32u8": (ts.TraceFormat(["u32"] * 16 + ["u16"] * 16 + ["u8"] * 32), trace),
    }

    gate = {"ms": 0.0, "last": -1e18, "lock": threading.Lock()}

    def start_gate():
        if gate["ms"] <= 0:
            return
        with gate["lock"]:
            while True:
                wait = gate["last"] + gate["ms"] * 1e-3 - time.perf_counter()
                if wait <= 0:
                    break
                time.sleep(min(wait, 2e-4))
            gate["last"] = time.perf_counter()

    def digest(proof) -> str:
        import hashlib
        return hashlib.blake2s(proof.words.tobytes(), digest_size=16).hexdigest()

    pool = ThreadPoolExecutor(max_workers=LANES)
    results, digests = {}, {}

    def run_leg(name, make):
        """make(lane) -> DeviceMatrix, called inside the timed region before every proof."""
        last = [None] * LANES

        def job(l):
            c, conf, air = lanes[l]
            for _ in range(per_lane):
                start_gate()
                last[l] = ts.prove(conf, air, ts.BfChallenger(), make(l), [])

        def sync():
            for c in ctxs:
                c.synchronize()

        gate["ms"] = 0.0
        list(pool.map(job, range(LANES)))  # warm-up: pool blocks, tables
        sync()
        c, conf, air = lanes[0]
        t0 = time.perf_counter()
        ts.prove(conf, air, ts.BfChallenger(), make(0), [])
        solo = 1e3 * (time.perf_counter() - t0)
        gate["ms"] = 0.25 * solo
        sampler = GpuSamplerProcess(0, 0.01)
        t0 = time.perf_counter()
        list(pool.map(job, range(LANES)))
        sync()
        t1 = time.perf_counter()
        sampler.stop()
        digests[name] = {digest(p) for p in last}
        steps = per_lane * LANES
        return {"ms_per_proof": round(1e3 * (t1 - t0) / steps, 4), "proofs": steps, "solo_ms": round(solo, 4),
                "start_gate_ms": round(gate["ms"], 4), "box": sampler.window(t0, t1)}

    resident = [ts.DeviceMatrix.upload(c, trace) for c in ctxs]
    r = run_leg("resident", lambda l: ts.DeviceMatrix.from_device_ptr(ctxs[l], resident[l].device_ptr(), n, W))
    r["note"] = "no upload: the trace is copied device to device before every proof (a proof consumes its trace)"
    results["resident"] = r
    for name, (fmt, words) in legs.items():
        if fmt is None:
            pins = [ts.PinnedHostMatrix(n, W) for _ in ctxs]
            for pin in pins:
                pin.array[:] = words
            nbytes = n * W * 4
            make = lambda l, pins=pins: ts.DeviceMatrix.upload_async(ctxs[l], pins[l])  # noqa: E731
        else:
            nbytes = fmt.nbytes(n, W)
            pins = [ts.PinnedHostBytes(nbytes) for _ in ctxs]
            fmt.pack(words, out=pins[0].array)
            for pin in pins[1:]:
                pin.array[:] = pins[0].array
            make = lambda l, pins=pins, fmt=fmt: ts.DeviceMatrix.upload_packed_async(ctxs[l], pins[l], fmt, n, W)  # noqa: E731
        r = run_leg(name, make)
        r["bytes_per_trace"] = nbytes
        r["link_GB_per_s"] = round(nbytes / (r["ms_per_proof"] * 1e-3) / 1e9, 2)
        results[name] = r
        del pins

    all_digests = set().union(*digests.values())
    assert len(all_digests) == 1, f"the legs did not prove the same thing: {digests}"
    out = {"workload": f"ByteMulAir-64 2^{log_n} x {W}, FRI {CFG}, {LANES} lanes, upload inside the timed region",
           "proof_digest_blake2s_all_legs": all_digests.pop(), "legs": results,
           "yardstick": "a_u32",
           "not_measured": "the host's canonical<->Montgomery pass that b_monty32 removes (no such host here)"}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
