"""Segmented specialisation of the quotient kernel (ts_air_compile_opts, ts_air_segment_plan) on the CPU:
the plan's invariants, a numpy run of the program segment by segment through a slab (tests/_air_segment.py)
against the unsegmented run, the segment kernels' resources through hiprtc for gfx950 (no GPU needed), and
the option refusals.  The reference's counterpart is the monomorphised `Air::eval` inside quotient_values
(uni-stark/src/prover.rs:170-181); the GPU half is tests/test_gpu_air_segment.py."""
import ctypes as C
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd import _lib
from tapstark_amd.airs import RandomAir, SynthExtAir, SynthMulAir, random_air_case, splitmix64_stream
from _air_program import run_program
from _air_segment import COMPUTED, max_live_across_cut, run_segmented, ssa

TS_ERR_INVALID = 1
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _cases():
    yield "SynthMulAir-64", ts.air_tape(SynthMulAir(64), 0), 0
    yield "SynthExt-163", ts.air_tape(SynthExtAir(163), 0), 0
    for seed in range(50):
        air, _ = random_air_case(seed)
        yield f"random-{seed}", ts.air_tape(air, air.n_public), air.n_public


CASES = list(_cases())


def _inputs(seed, w, n_public, m=5):
    vals = splitmix64_stream(seed + 31, 2 * m * w + 3 * m + max(n_public, 1))
    local = vals[:m * w].reshape(m, w).copy()
    nxt = vals[m * w:2 * m * w].reshape(m, w).copy()
    sels = vals[2 * m * w:2 * m * w + 3 * m].reshape(m, 3).copy()
    local[0, :] = 0
    nxt[1, :] = 0x78000000
    sels[0] = (1, 0, 1)
    return local, nxt, sels, vals[-max(n_public, 1):][:n_public]


def _plan(tape, S):
    cair = ts.CompiledAir(None, tape, segment_instr=S)
    prog = cair.program()
    if len(prog["code"]) <= S:  # the monolithic route: no plan
        with pytest.raises(_lib.TsError) as e:
            cair.segment_plan()
        assert e.value.code == TS_ERR_INVALID
        return cair, prog, None
    return cair, prog, cair.segment_plan()


@pytest.mark.parametrize("S", [8, 64, 1024])
def test_plan_invariants(S):
    n_planned = 0
    for name, tape, _ in CASES:
        _, prog, plan = _plan(tape, S)
        if plan is None:
            continue
        n_planned += 1
        code = prog["code"]
        n = len(code)
        opdefs, last_use = ssa(prog)
        segs = plan["segments"]
        # the segments tile the program, each within S instructions
        assert segs[0]["begin"] == 0 and segs[-1]["end"] == n, name
        for a, b in zip(segs, segs[1:]):
            assert a["end"] == b["begin"], name
        assert all(0 < sg["end"] - sg["begin"] <= S for sg in segs), name
        stored = {}
        for k, sg in enumerate(segs):
            b, e = sg["begin"], sg["end"]
            ins, outs = dict(sg["live_in"]), dict(sg["live_out"])
            # no leaf is slotted
            assert all(code[v][0] in COMPUTED for v in list(ins) + list(outs)), name
            # exactly the computed values from earlier segments used here, and those defined here used later
            want_in = {v for pc in range(b, e) for v in opdefs[pc] if v < b and code[v][0] in COMPUTED}
            want_out = {v for v in range(b, e) if code[v][0] in COMPUTED and last_use[v] >= e}
            assert set(ins) == want_in and set(outs) == want_out, (name, k)
            # every live-in was a live-out of an earlier segment, in the same slot
            for v, slot in ins.items():
                assert stored.get(v) == slot, (name, k, v)
            stored.update(outs)
            assert all(s < plan["slab_width"] for s in list(ins.values()) + list(outs.values())), name
        # the slab is as wide as the most values live across one cut, not the sum over cuts
        assert plan["slab_width"] == max_live_across_cut(prog, [sg["begin"] for sg in segs[1:]]), name
    assert n_planned >= (40 if S < 64 else 2)


@pytest.mark.parametrize("S", [8, 64, 1024])
def test_segmented_run_matches_program(S):
    for i, (name, tape, n_public) in enumerate(CASES):
        _, prog, plan = _plan(tape, S)
        if plan is None:
            continue
        local, nxt, sels, pis = _inputs(i, int(tape[2]), n_public)
        want = run_program(prog, local, nxt, pis, sels, int(tape[5]))
        got = run_segmented(prog, plan, local, nxt, pis, sels, int(tape[5]))
        assert (got == want).all(), f"{name} S={S}: segmented values differ"


def test_defaults_keep_todays_source():
    """segment_instr = 0, or a program of at most S instructions, is ts_air_compile: same source, no plan."""
    for name, tape, _ in CASES[:6]:
        base = ts.CompiledAir(None, tape)
        src = base.jit_source()
        assert "k_quotient_jit" in src and "k_quotient_seg" not in src
        assert ts.CompiledAir(None, tape, segment_instr=0).jit_source() == src, name
        assert ts.CompiledAir(None, tape, jit_jobs=3).jit_source() == src, name
        big = ts.CompiledAir(None, tape, segment_instr=len(base.program()["code"]))
        assert big.jit_source() == src, name
        with pytest.raises(_lib.TsError):
            big.segment_plan()
    seg = ts.CompiledAir(None, CASES[1][1], segment_instr=64)
    src = seg.jit_source()
    K = len(seg.segment_plan()["segments"])
    assert K > 1 and "k_quotient_jit" not in src
    assert all(f"k_quotient_seg{k}(" in src for k in range(K)) and f"k_quotient_seg{K}(" not in src


def _compile_opts(tape, **fields):
    l = _lib.lib()
    opt = _lib.AirOptionsC(C.sizeof(_lib.AirOptionsC), 64, 0, 0)
    for k, v in fields.items():
        setattr(opt, k, v)
    t = np.ascontiguousarray(tape, dtype=np.uint32)
    h = C.c_void_p()
    rc = l.ts_air_compile_opts(None, t.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(len(t)), C.byref(opt),
                               C.byref(h))
    if h.value:
        l.ts_air_free(None, h)
    return rc


def test_option_refusals():
    tape = CASES[1][1]
    assert _compile_opts(tape) == 0
    assert _compile_opts(tape, struct_size=C.sizeof(_lib.AirOptionsC) + 4) == TS_ERR_INVALID
    assert _compile_opts(tape, struct_size=0) == TS_ERR_INVALID
    assert _compile_opts(tape, reserved=1) == TS_ERR_INVALID
    assert _compile_opts(tape, jit_jobs=100) == 0  # clamped to 8
    l = _lib.lib()
    size = C.c_size_t()
    assert l.ts_air_segment_plan(None, None, 0, C.byref(size)) == TS_ERR_INVALID
    # the cap: 2^20 lowered instructions (a chain of additions over one column)
    n_nodes = (1 << 20) + 8
    nodes = np.zeros((n_nodes, 3), dtype=np.uint32)
    nodes[0] = (1, 0, 0)  # MAIN(local, column 0)
    nodes[1:, 0] = 6       # ADD(previous, node 0)
    nodes[1:, 1] = np.arange(n_nodes - 1, dtype=np.uint32)
    big = np.concatenate([np.array([0x54415354, 1, 1, 0, n_nodes, 1], dtype=np.uint32), nodes.ravel(),
                          np.array([n_nodes - 1], dtype=np.uint32)])
    assert _compile_opts(big, segment_instr=1024) == TS_ERR_INVALID
    assert _compile_opts(big, segment_instr=0) == 0  # the default route has no such cap (interpreter)


def _notes(code: bytes) -> list[dict]:
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code)
        f.flush()
        out = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    kernels = []
    for block in re.split(r"\n\s*- \.agpr_count:", out)[1:]:
        rec = {"name": re.search(r"\.name:\s+(\S+)", block).group(1)}
        for key in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count"):
            rec[key] = int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
        kernels.append(rec)
    return kernels


def _hiprtc_available() -> bool:
    try:
        C.CDLL("libhiprtc.so")
        return True
    except OSError:
        try:
            C.CDLL("/opt/rocm/lib/libhiprtc.so")
            return True
        except OSError:
            return False


@pytest.mark.parametrize("constraints", [1000, 6000])
def test_segment_kernels_do_not_spill(constraints):
    """200 columns x 1000 constraints (4.6k instructions) and x 6000 (37k: above TS_JIT_MAX_INSTR, which the
    monolithic kernel never compiles) at S = 1024: every kernel has no scratch, no spilled VGPR and at most 128
    VGPRs (4 waves per SIMD)."""
    if not _hiprtc_available() or not shutil.which(READELF):
        pytest.skip("hiprtc / llvm-readelf not available")
    air = RandomAir(4242, 200, constraints, 5, n_public=4, share_pct=35 if constraints == 1000 else 20, max_depth=7)
    cair = ts.CompiledAir(None, ts.air_tape(air, 4), segment_instr=1024)
    n_instr = len(cair.program()["code"])
    assert constraints == 1000 or n_instr > 32768
    K = len(cair.segment_plan()["segments"])
    code, _ = cair.jit_compile("gfx950")
    kernels = _notes(code)
    assert sorted(k["name"] for k in kernels) == sorted(f"k_quotient_seg{k}" for k in range(K))
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
        assert k["vgpr_count"] <= 128, k
