"""Python binding of the host-side mirror of the reference's prover interface.

The prover itself (orchestration, transcript, kernels) is C++/HIP behind the C ABI
(include/tapstark.h); this module only gives it the reference's names so that tests and benches
read like the reference's own:

* ``FriConfig``            -- reference fri/src/config.rs:11-16
* ``TwoAdicFriPcs``        -- reference fri/src/two_adic_pcs.rs:38-61 (commit/open on the device)
* ``StarkConfig``          -- reference uni-stark/src/config.rs:64-101
* ``BfChallenger``         -- reference basic/src/challenger/mod.rs:67-137
* ``prove``                -- reference uni-stark/src/prover.rs:25-35
* ``Proof``                -- reference uni-stark/src/proof.rs:17-37 + fri/src/proof.rs:13-33
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, fields as dataclass_fields

import numpy as np

from . import _lib
from .air import BaseAir, air_tape, aux_dims

P = 0x78000001
TSPF_MAGIC = 0x46505354


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def _p(a: np.ndarray):
    return a.ctypes.data_as(_lib.u32p)


class Context:
    """One per GPU (``ts_ctx``)."""

    def __init__(self, device: int = 0):
        self._l = _lib.lib()
        h = C.c_void_p()
        rc = self._l.ts_ctx_create(device, C.byref(h))
        if rc:
            raise _lib.TsError(rc, (self._l.ts_last_error(None) or b"").decode())
        self.h = h
        self.device = device

    def check(self, rc: int):
        if rc:
            raise _lib.TsError(rc, (self._l.ts_last_error(self.h) or b"").decode())

    def synchronize(self):
        self.check(self._l.ts_ctx_synchronize(self.h))

    @property
    def stream(self) -> int:
        return int(self._l.ts_ctx_stream(self.h) or 0)

    def alu_ceiling(self, kind: int) -> float:
        """Whole-chip NTT butterflies/s (kind 0) or Blake3 compressions/s (kind 1), no memory traffic."""
        r = C.c_double()
        self.check(self._l.ts_bench_alu(self.h, kind, C.byref(r)))
        return float(r.value)

    def bench_stage(self, stage: int, log_n: int, width: int, log_blowup: int, reps: int) -> float:
        """Mean ms of one repetition of a stage on resident data: 0 = coset LDE, 1 = Merkle hashing."""
        r = C.c_double()
        self.check(self._l.ts_bench_stage(self.h, stage, log_n, width, log_blowup, reps, C.byref(r)))
        return float(r.value)

    def set_timing(self, enabled: bool):
        self.check(self._l.ts_ctx_set_timing(self.h, int(enabled)))

    def take_timings(self) -> list[tuple[str, float]]:
        buf = C.create_string_buffer(1 << 16)
        self.check(self._l.ts_ctx_take_timings(self.h, buf, len(buf)))
        out = []
        for item in buf.value.decode().split(";"):
            if item:
                k, v = item.rsplit("=", 1)
                out.append((k, float(v)))
        return out

    def set_replay(self, mode: int):
        """``ts_ctx_set_replay`` (measurement aid: 1 record, 2 replay without the mid-proof syncs, 0 off)."""
        self.check(self._l.ts_ctx_set_replay(self.h, int(mode)))

    def set_kernel_timing(self, enabled: bool):
        self.check(self._l.ts_ctx_set_kernel_timing(self.h, int(enabled)))

    def take_kernel_timings(self) -> dict[str, tuple[int, float]]:
        """kernel name -> (launches, total ms), from HIP events on the context's stream."""
        buf = C.create_string_buffer(1 << 16)
        self.check(self._l.ts_ctx_take_kernel_timings(self.h, buf, len(buf)))
        out = {}
        for item in buf.value.decode().split(";"):
            if item:
                k, v = item.rsplit("=", 1)
                cnt, ms = v.split(":")
                out[k] = (int(cnt), float(ms))
        return out

    def graph_stats(self) -> dict:
        """``ts_ctx_graph_stats``: ``pool_bytes`` = bytes the device pool holds.  The other four counted
        the retired hipGraph replay of the FRI commit phase and are always 0."""
        out = (C.c_uint64 * 4)()
        self.check(self._l.ts_ctx_graph_stats(self.h, out))
        return {"replays": int(out[0]), "fallbacks": int(out[1]), "shapes": int(out[2]),
                "pool_bytes": int(out[3]), "reserve_failures": self.stat(4)}

    def stat(self, which: int) -> int:
        """``ts_ctx_stat``: 3 pool bytes, 5 local-quotient fall-backs, 6-8 proof-of-work witness counters,
        9 device blocks filled with the test pattern of ``TS_POOL_POISON`` (0 when it was unset at creation);
        11 pool blocks handed out and not yet given back; 0, 1, 2 and 4 (the retired graph replay's counters) are
        always 0; 10 is not used."""
        v = C.c_uint64()
        self.check(self._l.ts_ctx_stat(self.h, which, C.byref(v)))
        return int(v.value)

    def close(self):
        if self.h:
            self._l.ts_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class PinnedHostMatrix:
    """A row-major u32 matrix in page-locked host memory (``ts_host_alloc``), as a numpy view."""

    def __init__(self, height: int, width: int):
        self.shape = (height, width)
        p = C.c_void_p()
        rc = _lib.lib().ts_host_alloc(height * width * 4, C.byref(p))
        if rc:
            raise _lib.TsError(rc, "ts_host_alloc")
        self.ptr = p
        self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(height, width))

    def __del__(self):
        try:
            if self.ptr:
                _lib.lib().ts_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


class PinnedHostBytes:
    """``nbytes`` of page-locked host memory (``ts_host_alloc``; 16-byte aligned) as a numpy uint8 view: where a
    packed trace (``TraceFormat``) is assembled for ``DeviceMatrix.upload_packed_async``."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        rc = _lib.lib().ts_host_alloc(nbytes, C.byref(p))
        if rc:
            raise _lib.TsError(rc, "ts_host_alloc")
        self.ptr = p
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def __del__(self):
        try:
            if self.ptr:
                _lib.lib().ts_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


class TraceFormat:
    """``ts_trace_format``: how a host holds a trace -- per column ``"u32"`` (canonical word), ``"u16"`` / ``"u8"``
    (unsigned, zero-extended), ``"monty32"`` / ``"monty31"`` (word x stands for x * 2^-32 / x * 2^-31 mod p) -- in
    ``"rows"`` (columns packed back to back, rows ``row_stride`` bytes apart, 0 = tight) or ``"planar"`` (whole
    columns, each starting at the next multiple of 16 bytes).  ``kinds``: one kind for every column, or one per
    column."""

    KINDS = {"u32": 0, "u16": 1, "u8": 2, "monty32": 3, "monty31": 4}
    SIZES = {0: 4, 1: 2, 2: 1, 3: 4, 4: 4}
    LAYOUTS = {"rows": 0, "planar": 1}

    def __init__(self, kinds, layout: str = "rows", row_stride: int = 0):
        if isinstance(kinds, (str, int)):
            kinds = [kinds]
        self.kinds = np.array([self.KINDS[k] if isinstance(k, str) else int(k) for k in kinds], dtype=np.uint8)
        self.layout = self.LAYOUTS[layout] if isinstance(layout, str) else int(layout)
        self.row_stride = int(row_stride)

    def _c(self) -> "_lib.TraceFormatC":
        return _lib.TraceFormatC(C.sizeof(_lib.TraceFormatC), self.layout, self.row_stride, len(self.kinds), 0,
                                 self.kinds.ctypes.data_as(C.POINTER(C.c_uint8)))

    def nbytes(self, height: int, width: int) -> int:
        """``ts_trace_format_bytes``: the size of a height x width trace in this format (raises for a format the
        library refuses)."""
        l, fmt, n = _lib.lib(), self._c(), C.c_uint64()
        rc = l.ts_trace_format_bytes(C.byref(fmt), height, width, C.byref(n))
        if rc:
            raise _lib.TsError(rc, (l.ts_last_error(None) or b"").decode())
        return int(n.value)

    def pack(self, values, out: np.ndarray | None = None) -> np.ndarray:
        """Encodes an (h, w) array of column words into this format (numpy, for tests and examples): a uint8
        array of ``nbytes(h, w)``, or ``out`` filled.  A word must fit its column; Montgomery words go in as
        they are."""
        values = _u32(values)
        h, w = values.shape
        kinds = np.broadcast_to(self.kinds, (w,)) if len(self.kinds) == 1 else self.kinds
        sizes = [self.SIZES[int(k)] for k in kinds]
        total = self.nbytes(h, w)
        if out is None:  # 16-byte aligned, as the upload calls ask
            raw = np.zeros(total + 15, dtype=np.uint8)
            out = raw[(-raw.ctypes.data) % 16:][:total]
        assert out.dtype == np.uint8 and out.shape == (total,)
        le = values.astype("<u4").view(np.uint8).reshape(h, w, 4)  # little-endian bytes of every word
        off = 0
        stride = self.row_stride or sum(sizes)
        rows = out.reshape(h, stride) if self.layout == 0 else None
        for c, s in enumerate(sizes):
            assert s == 4 or int(values[:, c].max()) < (1 << (8 * s)), f"column {c} does not fit {s} byte(s)"
            if self.layout == 0:
                rows[:, off:off + s] = le[:, c, :s]
                off += s
            else:
                off = (off + 15) & ~15
                out[off:off + h * s] = le[:, c, :s].reshape(-1)
                off += h * s
        assert (off if self.layout else h * stride) == total
        return out


def _byte_ptr(buf):
    """(pointer, keep-alive) of a packed host buffer: ``PinnedHostBytes`` or a contiguous uint8 array."""
    if isinstance(buf, PinnedHostBytes):
        return buf.ptr, buf
    a = np.ascontiguousarray(buf, dtype=np.uint8)
    return C.c_void_p(a.ctypes.data), a


class DeviceMatrix:
    """``RowMajorMatrix<Val>`` resident in HBM (``ts_matrix``)."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self.h = handle

    @classmethod
    def upload(cls, ctx: Context, values) -> "DeviceMatrix":
        values = _u32(values)
        assert values.ndim == 2
        h = C.c_void_p()
        ctx.check(ctx._l.ts_matrix_upload(ctx.h, _p(values), values.shape[0], values.shape[1],
                                          C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def upload_async(cls, ctx: Context, pinned: "PinnedHostMatrix") -> "DeviceMatrix":
        """H2D from page-locked memory without waiting (``ts_matrix_upload_async``)."""
        h = C.c_void_p()
        ctx.check(ctx._l.ts_matrix_upload_async(ctx.h, pinned.ptr, pinned.shape[0], pinned.shape[1], C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_device_ptr(cls, ctx: Context, ptr: int, height: int, width: int) -> "DeviceMatrix":
        h = C.c_void_p()
        ctx.check(ctx._l.ts_matrix_from_device(ctx.h, C.c_void_p(ptr), height, width, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def _packed(cls, fn, ctx: Context, ptr, fmt: TraceFormat, height: int, width: int) -> "DeviceMatrix":
        h, f = C.c_void_p(), fmt._c()
        ctx.check(fn(ctx.h, ptr, C.byref(f), height, width, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def upload_packed(cls, ctx: Context, buf, fmt: TraceFormat, height: int, width: int) -> "DeviceMatrix":
        """``ts_matrix_upload_packed``: a trace held in ``fmt`` (a uint8 array or ``PinnedHostBytes`` of
        ``fmt.nbytes(height, width)``, 16-byte aligned) is copied as it is and widened / reduced on the device."""
        ptr, keep = _byte_ptr(buf)
        return cls._packed(ctx._l.ts_matrix_upload_packed, ctx, ptr, fmt, height, width)

    @classmethod
    def upload_packed_async(cls, ctx: Context, pinned: PinnedHostBytes, fmt: TraceFormat, height: int,
                            width: int) -> "DeviceMatrix":
        """The same without waiting (``ts_matrix_upload_packed_async``): ``pinned`` stays untouched until the next
        synchronisation of ``ctx``."""
        return cls._packed(ctx._l.ts_matrix_upload_packed_async, ctx, pinned.ptr, fmt, height, width)

    @classmethod
    def from_device_packed(cls, ctx: Context, ptr: int, fmt: TraceFormat, height: int, width: int) -> "DeviceMatrix":
        """``ts_matrix_from_device_packed``: ``ptr`` is a device pointer (a torch uint8 tensor's ``data_ptr()``)."""
        return cls._packed(ctx._l.ts_matrix_from_device_packed, ctx, C.c_void_p(ptr), fmt, height, width)

    @classmethod
    def fibonacci(cls, ctx: Context, a: int, b: int, n: int) -> "DeviceMatrix":
        """``generate_trace_rows(a, b, n)`` (uni-stark/tests/fib_air.rs:59-78) computed in HBM."""
        h = C.c_void_p()
        ctx.check(ctx._l.ts_trace_fibonacci(ctx.h, a, b, n, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def synth_mul(cls, ctx: Context, n: int, width: int = 64, seed: int | None = None) -> "DeviceMatrix":
        """The SynthMulAir-``width`` trace of ``airs.generate_synth_mul_trace``, computed in HBM."""
        from .airs import SPLITMIX_SEED
        h = C.c_void_p()
        ctx.check(ctx._l.ts_trace_synth_mul(ctx.h, n, width, SPLITMIX_SEED if seed is None else seed,
                                            C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def synth_ext(cls, ctx: Context, n: int, width: int = 163, seed: int | None = None) -> "DeviceMatrix":
        """The SynthExt-``width`` trace of ``airs.generate_synth_ext_trace``, computed in HBM."""
        from .airs import SPLITMIX_SEED
        h = C.c_void_p()
        ctx.check(ctx._l.ts_trace_synth_ext(ctx.h, n, width, SPLITMIX_SEED if seed is None else seed,
                                            C.byref(h)))
        return cls(ctx, h)

    def dims(self):
        hh, ww = C.c_uint64(), C.c_uint32()
        self.ctx.check(self.ctx._l.ts_matrix_dims(self.h, C.byref(hh), C.byref(ww)))
        return int(hh.value), int(ww.value)

    def download(self, monty_bits: int | None = None) -> np.ndarray:
        """Canonical words, or with ``monty_bits`` = 31 | 32 the Montgomery words value * 2^monty_bits mod p
        (``ts_matrix_download_monty``)."""
        hh, ww = self.dims()
        out = np.zeros((hh, ww), dtype=np.uint32)
        if monty_bits is None:
            self.ctx.check(self.ctx._l.ts_matrix_download(self.ctx.h, self.h, _p(out)))
        else:
            self.ctx.check(self.ctx._l.ts_matrix_download_monty(self.ctx.h, self.h, monty_bits, _p(out)))
        return out

    def bit_reverse_rows(self) -> "DeviceMatrix":
        """``bit_reverse_rows().to_row_major_matrix()`` as a new matrix (``ts_matrix_bit_reverse_rows``)."""
        h = C.c_void_p()
        self.ctx.check(self.ctx._l.ts_matrix_bit_reverse_rows(self.ctx.h, self.h, C.byref(h)))
        return DeviceMatrix(self.ctx, h)

    def sort_rows(self, keys, group_keys: int = 0, n_live: int | None = None, source_row: bool = False,
                  group_start: bool = False) -> "DeviceMatrix":
        """A new matrix with rows [0, n_live) in the stable order of the key columns ``keys`` (most significant
        first; words compared as stored, unsigned), the others in place; ``source_row`` and ``group_start`` append
        a column each, in that order (``ts_matrix_sort_rows``).  This matrix is only read."""
        keys = [int(k) for k in keys]
        spec = _lib.SortSpecC()
        spec.struct_size = C.sizeof(_lib.SortSpecC)
        spec.n_keys = len(keys)
        for q, k in enumerate(keys[:4]):
            spec.key_columns[q] = k
        spec.group_keys = group_keys
        spec.flags = (1 if source_row else 0) | (2 if group_start else 0)
        spec.n_live = self.dims()[0] if n_live is None else n_live
        h = C.c_void_p()
        self.ctx.check(self.ctx._l.ts_matrix_sort_rows(self.ctx.h, C.byref(spec), self.h, C.byref(h)))
        return DeviceMatrix(self.ctx, h)

    def gather_rows(self, index: "DeviceMatrix", column: int = 0) -> "DeviceMatrix":
        """``out[i] = self[index[i][column]]`` as a new matrix of ``index``'s height (``ts_matrix_gather_rows``)."""
        h = C.c_void_p()
        self.ctx.check(self.ctx._l.ts_matrix_gather_rows(self.ctx.h, self.h, index.h, column, C.byref(h)))
        return DeviceMatrix(self.ctx, h)

    def derive(self, program) -> "DeviceMatrix":
        """A new matrix of this height: the columns a row program names computed from this matrix, the others copied
        (``ts_matrix_derive``).  ``program`` is a ``derive.DeriveBuilder`` or its tape; this matrix is only read."""
        from .derive import _tape
        t = _tape(program)
        h = C.c_void_p()
        self.ctx.check(self.ctx._l.ts_matrix_derive(self.ctx.h, _p(t), len(t), self.h, C.byref(h)))
        return DeviceMatrix(self.ctx, h)

    def iterate(self, program) -> "DeviceMatrix":
        """The same call as ``derive`` for a program with carried state: ``program`` is an ``iterate.IterateBuilder`` or
        its TITR tape (include/tapstark.h "iterated columns").  One host wait."""
        return self.derive(program)

    def scan(self, spec, finals: bool = False):
        """A new matrix of this height: the columns the scans of ``spec`` (a ``scan.ScanSpec``) name hold linear
        recurrences down the rows of this matrix, the other kept columns are copied (``ts_matrix_scan``); this matrix is
        only read.  With ``finals`` the pair (matrix, the last value of each scan) -- and one host wait."""
        last = np.zeros(8, dtype=np.uint32)
        h = C.c_void_p()
        self.ctx.check(self.ctx._l.ts_matrix_scan(self.ctx.h, C.byref(spec.c_spec()), self.h, C.byref(h),
                                                  _p(last) if finals else None))
        out = DeviceMatrix(self.ctx, h)
        return (out, last[:len(spec.columns)].copy()) if finals else out

    def join_rows(self, table: "DeviceMatrix", spec, allow_missing: bool = False):
        """The triple (a new matrix, n_missing, first_missing): this matrix with columns of ``table`` fetched by key
        into its rows as ``spec`` (a ``join.JoinSpec``) says (``ts_matrix_join_rows``).  A miss is a row that takes part
        and finds its key in no table row: ``first_missing`` is the least such row or None; without ``allow_missing``
        any miss raises ``TsError``.  This matrix and ``table`` (which may be this matrix) are only read.  One host
        wait."""
        s, _keep = spec.c_spec()
        h, n, first = C.c_void_p(), C.c_uint64(), C.c_uint64()
        self.ctx.check(self.ctx._l.ts_matrix_join_rows(self.ctx.h, C.byref(s), self.h, table.h, C.byref(h),
                                                       C.byref(n) if allow_missing else None, C.byref(first)))
        first_missing = None if first.value == 0xFFFFFFFFFFFFFFFF else int(first.value)
        return DeviceMatrix(self.ctx, h), int(n.value), first_missing

    def expand_rows(self, spec, out_height: int = 0):
        """``expand_rows(self.ctx, spec, self, out_height)``."""
        return expand_rows(self.ctx, spec, self, out_height)

    def device_ptr(self) -> int:
        """Row-major device pointer (``ts_matrix_device_ptr``): valid until the matrix is freed or consumed,
        ordered on the context's stream; ``from_device_ptr`` is the opposite direction."""
        ptr = C.c_void_p()
        self.ctx.check(self.ctx._l.ts_matrix_device_ptr(self.ctx.h, self.h, C.byref(ptr)))
        return int(ptr.value or 0)

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx._l.ts_matrix_free(self.ctx.h, self.h)
        except Exception:
            pass


def collect_rows(ctx: Context, spec, sources, out_height: int = 0):
    """The pair (a new matrix, n_live): the rows the emitters of ``spec`` (a ``collect.CollectSpec`` or its tape) select
    from the resident matrices ``sources``, in (source, row, emitter) order, padded to ``out_height`` rows or to the
    least power of two that holds them (``ts_matrix_collect_rows``).  The sources are only read.  One host wait."""
    from .collect import _tape
    t = _tape(spec)
    sources = list(sources)
    handles = (C.c_void_p * max(len(sources), 4))(*[m.h for m in sources])
    h, live = C.c_void_p(), C.c_uint64()
    ctx.check(ctx._l.ts_matrix_collect_rows(ctx.h, _p(t), len(t), handles, out_height, C.byref(h), C.byref(live)))
    return DeviceMatrix(ctx, h), int(live.value)


def group_rows(ctx: Context, spec, src: DeviceMatrix, out_height: int = 0):
    """The pair (a new matrix, n_groups): one row per distinct key tuple among the rows of the resident matrix ``src``
    that take part, as ``spec`` (a ``group.GroupSpec`` or its tape) says, in order of first appearance, padded to
    ``out_height`` rows or to the least power of two that holds them (``ts_matrix_collect_rows`` with a TGRP tape).
    ``src`` is only read.  One host wait."""
    from .group import _tape
    t = _tape(spec)
    handles = (C.c_void_p * 4)(src.h)
    h, live = C.c_void_p(), C.c_uint64()
    ctx.check(ctx._l.ts_matrix_collect_rows(ctx.h, _p(t), len(t), handles, out_height, C.byref(h), C.byref(live)))
    return DeviceMatrix(ctx, h), int(live.value)


def expand_rows(ctx: Context, spec, src: DeviceMatrix, out_height: int = 0):
    """The pair (a new matrix, n_live): every row of the resident matrix ``src`` repeated by the count ``spec`` (an
    ``expand.ExpandSpec`` or its tape) reads from it, in (row, inner index) order, padded to ``out_height`` rows or to
    the least power of two that holds them (``ts_matrix_expand_rows``).  ``src`` is only read.  One host wait."""
    from .expand import _tape
    t = _tape(spec)
    h, live = C.c_void_p(), C.c_uint64()
    ctx.check(ctx._l.ts_matrix_expand_rows(ctx.h, _p(t), len(t), src.h, out_height, C.byref(h), C.byref(live)))
    return DeviceMatrix(ctx, h), int(live.value)


class Radix2Dft:
    """``TwoAdicSubgroupDft`` (the ``Dft`` of ``TwoAdicFriPcs::new``, fri/src/two_adic_pcs.rs:38-55;
    SURVEY.md App. A.5) on device matrices.  Every method takes a ``DeviceMatrix`` (or host values, which are
    uploaded), leaves it as it is and returns a new ``DeviceMatrix``: row-major, natural rows, canonical."""

    def __init__(self, ctx: "Context | None" = None):
        self.ctx = ctx or default_context()

    def _mat(self, m) -> "DeviceMatrix":
        return m if isinstance(m, DeviceMatrix) else DeviceMatrix.upload(self.ctx, m)

    def _dft(self, m, inverse: bool, shift: int) -> "DeviceMatrix":
        m, h = self._mat(m), C.c_void_p()
        self.ctx.check(self.ctx._l.ts_dft_batch(self.ctx.h, m.h, int(inverse), shift, C.byref(h)))
        return DeviceMatrix(self.ctx, h)

    def dft_batch(self, m) -> "DeviceMatrix":
        return self._dft(m, False, 1)

    def idft_batch(self, m) -> "DeviceMatrix":
        return self._dft(m, True, 1)

    def coset_dft_batch(self, m, shift: int) -> "DeviceMatrix":
        """out row k = sum_j m[j] (shift w_n^k)^j per column."""
        return self._dft(m, False, shift)

    def coset_idft_batch(self, m, shift: int) -> "DeviceMatrix":
        """Coefficients of the interpolant of ``m`` over shift * H_n."""
        return self._dft(m, True, shift)

    def coset_lde_batch(self, m, added_bits: int, shift: int, bit_reversed: bool = False) -> "DeviceMatrix":
        """``m``: evaluations over H_n; out row j (row bitrev(j) with ``bit_reversed``) = the interpolant at
        shift * w_N^j, N = n << added_bits."""
        m, h = self._mat(m), C.c_void_p()
        self.ctx.check(self.ctx._l.ts_coset_lde_batch(self.ctx.h, m.h, added_bits, shift, int(bit_reversed),
                                                      C.byref(h)))
        return DeviceMatrix(self.ctx, h)

    def lde_batch(self, m, added_bits: int) -> "DeviceMatrix":
        return self.coset_lde_batch(m, added_bits, 1)


class CompiledAir:
    """``ts_air``.  With ``ctx=None`` the AIR is host-only (degree rules, ``verify``): no GPU.

    ``segment_instr=S`` (``ts_air_compile_opts``): a program longer than S lowered instructions gets the
    segmented specialisation, compiled in the background by up to ``jit_jobs`` children (default 4, at most
    8); ``None`` or 0 is the default route."""

    def __init__(self, ctx: "Context | None", tape, segment_instr: int | None = None, jit_jobs: int | None = None):
        self.ctx = ctx
        self._l = _lib.lib()
        self.tape = _u32(tape)
        h = C.c_void_p()
        if segment_instr is None and jit_jobs is None:
            rc = self._l.ts_air_compile(ctx.h if ctx else None, _p(self.tape), len(self.tape), C.byref(h))
        else:
            opt = _lib.AirOptionsC(C.sizeof(_lib.AirOptionsC), int(segment_instr or 0), int(jit_jobs or 0), 0)
            rc = self._l.ts_air_compile_opts(ctx.h if ctx else None, _p(self.tape), len(self.tape), C.byref(opt),
                                             C.byref(h))
        if rc:
            msg = self._l.ts_last_error(ctx.h if ctx else None) or b""
            raise _lib.TsError(rc, msg.decode())
        self.h = h
        w, npub, deg, lqd = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._l.ts_air_info(h, C.byref(w), C.byref(npub), C.byref(deg), C.byref(lqd))
        self.width, self.n_public = int(w.value), int(npub.value)
        self.max_constraint_degree, self.log_quotient_degree = int(deg.value), int(lqd.value)
        pw = C.c_uint32()
        self._l.ts_air_preprocessed_width(h, C.byref(pw))
        self.preprocessed_width = int(pw.value)
        aw, nc, ne = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._l.ts_air_aux_info(h, C.byref(aw), C.byref(nc), C.byref(ne))
        self.aux_width, self.n_challenges, self.n_exposed = int(aw.value), int(nc.value), int(ne.value)

    @property
    def is_jit(self) -> bool:
        """The hiprtc-specialised quotient kernel is loaded (else the on-device interpreter runs;
        large programs are compiled in the background and switch over when ready)."""
        return bool(self._l.ts_air_is_jit(self.h))

    def jit_wait(self) -> tuple[int, float]:
        """Joins a background specialisation: (state 0 none | 3 loaded | 4 failed, compile seconds)."""
        st, secs = C.c_int(), C.c_double()
        rc = self._l.ts_air_jit_wait(self.ctx.h, self.h, C.byref(st), C.byref(secs))
        if rc:
            raise self._err(rc)
        return int(st.value), float(secs.value)

    def _err(self, rc: int):
        msg = self._l.ts_last_error(self.ctx.h if self.ctx else None) or b""
        return _lib.TsError(rc, msg.decode())

    def program(self) -> dict:
        """The register program the tape was lowered to (``ts_air_program``): ``n_regs``, ``code``
        (n_instr, 4) = {op, dst, a, b}, ``consts`` (canonical), ``const_public`` (index or 0xffffffff)."""
        n = C.c_size_t()
        self._l.ts_air_program(self.h, None, 0, C.byref(n))
        out = np.zeros(n.value, dtype=np.uint32)
        rc = self._l.ts_air_program(self.h, _p(out), len(out), C.byref(n))
        if rc:
            raise self._err(rc)
        n_regs, n_instr, n_consts = (int(v) for v in out[:3])
        code = out[3:3 + 4 * n_instr].reshape(n_instr, 4)
        consts = out[3 + 4 * n_instr:3 + 4 * n_instr + n_consts]
        return {"n_regs": n_regs, "code": code, "consts": consts, "const_public": out[3 + 4 * n_instr + n_consts:]}

    def segment_plan(self) -> dict:
        """The plan of a segmented AIR (``ts_air_segment_plan``): ``slab_width`` and ``segments``, each a dict
        of ``begin``, ``end``, ``pressure``, ``live_in`` and ``live_out`` as lists of (defining instruction,
        slot).  TsError(TS_ERR_INVALID) for an AIR that is not segmented."""
        n = C.c_size_t()
        rc = self._l.ts_air_segment_plan(self.h, None, 0, C.byref(n))
        if rc != 6:  # TS_ERR_BUFFER, with the size
            raise _lib.TsError(rc, "ts_air_segment_plan: not a segmented AIR")
        out = np.zeros(n.value, dtype=np.uint32)
        rc = self._l.ts_air_segment_plan(self.h, _p(out), len(out), C.byref(n))
        if rc:
            raise _lib.TsError(rc, "ts_air_segment_plan")
        w = out.tolist()
        segs, k = [], 2
        for _ in range(w[1]):
            b, e, n_in, n_out, pr = w[k:k + 5]
            k += 5
            li = [tuple(w[k + 2 * j:k + 2 * j + 2]) for j in range(n_in)]
            k += 2 * n_in
            lo = [tuple(w[k + 2 * j:k + 2 * j + 2]) for j in range(n_out)]
            k += 2 * n_out
            segs.append({"begin": b, "end": e, "pressure": pr, "live_in": li, "live_out": lo})
        return {"slab_width": w[0], "segments": segs}

    def jit_source(self) -> str:
        n = C.c_size_t()
        self._l.ts_air_jit_source(self.h, None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value)
        rc = self._l.ts_air_jit_source(self.h, buf, n.value, C.byref(n))
        if rc:
            raise self._err(rc)
        return buf.raw[:n.value].decode()

    def jit_compile(self, arch: str = "gfx950") -> tuple[bytes, float]:
        """(code object, compile seconds) of the hiprtc-specialised quotient kernel; no GPU needed."""
        cap = 64 << 20
        buf = C.create_string_buffer(cap)
        n, secs = C.c_size_t(), C.c_double()
        rc = self._l.ts_air_jit_compile(self.h, arch.encode(), buf, cap, C.byref(n), C.byref(secs))
        if rc:
            raise self._err(rc)
        return buf.raw[:n.value], float(secs.value)

    def __del__(self):
        try:
            if self.h and (self.ctx is None or self.ctx.h):
                self._l.ts_air_free(self.ctx.h if self.ctx else None, self.h)
        except Exception:
            pass


@dataclass
class FriConfig:
    """reference fri/src/config.rs:11-16; ``mmcs`` is the built-in Blake3 Merkle MMCS."""
    log_blowup: int
    num_queries: int
    proof_of_work_bits: int

    def blowup(self) -> int:
        return 1 << self.log_blowup

    def _c(self):
        return _lib.FriConfigC(self.log_blowup, self.num_queries, self.proof_of_work_bits)


class PcsData:
    """``Pcs::ProverData``: committed LDEs + Merkle tree in HBM (``ts_pcs_data``)."""

    def __init__(self, ctx: Context, handle, root: np.ndarray):
        self.ctx, self.h, self.root = ctx, handle, root
        n, lh = C.c_uint32(), C.c_uint32()
        ctx.check(ctx._l.ts_pcs_data_info(handle, C.byref(n), C.byref(lh)))
        self.n_mats, self.log_height = int(n.value), int(lh.value)
        self.dims = []  # (LDE height, width) per committed matrix
        for i in range(self.n_mats):
            hh, ww = C.c_uint64(), C.c_uint32()
            ctx.check(ctx._l.ts_pcs_data_matrix_info(handle, i, C.byref(hh), C.byref(ww)))
            self.dims.append((int(hh.value), int(ww.value)))

    def lde(self, idx: int, width: int | None = None) -> np.ndarray:
        out = np.zeros(self.dims[idx], dtype=np.uint32)
        self.ctx.check(self.ctx._l.ts_pcs_data_lde(self.ctx.h, self.h, idx, _p(out)))
        return out

    def digests(self, level: int) -> np.ndarray:
        out = np.zeros(((1 << self.log_height) >> level, 8), dtype=np.uint32)
        self.ctx.check(self.ctx._l.ts_pcs_data_digests(self.ctx.h, self.h, level, _p(out)))
        return out

    def open_batch(self, index: int, total_width: int | None = None):
        if total_width is None:
            total_width = sum(w for _, w in self.dims)
        rows = np.zeros(max(total_width, 1), dtype=np.uint32)
        path = np.zeros((max(self.log_height, 1), 8), dtype=np.uint32)
        self.ctx.check(self.ctx._l.ts_pcs_open_batch(self.ctx.h, self.h, index, _p(rows), _p(path)))
        return rows[:total_width], path[: self.log_height]

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx._l.ts_pcs_data_free(self.ctx.h, self.h)
        except Exception:
            pass


class Blake3Mmcs:
    """``BFMmcs`` (basic/src/mmcs/bf_mmcs.rs:17-68) with the build-defined Blake3 Merkle tree, on
    the device: ``commit`` to matrices as given (no LDE), ``open_batch`` via the returned PcsData."""

    def __init__(self, ctx: Context | None = None):
        self.ctx = ctx or default_context()

    def commit(self, inputs) -> tuple[np.ndarray, PcsData]:
        ctx = self.ctx
        mats = [m if isinstance(m, DeviceMatrix) else DeviceMatrix.upload(ctx, m) for m in inputs]
        arr = (C.c_void_p * len(mats))(*[m.h for m in mats])
        root = np.zeros(8, dtype=np.uint32)
        h = C.c_void_p()
        ctx.check(ctx._l.ts_mmcs_commit(ctx.h, len(mats), arr, _p(root), C.byref(h)))
        return root, PcsData(ctx, h, root)

    def commit_matrix(self, m):
        return self.commit([m])

    def open_batch(self, index: int, data: PcsData):
        return data.open_batch(index)


class TwoAdicFriPcs:
    """reference fri/src/two_adic_pcs.rs:38-61,203-419 on the device."""

    def __init__(self, fri: FriConfig, ctx: Context | None = None, host_only: bool = False):
        self.fri = fri
        self.ctx = None if host_only else (ctx or default_context())

    def natural_domain_for_degree(self, degree: int):
        return (degree.bit_length() - 1, 1)  # (log_n, shift), two_adic_pcs.rs:220-226

    def commit(self, evaluations) -> tuple[np.ndarray, PcsData]:
        """``evaluations``: list of ((log_n, shift), DeviceMatrix | ndarray). Matrices are consumed."""
        ctx = self.ctx
        mats, shifts = [], []
        for (log_n, shift), m in evaluations:
            if not isinstance(m, DeviceMatrix):
                m = DeviceMatrix.upload(ctx, m)
            assert m.dims()[0] == 1 << log_n
            mats.append(m)
            shifts.append(shift)
        arr = (C.c_void_p * len(mats))(*[m.h for m in mats])
        sh = _u32(shifts)
        root = np.zeros(8, dtype=np.uint32)
        h = C.c_void_p()
        cfg = self.fri._c()
        ctx.check(ctx._l.ts_pcs_commit(ctx.h, C.byref(cfg), len(mats), arr, _p(sh), _p(root),
                                       C.byref(h)))
        return root, PcsData(ctx, h, root)

    def get_evaluations_on_domain(self, data: PcsData, idx: int, log_size: int) -> DeviceMatrix:
        """two_adic_pcs.rs:247-258 kept in HBM: the first 2^log_size rows of committed LDE ``idx``,
        un-bit-reversed (``ts_pcs_data_evaluations_on_domain``)."""
        h = C.c_void_p()
        self.ctx.check(self.ctx._l.ts_pcs_data_evaluations_on_domain(self.ctx.h, data.h, idx, log_size, C.byref(h)))
        return DeviceMatrix(self.ctx, h)

    def quotient_chunks(self, trace_data: PcsData, air: CompiledAir, public_values, alpha, preprocessed=None,
                        aux=None, challenges=None, exposed=None):
        """``preprocessed``: the ``PreprocessedKey`` (or its ``PcsData``) of an AIR with preprocessed columns
        (``ts_quotient_chunks_pre``); None is ``ts_quotient_chunks``.  ``aux``: the committed aux trace (a
        ``PcsData``) of an AIR with challenge-phase columns, with its ``challenges`` and ``exposed`` words
        (``ts_quotient_chunks_aux``).  Both ``preprocessed`` and ``aux``: an AIR with both kinds of column
        (``ts_quotient_chunks_pre_aux``)."""
        qd = 1 << air.log_quotient_degree
        out = (C.c_void_p * qd)()
        pis = _u32(public_values)
        fn, key_args, aux_args = _single_call(self.ctx._l, "quotient_chunks",
                                              *_side_arguments(preprocessed, aux, challenges, exposed))
        key = getattr(preprocessed, "data", preprocessed)
        self.ctx.check(fn(self.ctx.h, *key_args(key.h if key is not None else None),
                          *aux_args(aux.h if aux is not None else None), trace_data.h, self.fri.log_blowup, air.h,
                          _p(pis) if len(pis) else None, len(pis), *aux_args(*_challenge_words(challenges, exposed)),
                          _p(_u32(alpha)), out))
        return [DeviceMatrix(self.ctx, C.c_void_p(out[c])) for c in range(qd)]

    def open_reduce(self, trace_data: PcsData, quotient_data: PcsData, width: int, zeta, batch_alpha):
        qd = quotient_data.n_mats
        opened = np.zeros((2 * width + 4 * qd, 4), dtype=np.uint32)
        ro = np.zeros((1 << trace_data.log_height, 4), dtype=np.uint32)
        cfg = self.fri._c()
        self.ctx.check(self.ctx._l.ts_pcs_open_reduce(self.ctx.h, C.byref(cfg), trace_data.h,
                                                      quotient_data.h, _p(_u32(zeta)),
                                                      _p(_u32(batch_alpha)), _p(opened), _p(ro)))
        return opened, ro

    def open(self, rounds, challenger: "BfChallenger"):
        """``Pcs::open`` (two_adic_pcs.rs:260-419).  ``rounds``: list of (PcsData, points) with
        ``points[m]`` the list of EF4 opening points of matrix m.  Returns (opened, fri_proof):
        ``opened[r][m][p]`` is a (width, 4) array, ``fri_proof`` the FriProof words (TSPF v1)."""
        n_pts, pts, total = [], [], 0
        for data, points in rounds:
            assert len(points) == data.n_mats
            for (_, w), pl in zip(data.dims, points):
                n_pts.append(len(pl))
                pts.extend(_u32(z).reshape(4) for z in pl)
                total += w * len(pl)
        handles = (C.c_void_p * len(rounds))(*[d.h for d, _ in rounds])
        n_pts_a = _u32(n_pts)
        pts_a = _u32(np.concatenate(pts)) if pts else np.zeros(4, dtype=np.uint32)
        opened = np.zeros((max(total, 1), 4), dtype=np.uint32)
        # exact FriProof size (DESIGN.md "Proof format")
        log_max = max(d.log_height for d, _ in rounds)
        R, Q = max(log_max - self.fri.log_blowup, 0), self.fri.num_queries
        per_q = 1 + sum(2 + d.n_mats + sum(w for _, w in d.dims) + 8 * d.log_height for d, _ in rounds)
        per_q += sum(9 + 8 * (log_max - 1 - i) for i in range(R))
        cap = 2 + 8 * R + Q * per_q + 5
        cfg = self.fri._c()
        proof = np.zeros(cap, dtype=np.uint32)
        n_o, n_p = C.c_size_t(), C.c_size_t()
        self.ctx.check(self.ctx._l.ts_pcs_open(self.ctx.h, C.byref(cfg), challenger.h, len(rounds),
                                               handles, _p(n_pts_a), _p(pts_a), _p(opened),
                                               opened.size, C.byref(n_o), _p(proof), cap,
                                               C.byref(n_p)))
        assert n_o.value == 4 * total
        out, k = [], 0
        for data, points in rounds:
            r_out = []
            for (_, w), pl in zip(data.dims, points):
                m_out = []
                for _ in pl:
                    m_out.append(opened[k:k + w].copy())
                    k += w
                r_out.append(m_out)
            out.append(r_out)
        return out, proof[: n_p.value].copy()

    def verify(self, rounds, fri_proof, challenger: "BfChallenger") -> None:
        """``Pcs::verify`` (two_adic_pcs.rs:421-534), host only.  ``rounds``: list of
        (commitment, mats) with ``mats[m] = (log_degree, [(point, values (width, 4)), ...])``.
        Raises :class:`VerificationError`."""
        roots, per_round, logs, widths, n_pts, pts, vals = [], [], [], [], [], [], []
        for root, mats in rounds:
            roots.append(_u32(root).reshape(8))
            per_round.append(len(mats))
            for log_degree, openings in mats:
                logs.append(log_degree)
                n_pts.append(len(openings))
                width = None
                for z, v in openings:
                    v = _u32(v).reshape(-1, 4)
                    width = len(v)
                    pts.append(_u32(z).reshape(4))
                    vals.append(v.reshape(-1))
                widths.append(width or 0)
        fri_proof = _u32(fri_proof)
        verdict = C.c_int(9)
        cfg = self.fri._c()
        cat = lambda xs: _u32(np.concatenate(xs)) if xs else np.zeros(4, dtype=np.uint32)  # noqa: E731
        rc = _lib.lib().ts_pcs_verify(C.byref(cfg), challenger.h, len(rounds), _p(cat(roots)),
                                      _p(_u32(per_round)), _p(_u32(logs)), _p(_u32(widths)),
                                      _p(_u32(n_pts)), _p(cat(pts)), _p(cat(vals)), _p(fri_proof),
                                      len(fri_proof), C.byref(verdict))
        if rc:
            raise _lib.TsError(rc, "ts_pcs_verify")
        if verdict.value:
            raise VerificationError(verdict.value)

    def fri_prove(self, inputs, challenger: "BfChallenger") -> np.ndarray:
        """``bf_prove`` alone (fri/src/prover.rs:19-63) the way fri/tests/fri.rs:100-119 calls it:
        ``inputs`` are (len, 4) EF4 vectors of strictly descending power-of-two lengths; the input
        opening proof is the literal reduced openings.  Returns the FriProof words."""
        ins = [_u32(v).reshape(-1, 4) for v in inputs]
        logs = _u32([len(v).bit_length() - 1 for v in ins])
        ptrs = (_lib.u32p * len(ins))(*[_p(v) for v in ins])
        R = max(int(logs[0]) - self.fri.log_blowup, 0)
        cap = 16 + 8 * R + self.fri.num_queries * (1 + 5 * len(ins) + sum(9 + 8 * (int(logs[0]) - 1 - i)
                                                                           for i in range(R)))
        out = np.zeros(cap, dtype=np.uint32)
        n = C.c_size_t()
        cfg = self.fri._c()
        self.ctx.check(self.ctx._l.ts_fri_prove(self.ctx.h, C.byref(cfg), challenger.h, len(ins),
                                                _p(logs), ptrs, _p(out), cap, C.byref(n)))
        return out[: n.value].copy()

    def fri_verify(self, proof, challenger: "BfChallenger") -> None:
        """fri/src/verifier.rs:20-98 for a proof of :meth:`fri_prove` (host only)."""
        proof = _u32(proof)
        verdict = C.c_int(9)
        cfg = self.fri._c()
        rc = _lib.lib().ts_fri_verify(C.byref(cfg), challenger.h, _p(proof), len(proof), C.byref(verdict))
        if rc:
            raise _lib.TsError(rc, "ts_fri_verify")
        if verdict.value:
            raise VerificationError(verdict.value)

    def fold_matrix(self, vec, beta) -> np.ndarray:
        vec = _u32(vec)
        h = vec.shape[0] // 2
        out = np.zeros((h, 4), dtype=np.uint32)
        self.ctx.check(self.ctx._l.ts_fri_fold(self.ctx.h, _p(vec), h, _p(_u32(beta)), _p(out)))
        return out


@dataclass
class StarkConfig:
    """reference uni-stark/src/config.rs:64-101 (Challenge = EF4, Challenger = BfChallenger)."""
    pcs: TwoAdicFriPcs


class BfChallenger:
    """reference basic/src/challenger/mod.rs:67-137 (host side, ``ts_challenger``)."""

    def __init__(self, permutation: int = 0, sample_ext: bool = True, _handle=None):
        self._l = _lib.lib()
        if _handle is None:
            h = C.c_void_p()
            rc = self._l.ts_chal_new(permutation, int(sample_ext), C.byref(h))
            if rc:
                raise _lib.TsError(rc, "ts_chal_new")
            _handle = h
        self.h = _handle

    def clone(self) -> "BfChallenger":
        h = C.c_void_p()
        rc = self._l.ts_chal_clone(self.h, C.byref(h))
        if rc:
            raise _lib.TsError(rc, "ts_chal_clone")
        return BfChallenger(_handle=h)

    def observe(self, word: int):
        self._l.ts_chal_observe(self.h, word)

    def observe_commitment(self, d):
        self._l.ts_chal_observe_commitment(self.h, _p(_u32(d)))

    def sample(self) -> np.ndarray:
        out = np.zeros(4, dtype=np.uint32)
        self._l.ts_chal_sample(self.h, _p(out))
        return out

    def sample_bits(self, bits: int) -> int:
        return int(self._l.ts_chal_sample_bits(self.h, bits))

    def check_witness(self, bits: int, witness: int) -> bool:
        return bool(self._l.ts_chal_check_witness(self.h, bits, witness))

    def grind(self, bits: int) -> int:
        w = C.c_uint32()
        rc = self._l.ts_chal_grind(self.h, bits, C.byref(w))
        if rc:
            raise _lib.TsError(rc, "failed to find witness")
        return int(w.value)

    def state(self) -> np.ndarray:
        out = np.zeros(34, dtype=np.uint32)
        self._l.ts_chal_state(self.h, _p(out))
        return out

    def __del__(self):
        try:
            if self.h:
                self._l.ts_chal_free(self.h)
        except Exception:
            pass


# ------------------------------------------------------------------------ Proof
@dataclass
class BatchOpening:
    """reference fri/src/two_adic_pcs.rs:63-68"""
    opened_values: list
    opening_proof: np.ndarray


@dataclass
class QueryProof:
    """reference fri/src/proof.rs:28-33"""
    input_proof: list
    commit_phase_openings: list


class _Words:
    """The words of a proof, taken in order: ``take(n)`` raises ``ValueError`` past the end."""

    def __init__(self, w):
        self.w, self.pos = w, 0

    def __call__(self, n):
        out = self.w[self.pos:self.pos + n]
        if len(out) != n:
            raise ValueError("truncated proof")
        self.pos += n
        return out


def _parse_fri_tail(take: _Words, R_shape) -> dict:
    """The FriProof (fri/src/proof.rs:13-21) that ends every TSPF format, and nothing behind it: the commit-phase
    roots (``R_shape`` words each: (8,), or (num_queries, 8) over taptrees), the query proofs, the final polynomial
    and the proof-of-work witness."""
    R = int(take(1)[0])
    d = {"commit_phase_commits": take(int(np.prod(R_shape)) * R).reshape(R, *R_shape), "query_proofs": []}
    for _ in range(int(take(1)[0])):
        batches = []
        for _ in range(int(take(1)[0])):
            vals = [take(int(take(1)[0])) for _ in range(int(take(1)[0]))]
            plen = int(take(1)[0])
            batches.append(BatchOpening(vals, take(8 * plen).reshape(plen, 8)))
        steps = []
        for _ in range(R):
            vals = take(8).reshape(2, 4)
            plen = int(take(1)[0])
            steps.append((vals, take(8 * plen).reshape(plen, 8)))
        d["query_proofs"].append(QueryProof(batches, steps))
    d["final_poly"] = take(4)
    d["pow_witness"] = int(take(1)[0])
    if take.pos != len(take.w):
        raise ValueError("trailing words in proof")
    return d


class Proof:
    """reference uni-stark/src/proof.rs:17-37 (+ FriProof fri/src/proof.rs:13-21) over the TSPF v1
    words the library writes; ``words`` keeps the wire form.  The structured fields (``degree_bits``,
    ``trace_commit``, ``quotient_commit``, ``trace_local``, ``trace_next``, ``quotient_chunks``,
    ``commit_phase_commits``, ``query_proofs``, ``final_poly``, ``pow_witness``) are parsed on first
    access: ``prove()`` hands back the words without spending interpreter time on them."""

    _FIELDS = ("degree_bits", "trace_commit", "quotient_commit", "preprocessed_local", "preprocessed_next",
               "version", "aux_width", "n_challenges", "aux_commit", "exposed", "aux_local", "aux_next",
               "trace_local", "trace_next", "quotient_chunks", "commit_phase_commits", "query_proofs", "final_poly", "pow_witness")
    # TSPF version -> (the header words behind magic, version, degree_bits, width and quotient degree; whether a
    # commitment is `nr` roots, the commitment fields then (nr, 8) arrays).  v2 (ts_prove_tap, over the taptree MMCS):
    # num_queries roots per commitment.  v3 (ts_prove_pre): the preprocessed width.  v4 (ts_prove_aux): aux width,
    # challenge and exposed counts.  v5 (ts_prove_pre_aux): the v4 header, then the preprocessed width.
    _HEADER = {1: ((), False), 2: (("nr",), True), 3: (("pw",), False), 4: (("aw", "nc", "ne"), False),
               5: (("aw", "nc", "ne", "pw"), False)}

    def __init__(self, words):
        self.words = np.asarray(words, dtype=np.uint32)

    def __getattr__(self, name):  # only reached for attributes not set yet
        if name in Proof._FIELDS:
            self._parse()
            return self.__dict__[name]
        raise AttributeError(name)

    def to_postcard(self) -> bytes:
        """postcard bytes of the reference's serde ``Proof`` (``ts_proof_to_postcard``)."""
        l = _lib.lib()
        w = _u32(self.words)
        out = np.zeros(5 * len(w) + 16, dtype=np.uint8)  # a varint takes at most 5 bytes per word
        n = C.c_size_t()
        rc = l.ts_proof_to_postcard(_p(w), len(w), out.ctypes.data_as(C.POINTER(C.c_uint8)), len(out),
                                    C.byref(n))
        if rc:
            raise _lib.TsError(rc, "ts_proof_to_postcard")
        return out[: n.value].tobytes()

    @classmethod
    def from_postcard(cls, data: bytes, version: int = 0) -> "Proof":
        """``version``: 0 infers TSPF v1 / v2 from the number of roots per commitment; 2 must be
        given for a proof over taptrees made with one query (``ts_proof_from_postcard_v``)."""
        l = _lib.lib()
        b = np.frombuffer(data, dtype=np.uint8).copy()
        out = np.zeros(len(b) + 16, dtype=np.uint32)  # every word takes at least one byte
        n = C.c_size_t()
        rc = l.ts_proof_from_postcard_v(b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), int(version),
                                        _p(out), len(out), C.byref(n))
        if rc:
            raise _lib.TsError(rc, "ts_proof_from_postcard")
        return cls.parse(out[: n.value].copy())

    @classmethod
    def parse(cls, words: np.ndarray) -> "Proof":
        """Eager form: raises ``ValueError`` on a malformed buffer."""
        pf = cls(words)
        pf._parse()
        return pf

    def _parse(self) -> None:
        take = _Words(self.words)
        magic, version, degree_bits, width, qd = (int(x) for x in take(5))
        if magic != TSPF_MAGIC or version not in self._HEADER:
            raise ValueError("not a TSPF v1/v2/v3/v4/v5 proof")
        extras, many_roots = self._HEADER[version]
        h = {"nr": 1, "pw": 0, "aw": 0, "nc": 0, "ne": 0}
        h.update(zip(extras, (int(x) for x in take(len(extras)))))
        nr, pw, aw, nc, ne = (h[k] for k in ("nr", "pw", "aw", "nc", "ne"))
        commitment = (lambda: take(8 * nr).reshape(nr, 8)) if many_roots else (lambda: take(8))
        d = {"degree_bits": degree_bits, "version": version, "preprocessed_width": pw,
             "aux_width": aw, "n_challenges": nc, "aux_commit": None, "exposed": np.zeros(0, dtype=np.uint32)}
        d["trace_commit"] = commitment()
        if aw:  # the aux root and the exposed words sit between the two commitments
            d["aux_commit"], d["exposed"] = take(8), take(ne)
        d["quotient_commit"] = commitment()
        # the opened rows of the key, then of the aux trace, lead the opened values; every query's input proof holds
        # one BatchOpening for each of them before the trace's and the chunks'
        d["preprocessed_local"] = take(4 * pw).reshape(pw, 4)
        d["preprocessed_next"] = take(4 * pw).reshape(pw, 4)
        d["aux_local"] = take(4 * aw).reshape(aw, 4)
        d["aux_next"] = take(4 * aw).reshape(aw, 4)
        d["trace_local"] = take(4 * width).reshape(width, 4)
        d["trace_next"] = take(4 * width).reshape(width, 4)
        d["quotient_chunks"] = take(16 * qd).reshape(qd, 4, 4)
        d.update(_parse_fri_tail(take, (nr, 8) if many_roots else (8,)))
        self.__dict__.update(d)


class PreprocessedKey:
    """The preprocessed (fixed) columns of an AIR, committed once: ``ts_pcs_commit`` of the one (n, P) matrix
    on the natural domain.  ``data`` is the ``PcsData`` the prover reads (never consumed: one key serves any
    number of proofs on its context), ``root`` what the verifier holds.  ``keep_values=True`` (an array given)
    keeps a second, row-major device copy of the values in ``values``: the commit consumes its matrix, and a LogUp
    aux source that reads the table (``LogUp.build(..., preprocessed=key.values)``) needs the rows."""

    def __init__(self, config: "StarkConfig", matrix, keep_values: bool = False):
        pcs = config.pcs
        self.values = None
        if keep_values:
            if isinstance(matrix, DeviceMatrix):
                raise ValueError("keep_values needs the values as an array: a DeviceMatrix is consumed by the commit")
            self.values = DeviceMatrix.upload(pcs.ctx, _u32(matrix))
        if not isinstance(matrix, DeviceMatrix):
            matrix = DeviceMatrix.upload(pcs.ctx, _u32(matrix))
        n = matrix.dims()[0]
        self.root, self.data = pcs.commit([(pcs.natural_domain_for_degree(n), matrix)])
        self.root = self.root.copy()


def _preprocessed_width(air) -> int:
    f = getattr(air, "preprocessed_width", 0)
    return int(f() if callable(f) else f)


def _air_tape_of(air, n_public: int):
    return air_tape(air, n_public, _preprocessed_width(air), *aux_dims(air))


def _single_call(l, op: str, has_key: bool, has_aux: bool):
    """The one dispatch of the single-table calls: the entry point ``ts_<op>[_pre][_aux]`` for a call with a key
    argument, an aux argument or both, and two filters ``key_args(*a)`` / ``aux_args(*a)`` that give ``a`` where the
    entry point has such arguments and ``()`` where it has not."""
    fn = getattr(l, "ts_" + op + ("_pre" if has_key else "") + ("_aux" if has_aux else ""))
    return fn, (lambda *a: a if has_key else ()), (lambda *a: a if has_aux else ())


def _side_arguments(preprocessed, aux, challenges, exposed):
    """(has_key, has_aux) of a quotient_chunks or check_constraints call: challenge or exposed words alone select the
    aux call, and without the aux argument itself that call is the one without a key."""
    has_aux = aux is not None or challenges is not None or exposed is not None
    return preprocessed is not None and (aux is not None or not has_aux), has_aux


def _challenge_words(challenges, exposed):
    """The two pointer arguments of the aux calls (None for no words)."""
    ch, ex = _u32(challenges if challenges is not None else []), _u32(exposed if exposed is not None else [])
    return _p(ch) if len(ch) else None, _p(ex) if len(ex) else None


def _aux_callback(ctx, air, aux, failure: list):
    """The ``ts_aux_fn`` around ``aux(trace, challenges) -> (DeviceMatrix | ndarray, exposed)``.  An exception
    inside becomes TS_ERR_INVALID and is kept in ``failure`` for the caller to re-raise after the call."""

    def fn(_user, _ctx, trace_h, challenges, n_challenges, aux_out, exposed_out):
        view = DeviceMatrix(ctx, C.c_void_p(trace_h))
        try:
            ch = np.array([challenges[k] for k in range(4 * n_challenges)], dtype=np.uint32)
            m, exposed = aux(view, ch)
            if not isinstance(m, DeviceMatrix):
                m = DeviceMatrix.upload(ctx, _u32(m))
            exposed = _u32(exposed if exposed is not None else [])
            if len(exposed) != air.n_exposed:
                raise ValueError(f"the aux source returned {len(exposed)} exposed words, the AIR has {air.n_exposed}")
            for k in range(len(exposed)):
                exposed_out[k] = int(exposed[k])
            aux_out[0] = m.h.value
            m.h = None  # consumed by the prover
            return 0
        except BaseException as e:  # nothing may unwind through the C frames
            failure.append(e)
            return 1
        finally:
            view.h = None  # the prover's trace: borrowed, never freed here

    return _lib.AUX_FN(fn)


def prove(config: StarkConfig, air, challenger: BfChallenger, trace, public_values, preprocessed=None,
          aux=None) -> Proof:
    """``uni_stark::prove`` (reference uni-stark/src/prover.rs:25-35).

    ``air`` is a ``BaseAir`` (captured symbolically like ``get_symbolic_constraints``) or an
    already ``CompiledAir``; ``trace`` an (n, w) array or a ``DeviceMatrix`` (consumed).
    ``preprocessed``: the ``PreprocessedKey`` of an AIR with preprocessed columns (``ts_prove_pre``; the proof
    is TSPF v3); None is ``ts_prove``.
    ``aux``: the aux source of an AIR with challenge-phase columns, a callable ``(trace: DeviceMatrix, challenges:
    ndarray of 4 * n_challenges words) -> (DeviceMatrix | ndarray, exposed words)`` called once after the trace is
    committed (``ts_prove_aux``; the proof is TSPF v4).  The trace it sees is the prover's: read it, do not keep it.
    An exception inside it ends the proof with TS_ERR_INVALID and is re-raised here.
    Both ``preprocessed`` and ``aux``: an AIR with both kinds of column (``ts_prove_pre_aux``; TSPF v5).
    """
    pcs = config.pcs
    ctx = pcs.ctx
    pis = _u32(public_values)
    if isinstance(air, BaseAir):
        air = CompiledAir(ctx, _air_tape_of(air, len(pis)))
    if not isinstance(trace, DeviceMatrix):
        trace = DeviceMatrix.upload(ctx, trace)
    n, w = trace.dims()
    out = _proof_buffer(ctx, _proof_capacity(n, w + air.preprocessed_width + air.aux_width, air.log_quotient_degree,
                                             pcs.fri) + air.n_exposed + 16)
    n_words = C.c_size_t()
    cfg = pcs.fri._c()
    has_key, has_aux = preprocessed is not None, aux is not None
    if has_key and has_aux:
        # one more Merkle path and batch header per query than _proof_capacity counts
        extra = pcs.fri.num_queries * (8 * (max(n, 1).bit_length() - 1 + pcs.fri.log_blowup) + 8)
        out = _proof_buffer(ctx, len(out) + extra)
    fn, key_args, aux_args = _single_call(ctx._l, "prove", has_key, has_aux)
    failure: list = []
    cb = _aux_callback(ctx, air, aux, failure) if has_aux else None
    rc = fn(ctx.h, C.byref(cfg), air.h, challenger.h, *key_args(preprocessed.data.h if has_key else None), trace.h,
            _p(pis) if len(pis) else None, len(pis), *aux_args(cb, None), _p(out), len(out), C.byref(n_words))
    if failure:
        raise failure[0]
    ctx.check(rc)
    return Proof(out[: n_words.value].copy())


@dataclass
class MultiTableOpening:
    """One table of a :class:`MultiProof`: its header words and its opened values."""
    log_degree: int
    width: int
    qd: int
    trace_local: np.ndarray      # (width, 4)
    trace_next: np.ndarray       # (width, 4)
    quotient_chunks: np.ndarray  # (qd, 4, 4)


class MultiProof:
    """A TSPF v6 proof (``ts_prove_multi``): several AIR tables of mixed heights under one trace commitment, one
    quotient commitment and one FRI proof.  ``words`` keeps the wire form; ``tables`` (a list of
    :class:`MultiTableOpening`), ``trace_commit``, ``quotient_commit``, ``commit_phase_commits``, ``query_proofs``,
    ``final_poly`` and ``pow_witness`` are parsed on first access, as ``Proof`` does.  ``fri_words`` are the
    FriProof words, ``opened_words`` the opened values in (round, matrix, point, column) order."""

    _FIELDS = ("tables", "trace_commit", "quotient_commit", "opened_words", "fri_words", "commit_phase_commits",
               "query_proofs", "final_poly", "pow_witness")
    _VERSION = 6
    _OPENING = MultiTableOpening

    def __init__(self, words):
        self.words = np.asarray(words, dtype=np.uint32)

    def __getattr__(self, name):  # only reached for attributes not set yet
        if name in self._FIELDS:
            self._parse()
            return self.__dict__[name]
        raise AttributeError(name)

    @classmethod
    def parse(cls, words) -> "MultiProof":
        """Eager form: raises ``ValueError`` on a malformed buffer."""
        pf = cls(words)
        pf._parse()
        return pf

    def _parse(self) -> None:
        """The one parser of TSPF v6, v7 and v8, keyed on ``_VERSION``: per table v7 adds (aux_width, n_exposed) to
        the header and v8 the preprocessed width; the aux root and the exposed words are there for v7 always and for
        v8 with an aux table; the opened values are every key matrix's, every aux matrix's, every trace's, then every
        chunk's."""
        w, V = self.words, self._VERSION
        take = _Words(w)
        magic, version, T = (int(x) for x in take(3))
        if magic != TSPF_MAGIC or version != V or not 1 <= T <= 64:
            raise ValueError(f"not a TSPF v{V} proof")
        SW = {6: 3, 7: 5, 8: 6}[V]
        shapes = [tuple(int(x) for x in row) + (0,) * (6 - SW) for row in take(SW * T).reshape(T, SW)]
        has_aux = V == 7 or any(aw for _, _, _, aw, _, _ in shapes)
        d = {"trace_commit": take(8), "aux_commit": take(8) if has_aux else None}
        d["exposed"] = take(sum(ne for _, _, _, aw, ne, _ in shapes if aw))
        d["bus_sum"] = (d["exposed"].reshape(-1, 4).astype(np.uint64).sum(axis=0) % np.uint64(P)).astype(np.uint32)
        d["quotient_commit"] = take(8)
        start = take.pos
        empty = (w[:0].reshape(0, 4),) * 2
        prep = [(take(4 * pw).reshape(-1, 4), take(4 * pw).reshape(-1, 4)) if pw else empty for *_, pw in shapes]
        aux = [(take(4 * aw).reshape(-1, 4), take(4 * aw).reshape(-1, 4)) if aw else empty
               for _, _, _, aw, _, _ in shapes]
        locals_ = [(take(4 * wd).reshape(-1, 4), take(4 * wd).reshape(-1, 4)) for _, wd, *_ in shapes]
        d["tables"], e = [], 0
        n_fields = len(dataclass_fields(self._OPENING))  # each opening class extends the one before
        for (ld, wd, qd, aw, ne, pw), (pl, pn), (al, an), (tl, tn) in zip(shapes, prep, aux, locals_):
            ex = d["exposed"][e:e + ne] if aw else w[:0]
            e += ne if aw else 0
            chunks = take(16 * qd).reshape(-1, 4, 4)
            d["tables"].append(self._OPENING(*(ld, wd, qd, tl, tn, chunks, aw, ne, al, an, ex, pw, pl, pn)[:n_fields]))
        d["opened_words"] = w[start:take.pos]
        d["fri_words"] = w[take.pos:]
        d.update(_parse_fri_tail(take, (8,)))
        self.__dict__.update({k: d[k] for k in self._FIELDS})


def _multi_capacity(shapes, fri: FriConfig) -> int:
    """Exact TSPF v6 words of a proof over ``shapes`` = [(n, w, log_quotient_degree), ...]."""
    logs = [max(n, 1).bit_length() - 1 + fri.log_blowup for n, _, _ in shapes]
    log_max, Q = max(logs), fri.num_queries
    R = log_max - fri.log_blowup
    n_chunks = sum(1 << lqd for _, _, lqd in shapes)
    w_total = sum(w for _, w, _ in shapes)
    per_q = 1 + (2 + len(shapes) + w_total + 8 * log_max) + (2 + n_chunks + 4 * n_chunks + 8 * log_max)
    per_q += sum(9 + 8 * (log_max - 1 - i) for i in range(R))
    return 3 + 3 * len(shapes) + 16 + 8 * w_total + 16 * n_chunks + 2 + 8 * R + Q * per_q + 5


def _multi_tables_c(ctx, airs, traces, pis, logups, struct):
    """The table array of the multi-table calls: ``struct`` is ``MultiTableC`` (``logups`` None) or
    ``MultiBusTableC``.  ``BaseAir``s are compiled on ``ctx`` and arrays uploaded to it.  Returns ``(airs, traces,
    tabs, keep)``; ``keep`` owns the public values and the specs ``tabs`` points at."""
    T = len(airs)
    airs = [CompiledAir(ctx, _air_tape_of(a, len(p))) if isinstance(a, BaseAir) else a for a, p in zip(airs, pis)]
    traces = [t if isinstance(t, DeviceMatrix) else DeviceMatrix.upload(ctx, t) for t in traces]
    tabs = (struct * max(T, 1))()
    keep = [pis]
    for k in range(T):
        tabs[k].struct_size = C.sizeof(struct)
        tabs[k].n_public = len(pis[k])
        tabs[k].air = airs[k].h
        tabs[k].trace = traces[k].h
        tabs[k].public_values = _p(pis[k]) if len(pis[k]) else None
        if logups is not None and logups[k] is not None:
            keep.append(logups[k]._spec_c())
            tabs[k].logup = C.pointer(keep[-1][0])
    return airs, traces, tabs, keep


def _verify_multi_call(name, config, airs, challenger, proof, public_values, key_root=None, check_bus=False):
    """``ts_verify_multi`` (nothing handed back), ``ts_verify_multi_bus`` and ``ts_verify_multi_key`` (``key_root``
    leads the tables; both hand back the exposed words and their sum)."""
    T = len(airs)
    if len(public_values) != T:
        raise ValueError(f"{name}: one public-value list per AIR")
    pis = [_u32(p) for p in public_values]
    airs = [CompiledAir(None, _air_tape_of(a, len(p))) if isinstance(a, BaseAir) else a for a, p in zip(airs, pis)]
    words = _u32(proof.words if isinstance(proof, MultiProof) else proof)
    root = None if key_root is None else _u32(key_root).reshape(-1)
    if root is not None and len(root) != 8:
        raise ValueError(f"{name}: the key root has eight words")
    l = _lib.lib()
    handles = (C.c_void_p * max(T, 1))(*[a.h for a in airs])
    pv = (_lib.u32p * max(T, 1))(*[_p(p) if len(p) else None for p in pis])
    n_pub = _u32([len(p) for p in pis] or [0])
    cfg = config.pcs.fri._c()
    verdict = C.c_int(-1)
    exposed, bus_sum = np.zeros(4 * max(T, 1), dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    outs = () if name == "verify_multi" else (_p(exposed), len(exposed), _p(bus_sum))
    rc = getattr(l, "ts_" + name)(C.byref(cfg), challenger.h, *(() if root is None else (_p(root),)), handles, T, pv,
                                  _p(n_pub), _p(words), len(words), *outs, C.byref(verdict))
    if rc:
        raise _lib.TsError(rc, (l.ts_last_error(None) or ("ts_" + name).encode()).decode())
    if verdict.value != 0:
        raise VerificationError(verdict.value)
    if not outs:
        return None
    if check_bus and bus_sum.any():
        raise ValueError(f"{name}: the exposed sums of the tables do not add up to zero: the bus does not balance")
    return exposed[: 4 * sum(1 for a in airs if a.aux_width)], bus_sum


def prove_multi(config: StarkConfig, airs, challenger: BfChallenger, traces, public_values) -> MultiProof:
    """``ts_prove_multi``: one proof over several plain AIR tables of mixed heights (TSPF v6).  ``airs``: one
    ``BaseAir`` or ``CompiledAir`` per table (no preprocessed, no aux columns); ``traces``: (n_t, w_t) arrays or
    ``DeviceMatrix`` (consumed); ``public_values``: one sequence per table.  The transcript observes the table
    count and every log-degree, commits all traces in one batch and all quotient chunks in another, and opens
    both in one FRI proof (include/tapstark.h)."""
    pcs = config.pcs
    ctx = pcs.ctx
    T = len(airs)
    if len(traces) != T or len(public_values) != T:
        raise ValueError("prove_multi: one trace and one public-value list per AIR")
    airs, traces, tabs, keep = _multi_tables_c(ctx, airs, traces, [_u32(p) for p in public_values], None,
                                               _lib.MultiTableC)
    shapes = [(*t.dims(), a.log_quotient_degree) for t, a in zip(traces, airs)]
    out = _proof_buffer(ctx, _multi_capacity(shapes, pcs.fri) if T else 1)
    n_words = C.c_size_t()
    cfg = pcs.fri._c()
    ctx.check(ctx._l.ts_prove_multi(ctx.h, C.byref(cfg), challenger.h, tabs, T, _p(out), len(out),
                                    C.byref(n_words)))
    del keep
    return MultiProof(out[: n_words.value].copy())


def verify_multi(config: StarkConfig, airs, challenger: BfChallenger, proof, public_values) -> None:
    """``ts_verify_multi``; host only, no GPU (host-only ``CompiledAir``s serve, as in ``verify``).  Raises
    ``VerificationError``; returns None on acceptance."""
    _verify_multi_call("verify_multi", config, airs, challenger, proof, public_values)


@dataclass
class MultiBusTableOpening(MultiTableOpening):
    """One table of a :class:`MultiBusProof`: what :class:`MultiTableOpening` holds, its aux header words and
    opened aux rows, and its four exposed words (its share of the bus sum); empty arrays for a plain table."""
    aux_width: int = 0
    n_exposed: int = 0
    aux_local: np.ndarray = None   # (aux_width, 4)
    aux_next: np.ndarray = None    # (aux_width, 4)
    exposed: np.ndarray = None     # (n_exposed,)


class MultiBusProof(MultiProof):
    """A TSPF v7 proof (``ts_prove_multi_bus``): a :class:`MultiProof` whose tables are tied by a LogUp bus.  Beside
    the fields of ``MultiProof`` (``tables`` holds :class:`MultiBusTableOpening`): ``aux_commit``, ``exposed`` (the
    exposed words, four per table with aux columns, in table order) and ``bus_sum`` (their EF4 sum over the tables:
    zero exactly when the bus balances)."""

    _FIELDS = MultiProof._FIELDS + ("aux_commit", "exposed", "bus_sum")
    _VERSION = 7
    _OPENING = MultiBusTableOpening


def _multi_bus_capacity(shapes, fri: FriConfig) -> int:
    """An upper bound (exact when the tallest table has aux columns) on the TSPF v7 words of a proof over
    ``shapes`` = [(n, w, log_quotient_degree, aux_width), ...]."""
    v6 = _multi_capacity([(n, w, lqd) for n, w, lqd, _ in shapes], fri)
    log_max = max(max(n, 1).bit_length() - 1 for n, *_ in shapes) + fri.log_blowup
    aux = [aw for *_, aw in shapes if aw]
    return v6 + 2 * len(shapes) + 8 + 4 * len(aux) + 8 * sum(aux) + fri.num_queries * (
        2 + len(aux) + sum(aux) + 8 * log_max)


def prove_multi_bus(config: StarkConfig, airs, challenger: BfChallenger, traces, public_values, logups) -> MultiBusProof:
    """``ts_prove_multi_bus``: ``prove_multi`` with a LogUp bus across the tables (TSPF v7).  ``logups``: per table
    the :class:`~tapstark_amd.air.LogUp` whose columns are the AIR's aux columns, or None for a plain table.  Gamma
    and beta are sampled once for every table; ``proof.bus_sum`` is zero exactly when everything sent on the bus
    is received (``verify_multi_bus`` checks it).  An AIR given as a ``BaseAir`` is compiled with the aux
    dimensions of its ``LogUp``."""
    pcs = config.pcs
    ctx = pcs.ctx
    T = len(airs)
    if len(traces) != T or len(public_values) != T or len(logups) != T:
        raise ValueError("prove_multi_bus: one trace, one public-value list and one LogUp (or None) per AIR")
    airs, traces, tabs, keep = _multi_tables_c(ctx, airs, traces, [_u32(p) for p in public_values], logups,
                                               _lib.MultiBusTableC)
    shapes = [(*t.dims(), a.log_quotient_degree, lg.aux_width if lg is not None else 0)
              for t, a, lg in zip(traces, airs, logups)]
    out = _proof_buffer(ctx, _multi_bus_capacity(shapes, pcs.fri) if T else 1)
    n_words = C.c_size_t()
    cfg = pcs.fri._c()
    ctx.check(ctx._l.ts_prove_multi_bus(ctx.h, C.byref(cfg), challenger.h, tabs, T, _p(out), len(out),
                                        C.byref(n_words)))
    del keep
    return MultiBusProof(out[: n_words.value].copy())


def verify_multi_bus(config: StarkConfig, airs, challenger: BfChallenger, proof, public_values, check_bus: bool = True):
    """``ts_verify_multi_bus``; host only.  Raises ``VerificationError`` on a rejected proof and, with ``check_bus``,
    ``ValueError`` when the exposed sums of the tables do not add up to zero (something sent on the bus is not
    received).  Returns ``(exposed, bus_sum)``: the exposed words, four per table with aux columns, and their sum."""
    return _verify_multi_call("verify_multi_bus", config, airs, challenger, proof, public_values, check_bus=check_bus)


@dataclass
class MultiKeyTableOpening(MultiBusTableOpening):
    """One table of a :class:`MultiKeyProof`: what :class:`MultiBusTableOpening` holds, its preprocessed width and the
    opened rows of its key matrix; empty arrays for a table without preprocessed columns."""
    preprocessed_width: int = 0
    preprocessed_local: np.ndarray = None   # (preprocessed_width, 4)
    preprocessed_next: np.ndarray = None    # (preprocessed_width, 4)


class MultiKeyProof(MultiBusProof):
    """A TSPF v8 proof (``ts_prove_multi_key``): a :class:`MultiBusProof` against a commit-once :class:`MultiKey`.
    ``tables`` holds :class:`MultiKeyTableOpening`; without any aux table ``aux_commit`` is None, ``exposed`` empty
    and ``bus_sum`` zero.  The key root is not in the proof."""

    _VERSION = 8
    _OPENING = MultiKeyTableOpening


class _BorrowedMatrix(DeviceMatrix):
    """A handle owned by another object (``owner`` is kept alive with it) and never freed from here."""

    def __init__(self, ctx, handle, owner):
        super().__init__(ctx, handle)
        self._owner = owner

    def __del__(self):
        pass


class MultiKey:
    """``ts_multi_key``: the preprocessed matrices of a multi-table proof, committed ONCE in one batch on their natural
    domains (mixed power-of-two heights).  Never consumed: one key serves any number of ``prove_multi_key`` calls on
    its context; ``root`` is what the verifier holds.  ``matrices``: arrays or ``DeviceMatrix`` (consumed).  With
    ``keep_values`` (default) the row-major inputs stay alive inside the key without a second copy and ``values(i)``
    lends matrix i for ``logup_build_multi(..., preprocessed=)``, ``logup_multiplicities_bus(..., table_preprocessed=)``
    and for ``("prep", c)`` terms inside the proof."""

    def __init__(self, config: "StarkConfig", matrices, keep_values: bool = True):
        pcs = config.pcs
        self.ctx = ctx = pcs.ctx
        self.h = None
        mats = [m if isinstance(m, DeviceMatrix) else DeviceMatrix.upload(ctx, _u32(m)) for m in matrices]
        handles = (C.c_void_p * max(len(mats), 1))(*[m.h for m in mats])
        cfg = pcs.fri._c()
        self.root = np.zeros(8, dtype=np.uint32)
        h = C.c_void_p()
        ctx.check(ctx._l.ts_multi_key_commit(ctx.h, C.byref(cfg), len(mats), handles, 1 if keep_values else 0,
                                             _p(self.root), C.byref(h)))
        self.h = h
        self.n = len(mats)
        self.keep_values = bool(keep_values)

    def info(self, i: int):
        """(height, width) of matrix ``i``."""
        hh, ww = C.c_uint64(), C.c_uint32()
        self.ctx.check(self.ctx._l.ts_multi_key_info(self.h, i, C.byref(hh), C.byref(ww)))
        return int(hh.value), int(ww.value)

    def values(self, i: int) -> DeviceMatrix:
        """The row-major values of matrix ``i``, borrowed from the key (``ts_multi_key_values``)."""
        h = C.c_void_p()
        rc = self.ctx._l.ts_multi_key_values(self.h, i, C.byref(h))
        if rc:
            raise _lib.TsError(rc, "ts_multi_key_values: no such matrix, or the key was made without keep_values")
        return _BorrowedMatrix(self.ctx, h, self)

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx._l.ts_multi_key_free(self.ctx.h, self.h)
        except Exception:
            pass


def _multi_key_capacity(shapes, fri: FriConfig) -> int:
    """An upper bound (exact when the tallest table has a key matrix) on the TSPF v8 words of a proof over ``shapes`` =
    [(n, w, log_quotient_degree, aux_width, preprocessed_width), ...]."""
    aux = [aw for *_, aw, _ in shapes if aw]
    log_max = max(max(n, 1).bit_length() - 1 for n, *_ in shapes) + fri.log_blowup
    if aux:
        v7 = _multi_bus_capacity([sh[:4] for sh in shapes], fri)
    else:  # no aux root, no exposed words, no aux round
        v7 = _multi_capacity([sh[:3] for sh in shapes], fri) + 2 * len(shapes)
    pre = [pw for *_, pw in shapes if pw]
    return v7 + len(shapes) + 8 * sum(pre) + fri.num_queries * (2 + len(pre) + sum(pre) + 8 * log_max)


def prove_multi_key(config: StarkConfig, key: MultiKey, airs, challenger: BfChallenger, traces, public_values,
                    logups) -> MultiKeyProof:
    """``ts_prove_multi_key``: ``prove_multi_bus`` against a commit-once key (TSPF v8).  The i-th AIR with preprocessed
    columns, in table order, reads matrix i of ``key``.  ``logups`` as in ``prove_multi_bus``; their terms may be
    ``("prep", c)``: column c of that table's key matrix (the key then keeps its values).  Without any aux table the
    challenge phase is skipped."""
    pcs = config.pcs
    ctx = pcs.ctx
    T = len(airs)
    if len(traces) != T or len(public_values) != T or len(logups) != T:
        raise ValueError("prove_multi_key: one trace, one public-value list and one LogUp (or None) per AIR")
    airs, traces, tabs, keep = _multi_tables_c(ctx, airs, traces, [_u32(p) for p in public_values], logups,
                                               _lib.MultiBusTableC)
    shapes = [(*t.dims(), a.log_quotient_degree, lg.aux_width if lg is not None else 0, a.preprocessed_width)
              for t, a, lg in zip(traces, airs, logups)]
    out = _proof_buffer(ctx, _multi_key_capacity(shapes, pcs.fri) if T else 1)
    n_words = C.c_size_t()
    cfg = pcs.fri._c()
    ctx.check(ctx._l.ts_prove_multi_key(ctx.h, C.byref(cfg), challenger.h, key.h if key is not None else None, tabs, T,
                                        _p(out), len(out), C.byref(n_words)))
    del keep
    return MultiKeyProof(out[: n_words.value].copy())


def verify_multi_key(config: StarkConfig, key_root, airs, challenger: BfChallenger, proof, public_values,
                     check_bus: bool = True):
    """``ts_verify_multi_key``; host only.  ``key_root``: the eight words of the key's commitment (``MultiKey.root``).
    Raises ``VerificationError`` on a rejected proof and, with ``check_bus``, ``ValueError`` when the exposed sums do
    not add up to zero.  Returns ``(exposed, bus_sum)`` as ``verify_multi_bus`` does; both empty / zero without an aux
    table."""
    return _verify_multi_call("verify_multi_key", config, airs, challenger, proof, public_values, key_root=key_root,
                              check_bus=check_bus)


def check_multi(key, airs, traces, public_values, logups, challenges, ctx: Context | None = None):
    """``ts_check_multi``: the debug counterpart of ``prove_multi_bus`` / ``prove_multi_key``, to be run before them.
    ``key``: the :class:`MultiKey` (with kept values) or None when no AIR has preprocessed columns; ``traces`` are NOT
    consumed (arrays are uploaded to ``ctx``); ``challenges``: any gamma and beta, eight canonical words.  Builds the
    LogUp columns, checks every table's constraints in order and then the exact balance of the bus.  Returns
    ``(bad_table, first_violation, report)``: the first table with a violated constraint and what
    ``check_constraints`` gives for it (both -1 when all hold), and the :class:`~tapstark_amd.air.BusReport` of
    ``bus_check``."""
    from .air import BusReport
    T = len(airs)
    if len(traces) != T or len(public_values) != T or len(logups) != T:
        raise ValueError("check_multi: one trace, one public-value list and one LogUp (or None) per AIR")
    if ctx is None:
        ctx = key.ctx if key is not None else next((t.ctx for t in traces if isinstance(t, DeviceMatrix)), None)
    ctx = ctx or default_context()
    airs, traces, tabs, keep = _multi_tables_c(ctx, airs, traces, [_u32(p) for p in public_values], logups,
                                               _lib.MultiBusTableC)
    ch = _u32(challenges).reshape(-1)
    if len(ch) != 8:
        raise ValueError("check_multi: two challenges (eight words)")
    bad, fv = C.c_int32(-1), C.c_int64(-1)
    rep = _lib.BusReportC(struct_size=C.sizeof(_lib.BusReportC))
    shares = (_lib.BusShareC * max(T, 1))()
    ctx.check(ctx._l.ts_check_multi(ctx.h, key.h if key is not None else None, tabs, T, _p(ch), C.byref(bad),
                                    C.byref(fv), C.byref(rep), shares))
    del keep
    return int(bad.value), int(fv.value), BusReport._from_c(rep, shares, T)


def prove_stream(lanes, traces, lane_of, public_values, gate_ms: float = 0.0, want_times: bool = True):
    """``ts_prove_stream``: ``len(traces)`` independent proofs on the contexts of ``lanes`` = [(StarkConfig,
    CompiledAir), ...] (one context each, same device, same FriConfig), one host thread per lane INSIDE the
    library; proof i runs on lane ``lane_of[i]`` with ``traces[i]`` (a DeviceMatrix made on that lane's context;
    consumed) and a fresh challenger.  Returns (Proof of the highest index, start_ms array, wall_ms array)."""
    n_l, n = len(lanes), len(traces)
    l = _lib.lib()
    ctxs, airs, fri = _lane_arrays(lanes)
    mats = (C.c_void_p * max(n, 1))(*[t.h for t in traces])
    lo = _u32(lane_of)
    pis = _u32(public_values)
    cfg = fri._c()
    # sized for the proof that comes back: that of the highest index
    cap = _proof_capacity(*traces[-1].dims(), _lane_lqd(lanes, lane_of[-1]), fri) if n else 1
    out = _proof_buffer(lanes[0][0].pcs.ctx, cap)
    n_words = C.c_size_t()
    st = np.zeros(max(n, 1), dtype=np.float64)
    wl = np.zeros(max(n, 1), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    rc = l.ts_prove_stream(ctxs, airs, n_l, C.byref(cfg), mats, _p(lo), n, _p(pis) if len(pis) else None, len(pis),
                           float(gate_ms), _p(out), len(out), C.byref(n_words),
                           st.ctypes.data_as(dp) if want_times else None, wl.ctypes.data_as(dp) if want_times else None)
    if rc:  # the failing lane's context holds the message
        msg = next(filter(None, (_lane_error(lanes, k) for k in range(n_l))), "ts_prove_stream")
        raise _lib.TsError(rc, msg)
    return Proof(out[: n_words.value].copy()), st[:n], wl[:n]


def _proof_capacity(n: int, w: int, log_quotient_degree: int, fri: FriConfig) -> int:
    """Upper bound on the TSPF v1 words of one proof of an n x w trace."""
    log_N = max(n, 1).bit_length() - 1 + fri.log_blowup
    qd = 1 << log_quotient_degree
    R = log_N - fri.log_blowup
    Q = fri.num_queries
    # (three Merkle paths of the input proof: a TSPF v3 proof opens the preprocessed key's round as well)
    return 64 + 8 * w + 16 * qd + 8 * R + Q * (18 + w + 5 * qd + 3 * 8 * log_N + R * (9 + 8 * log_N))


def _proof_buffer(ctx, cap: int) -> np.ndarray:
    """One output buffer per context, kept for its lifetime (a context is driven by one thread): no
    half-megabyte allocation, zero-fill and release per proof."""
    out = getattr(ctx, "_proof_buf", None)
    if out is None or len(out) < cap:
        out = ctx._proof_buf = np.zeros(cap, dtype=np.uint32)
    return out


def _lane_arrays(lanes):
    """The ``ctxs`` / ``airs`` arrays of a lane call and its FriConfig (that of lane 0: all lanes share it)."""
    ctxs = (C.c_void_p * len(lanes))(*[conf.pcs.ctx.h for conf, _ in lanes])
    airs = (C.c_void_p * len(lanes))(*[a.h for _, a in lanes])
    return ctxs, airs, lanes[0][0].pcs.fri


def _lane_lqd(lanes, lane: int) -> int:
    """log_quotient_degree of a lane's AIR (0 for a lane index the library will refuse)."""
    return lanes[lane][1].log_quotient_degree if 0 <= lane < len(lanes) else 0


def _lane_error(lanes, lane: int) -> str:
    """The error text of a lane's context ('' if it holds none)."""
    if not 0 <= lane < len(lanes):
        return f"lane {lane} out of range"
    return (_lib.lib().ts_last_error(lanes[lane][0].pcs.ctx.h) or b"").decode()


@dataclass
class BatchResult:
    """What ``prove_batch`` returns, one entry per item: ``proofs[i]`` is None unless ``status[i]`` is 0
    (-1 = not attempted: an earlier item of its lane hit a device error); ``n_words[i]`` is also set on
    TS_ERR_BUFFER; ``digests`` (n x 8 words: Blake3 of the proof words) only with ``digests=True``;
    ``final_states`` (n x 34) is ``BfChallenger.state()`` of the challenger after the proof; ``rc`` is the
    call's status (that of the lowest-index failed item); ``errors[i]`` the text of item i's lane context."""
    rc: int
    proofs: list
    status: np.ndarray
    n_words: np.ndarray
    digests: np.ndarray | None
    final_states: np.ndarray
    start_ms: np.ndarray
    wall_ms: np.ndarray
    errors: list = field(default_factory=list)


def _is_vector(v) -> bool:
    return v.ndim == 1 if isinstance(v, np.ndarray) else all(np.isscalar(x) for x in v)


def _per_item(value, n: int, is_single, what: str) -> list:
    if value is None or is_single(value):
        return [value] * n
    value = list(value)
    if len(value) != n:
        raise ValueError(f"prove_batch: {len(value)} {what} for {n} traces")
    return value


def prove_batch(lanes, traces, lane_of, public_values=None, challengers=None, gate_ms: float = 0.0,
                digests: bool = False, check: bool = True, _struct_size: int | None = None,
                _cap_words=None) -> BatchResult:
    """``ts_prove_batch``: ``len(traces)`` distinct statements (reference uni-stark/src/prover.rs:25-39, one
    call each) on the contexts of ``lanes`` = [(StarkConfig, CompiledAir), ...] (one context each, same device,
    same FriConfig; the AIRs may differ), one host thread per lane inside the library, every proof returned.

    ``traces[i]``: a ``DeviceMatrix`` made on lane ``lane_of[i]``'s context (consumed), a ``PinnedHostMatrix``
    or an (h, w) uint32 array (uploaded on the lane's stream just before its proof).  ``public_values``: one
    vector for every item or one per item; ``challengers``: None (a fresh ``BfChallenger()``), one
    ``BfChallenger`` for every item or one (or None) per item -- a clone is used, the objects are not modified.
    With ``check`` a failed item raises ``TsError`` once every item has run; otherwise see ``status``.
    (``_struct_size`` / ``_cap_words``: test hooks -- another struct layout, per-item proof buffer sizes.)"""
    n, n_l = len(traces), len(lanes)
    lane_of = [int(x) for x in lane_of]
    if len(lane_of) != n:
        raise ValueError(f"prove_batch: {len(lane_of)} lane indices for {n} traces")
    pis = [np.zeros(0, dtype=np.uint32) if p is None else _u32(p).reshape(-1)
           for p in _per_item(public_values, n, _is_vector, "public-value vectors")]
    chals = _per_item(challengers, n, lambda v: isinstance(v, BfChallenger), "challengers")
    caps = _per_item(_cap_words, n, lambda v: isinstance(v, int), "buffer sizes")
    if not lanes:
        raise ValueError("prove_batch: no lanes")
    l = _lib.lib()
    ctxs, airs, fri = _lane_arrays(lanes)
    cfg = fri._c()
    items = (_lib.BatchItemC * max(n, 1))()
    keep, outs = [], []  # host buffers that must outlive the call
    for i, t in enumerate(traces):
        it = items[i]
        it.struct_size = C.sizeof(_lib.BatchItemC) if _struct_size is None else _struct_size
        it.lane = lane_of[i]
        it.status = -1
        if isinstance(t, DeviceMatrix):
            it.trace = t.h
            h, w = t.dims()
        elif isinstance(t, PinnedHostMatrix):
            it.host_trace = t.ptr
            h, w = t.shape
        else:
            a = _u32(t)
            if a.ndim != 2:
                raise ValueError(f"prove_batch: trace {i} is not a 2-D array")
            keep.append(a)
            it.host_trace = a.ctypes.data
            h, w = a.shape
        it.height, it.width = h, w
        it.n_public = len(pis[i])
        it.public_values = pis[i].ctypes.data if len(pis[i]) else None
        it.challenger = chals[i].h if chals[i] is not None else None
        cap = _proof_capacity(h, w, _lane_lqd(lanes, lane_of[i]), fri) if caps[i] is None else caps[i]
        out = np.zeros(max(cap, 1), dtype=np.uint32)
        outs.append(out)
        it.proof_out = out.ctypes.data
        it.cap_words = cap
    rc = l.ts_prove_batch(ctxs, airs, n_l, C.byref(cfg), items, n, float(gate_ms),
                          _lib.BATCH_DIGEST if digests else 0)
    status = np.array([items[i].status for i in range(n)], dtype=np.int32)
    if rc and (status == -1).all():  # the whole call was refused: no item was touched
        msg = "ts_prove_batch refused the call (null arrays, lane count, a repeated context, FriConfig or struct_size)"
        raise _lib.TsError(rc, msg)
    n_words = np.array([items[i].n_words for i in range(n)], dtype=np.int64)
    errors = [None if s == 0 else _lane_error(lanes, lane_of[i]) for i, s in enumerate(status)]
    res = BatchResult(
        rc=int(rc),
        proofs=[Proof(outs[i][: n_words[i]].copy()) if status[i] == 0 else None for i in range(n)],
        status=status, n_words=n_words,
        digests=np.array([list(items[i].proof_blake3) for i in range(n)], dtype=np.uint32).reshape(n, 8)
        if digests else None,
        final_states=np.array([list(items[i].final_state) for i in range(n)], dtype=np.uint32).reshape(n, 34),
        start_ms=np.array([items[i].start_ms for i in range(n)]),
        wall_ms=np.array([items[i].wall_ms for i in range(n)]),
        errors=errors)
    if check and rc:
        bad = next(i for i in range(n) if status[i] != 0)
        raise _lib.TsError(int(status[bad]), f"item {bad}: {errors[bad] or 'not attempted'}")
    return res


@dataclass
class BatchLookupResult(BatchResult):
    """``BatchResult`` of ``prove_batch_lookup``: also ``exposed[i]`` (the exposed words of item i's proof, None
    unless ``status[i]`` is 0) and ``n_missing[i]`` / ``first_missing[i]`` (those of the item's first multiplicity
    fill that missed; 0 and ``2**64 - 1`` when none did)."""
    exposed: list = field(default_factory=list)
    n_missing: np.ndarray | None = None
    first_missing: np.ndarray | None = None


def _per_lane(value, n_lanes: int, what: str) -> list:
    if value is None:
        return [None] * n_lanes
    value = list(value)
    if len(value) != n_lanes:
        raise ValueError(f"prove_batch_lookup: {len(value)} {what} for {n_lanes} lanes")
    return value


def prove_batch_lookup(lanes, traces, lane_of, public_values=None, challengers=None, keys=None, logups=None,
                       fills=None, gate_ms: float = 0.0, digests: bool = False, check: bool = True,
                       _struct_size: int | None = None, _cap_words=None, _edit_items=None) -> BatchLookupResult:
    """``ts_prove_batch_lookup``: ``prove_batch`` for AIRs with preprocessed columns, challenge-phase columns or
    both.  Every proof is the TSPF v5 proof ``prove(..., preprocessed=key, aux=source)`` gives on the lane's context.

    ``lanes``, ``traces``, ``lane_of``, ``public_values``, ``challengers``, ``gate_ms``, ``digests``, ``check``: as
    ``prove_batch``.  Per LANE: ``keys[l]`` a ``PreprocessedKey`` made on the lane's context or None (its ``.values``,
    when kept, is the table that ``("prep", c)`` terms read); ``logups[l]`` a ``LogUp`` or None, the aux source of
    every item of lane l, run by the library on the lane's stream (no Python callback per proof); ``fills[l]`` a
    list of ``LogUp.mult_spec(...)`` dicts or None: the multiplicity columns filled in the resident trace of every
    item of lane l after its upload and before its commit.  A device trace of a lane with a ``LogUp`` or fills must
    be row-major.  (``_struct_size`` / ``_cap_words``: test hooks, as in ``prove_batch``; ``_edit_items(items,
    lanes_c)``: a test hook that may change the ctypes records before the call.)"""
    from .air import mult_spec_c

    n, n_l = len(traces), len(lanes)
    lane_of = [int(x) for x in lane_of]
    if len(lane_of) != n:
        raise ValueError(f"prove_batch_lookup: {len(lane_of)} lane indices for {n} traces")
    pis = [np.zeros(0, dtype=np.uint32) if p is None else _u32(p).reshape(-1)
           for p in _per_item(public_values, n, _is_vector, "public-value vectors")]
    chals = _per_item(challengers, n, lambda v: isinstance(v, BfChallenger), "challengers")
    caps = _per_item(_cap_words, n, lambda v: isinstance(v, int), "buffer sizes")
    if not lanes:
        raise ValueError("prove_batch_lookup: no lanes")
    keys = _per_lane(keys, n_l, "keys")
    logups = _per_lane(logups, n_l, "LogUp specs")
    fills = _per_lane(fills, n_l, "fill lists")
    l = _lib.lib()
    ctxs, airs, fri = _lane_arrays(lanes)
    cfg = fri._c()
    keep, outs, exps = [], [], []  # host buffers that must outlive the call
    lanes_c = (_lib.BatchLaneC * n_l)()
    specs, mults = [None] * n_l, [None] * n_l
    for k in range(n_l):
        lanes_c[k].struct_size = C.sizeof(_lib.BatchLaneC)
        if keys[k] is not None:
            lanes_c[k].key = keys[k].data.h
            if keys[k].values is not None:
                lanes_c[k].key_values = keys[k].values.h
        if logups[k] is not None:
            specs[k] = logups[k]._spec_c()
        if fills[k]:
            made = [mult_spec_c(**f) for f in fills[k]]
            arr = (_lib.LogupMultSpecC * len(made))(*[m[0] for m in made])
            mults[k] = (arr, made)
    items = (_lib.BatchLookupItemC * max(n, 1))()
    for i, t in enumerate(traces):
        it = items[i]
        it.struct_size = C.sizeof(_lib.BatchLookupItemC) if _struct_size is None else _struct_size
        lane = lane_of[i]
        it.lane = lane
        it.status = -1
        if isinstance(t, DeviceMatrix):
            it.trace = t.h
            h, w = t.dims()
        elif isinstance(t, PinnedHostMatrix):
            it.host_trace = t.ptr
            h, w = t.shape
        else:
            a = _u32(t)
            if a.ndim != 2:
                raise ValueError(f"prove_batch_lookup: trace {i} is not a 2-D array")
            keep.append(a)
            it.host_trace = a.ctypes.data
            h, w = a.shape
        it.height, it.width = h, w
        it.n_public = len(pis[i])
        it.public_values = pis[i].ctypes.data if len(pis[i]) else None
        it.challenger = chals[i].h if chals[i] is not None else None
        air = lanes[lane][1] if 0 <= lane < n_l else None
        if air is not None:
            if specs[lane] is not None:
                it.logup = C.pointer(specs[lane][0])
            if mults[lane] is not None:
                it.mult = mults[lane][0]
                it.n_mult = len(mults[lane][0])
        n_exp = air.n_exposed if air is not None else 0
        if caps[i] is not None:
            cap = caps[i]
        else:  # as prove() sizes the buffer of a pre+aux proof
            pw, aw = (air.preprocessed_width, air.aux_width) if air is not None else (0, 0)
            log_N = max(h, 1).bit_length() - 1 + fri.log_blowup
            cap = (_proof_capacity(h, w + pw + aw, _lane_lqd(lanes, lane), fri) + n_exp + 16 +
                   fri.num_queries * (8 * log_N + 8))
        out = np.zeros(max(cap, 1), dtype=np.uint32)
        outs.append(out)
        it.proof_out = out.ctypes.data
        it.cap_words = cap
        ex = np.zeros(max(n_exp, 1), dtype=np.uint32)
        exps.append(ex)
        it.exposed_out = ex.ctypes.data
        it.cap_exposed = n_exp
    if _edit_items is not None:
        hold = _edit_items(items, lanes_c)  # noqa: F841  (what the hook made stays alive over the call)
    rc = l.ts_prove_batch_lookup(ctxs, airs, lanes_c, n_l, C.byref(cfg), items, n, float(gate_ms),
                                 _lib.BATCH_DIGEST if digests else 0)
    del keep, specs, mults
    status = np.array([items[i].status for i in range(n)], dtype=np.int32)
    if rc and (status == -1).all():  # the whole call was refused: no item was touched
        msg = ("ts_prove_batch_lookup refused the call (null arrays, lane count, a repeated context, FriConfig, "
               "struct_size or a missing lane array)")
        raise _lib.TsError(rc, msg)
    n_words = np.array([items[i].n_words for i in range(n)], dtype=np.int64)
    errors = [None if s == 0 else _lane_error(lanes, lane_of[i]) for i, s in enumerate(status)]
    res = BatchLookupResult(
        rc=int(rc),
        proofs=[Proof(outs[i][: n_words[i]].copy()) if status[i] == 0 else None for i in range(n)],
        status=status, n_words=n_words,
        digests=np.array([list(items[i].proof_blake3) for i in range(n)], dtype=np.uint32).reshape(n, 8)
        if digests else None,
        final_states=np.array([list(items[i].final_state) for i in range(n)], dtype=np.uint32).reshape(n, 34),
        start_ms=np.array([items[i].start_ms for i in range(n)]),
        wall_ms=np.array([items[i].wall_ms for i in range(n)]),
        errors=errors,
        exposed=[exps[i][: items[i].n_exposed].copy() if status[i] == 0 else None for i in range(n)],
        n_missing=np.array([items[i].n_missing for i in range(n)], dtype=np.uint64),
        first_missing=np.array([items[i].first_missing for i in range(n)], dtype=np.uint64))
    if check and rc:
        bad = next(i for i in range(n) if status[i] != 0)
        raise _lib.TsError(int(status[bad]), f"item {bad}: {errors[bad] or 'not attempted'}")
    return res


def prove_sharded(config: StarkConfig, air, challenger: BfChallenger, trace_rows, public_values,
                  comm, min_local_log: int = 0, trace_replicated: bool = False,
                  local_quotient: bool = False, _options_struct_size: int | None = None) -> Proof:
    """One proof over ``comm.world`` GPUs (``ts_prove_sharded``).

    Every rank calls this with its own context, a challenger in the same state and its row slice
    ``trace_rows`` = natural rows [g n/G, (g+1) n/G) of the trace; every rank gets the whole proof,
    bit-identical to :func:`prove` on the whole trace.  ``comm`` is a ``dist.TorchComm``.
    ``trace_replicated``: ``trace_rows`` is the whole trace on every rank (no all-gather of it).
    ``local_quotient``: every rank computes the quotient on its own cosets (no chunk broadcast; for a
    trace that violates its constraints all ranks fall back to the broadcast path, so the proof is
    :func:`prove`'s for every trace -- ``ts_shard_options.local_quotient`` in include/tapstark.h).
    """
    pcs = config.pcs
    ctx = pcs.ctx
    pis = _u32(public_values)
    if isinstance(air, BaseAir):
        air = CompiledAir(ctx, air_tape(air, len(pis)))
    if not isinstance(trace_rows, DeviceMatrix):
        trace_rows = DeviceMatrix.upload(ctx, trace_rows)
    n_loc, w = trace_rows.dims()
    n = n_loc if trace_replicated else n_loc * comm.world
    cap = _proof_capacity(n, w, air.log_quotient_degree, pcs.fri)
    out = np.zeros(cap, dtype=np.uint32)
    n_words = C.c_size_t()
    cfg = pcs.fri._c()
    pis_p = _p(pis) if len(pis) else None
    # (_options_struct_size: test hook -- a caller built against another layout of ts_shard_options)
    opts = _lib.ShardOptionsC(C.sizeof(_lib.ShardOptionsC) if _options_struct_size is None else _options_struct_size,
                              min_local_log, int(trace_replicated), int(local_quotient))
    rc = ctx._l.ts_prove_sharded(ctx.h, C.byref(cfg), C.byref(comm.c), air.h, challenger.h,
                                 trace_rows.h, pis_p, len(pis), C.byref(opts), _p(out), cap,
                                 C.byref(n_words))
    if rc == 7 and getattr(comm, "error", None):
        raise RuntimeError("communicator callback failed:\n" + comm.error)
    ctx.check(rc)
    return Proof(out[: n_words.value].copy())


VERIFY_ERRORS = {0: "Ok", 1: "InvalidProofShape", 2: "InvalidOpeningArgument(InvalidProofShape)",
                 3: "InvalidOpeningArgument(InvalidPowWitness)", 4: "InvalidOpeningArgument(InputError)",
                 5: "InvalidOpeningArgument(CommitPhaseMmcsError)",
                 6: "InvalidOpeningArgument(FinalPolyMismatch)", 7: "OodEvaluationMismatch",
                 8: "folded evaluation mismatch", 9: "malformed proof"}


class VerificationError(Exception):
    """reference uni-stark/src/verifier.rs:163-171 / fri/src/error.rs:21-29"""

    def __init__(self, code: int):
        super().__init__(VERIFY_ERRORS.get(code, str(code)))
        self.code = code


def verify(config: StarkConfig, air, challenger: BfChallenger, proof, public_values, preprocessed_root=None):
    """``uni_stark::verify`` (reference uni-stark/src/verifier.rs:19-25); host only, no GPU.
    Raises ``VerificationError``; returns None on acceptance (``Ok(())``).
    ``preprocessed_root``: the root of the ``PreprocessedKey`` a TSPF v3 proof was made against
    (``ts_verify_pre``); None is ``ts_verify``.
    A TSPF v4 proof (``ts_prove_aux``) goes to ``ts_verify_aux``, and its exposed words are returned: the statement
    about them (``LogUp.verify``: the sum is zero) is the caller's to check.  A TSPF v5 proof (``ts_prove_pre_aux``)
    with its ``preprocessed_root`` goes to ``ts_verify_pre_aux`` and returns its exposed words likewise."""
    words = _u32(proof.words if isinstance(proof, Proof) else proof)
    version = int(words[1]) if len(words) >= 2 and words[0] == TSPF_MAGIC else 0
    has_key = preprocessed_root is not None
    return _verify_call(has_key, version == (5 if has_key else 4), config, air, challenger, words, public_values,
                        preprocessed_root)


def _verify_call(has_key: bool, has_aux: bool, config, air, challenger, words, public_values, preprocessed_root):
    """One ``ts_verify[_pre][_aux]`` call: the exposed words from the entry points that hand them back, else None."""
    pis = _u32(public_values)
    if isinstance(air, BaseAir):
        air = CompiledAir(None, _air_tape_of(air, len(pis)))
    l = _lib.lib()
    fn, key_args, aux_args = _single_call(l, "verify", has_key, has_aux)
    cfg = config.pcs.fri._c()
    verdict = C.c_int(-1)
    exposed = np.zeros(air.n_exposed, dtype=np.uint32) if has_aux else None
    rc = fn(C.byref(cfg), air.h, challenger.h,
            *key_args(_p(_u32(preprocessed_root)) if preprocessed_root is not None else None), _p(words), len(words),
            _p(pis) if len(pis) else None, len(pis),
            *aux_args(_p(exposed) if has_aux and len(exposed) else None, len(exposed) if has_aux else 0),
            C.byref(verdict))
    if rc and verdict.value <= 0:  # (a proof of another version or width is refused WITH a verdict)
        raise _lib.TsError(rc, (l.ts_last_error(None) or b"ts_verify").decode())
    if verdict.value != 0:
        raise VerificationError(verdict.value)
    return exposed


def verify_pre_aux(config: StarkConfig, air, challenger: BfChallenger, proof, public_values, preprocessed_root=None):
    """``ts_verify_pre_aux`` whatever the AIR's widths: the verifier of every ``prove_batch_lookup`` proof (TSPF v5
    also for an AIR without a key, which ``verify`` routes there only together with a root).  ``preprocessed_root``
    is None exactly for an AIR without preprocessed columns.  Returns the exposed words; raises as ``verify``."""
    words = _u32(proof.words if isinstance(proof, Proof) else proof)
    return _verify_call(True, True, config, air, challenger, words, public_values, preprocessed_root)


def check_constraints(air, trace, public_values, ctx: Context | None = None, preprocessed=None, aux=None,
                      challenges=None, exposed=None) -> int:
    """reference uni-stark/src/check_constraints.rs:11-39 on the GPU.  Returns -1 if every
    constraint holds on every row, else ``row * 65536 + constraint_index`` of the first failure.
    ``preprocessed``: the (n, P) matrix of an AIR with preprocessed columns (``ts_check_constraints_pre``).
    ``aux``, ``challenges``, ``exposed``: the (n, aux_width) aux matrix of an AIR with challenge-phase columns, the
    challenge words it was built for and its exposed words (``ts_check_constraints_aux``).  Both ``preprocessed``
    and ``aux``: an AIR with both kinds of column (``ts_check_constraints_pre_aux``)."""
    ctx = ctx or default_context()
    pis = _u32(public_values)
    if isinstance(air, BaseAir):
        air = CompiledAir(ctx, _air_tape_of(air, len(pis)))
    if not isinstance(trace, DeviceMatrix):
        trace = DeviceMatrix.upload(ctx, trace)
    out = C.c_int64(-1)
    has_key, has_aux = _side_arguments(preprocessed, aux, challenges, exposed)
    fn, key_args, aux_args = _single_call(ctx._l, "check_constraints", has_key, has_aux)
    if has_key and not isinstance(preprocessed, DeviceMatrix):
        preprocessed = DeviceMatrix.upload(ctx, _u32(preprocessed))
    if aux is not None and not isinstance(aux, DeviceMatrix):
        aux = DeviceMatrix.upload(ctx, _u32(aux))
    ctx.check(fn(ctx.h, air.h, *key_args(preprocessed.h if has_key else None),
                 *aux_args(aux.h if aux is not None else None), trace.h, _p(pis) if len(pis) else None, len(pis),
                 *aux_args(*_challenge_words(challenges, exposed)), C.byref(out)))
    return int(out.value)
