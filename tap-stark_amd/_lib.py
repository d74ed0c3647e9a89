"""ctypes loader of the C-ABI HIP library (include/tapstark.h).

There is no CPU fallback: if the library is missing or no HIP device is present, every product
entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# TS_LIB_PATH points the binding at another build of the same library (same-box A/B of kernels)
LIB_PATH = os.environ.get("TS_LIB_PATH") or os.path.join(PKG, "lib", "libtapstark_hip.so")

u32p = C.POINTER(C.c_uint32)
voidpp = C.POINTER(C.c_void_p)

# every symbol include/tapstark.h declares (tests check the built library exports all of them)
ABI_SYMBOLS = [
    "ts_abi_version", "ts_device_count", "ts_ctx_create", "ts_ctx_destroy", "ts_last_error", "ts_ctx_synchronize",
    "ts_ctx_stream", "ts_ctx_set_timing", "ts_ctx_take_timings", "ts_ctx_set_replay", "ts_ctx_set_kernel_timing",
    "ts_ctx_take_kernel_timings", "ts_ctx_graph_stats", "ts_ctx_stat", "ts_matrix_upload",
    "ts_matrix_from_device", "ts_trace_fibonacci", "ts_trace_synth_mul", "ts_trace_synth_ext", "ts_matrix_dims", "ts_matrix_download", "ts_matrix_free",
    "ts_air_compile", "ts_air_compile_opts", "ts_air_segment_plan", "ts_air_info", "ts_air_is_jit", "ts_air_jit_wait", "ts_air_free", "ts_air_program", "ts_air_jit_source", "ts_air_jit_compile", "ts_pcs_commit", "ts_mmcs_commit", "ts_pcs_data_lde",
    "ts_pcs_data_info", "ts_pcs_data_matrix_info", "ts_pcs_data_digests", "ts_pcs_open_batch", "ts_pcs_data_free",
    "ts_quotient_chunks", "ts_pcs_open_reduce", "ts_pcs_open", "ts_pcs_verify", "ts_fri_prove", "ts_fri_verify", "ts_fri_fold", "ts_fri_fold_device", "ts_chal_new", "ts_chal_clone",
    "ts_chal_free", "ts_chal_observe", "ts_chal_observe_commitment", "ts_chal_sample",
    "ts_chal_sample_bits", "ts_chal_check_witness", "ts_chal_grind", "ts_chal_state", "ts_prove", "ts_prove_stream", "ts_prove_batch", "ts_prove_sharded", "ts_verify", "ts_check_constraints",
    "ts_air_preprocessed_width", "ts_quotient_chunks_pre", "ts_prove_pre", "ts_verify_pre", "ts_check_constraints_pre",
    "ts_air_aux_info", "ts_quotient_chunks_aux", "ts_check_constraints_aux", "ts_prove_aux", "ts_verify_aux",
    "ts_logup_aux_width", "ts_logup_aux_build", "ts_logup_aux_build_pre",
    "ts_logup_multiplicities",
    "ts_prove_pre_aux", "ts_verify_pre_aux", "ts_quotient_chunks_pre_aux", "ts_check_constraints_pre_aux",
    "ts_prove_batch_lookup",
    "ts_prove_multi", "ts_verify_multi",
    "ts_prove_multi_bus", "ts_verify_multi_bus", "ts_logup_aux_build_multi", "ts_logup_multiplicities_bus",
    "ts_multi_key_commit", "ts_multi_key_info", "ts_multi_key_values", "ts_multi_key_free",
    "ts_prove_multi_key", "ts_verify_multi_key", "ts_logup_aux_build_multi_pre", "ts_logup_multiplicities_bus_pre",
    "ts_bus_check", "ts_check_multi",
    "ts_matrix_sort_rows", "ts_matrix_gather_rows",
    "ts_matrix_derive", "ts_derive_check", "ts_derive_rows_host",
    "ts_matrix_scan", "ts_scan_rows_host",
    "ts_matrix_collect_rows", "ts_collect_check", "ts_collect_rows_host",
    "ts_matrix_join_rows", "ts_join_check", "ts_join_rows_host",
    "ts_matrix_expand_rows", "ts_expand_check", "ts_expand_rows_host",
    "ts_proof_to_postcard", "ts_proof_from_postcard", "ts_proof_from_postcard_v",
    "ts_rccl_available", "ts_rccl_unique_id", "ts_comm_rccl_create", "ts_comm_rccl_destroy",
    "ts_comm_rccl_info",
    "ts_comm_local_group_create", "ts_comm_local_get", "ts_comm_local_group_destroy",
    "ts_comm_local_group_reset", "ts_comm_local_group_set_timeout",
    "ts_bench_alu", "ts_bench_stage", "ts_host_alloc", "ts_host_free", "ts_matrix_upload_async",
    "ts_tapleaf_hash", "ts_tapbranch_hash", "ts_tap_winternitz_lock_script", "ts_tap_leaf_script",
    "ts_taptree_from_scripts", "ts_taptree_combine", "ts_taptree_info", "ts_taptree_leaf_proof",
    "ts_taptree_verify_inclusion", "ts_taptree_free", "ts_tap_mmcs_commit", "ts_tap_mmcs_info",
    "ts_tap_mmcs_open_batch", "ts_tap_mmcs_verify_batch", "ts_tap_mmcs_free",
    "ts_prove_tap", "ts_prove_tap_sharded", "ts_verify_tap",
    "ts_dft_batch", "ts_coset_lde_batch", "ts_matrix_bit_reverse_rows", "ts_pcs_data_evaluations_on_domain",
    "ts_matrix_device_ptr",
    "ts_trace_format_bytes", "ts_matrix_upload_packed", "ts_matrix_upload_packed_async",
    "ts_matrix_from_device_packed", "ts_matrix_download_monty",
]

STATUS = {0: "TS_OK", 1: "TS_ERR_INVALID", 2: "TS_ERR_HIP", 3: "TS_ERR_OOM",
          4: "TS_ERR_UNSUPPORTED", 5: "TS_ERR_INVARIANT", 6: "TS_ERR_BUFFER", 7: "TS_ERR_COMM"}


class AirOptionsC(C.Structure):
    """``ts_air_options`` (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("segment_instr", C.c_uint32), ("jit_jobs", C.c_uint32),
                ("reserved", C.c_uint32)]


class TraceFormatC(C.Structure):
    """``ts_trace_format`` (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("layout", C.c_uint32), ("row_stride_bytes", C.c_uint64),
                ("n_kinds", C.c_uint32), ("reserved", C.c_uint32), ("kinds", C.POINTER(C.c_uint8))]


class TsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class FriConfigC(C.Structure):
    _fields_ = [("log_blowup", C.c_uint32), ("num_queries", C.c_uint32),
                ("proof_of_work_bits", C.c_uint32)]


ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
BROADCAST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
ABORT_FN = C.CFUNCTYPE(None, C.c_void_p)


class CommC(C.Structure):
    """``ts_comm`` (include/tapstark.h)."""
    _fields_ = [("rank", C.c_int), ("world", C.c_int), ("user", C.c_void_p),
                ("all_gather", ALL_GATHER_FN), ("broadcast", BROADCAST_FN), ("abort", ABORT_FN)]


class RcclInfoC(C.Structure):
    """``ts_rccl_info`` (include/tapstark.h)."""
    _fields_ = [("rank", C.c_int), ("world", C.c_int), ("comm_count", C.c_int),
                ("comm_user_rank", C.c_int), ("comm_device", C.c_int), ("rccl_version", C.c_int),
                ("aborted", C.c_int), ("checked", C.c_int)]


class ShardOptionsC(C.Structure):
    """``ts_shard_options`` (include/tapstark.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("min_local_log", C.c_uint32), ("trace_replicated", C.c_uint32),
                ("local_quotient", C.c_uint32)]


class BatchItemC(C.Structure):
    """``ts_batch_item`` (include/tapstark.h): one statement of ``ts_prove_batch``, inputs then outputs."""
    _fields_ = [("struct_size", C.c_uint32), ("lane", C.c_uint32), ("trace", C.c_void_p),
                ("host_trace", C.c_void_p), ("height", C.c_uint64), ("width", C.c_uint32),
                ("n_public", C.c_uint32), ("public_values", C.c_void_p), ("challenger", C.c_void_p),
                ("proof_out", C.c_void_p), ("cap_words", C.c_size_t),
                ("status", C.c_int), ("n_words", C.c_size_t), ("proof_blake3", C.c_uint32 * 8),
                ("final_state", C.c_uint32 * 34), ("start_ms", C.c_double), ("wall_ms", C.c_double)]


BATCH_DIGEST = 1  # TS_BATCH_DIGEST


class LogupTermC(C.Structure):
    """``ts_logup_term``."""
    _fields_ = [("kind", C.c_uint32), ("value", C.c_uint32)]


class LogupInteractionC(C.Structure):
    """``ts_logup_interaction``."""
    _fields_ = [("multiplicity", LogupTermC), ("n_values", C.c_uint32), ("values", C.POINTER(LogupTermC))]


class LogupSpecC(C.Structure):
    """``ts_logup_spec`` (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_interactions", C.c_uint32),
                ("interactions", C.POINTER(LogupInteractionC))]


class LogupMultSpecC(C.Structure):
    """``ts_logup_mult_spec`` (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_values", C.c_uint32), ("table", C.POINTER(LogupTermC)),
                ("n_lookups", C.c_uint32), ("lookups", C.POINTER(LogupTermC)), ("weights", C.POINTER(LogupTermC)),
                ("out_column", C.c_uint32), ("negate", C.c_uint32)]


# ``ts_aux_fn``: (user, ctx, trace, challenges, n_challenges, aux_out, exposed_out) -> status
AUX_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32,
                     C.POINTER(C.c_void_p), C.POINTER(C.c_uint32))


class BatchLaneC(C.Structure):
    """``ts_batch_lane``: what a lane of ``ts_prove_batch_lookup`` owns for all of its items."""
    _fields_ = [("struct_size", C.c_uint32), ("key", C.c_void_p), ("key_values", C.c_void_p)]


class MultiTableC(C.Structure):
    """``ts_multi_table``: one table of ``ts_prove_multi``."""
    _fields_ = [("struct_size", C.c_uint32), ("n_public", C.c_uint32), ("air", C.c_void_p), ("trace", C.c_void_p),
                ("public_values", C.POINTER(C.c_uint32))]


class LogupBusLookerC(C.Structure):
    """``ts_logup_bus_looker``: the lookups one looker trace brings to ``ts_logup_multiplicities_bus``."""
    _fields_ = [("n_lookups", C.c_uint32), ("pad", C.c_uint32), ("lookups", C.POINTER(LogupTermC)),
                ("weights", C.POINTER(LogupTermC))]


class LogupMultBusSpecC(C.Structure):
    """``ts_logup_mult_bus_spec`` (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_values", C.c_uint32), ("table", C.POINTER(LogupTermC)),
                ("n_lookers", C.c_uint32), ("out_column", C.c_uint32), ("lookers", C.POINTER(LogupBusLookerC)),
                ("negate", C.c_uint32), ("pad", C.c_uint32)]


class MultiBusTableC(C.Structure):
    """``ts_multi_bus_table``: one table of ``ts_prove_multi_bus``."""
    _fields_ = [("struct_size", C.c_uint32), ("n_public", C.c_uint32), ("air", C.c_void_p), ("trace", C.c_void_p),
                ("public_values", C.POINTER(C.c_uint32)), ("logup", C.POINTER(LogupSpecC))]


class BusShareC(C.Structure):
    """``ts_bus_share``: one table's part of the tuple a ``ts_bus_report`` names."""
    _fields_ = [("count", C.c_uint64), ("sum", C.c_uint32), ("first_row", C.c_uint32),
                ("first_interaction", C.c_uint32), ("pad", C.c_uint32)]


class BusReportC(C.Structure):
    """``ts_bus_report`` (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("pad", C.c_uint32), ("n_contributions", C.c_uint64),
                ("n_tuples", C.c_uint64), ("n_unbalanced", C.c_uint64), ("first_table", C.c_uint32),
                ("first_row", C.c_uint32), ("first_interaction", C.c_uint32), ("n_values", C.c_uint32),
                ("tuple", C.c_uint32 * 8), ("sum", C.c_uint32), ("pad2", C.c_uint32)]


class SortSpecC(C.Structure):
    """``ts_sort_spec`` (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_keys", C.c_uint32), ("key_columns", C.c_uint32 * 4),
                ("group_keys", C.c_uint32), ("flags", C.c_uint32), ("n_live", C.c_uint64)]


class ScanTermC(C.Structure):
    """``ts_scan_term``."""
    _fields_ = [("kind", C.c_uint32), ("value", C.c_uint32)]


class ScanColumnC(C.Structure):
    """``ts_scan_column``."""
    _fields_ = [("a", ScanTermC), ("b", ScanTermC), ("init", C.c_uint32), ("reset_column", C.c_uint32),
                ("dst_column", C.c_uint32), ("flags", C.c_uint32)]


class ScanSpecC(C.Structure):
    """``ts_scan_spec`` (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_columns", C.c_uint32), ("columns", ScanColumnC * 8),
                ("out_width", C.c_uint32), ("pad", C.c_uint32)]


class JoinSpecC(C.Structure):
    """``ts_join_spec`` (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_keys", C.c_uint32), ("src_keys", C.POINTER(LogupTermC)),
                ("table_keys", C.POINTER(LogupTermC)), ("when", LogupTermC), ("n_fetch", C.c_uint32),
                ("table_columns", C.POINTER(C.c_uint32)), ("dst_columns", C.POINTER(C.c_uint32)),
                ("defaults", C.POINTER(C.c_uint32)), ("flags", C.c_uint32), ("table_rows", C.c_uint64)]


class BatchLookupItemC(C.Structure):
    """``ts_batch_lookup_item``: one statement of ``ts_prove_batch_lookup``, inputs then outputs."""
    _fields_ = [("struct_size", C.c_uint32), ("lane", C.c_uint32), ("trace", C.c_void_p),
                ("host_trace", C.c_void_p), ("height", C.c_uint64), ("width", C.c_uint32),
                ("n_public", C.c_uint32), ("public_values", C.c_void_p), ("challenger", C.c_void_p),
                ("proof_out", C.c_void_p), ("cap_words", C.c_size_t),
                ("logup", C.POINTER(LogupSpecC)), ("aux_fn", C.c_void_p), ("aux_user", C.c_void_p),
                ("mult", C.POINTER(LogupMultSpecC)), ("n_mult", C.c_uint32), ("cap_exposed", C.c_uint32),
                ("exposed_out", C.c_void_p),
                ("status", C.c_int), ("n_exposed", C.c_uint32), ("n_words", C.c_size_t),
                ("n_missing", C.c_uint64), ("first_missing", C.c_uint64), ("proof_blake3", C.c_uint32 * 8),
                ("final_state", C.c_uint32 * 34), ("start_ms", C.c_double), ("wall_ms", C.c_double)]

_lib = None


def lib() -> C.CDLL:
    """Loads the library; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TsError(2, f"{LIB_PATH} is missing: run __graft_entry__.build() "
                             "(python -m tapstark_amd.build); there is no CPU fallback")
        # PyTorch-ROCm wheels carry their own libamdhip64; a process that loaded the system copy
        # first cannot initialise torch's afterwards ("No HIP GPUs are available").  Loading torch's
        # first makes both sides share one runtime (same SONAME), which the sharded prover needs
        # (tap-stark_amd/dist.py).  TS_PRELOAD_TORCH=0 skips it for torch-free hosts.
        if os.environ.get("TS_PRELOAD_TORCH", "1") != "0":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        l = C.CDLL(LIB_PATH)
        l.ts_last_error.restype = C.c_char_p
        l.ts_last_error.argtypes = [C.c_void_p]
        l.ts_ctx_stream.restype = C.c_void_p
        l.ts_ctx_stream.argtypes = [C.c_void_p]
        l.ts_chal_sample_bits.restype = C.c_uint64
        l.ts_abi_version.restype = C.c_uint32
        for name in ("ts_ctx_destroy", "ts_matrix_free", "ts_air_free", "ts_pcs_data_free",
                     "ts_chal_free", "ts_chal_observe", "ts_chal_observe_commitment",
                     "ts_chal_sample", "ts_chal_state"):
            getattr(l, name).restype = None
        l.ts_ctx_destroy.argtypes = [C.c_void_p]
        l.ts_matrix_free.argtypes = [C.c_void_p, C.c_void_p]
        l.ts_air_free.argtypes = [C.c_void_p, C.c_void_p]
        l.ts_pcs_data_free.argtypes = [C.c_void_p, C.c_void_p]
        l.ts_chal_free.argtypes = [C.c_void_p]
        l.ts_chal_observe.argtypes = [C.c_void_p, C.c_uint32]
        l.ts_chal_observe_commitment.argtypes = [C.c_void_p, u32p]
        l.ts_chal_sample.argtypes = [C.c_void_p, u32p]
        l.ts_chal_state.argtypes = [C.c_void_p, u32p]
        l.ts_chal_sample_bits.argtypes = [C.c_void_p, C.c_uint32]
        l.ts_chal_check_witness.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        l.ts_chal_grind.argtypes = [C.c_void_p, C.c_uint32, u32p]
        l.ts_chal_new.argtypes = [C.c_int, C.c_int, voidpp]
        l.ts_chal_clone.argtypes = [C.c_void_p, voidpp]
        l.ts_ctx_create.argtypes = [C.c_int, voidpp]
        l.ts_ctx_synchronize.argtypes = [C.c_void_p]
        l.ts_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
        l.ts_ctx_take_timings.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        l.ts_ctx_set_kernel_timing.argtypes = [C.c_void_p, C.c_int]
        l.ts_ctx_set_replay.argtypes = [C.c_void_p, C.c_int]
        l.ts_ctx_take_kernel_timings.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        l.ts_matrix_upload.argtypes = [C.c_void_p, u32p, C.c_uint64, C.c_uint32, voidpp]
        l.ts_matrix_from_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, voidpp]
        l.ts_trace_fibonacci.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, voidpp]
        l.ts_trace_synth_mul.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, voidpp]
        l.ts_trace_synth_ext.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, voidpp]
        l.ts_matrix_dims.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), u32p]
        l.ts_matrix_download.argtypes = [C.c_void_p, C.c_void_p, u32p]
        l.ts_air_compile.argtypes = [C.c_void_p, u32p, C.c_size_t, voidpp]
        l.ts_air_info.argtypes = [C.c_void_p, u32p, u32p, u32p, u32p]
        l.ts_air_is_jit.argtypes = [C.c_void_p]
        l.ts_air_jit_wait.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        l.ts_air_program.argtypes = [C.c_void_p, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_air_jit_source.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_air_jit_compile.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_double)]
        l.ts_pcs_commit.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_uint32, voidpp, u32p,
                                    u32p, voidpp]
        l.ts_mmcs_commit.argtypes = [C.c_void_p, C.c_uint32, voidpp, u32p, voidpp]
        l.ts_pcs_data_lde.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, u32p]
        l.ts_pcs_data_info.argtypes = [C.c_void_p, u32p, u32p]
        l.ts_pcs_data_digests.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, u32p]
        l.ts_pcs_open_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, u32p, u32p]
        l.ts_quotient_chunks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, u32p,
                                         C.c_uint32, u32p, voidpp]
        l.ts_pcs_open_reduce.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_void_p,
                                         u32p, u32p, u32p, u32p]
        l.ts_pcs_data_matrix_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), u32p]
        l.ts_pcs_open.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_uint32, voidpp,
                                  u32p, u32p, u32p, C.c_size_t, C.POINTER(C.c_size_t), u32p,
                                  C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_pcs_verify.argtypes = [C.POINTER(FriConfigC), C.c_void_p, C.c_uint32, u32p, u32p, u32p, u32p,
                                    u32p, u32p, u32p, u32p, C.c_size_t, C.POINTER(C.c_int)]
        l.ts_fri_prove.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_uint32, u32p,
                                   C.POINTER(u32p), u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_fri_verify.argtypes = [C.POINTER(FriConfigC), C.c_void_p, u32p, C.c_size_t,
                                    C.POINTER(C.c_int)]
        l.ts_fri_fold.argtypes = [C.c_void_p, u32p, C.c_uint64, u32p, u32p]
        l.ts_fri_fold_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, u32p, C.c_void_p]
        l.ts_prove.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, C.c_void_p,
                               u32p, C.c_uint32, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_prove_stream.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(FriConfigC),
                                      C.POINTER(C.c_void_p), u32p, C.c_uint32, u32p, C.c_uint32, C.c_double,
                                      u32p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double)]
        l.ts_prove_batch.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(FriConfigC),
                                     C.POINTER(BatchItemC), C.c_uint32, C.c_double, C.c_uint32]
        l.ts_prove_sharded.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.POINTER(CommC), C.c_void_p,
                                       C.c_void_p, C.c_void_p, u32p, C.c_uint32,
                                       C.POINTER(ShardOptionsC), u32p, C.c_size_t,
                                       C.POINTER(C.c_size_t)]
        u8p = C.POINTER(C.c_uint8)
        l.ts_rccl_unique_id.argtypes = [u8p]
        l.ts_comm_rccl_create.argtypes = [C.c_void_p, u8p, C.c_int, C.c_int, C.POINTER(CommC), voidpp]
        l.ts_comm_rccl_destroy.argtypes = [C.c_void_p]
        l.ts_comm_rccl_destroy.restype = None
        l.ts_comm_rccl_info.argtypes = [C.c_void_p, C.POINTER(RcclInfoC)]
        l.ts_comm_local_group_reset.argtypes = [C.c_void_p]
        l.ts_comm_local_group_set_timeout.argtypes = [C.c_void_p, C.c_int]
        l.ts_comm_local_group_create.argtypes = [C.c_int, voidpp]
        l.ts_comm_local_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(CommC)]
        l.ts_comm_local_group_destroy.argtypes = [C.c_void_p]
        l.ts_comm_local_group_destroy.restype = None
        u64p = C.POINTER(C.c_uint64)
        szp = C.POINTER(C.c_size_t)
        l.ts_bench_alu.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        l.ts_bench_stage.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint32, C.c_uint, C.c_uint32,
                                     C.POINTER(C.c_double)]
        l.ts_ctx_graph_stats.argtypes = [C.c_void_p, u64p]
        l.ts_ctx_stat.argtypes = [C.c_void_p, C.c_int, u64p]
        l.ts_host_alloc.argtypes = [C.c_size_t, voidpp]
        l.ts_host_free.argtypes = [C.c_void_p]
        l.ts_host_free.restype = None
        l.ts_matrix_upload_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, voidpp]
        l.ts_tapleaf_hash.argtypes = [C.c_char_p, C.c_size_t, u8p]
        l.ts_tapbranch_hash.argtypes = [u8p, u8p, u8p]
        l.ts_tap_winternitz_lock_script.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, u8p, C.c_size_t, szp]
        l.ts_tap_leaf_script.argtypes = [C.c_char_p, u64p, C.c_uint32, C.c_uint32, C.c_uint64, u32p, u8p,
                                         C.c_size_t, szp]
        l.ts_taptree_from_scripts.argtypes = [C.c_void_p, C.c_char_p, u64p, C.c_uint64, voidpp]
        l.ts_taptree_combine.argtypes = [C.c_void_p, C.c_void_p, voidpp]
        l.ts_taptree_info.argtypes = [C.c_void_p, u64p, u8p]
        l.ts_taptree_leaf_proof.argtypes = [C.c_void_p, C.c_uint64, u8p, u8p, C.c_uint32, u32p]
        l.ts_taptree_verify_inclusion.argtypes = [u8p, u8p, u8p, C.c_uint32]
        l.ts_taptree_free.argtypes = [C.c_void_p]
        l.ts_taptree_free.restype = None
        l.ts_tap_mmcs_commit.argtypes = [C.c_void_p, C.c_uint32, voidpp, C.c_uint32, C.c_uint32, C.c_char_p,
                                         u64p, u8p, voidpp]
        l.ts_tap_mmcs_info.argtypes = [C.c_void_p, u32p, u32p, u32p, u32p]
        l.ts_tap_mmcs_open_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, u32p, u8p, u8p, C.c_size_t, szp]
        l.ts_tap_mmcs_verify_batch.argtypes = [C.c_char_p, u64p, C.c_uint32, C.c_uint32, C.c_uint64, u32p, u8p,
                                               C.c_uint32, u8p, C.POINTER(C.c_int)]
        l.ts_prove_tap.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, C.c_void_p, u32p,
                                   C.c_uint32, C.c_char_p, u64p, C.c_size_t, u32p, C.c_size_t, szp]
        l.ts_prove_tap_sharded.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, u32p, C.c_uint32, C.c_char_p, u64p, C.c_size_t, u32p,
                                           C.c_size_t, szp]
        l.ts_verify_tap.argtypes = [C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, u32p, C.c_size_t, u32p,
                                    C.c_uint32, C.c_char_p, u64p, C.c_size_t, C.POINTER(C.c_int)]
        l.ts_tap_mmcs_free.argtypes = [C.c_void_p]
        l.ts_tap_mmcs_free.restype = None
        l.ts_proof_to_postcard.argtypes = [u32p, C.c_size_t, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_proof_from_postcard.argtypes = [u8p, C.c_size_t, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_proof_from_postcard_v.argtypes = [u8p, C.c_size_t, C.c_int, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_check_constraints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, u32p, C.c_uint32,
                                           C.POINTER(C.c_int64)]
        l.ts_verify.argtypes = [C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, u32p, C.c_size_t, u32p,
                                C.c_uint32, C.POINTER(C.c_int)]
        # preprocessed columns (tape version 2): the key / root / matrix argument may be NULL (preprocessed_width 0)
        l.ts_air_preprocessed_width.argtypes = [C.c_void_p, u32p]
        l.ts_quotient_chunks_pre.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, u32p,
                                             C.c_uint32, u32p, voidpp]
        l.ts_prove_pre.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   u32p, C.c_uint32, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_verify_pre.argtypes = [C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, u32p, u32p, C.c_size_t, u32p,
                                    C.c_uint32, C.POINTER(C.c_int)]
        l.ts_check_constraints_pre.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u32p, C.c_uint32,
                                               C.POINTER(C.c_int64)]
        # challenge-phase (aux) columns (tape version 3) and the LogUp builder
        l.ts_air_aux_info.argtypes = [C.c_void_p, u32p, u32p, u32p]
        l.ts_quotient_chunks_aux.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, u32p,
                                             C.c_uint32, u32p, u32p, u32p, voidpp]
        l.ts_check_constraints_aux.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u32p, C.c_uint32,
                                               u32p, u32p, C.POINTER(C.c_int64)]
        l.ts_prove_aux.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, C.c_void_p, u32p,
                                   C.c_uint32, AUX_FN, C.c_void_p, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_verify_aux.argtypes = [C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, u32p, C.c_size_t, u32p,
                                    C.c_uint32, u32p, C.c_uint32, C.POINTER(C.c_int)]
        l.ts_logup_aux_width.argtypes = [C.POINTER(LogupSpecC), u32p]
        l.ts_logup_aux_build.argtypes = [C.c_void_p, C.POINTER(LogupSpecC), C.c_void_p, u32p, voidpp, u32p]
        l.ts_logup_aux_build_pre.argtypes = [C.c_void_p, C.POINTER(LogupSpecC), C.c_void_p, C.c_void_p, u32p, voidpp,
                                             u32p]
        l.ts_logup_multiplicities.argtypes = [C.c_void_p, C.POINTER(LogupMultSpecC), C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        # preprocessed and aux columns together: the key / root / aux arguments may be NULL (a width of 0)
        l.ts_quotient_chunks_pre_aux.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                 C.c_void_p, u32p, C.c_uint32, u32p, u32p, u32p, voidpp]
        l.ts_check_constraints_pre_aux.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u32p,
                                                   C.c_uint32, u32p, u32p, C.POINTER(C.c_int64)]
        l.ts_prove_pre_aux.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, u32p, C.c_uint32, AUX_FN, C.c_void_p, u32p, C.c_size_t,
                                       C.POINTER(C.c_size_t)]
        l.ts_verify_pre_aux.argtypes = [C.POINTER(FriConfigC), C.c_void_p, C.c_void_p, u32p, u32p, C.c_size_t, u32p,
                                        C.c_uint32, u32p, C.c_uint32, C.POINTER(C.c_int)]
        l.ts_prove_batch_lookup.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(BatchLaneC),
                                            C.c_uint32, C.POINTER(FriConfigC), C.POINTER(BatchLookupItemC),
                                            C.c_uint32, C.c_double, C.c_uint32]
        l.ts_prove_multi.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.POINTER(MultiTableC),
                                     C.c_uint32, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_verify_multi.argtypes = [C.POINTER(FriConfigC), C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32,
                                      C.POINTER(u32p), u32p, u32p, C.c_size_t, C.POINTER(C.c_int)]
        l.ts_prove_multi_bus.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.POINTER(MultiBusTableC),
                                         C.c_uint32, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_verify_multi_bus.argtypes = [C.POINTER(FriConfigC), C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32,
                                          C.POINTER(u32p), u32p, u32p, C.c_size_t, u32p, C.c_uint32, u32p,
                                          C.POINTER(C.c_int)]
        l.ts_logup_multiplicities_bus.argtypes = [C.c_void_p, C.POINTER(LogupMultBusSpecC), C.c_void_p,
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        l.ts_logup_aux_build_multi.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(LogupSpecC)),
                                               C.POINTER(C.c_void_p), u32p, C.POINTER(C.c_void_p), u32p]
        l.ts_multi_key_commit.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_uint32, C.POINTER(C.c_void_p), C.c_int,
                                          u32p, C.POINTER(C.c_void_p)]
        l.ts_multi_key_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), u32p]
        l.ts_multi_key_values.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        l.ts_multi_key_free.argtypes = [C.c_void_p, C.c_void_p]
        l.ts_prove_multi_key.argtypes = [C.c_void_p, C.POINTER(FriConfigC), C.c_void_p, C.c_void_p,
                                         C.POINTER(MultiBusTableC), C.c_uint32, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.ts_verify_multi_key.argtypes = [C.POINTER(FriConfigC), C.c_void_p, u32p, C.POINTER(C.c_void_p), C.c_uint32,
                                          C.POINTER(u32p), u32p, u32p, C.c_size_t, u32p, C.c_uint32, u32p,
                                          C.POINTER(C.c_int)]
        l.ts_logup_multiplicities_bus_pre.argtypes = [C.c_void_p, C.POINTER(LogupMultBusSpecC), C.c_void_p, C.c_void_p,
                                                      C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                                      C.POINTER(C.c_uint64)]
        l.ts_logup_aux_build_multi_pre.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(LogupSpecC)),
                                                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), u32p,
                                                   C.POINTER(C.c_void_p), u32p]
        l.ts_bus_check.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(LogupSpecC)), C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_void_p), C.POINTER(BusReportC), C.POINTER(BusShareC)]
        l.ts_check_multi.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MultiBusTableC), C.c_uint32, u32p,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(BusReportC),
                                     C.POINTER(BusShareC)]
        l.ts_matrix_sort_rows.argtypes = [C.c_void_p, C.POINTER(SortSpecC), C.c_void_p, voidpp]
        l.ts_matrix_gather_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, voidpp]
        l.ts_matrix_derive.argtypes = [C.c_void_p, u32p, C.c_size_t, C.c_void_p, voidpp]
        l.ts_derive_check.argtypes = [u32p, C.c_size_t, C.c_uint32, u32p, u32p, u32p]
        l.ts_derive_rows_host.argtypes = [u32p, C.c_size_t, u32p, C.c_uint64, C.c_uint32, u32p, C.c_size_t]
        l.ts_matrix_scan.argtypes = [C.c_void_p, C.POINTER(ScanSpecC), C.c_void_p, voidpp, u32p]
        l.ts_scan_rows_host.argtypes = [C.POINTER(ScanSpecC), u32p, C.c_uint64, C.c_uint32, u32p, C.c_size_t, u32p]
        l.ts_matrix_collect_rows.argtypes = [C.c_void_p, u32p, C.c_size_t, C.POINTER(C.c_void_p), C.c_uint64, voidpp, u64p]
        l.ts_collect_check.argtypes = [u32p, C.c_size_t, u32p, u32p]
        l.ts_collect_rows_host.argtypes = [u32p, C.c_size_t, C.POINTER(u32p), u64p, C.c_uint64, u32p, C.c_size_t, u64p,
                                           u64p]
        l.ts_matrix_join_rows.argtypes = [C.c_void_p, C.POINTER(JoinSpecC), C.c_void_p, C.c_void_p, voidpp, u64p, u64p]
        l.ts_join_check.argtypes = [C.POINTER(JoinSpecC), C.c_uint32, C.c_uint32, u32p]
        l.ts_join_rows_host.argtypes = [C.POINTER(JoinSpecC), u32p, C.c_uint64, C.c_uint32, u32p, C.c_uint64, C.c_uint32,
                                        u32p, C.c_uint64, u64p, u64p]
        l.ts_matrix_expand_rows.argtypes = [C.c_void_p, u32p, C.c_size_t, C.c_void_p, C.c_uint64, voidpp, u64p]
        l.ts_expand_check.argtypes = [u32p, C.c_size_t, u32p, u32p]
        l.ts_expand_rows_host.argtypes = [u32p, C.c_size_t, u32p, C.c_uint64, C.c_uint64, u32p, C.c_size_t, u64p, u64p]
        l.ts_dft_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, voidpp]
        l.ts_coset_lde_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, voidpp]
        l.ts_matrix_bit_reverse_rows.argtypes = [C.c_void_p, C.c_void_p, voidpp]
        l.ts_pcs_data_evaluations_on_domain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, voidpp]
        l.ts_matrix_device_ptr.argtypes = [C.c_void_p, C.c_void_p, voidpp]
        fmtp = C.POINTER(TraceFormatC)
        l.ts_trace_format_bytes.argtypes = [fmtp, C.c_uint64, C.c_uint32, u64p]
        for name in ("ts_matrix_upload_packed", "ts_matrix_upload_packed_async", "ts_matrix_from_device_packed"):
            getattr(l, name).argtypes = [C.c_void_p, C.c_void_p, fmtp, C.c_uint64, C.c_uint32, voidpp]
        l.ts_matrix_download_monty.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, u32p]
        _lib = l
    return _lib
