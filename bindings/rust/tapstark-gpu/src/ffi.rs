//! `extern "C"` declarations of include/tapstark.h (ABI version 5).  One line per entry point the
//! Rust side uses; the header is the authority for argument meaning.
#![allow(non_camel_case_types)]
use core::ffi::{c_char, c_int, c_uint, c_void};

macro_rules! opaque { ($($n:ident),*) => { $( #[repr(C)] pub struct $n { _p: [u8; 0] } )* } }
opaque!(ts_ctx, ts_matrix, ts_air, ts_pcs_data, ts_challenger, ts_rccl_comm, ts_comm_group, ts_taptree,
        ts_tap_mmcs_data, ts_multi_key);

pub type ts_status = c_int;
pub const TS_OK: ts_status = 0;
pub const TS_ERR_INVARIANT: ts_status = 5; // where the reference would have panicked
pub const TS_ERR_BUFFER: ts_status = 6;

/// `ts_air_options` (struct_size first): the segmented specialisation of `ts_air_compile_opts`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_air_options {
    pub struct_size: u32,
    pub segment_instr: u32,
    pub jit_jobs: u32,
    pub reserved: u32,
}

/// `ts_logup_term`: kind 0 = the canonical constant `value`, 1 = main column `value` (local row), 2 = preprocessed
/// column `value` (local row; `ts_logup_aux_build_pre` only).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_logup_term {
    pub kind: u32,
    pub value: u32,
}

/// `ts_logup_interaction`: the multiplicity and the tuple of values of one interaction.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_logup_interaction {
    pub multiplicity: ts_logup_term,
    pub n_values: u32,
    pub values: *const ts_logup_term,
}

/// `ts_logup_spec` (struct_size first).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_logup_spec {
    pub struct_size: u32,
    pub n_interactions: u32,
    pub interactions: *const ts_logup_interaction,
}

/// `ts_logup_mult_spec` (struct_size first): the table's tuple, the lookups' tuples and weights, and the main
/// column that receives the multiplicities (`ts_logup_multiplicities`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_logup_mult_spec {
    pub struct_size: u32,
    pub n_values: u32,
    pub table: *const ts_logup_term,
    pub n_lookups: u32,
    pub lookups: *const ts_logup_term,
    pub weights: *const ts_logup_term,
    pub out_column: u32,
    pub negate: u32,
}

/// `ts_aux_fn`: the aux source of `ts_prove_aux` (user, ctx, live trace, challenge words, n_challenges, aux_out,
/// exposed_out) -> status.  `None` for an AIR without aux columns.
pub type ts_aux_fn = Option<
    unsafe extern "C" fn(*mut c_void, *mut ts_ctx, *const ts_matrix, *const u32, u32, *mut *mut ts_matrix, *mut u32) -> ts_status,
>;

/// `ts_trace_format` (struct_size first): how the host holds a trace (packed columns, Montgomery words).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_trace_format {
    pub struct_size: u32,
    pub layout: u32,
    pub row_stride_bytes: u64,
    pub n_kinds: u32,
    pub reserved: u32,
    pub kinds: *const u8,
}
pub const TS_COL_MONTY32: u8 = 3;
pub const TS_COL_MONTY31: u8 = 4;
pub const TS_LAYOUT_ROWS: u32 = 0;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_fri_config {
    pub log_blowup: u32,
    pub num_queries: u32,
    pub proof_of_work_bits: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ts_comm {
    pub rank: c_int,
    pub world: c_int,
    pub user: *mut c_void,
    pub all_gather: Option<unsafe extern "C" fn(*mut c_void, *const c_void, *mut c_void, usize, *mut c_void) -> c_int>,
    pub broadcast: Option<unsafe extern "C" fn(*mut c_void, *mut c_void, usize, c_int, *mut c_void) -> c_int>,
    pub abort: Option<unsafe extern "C" fn(*mut c_void)>,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct ts_shard_options {
    pub struct_size: u32, // = size_of::<ts_shard_options>() (the library refuses any other layout)
    pub min_local_log: u32,
    pub trace_replicated: u32,
    pub local_quotient: u32,
}

/// One statement of `ts_prove_batch`: inputs, then what the library writes back.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ts_batch_item {
    pub struct_size: u32, // = size_of::<ts_batch_item>() (the library refuses the whole call otherwise)
    pub lane: u32,
    pub trace: *mut ts_matrix,   // device trace made on the lane's context (consumed) ...
    pub host_trace: *const u32,  // ... or canonical row-major host values; exactly one is set
    pub height: u64,
    pub width: u32,
    pub n_public: u32,
    pub public_values: *const u32,
    pub challenger: *const ts_challenger, // null = fresh; else cloned, never modified
    pub proof_out: *mut u32,
    pub cap_words: usize,
    pub status: ts_status, // -1 = not attempted
    pub n_words: usize,
    pub proof_blake3: [u32; 8],
    pub final_state: [u32; 34],
    pub start_ms: f64,
    pub wall_ms: f64,
}
pub const TS_BATCH_DIGEST: u32 = 1;

/// What a lane of `ts_prove_batch_lookup` owns for all of its items: the AIR's committed key and the row-major
/// table its kind-2 terms read; neither is consumed.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ts_batch_lane {
    pub struct_size: u32, // = size_of::<ts_batch_lane>()
    pub key: *const ts_pcs_data,     // null iff preprocessed_width == 0
    pub key_values: *const ts_matrix, // may be null
}

/// One table of `ts_prove_multi`: a plain AIR (no preprocessed, no aux columns), its trace (consumed) and its
/// public values.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ts_multi_table {
    pub struct_size: u32, // = size_of::<ts_multi_table>()
    pub n_public: u32,
    pub air: *const ts_air,
    pub trace: *mut ts_matrix,
    pub public_values: *const u32,
}

/// One table of `ts_prove_multi_bus`: a `ts_multi_table` whose AIR may have LogUp aux columns (2 challenges, 4
/// exposed words), built by the library from `logup` (null exactly for an AIR without aux columns).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ts_multi_bus_table {
    pub struct_size: u32, // = size_of::<ts_multi_bus_table>()
    pub n_public: u32,
    pub air: *const ts_air,
    pub trace: *mut ts_matrix, // consumed; row-major where the AIR has aux columns
    pub public_values: *const u32,
    pub logup: *const ts_logup_spec,
}

/// `ts_logup_bus_looker`: the lookups one looker trace brings to `ts_logup_multiplicities_bus`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_logup_bus_looker {
    pub n_lookups: u32,
    pub pad: u32,
    pub lookups: *const ts_logup_term, // n_lookups * n_values, over this looker's row
    pub weights: *const ts_logup_term, // n_lookups
}

/// `ts_logup_mult_bus_spec` (struct_size first): the table's tuple over the table trace, the lookers, and the
/// column of the table trace that receives the multiplicities.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_logup_mult_bus_spec {
    pub struct_size: u32,
    pub n_values: u32,
    pub table: *const ts_logup_term,
    pub n_lookers: u32,
    pub out_column: u32,
    pub lookers: *const ts_logup_bus_looker,
    pub negate: u32,
    pub pad: u32,
}

/// `ts_bus_share`: one table's part of the tuple a `ts_bus_report` names (`first_*` are `!0` without a contribution).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_bus_share {
    pub count: u64,
    pub sum: u32,
    pub first_row: u32,
    pub first_interaction: u32,
    pub pad: u32,
}

/// `ts_bus_report`: what `ts_bus_check` says about a bus (`struct_size` is an input; `first_*` are `!0` when balanced).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_bus_report {
    pub struct_size: u32,
    pub pad: u32,
    pub n_contributions: u64,
    pub n_tuples: u64,
    pub n_unbalanced: u64,
    pub first_table: u32,
    pub first_row: u32,
    pub first_interaction: u32,
    pub n_values: u32,
    pub tuple: [u32; 8],
    pub sum: u32,
    pub pad2: u32,
}

/// `ts_sort_spec`: the keys of `ts_matrix_sort_rows` (most significant first), the leading keys that define a group,
/// the appended columns (bit 0: source row, bit 1: group start) and the rows that are sorted.  Like the rest of this
/// file the declaration has not been compiled: there is no Rust toolchain where the library is built.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_sort_spec {
    pub struct_size: u32, // = size_of::<ts_sort_spec>()
    pub n_keys: u32,
    pub key_columns: [u32; 4],
    pub group_keys: u32,
    pub flags: u32,
    pub n_live: u64,
}

/// A term of a scan: kind 0 a constant below p, kind 1 column `value` of the source.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_scan_term {
    pub kind: u32,
    pub value: u32,
}

/// One recurrence of `ts_matrix_scan`: y[i] = a[i] y[i-1] + b[i], y[-1] = init.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_scan_column {
    pub a: ts_scan_term,
    pub b: ts_scan_term,
    pub init: u32,
    pub reset_column: u32, // TS_SCAN_NO_RESET or a column of the source
    pub dst_column: u32,
    pub flags: u32, // bit 0: TS_SCAN_EXCLUSIVE
}

pub const TS_SCAN_MAX_COLUMNS: usize = 8;
pub const TS_SCAN_NO_RESET: u32 = 0xFFFF_FFFF;
pub const TS_SCAN_EXCLUSIVE: u32 = 1;
/// The limits of a `ts_matrix_collect_rows` spec.
pub const TS_COLLECT_MAX_SOURCES: usize = 4;
pub const TS_COLLECT_MAX_EMITTERS: usize = 16;
pub const TS_COLLECT_MAX_WIDTH: usize = 64;
/// The limits of the group form ("TGRP") of a `ts_matrix_collect_rows` spec.
pub const TS_GROUP_MAX_KEYS: usize = 8;
pub const TS_GROUP_MAX_AGGREGATES: usize = 16;
pub const TS_GROUP_MAX_WIDTH: usize = 64;
/// The limits and the flags of a `ts_matrix_join_rows` spec.
pub const TS_JOIN_MAX_KEYS: usize = 8;
pub const TS_JOIN_MAX_FETCH: usize = 32;
pub const TS_JOIN_TABLE_ROW: u32 = 1;
pub const TS_JOIN_HIT: u32 = 2;
pub const TS_JOIN_KEEP: u32 = 4;

/// The keyed fetch of one `ts_matrix_join_rows` call: the arrays are the caller's and are read during the call only.
/// Like every declaration of this file it has not been compiled.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_join_spec {
    pub struct_size: u32, // = size_of::<ts_join_spec>()
    pub n_keys: u32,
    pub src_keys: *const ts_logup_term,
    pub table_keys: *const ts_logup_term,
    pub when: ts_logup_term,
    pub n_fetch: u32,
    pub table_columns: *const u32,
    pub dst_columns: *const u32,
    pub defaults: *const u32,
    pub flags: u32,
    pub table_rows: u64,
}

/// The scans of one `ts_matrix_scan` call.  Like every declaration of this file it has not been compiled.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ts_scan_spec {
    pub struct_size: u32, // = size_of::<ts_scan_spec>()
    pub n_columns: u32,
    pub columns: [ts_scan_column; TS_SCAN_MAX_COLUMNS],
    pub out_width: u32,
    pub pad: u32,
}

/// One statement of `ts_prove_batch_lookup`: `ts_batch_item`'s inputs, the aux source (exactly one of `logup` /
/// `aux_fn` for an AIR with aux columns), the multiplicity fills, then what the library writes back.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ts_batch_lookup_item {
    pub struct_size: u32, // = size_of::<ts_batch_lookup_item>() (the library refuses the whole call otherwise)
    pub lane: u32,
    pub trace: *mut ts_matrix,
    pub host_trace: *const u32,
    pub height: u64,
    pub width: u32,
    pub n_public: u32,
    pub public_values: *const u32,
    pub challenger: *const ts_challenger,
    pub proof_out: *mut u32,
    pub cap_words: usize,
    pub logup: *const ts_logup_spec, // run by the library on the lane's stream ...
    pub aux_fn: ts_aux_fn,           // ... or a callback on the lane's thread
    pub aux_user: *mut c_void,
    pub mult: *const ts_logup_mult_spec, // n_mult fills of the resident trace, before the commit
    pub n_mult: u32,
    pub cap_exposed: u32,
    pub exposed_out: *mut u32,
    pub status: ts_status, // -1 = not attempted
    pub n_exposed: u32,
    pub n_words: usize,
    pub n_missing: u64,
    pub first_missing: u64,
    pub proof_blake3: [u32; 8],
    pub final_state: [u32; 34],
    pub start_ms: f64,
    pub wall_ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct ts_rccl_info {
    pub rank: c_int,
    pub world: c_int,
    pub comm_count: c_int,
    pub comm_user_rank: c_int,
    pub comm_device: c_int,
    pub rccl_version: c_int,
    pub aborted: c_int,
    pub checked: c_int,
}

extern "C" {
    pub fn ts_abi_version() -> u32;
    pub fn ts_ctx_graph_stats(ctx: *mut ts_ctx, out: *mut u64) -> ts_status;
    pub fn ts_ctx_stat(ctx: *mut ts_ctx, which: c_int, out: *mut u64) -> ts_status;
    pub fn ts_device_count() -> c_int;
    pub fn ts_bench_stage(ctx: *mut ts_ctx, stage: c_int, log_n: c_uint, width: u32, log_blowup: c_uint,
                          reps: u32, ms_per_rep: *mut f64) -> ts_status;
    pub fn ts_ctx_create(device: c_int, out: *mut *mut ts_ctx) -> ts_status;
    pub fn ts_ctx_destroy(ctx: *mut ts_ctx);
    pub fn ts_last_error(ctx: *const ts_ctx) -> *const c_char;
    pub fn ts_ctx_synchronize(ctx: *mut ts_ctx) -> ts_status;

    pub fn ts_matrix_upload(ctx: *mut ts_ctx, host_row_major: *const u32, height: u64, width: u32,
                            out: *mut *mut ts_matrix) -> ts_status;
    /// page-locked host memory + asynchronous upload on the context's stream (the PCIe-rate path)
    pub fn ts_host_alloc(bytes: usize, out: *mut *mut c_void) -> ts_status;
    pub fn ts_host_free(p: *mut c_void);
    pub fn ts_matrix_upload_async(ctx: *mut ts_ctx, host_pinned: *const u32, height: u64, width: u32,
                                  out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_matrix_download(ctx: *mut ts_ctx, m: *const ts_matrix, host_row_major: *mut u32) -> ts_status;
    /// a trace as the host holds it: widened / Montgomery-reduced on the device
    pub fn ts_trace_format_bytes(format: *const ts_trace_format, height: u64, width: u32, bytes: *mut u64) -> ts_status;
    pub fn ts_matrix_upload_packed(ctx: *mut ts_ctx, host: *const c_void, format: *const ts_trace_format, height: u64,
                                   width: u32, out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_matrix_upload_packed_async(ctx: *mut ts_ctx, host_pinned: *const c_void, format: *const ts_trace_format,
                                         height: u64, width: u32, out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_matrix_from_device_packed(ctx: *mut ts_ctx, dev: *const c_void, format: *const ts_trace_format,
                                        height: u64, width: u32, out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_matrix_download_monty(ctx: *mut ts_ctx, m: *const ts_matrix, monty_bits: u32,
                                    host_row_major: *mut u32) -> ts_status;
    pub fn ts_matrix_dims(m: *const ts_matrix, height: *mut u64, width: *mut u32) -> ts_status;
    pub fn ts_matrix_free(ctx: *mut ts_ctx, m: *mut ts_matrix);

    pub fn ts_matrix_device_ptr(ctx: *mut ts_ctx, m: *mut ts_matrix, ptr: *mut *const u32) -> ts_status;
    // TwoAdicSubgroupDft on device matrices (csrc/ntt_dft.hip): the input is read, a new matrix returned
    pub fn ts_dft_batch(ctx: *mut ts_ctx, input: *const ts_matrix, inverse: c_int, shift: u32,
                        out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_coset_lde_batch(ctx: *mut ts_ctx, input: *const ts_matrix, added_bits: u32, shift: u32,
                              bit_reversed: c_int, out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_matrix_bit_reverse_rows(ctx: *mut ts_ctx, input: *const ts_matrix, out: *mut *mut ts_matrix) -> ts_status;

    pub fn ts_air_compile(ctx: *mut ts_ctx, tape: *const u32, n_words: usize, out: *mut *mut ts_air) -> ts_status;
    pub fn ts_air_info(air: *const ts_air, width: *mut u32, n_public: *mut u32, max_degree: *mut u32,
                       log_quotient_degree: *mut u32) -> ts_status;
    pub fn ts_air_preprocessed_width(air: *const ts_air, preprocessed_width: *mut u32) -> ts_status;
    pub fn ts_air_free(ctx: *mut ts_ctx, air: *mut ts_air);
    pub fn ts_air_is_jit(air: *const ts_air) -> c_int;
    pub fn ts_air_jit_wait(ctx: *mut ts_ctx, air: *mut ts_air, state: *mut c_int, compile_seconds: *mut f64) -> ts_status;
    pub fn ts_air_program(air: *const ts_air, out: *mut u32, cap_words: usize, n_words: *mut usize) -> ts_status;
    pub fn ts_air_compile_opts(ctx: *mut ts_ctx, tape: *const u32, n_words: usize, opt: *const ts_air_options,
                               out: *mut *mut ts_air) -> ts_status;
    pub fn ts_air_segment_plan(air: *const ts_air, out: *mut u32, cap_words: usize, n_words: *mut usize) -> ts_status;

    pub fn ts_pcs_commit(ctx: *mut ts_ctx, cfg: *const ts_fri_config, n_mats: u32,
                         evals: *const *mut ts_matrix, domain_shifts: *const u32, root_out: *mut u32,
                         out: *mut *mut ts_pcs_data) -> ts_status;
    pub fn ts_pcs_data_info(d: *const ts_pcs_data, n_mats: *mut u32, log_height: *mut u32) -> ts_status;
    pub fn ts_pcs_data_matrix_info(d: *const ts_pcs_data, idx: u32, height: *mut u64, width: *mut u32) -> ts_status;
    pub fn ts_pcs_data_lde(ctx: *mut ts_ctx, d: *const ts_pcs_data, idx: u32, host_row_major: *mut u32) -> ts_status;
    pub fn ts_pcs_data_evaluations_on_domain(ctx: *mut ts_ctx, d: *const ts_pcs_data, idx: u32, log_size: u32,
                                             out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_pcs_data_free(ctx: *mut ts_ctx, d: *mut ts_pcs_data);
    pub fn ts_quotient_chunks(ctx: *mut ts_ctx, trace_data: *const ts_pcs_data, log_blowup: u32,
                              air: *const ts_air, public_values: *const u32, n_public: u32,
                              alpha: *const u32, chunks_out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_pcs_open(ctx: *mut ts_ctx, cfg: *const ts_fri_config, chal: *mut ts_challenger, n_rounds: u32,
                       rounds: *const *const ts_pcs_data, n_points: *const u32, points: *const u32,
                       opened_out: *mut u32, opened_cap_words: usize, n_opened_words: *mut usize,
                       proof_out: *mut u32, proof_cap_words: usize, n_proof_words: *mut usize) -> ts_status;
    pub fn ts_pcs_verify(cfg: *const ts_fri_config, chal: *mut ts_challenger, n_rounds: u32,
                         commitments: *const u32, mats_per_round: *const u32, log_degrees: *const u32,
                         widths: *const u32, n_points: *const u32, points: *const u32,
                         opened_values: *const u32, fri_proof: *const u32, n_words: usize,
                         verdict: *mut c_int) -> ts_status;

    pub fn ts_chal_new(permutation: c_int, sample_ext: c_int, out: *mut *mut ts_challenger) -> ts_status;
    pub fn ts_chal_free(c: *mut ts_challenger);
    pub fn ts_chal_observe(c: *mut ts_challenger, word: u32);
    pub fn ts_chal_observe_commitment(c: *mut ts_challenger, d: *const u32);
    pub fn ts_chal_sample(c: *mut ts_challenger, out: *mut u32);
    pub fn ts_chal_state(c: *const ts_challenger, out: *mut u32);

    pub fn ts_prove(ctx: *mut ts_ctx, cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger,
                    trace: *mut ts_matrix, public_values: *const u32, n_public: u32, proof_out: *mut u32,
                    cap_words: usize, n_words_out: *mut usize) -> ts_status;
    pub fn ts_prove_batch(ctxs: *const *mut ts_ctx, airs: *const *const ts_air, n_lanes: u32,
                          cfg: *const ts_fri_config, items: *mut ts_batch_item, n_items: u32, gate_ms: f64,
                          flags: u32) -> ts_status;
    pub fn ts_prove_sharded(ctx: *mut ts_ctx, cfg: *const ts_fri_config, comm: *const ts_comm,
                            air: *const ts_air, chal: *mut ts_challenger, trace_rows: *mut ts_matrix,
                            public_values: *const u32, n_public: u32, options: *const ts_shard_options,
                            proof_out: *mut u32, cap_words: usize, n_words_out: *mut usize) -> ts_status;
    pub fn ts_verify(cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger,
                     proof: *const u32, n_words: usize, public_values: *const u32, n_public: u32,
                     verdict: *mut c_int) -> ts_status;
    // AIRs with preprocessed columns, proved against a commit-once key (include/tapstark.h "preprocessed
    // columns"): `preprocessed` is the ts_pcs_data of ts_pcs_commit over the one preprocessed matrix, never
    // consumed; null (key, root, matrix) exactly for an AIR with preprocessed_width 0
    pub fn ts_quotient_chunks_pre(ctx: *mut ts_ctx, preprocessed: *const ts_pcs_data, trace_data: *const ts_pcs_data,
                                  log_blowup: u32, air: *const ts_air, public_values: *const u32, n_public: u32,
                                  alpha: *const u32, chunks_out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_prove_pre(ctx: *mut ts_ctx, cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger,
                        preprocessed: *const ts_pcs_data, trace: *mut ts_matrix, public_values: *const u32,
                        n_public: u32, proof_out: *mut u32, cap_words: usize, n_words_out: *mut usize) -> ts_status;
    pub fn ts_verify_pre(cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger,
                         preprocessed_root: *const u32, proof: *const u32, n_words: usize,
                         public_values: *const u32, n_public: u32, verdict: *mut c_int) -> ts_status;
    pub fn ts_check_constraints_pre(ctx: *mut ts_ctx, air: *const ts_air, preprocessed: *const ts_matrix,
                                    trace: *const ts_matrix, public_values: *const u32, n_public: u32,
                                    first_violation: *mut i64) -> ts_status;
    // challenge-phase (aux) columns, tape version 3, and the LogUp builder (include/tapstark.h)
    pub fn ts_air_aux_info(air: *const ts_air, aux_width: *mut u32, n_challenges: *mut u32, n_exposed: *mut u32) -> ts_status;
    pub fn ts_quotient_chunks_aux(ctx: *mut ts_ctx, aux_data: *const ts_pcs_data, trace_data: *const ts_pcs_data,
                                  log_blowup: u32, air: *const ts_air, public_values: *const u32, n_public: u32,
                                  challenges: *const u32, exposed: *const u32, alpha: *const u32,
                                  chunks_out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_check_constraints_aux(ctx: *mut ts_ctx, air: *const ts_air, aux: *const ts_matrix, trace: *const ts_matrix,
                                    public_values: *const u32, n_public: u32, challenges: *const u32,
                                    exposed: *const u32, first_violation: *mut i64) -> ts_status;
    pub fn ts_prove_aux(ctx: *mut ts_ctx, cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger,
                        trace: *mut ts_matrix, public_values: *const u32, n_public: u32, aux_fn: ts_aux_fn,
                        user: *mut c_void, proof_out: *mut u32, cap_words: usize, n_words_out: *mut usize) -> ts_status;
    pub fn ts_verify_aux(cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger, proof: *const u32,
                         n_words: usize, public_values: *const u32, n_public: u32, exposed_out: *mut u32,
                         cap_exposed: u32, verdict: *mut c_int) -> ts_status;
    pub fn ts_logup_aux_width(spec: *const ts_logup_spec, aux_width: *mut u32) -> ts_status;
    pub fn ts_logup_aux_build(ctx: *mut ts_ctx, spec: *const ts_logup_spec, trace: *const ts_matrix,
                              challenges: *const u32, aux_out: *mut *mut ts_matrix, exposed_out: *mut u32) -> ts_status;
    /// terms of kind 2 read column `value` of `preprocessed` (row-major n x preprocessed_width, not consumed)
    pub fn ts_logup_aux_build_pre(ctx: *mut ts_ctx, spec: *const ts_logup_spec, preprocessed: *const ts_matrix,
                                  trace: *const ts_matrix, challenges: *const u32, aux_out: *mut *mut ts_matrix,
                                  exposed_out: *mut u32) -> ts_status;
    /// fills main column `spec.out_column` of the resident `trace` in place; `n_missing` / `first_missing` may be null
    pub fn ts_logup_multiplicities(ctx: *mut ts_ctx, spec: *const ts_logup_mult_spec, preprocessed: *const ts_matrix,
                                   trace: *mut ts_matrix, n_missing: *mut u64, first_missing: *mut u64) -> ts_status;
    // preprocessed AND aux columns together (TSPF v5): the _pre and _aux calls' contracts; a NULL key / root / aux
    // argument exactly for a width of 0
    pub fn ts_prove_pre_aux(ctx: *mut ts_ctx, cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger,
                            key: *const ts_pcs_data, trace: *mut ts_matrix, public_values: *const u32, n_public: u32,
                            aux_fn: ts_aux_fn, user: *mut c_void, proof_out: *mut u32, cap_words: usize,
                            n_words_out: *mut usize) -> ts_status;
    pub fn ts_verify_pre_aux(cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger,
                             preprocessed_root: *const u32, proof: *const u32, n_words: usize,
                             public_values: *const u32, n_public: u32, exposed_out: *mut u32, cap_exposed: u32,
                             verdict: *mut c_int) -> ts_status;
    /// several plain AIR tables of mixed heights in one proof (TSPF v6): one trace commit, one chunk commit, one FRI
    pub fn ts_prove_multi(ctx: *mut ts_ctx, cfg: *const ts_fri_config, chal: *mut ts_challenger,
                          tables: *mut ts_multi_table, n_tables: u32, proof_out: *mut u32, cap_words: usize,
                          n_words_out: *mut usize) -> ts_status;
    /// host only; verdict codes as ts_verify
    pub fn ts_verify_multi(cfg: *const ts_fri_config, chal: *mut ts_challenger, airs: *const *const ts_air,
                           n_tables: u32, public_values: *const *const u32, n_public: *const u32, proof: *const u32,
                           n_words: usize, verdict: *mut c_int) -> ts_status;
    /// ts_prove_multi with a LogUp bus across the tables (TSPF v7): gamma and beta once for every table, one commit
    /// of all aux matrices, three rounds opened
    pub fn ts_prove_multi_bus(ctx: *mut ts_ctx, cfg: *const ts_fri_config, chal: *mut ts_challenger,
                              tables: *mut ts_multi_bus_table, n_tables: u32, proof_out: *mut u32, cap_words: usize,
                              n_words_out: *mut usize) -> ts_status;
    /// host only; on verdict 0 `exposed_out` holds 4 words per table with aux columns and `bus_sum` their EF4 sum
    pub fn ts_verify_multi_bus(cfg: *const ts_fri_config, chal: *mut ts_challenger, airs: *const *const ts_air,
                               n_tables: u32, public_values: *const *const u32, n_public: *const u32,
                               proof: *const u32, n_words: usize, exposed_out: *mut u32, cap_exposed: u32,
                               bus_sum: *mut u32, verdict: *mut c_int) -> ts_status;
    /// n ts_logup_aux_build calls with one set of challenges in three launches; `aux_out`: n handles, `exposed_out`:
    /// 4 n words
    pub fn ts_logup_aux_build_multi(ctx: *mut ts_ctx, n: u32, specs: *const *const ts_logup_spec,
                                    traces: *const *const ts_matrix, challenges: *const u32,
                                    aux_out: *mut *mut ts_matrix, exposed_out: *mut u32) -> ts_status;
    /// ts_logup_multiplicities with the lookups on the rows of `lookers` (n_lookers traces of any heights);
    /// `first_missing`: (looker, row, lookup), may be null
    pub fn ts_logup_multiplicities_bus(ctx: *mut ts_ctx, spec: *const ts_logup_mult_bus_spec,
                                       table_trace: *mut ts_matrix, lookers: *const *const ts_matrix,
                                       n_missing: *mut u64, first_missing: *mut u64) -> ts_status;
    /// the key of a multi-table proof: ONE committed batch of 1..64 preprocessed matrices of mixed heights (the root of
    /// ts_pcs_commit of the same list); made once, consumed by no proof.  keep_values = 1 keeps the row-major inputs
    /// alive inside the key (no second copy) for ts_multi_key_values
    pub fn ts_multi_key_commit(ctx: *mut ts_ctx, cfg: *const ts_fri_config, n_mats: u32, mats: *const *mut ts_matrix,
                               keep_values: c_int, root_out: *mut u32, out: *mut *mut ts_multi_key) -> ts_status;
    pub fn ts_multi_key_info(key: *const ts_multi_key, idx: u32, height: *mut u64, width: *mut u32) -> ts_status;
    /// a borrowed handle (lives as long as the key; never freed or consumed by the caller)
    pub fn ts_multi_key_values(key: *const ts_multi_key, idx: u32, out: *mut *const ts_matrix) -> ts_status;
    pub fn ts_multi_key_free(ctx: *mut ts_ctx, key: *mut ts_multi_key) -> ts_status;
    /// ts_prove_multi_bus against a key (TSPF v8): the i-th table with preprocessed columns reads key matrix i; specs
    /// may use kind-2 terms; without any aux table the challenge phase is skipped
    pub fn ts_prove_multi_key(ctx: *mut ts_ctx, cfg: *const ts_fri_config, chal: *mut ts_challenger,
                              key: *const ts_multi_key, tables: *mut ts_multi_bus_table, n_tables: u32,
                              proof_out: *mut u32, cap_words: usize, n_words_out: *mut usize) -> ts_status;
    /// host only; `key_root`: the eight words the verifier holds; outputs as ts_verify_multi_bus (none without aux tables)
    pub fn ts_verify_multi_key(cfg: *const ts_fri_config, chal: *mut ts_challenger, key_root: *const u32,
                               airs: *const *const ts_air, n_tables: u32, public_values: *const *const u32,
                               n_public: *const u32, proof: *const u32, n_words: usize, exposed_out: *mut u32,
                               cap_exposed: u32, bus_sum: *mut u32, verdict: *mut c_int) -> ts_status;
    /// ts_logup_aux_build_multi with kind-2 terms: table k's read `preprocessed[k]` (entries may be null)
    pub fn ts_logup_aux_build_multi_pre(ctx: *mut ts_ctx, n: u32, specs: *const *const ts_logup_spec,
                                        preprocessed: *const *const ts_matrix, traces: *const *const ts_matrix,
                                        challenges: *const u32, aux_out: *mut *mut ts_matrix,
                                        exposed_out: *mut u32) -> ts_status;
    /// ts_logup_multiplicities_bus whose table terms may be of kind 2: columns of `table_preprocessed`
    pub fn ts_logup_multiplicities_bus_pre(ctx: *mut ts_ctx, spec: *const ts_logup_mult_bus_spec,
                                           table_preprocessed: *const ts_matrix, table_trace: *mut ts_matrix,
                                           lookers: *const *const ts_matrix, n_missing: *mut u64,
                                           first_missing: *mut u64) -> ts_status;
    /// the exact balance of a LogUp bus from the resident traces: a hash join over every table, no challenge
    pub fn ts_bus_check(ctx: *mut ts_ctx, n: u32, specs: *const *const ts_logup_spec,
                        preprocessed: *const *const ts_matrix, traces: *const *const ts_matrix,
                        report: *mut ts_bus_report, shares: *mut ts_bus_share) -> ts_status;
    /// the debug counterpart of ts_prove_multi_bus / ts_prove_multi_key: the traces are not consumed
    pub fn ts_check_multi(ctx: *mut ts_ctx, key: *const ts_multi_key, tables: *const ts_multi_bus_table, n_tables: u32,
                          challenges: *const u32, bad_table: *mut i32, first_violation: *mut i64,
                          report: *mut ts_bus_report, shares: *mut ts_bus_share) -> ts_status;
    /// the rows of a resident matrix in the stable order of up to four key columns; `src` is only read
    pub fn ts_matrix_sort_rows(ctx: *mut ts_ctx, spec: *const ts_sort_spec, src: *const ts_matrix,
                               out: *mut *mut ts_matrix) -> ts_status;
    /// out[i] = src[index[i][index_column]]: the sort's last kernel over a caller's index
    pub fn ts_matrix_gather_rows(ctx: *mut ts_ctx, src: *const ts_matrix, index: *const ts_matrix, index_column: u32,
                                 out: *mut *mut ts_matrix) -> ts_status;
    /// a new matrix whose named columns are a row program ("TDER" word tape) over `src`, the others copied; `src` is
    /// only read
    pub fn ts_matrix_derive(ctx: *mut ts_ctx, program: *const u32, n_words: usize, src: *const ts_matrix,
                            out: *mut *mut ts_matrix) -> ts_status;
    /// host only: the checks of a row program that need no matrix, and what it lowers to (each output may be null)
    pub fn ts_derive_check(program: *const u32, n_words: usize, src_width: u32, out_width: *mut u32,
                           n_instructions: *mut u32, n_live: *mut u32) -> ts_status;
    /// host only: the lowered program over `height` host rows of `src_width` words
    pub fn ts_derive_rows_host(program: *const u32, n_words: usize, src_row_major: *const u32, height: u64,
                               src_width: u32, out_row_major: *mut u32, out_cap_words: usize) -> ts_status;
    /// a new matrix whose dst columns hold linear recurrences y[i] = a[i] y[i-1] + b[i] down the rows of `src`, the
    /// other kept columns copied; `finals` (n_columns words, y[h-1] of each) may be null; `src` is only read
    pub fn ts_matrix_scan(ctx: *mut ts_ctx, spec: *const ts_scan_spec, src: *const ts_matrix, out: *mut *mut ts_matrix,
                          finals: *mut u32) -> ts_status;
    /// host only: the same scans as a sequential loop over `height` host rows of `src_width` words
    pub fn ts_scan_rows_host(spec: *const ts_scan_spec, src_row_major: *const u32, height: u64, src_width: u32,
                             out_row_major: *mut u32, out_cap_words: usize, finals: *mut u32) -> ts_status;
    /// a new matrix of the rows that the emitters of a "TCOL" word tape select from `n_sources` resident matrices, in
    /// (source, row, emitter) order, padded to `out_height` rows (0: the least power of two that holds them); `n_live`
    /// receives the number of selected rows; the sources are only read.  Like every declaration of this file it has
    /// not been compiled.
    pub fn ts_matrix_collect_rows(ctx: *mut ts_ctx, spec: *const u32, n_words: usize, sources: *const *const ts_matrix,
                                  out_height: u64, out: *mut *mut ts_matrix, n_live: *mut u64) -> ts_status;
    /// host only: the checks of a collect spec that need no matrix (each output may be null)
    pub fn ts_collect_check(spec: *const u32, n_words: usize, n_sources: *mut u32, out_width: *mut u32) -> ts_status;
    /// host only: the same collection as a sequential loop over host rows, `heights[s]` rows for source s
    pub fn ts_collect_rows_host(spec: *const u32, n_words: usize, src_row_major: *const *const u32, heights: *const u64,
                                out_height: u64, out_row_major: *mut u32, out_cap_words: usize,
                                out_height_used: *mut u64, n_live: *mut u64) -> ts_status;
    /// a new matrix of `src`'s height: `src` with columns of the `table` row that carries the same key tuple fetched
    /// into its rows; `n_missing` (null: a miss is an error) and `first_missing` report the rows that take part and
    /// find no table row; `src` and `table` (which may be one handle) are only read.  Like every declaration of this
    /// file it has not been compiled.
    pub fn ts_matrix_join_rows(ctx: *mut ts_ctx, spec: *const ts_join_spec, src: *const ts_matrix,
                               table: *const ts_matrix, out: *mut *mut ts_matrix, n_missing: *mut u64,
                               first_missing: *mut u64) -> ts_status;
    /// host only: the checks of a join spec that need no matrix but the two widths (`out_width` may be null)
    pub fn ts_join_check(spec: *const ts_join_spec, src_width: u32, table_width: u32, out_width: *mut u32) -> ts_status;
    /// host only: the same join as a sequential loop over host rows
    pub fn ts_join_rows_host(spec: *const ts_join_spec, src: *const u32, src_height: u64, src_width: u32,
                             table: *const u32, table_height: u64, table_width: u32, out: *mut u32, out_words: u64,
                             n_missing: *mut u64, first_missing: *mut u64) -> ts_status;
    /// a new matrix: every row of `src` repeated by the count the "TEXP" word tape `spec` reads from it, in (row,
    /// inner index) order, padded to `out_height` rows (0: the least power of two that holds them); `src` is only
    /// read.  A row over the spec's max_count is TS_ERR_INVARIANT, a total over the height TS_ERR_INVALID.  Like every
    /// declaration of this file it has not been compiled.
    pub fn ts_matrix_expand_rows(ctx: *mut ts_ctx, spec: *const u32, n_words: usize, src: *const ts_matrix,
                                 out_height: u64, out: *mut *mut ts_matrix, n_live: *mut u64) -> ts_status;
    /// host only: the checks of an expand spec that need no matrix (each output may be null)
    pub fn ts_expand_check(spec: *const u32, n_words: usize, src_width: *mut u32, out_width: *mut u32) -> ts_status;
    /// host only: the same expansion as a sequential loop over `height` host rows
    pub fn ts_expand_rows_host(spec: *const u32, n_words: usize, src_row_major: *const u32, height: u64,
                               out_height: u64, out_row_major: *mut u32, out_cap_words: usize,
                               out_height_used: *mut u64, n_live: *mut u64) -> ts_status;
    /// ts_prove_batch's lanes for AIRs with a key, aux columns or both: per item the work of ts_prove_pre_aux
    pub fn ts_prove_batch_lookup(ctxs: *const *mut ts_ctx, airs: *const *const ts_air, lanes: *const ts_batch_lane,
                                 n_lanes: u32, cfg: *const ts_fri_config, items: *mut ts_batch_lookup_item,
                                 n_items: u32, gate_ms: f64, flags: u32) -> ts_status;
    pub fn ts_quotient_chunks_pre_aux(ctx: *mut ts_ctx, key: *const ts_pcs_data, aux_data: *const ts_pcs_data,
                                      trace_data: *const ts_pcs_data, log_blowup: u32, air: *const ts_air,
                                      public_values: *const u32, n_public: u32, challenges: *const u32,
                                      exposed: *const u32, alpha: *const u32,
                                      chunks_out: *mut *mut ts_matrix) -> ts_status;
    pub fn ts_check_constraints_pre_aux(ctx: *mut ts_ctx, air: *const ts_air, preprocessed: *const ts_matrix,
                                        aux: *const ts_matrix, trace: *const ts_matrix, public_values: *const u32,
                                        n_public: u32, challenges: *const u32, exposed: *const u32,
                                        first_violation: *mut i64) -> ts_status;
    pub fn ts_proof_to_postcard(proof: *const u32, n_words: usize, out: *mut u8, cap_bytes: usize,
                                n_bytes_out: *mut usize) -> ts_status;
    /// tspf_version: 0 infer, 1 / 2 explicit (a taptree proof with one query needs 2)
    pub fn ts_proof_from_postcard_v(bytes: *const u8, n_bytes: usize, tspf_version: c_int, proof_out: *mut u32,
                                    cap_words: usize, n_words_out: *mut usize) -> ts_status;
    pub fn ts_fri_fold_device(ctx: *mut ts_ctx, in_dev: *const u32, h: u64, beta: *const u32,
                              out_dev: *mut u32) -> ts_status;

    // the reference's own MMCS: TapTreeMmcs (csrc/taptree.cpp, tap_prover.cpp)
    pub fn ts_tapleaf_hash(script: *const u8, len: usize, out: *mut u8) -> ts_status;
    pub fn ts_tapbranch_hash(a: *const u8, b: *const u8, out: *mut u8) -> ts_status;
    pub fn ts_tap_mmcs_commit(ctx: *mut ts_ctx, n_mats: u32, mats: *const *mut ts_matrix, u32_size: u32,
                              num_queries: u32, lock_scripts: *const u8, lock_offsets: *const u64,
                              roots_out: *mut u8, out: *mut *mut ts_tap_mmcs_data) -> ts_status;
    pub fn ts_tap_mmcs_info(d: *const ts_tap_mmcs_data, n_mats: *mut u32, log_max_height: *mut u32,
                            n_evals: *mut u32, num_queries: *mut u32) -> ts_status;
    pub fn ts_tap_mmcs_open_batch(d: *const ts_tap_mmcs_data, query_times_index: u32, index: u64,
                                  rows_out: *mut u32, path_out: *mut u8, script_out: *mut u8, script_cap: usize,
                                  script_len: *mut usize) -> ts_status;
    pub fn ts_tap_mmcs_verify_batch(lock_scripts: *const u8, lock_offsets: *const u64, n_evals: u32, u32_size: u32,
                                    index: u64, opened_values: *const u32, path: *const u8, depth: u32,
                                    root: *const u8, ok: *mut c_int) -> ts_status;
    pub fn ts_tap_mmcs_free(d: *mut ts_tap_mmcs_data);
    pub fn ts_prove_tap(ctx: *mut ts_ctx, cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger,
                        trace: *mut ts_matrix, public_values: *const u32, n_public: u32, lock_scripts: *const u8,
                        lock_offsets: *const u64, n_scripts: usize, proof_out: *mut u32, cap_words: usize,
                        n_words_out: *mut usize) -> ts_status;
    pub fn ts_prove_tap_sharded(ctx: *mut ts_ctx, cfg: *const ts_fri_config, comm: *const ts_comm,
                                air: *const ts_air, chal: *mut ts_challenger, trace: *mut ts_matrix,
                                public_values: *const u32, n_public: u32, lock_scripts: *const u8,
                                lock_offsets: *const u64, n_scripts: usize, proof_out: *mut u32, cap_words: usize,
                                n_words_out: *mut usize) -> ts_status;
    pub fn ts_verify_tap(cfg: *const ts_fri_config, air: *const ts_air, chal: *mut ts_challenger,
                         proof: *const u32, n_words: usize, public_values: *const u32, n_public: u32,
                         lock_scripts: *const u8, lock_offsets: *const u64, n_scripts: usize,
                         verdict: *mut c_int) -> ts_status;

    // native communicators (csrc/comm.cpp)
    pub fn ts_rccl_available() -> c_int;
    pub fn ts_rccl_unique_id(out: *mut u8) -> ts_status;
    pub fn ts_comm_rccl_create(ctx: *mut ts_ctx, unique_id: *const u8, rank: c_int, world: c_int,
                               out: *mut ts_comm, handle: *mut *mut ts_rccl_comm) -> ts_status;
    pub fn ts_comm_rccl_destroy(handle: *mut ts_rccl_comm);
    pub fn ts_comm_rccl_info(handle: *const ts_rccl_comm, out: *mut ts_rccl_info) -> ts_status;
    pub fn ts_comm_local_group_reset(group: *mut ts_comm_group) -> ts_status;
    pub fn ts_comm_local_group_set_timeout(group: *mut ts_comm_group, seconds: c_int) -> ts_status;
    pub fn ts_comm_local_group_create(world: c_int, out: *mut *mut ts_comm_group) -> ts_status;
    pub fn ts_comm_local_get(group: *mut ts_comm_group, rank: c_int, out: *mut ts_comm) -> ts_status;
    pub fn ts_comm_local_group_destroy(group: *mut ts_comm_group);
}
