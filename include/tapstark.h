/*
 * tapstark.h -- C ABI of the MI355X-native tap-stark prover hot path (libtapstark_hip.so).
 *
 * Drop-in boundary for the reference's uni-stark/fri prover.  Every entry
 * point names the reference interface it replaces (paths relative to the tap-stark repository).
 * Conventions:
 *   - field elements cross the boundary as CANONICAL u32 (reference basic/src/field/mod.rs:48-63
 *     `as_u32_vec`); an EF4 element is its 4 coefficients [c0,c1,c2,c3];
 *   - digests/commitments are 8 u32 words = the reference's [[u8;4];8] (little-endian words);
 *   - host buffers are caller-owned and only read during the call; device objects are
 *     library-owned handles, freed explicitly;
 *   - every function returns a ts_status (0 = ok) and never throws or aborts; where the reference
 *     panics (assert!/expect) the status is TS_ERR_INVARIANT and ts_last_error() holds the text;
 *   - a context is driven by one host thread; different contexts are independent;
 *   - there is NO CPU fallback: without a HIP device ts_ctx_create fails.
 */
#ifndef TAPSTARK_H
#define TAPSTARK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int ts_status;
enum {
    TS_OK = 0,
    TS_ERR_INVALID = 1,
    TS_ERR_HIP = 2,
    TS_ERR_OOM = 3,
    TS_ERR_UNSUPPORTED = 4,
    TS_ERR_INVARIANT = 5,
    TS_ERR_BUFFER = 6,
    TS_ERR_COMM = 7 /* a ts_comm callback reported failure */
};

typedef struct ts_ctx ts_ctx;               /* one per GPU */
typedef struct ts_matrix ts_matrix;         /* device-resident RowMajorMatrix<Val> */
typedef struct ts_pcs_data ts_pcs_data;     /* Pcs::ProverData / BFMmcs::ProverData */
typedef struct ts_air ts_air;               /* compiled constraint tape */
typedef struct ts_challenger ts_challenger; /* BfChallenger (host side) */

/* reference fri/src/config.rs:11-16 FriConfig (the `mmcs` field is the built-in Blake3 Merkle
 * MMCS) */
typedef struct {
    uint32_t log_blowup;
    uint32_t num_queries;
    uint32_t proof_of_work_bits;
} ts_fri_config;

/* Number of HIP devices this process sees (0 without a GPU or a driver): lets a multi-rank caller
 * check "one device per rank" before it starts any rank (examples/prove_sharded.cpp). */
int ts_device_count(void);
/* ------------------------------------------------------------------ context */
ts_status ts_ctx_create(int device, ts_ctx** out);
void ts_ctx_destroy(ts_ctx* ctx);
const char* ts_last_error(const ts_ctx* ctx);
ts_status ts_ctx_synchronize(ts_ctx* ctx);
/* HIP stream every kernel of this context is launched on (as a void*), for event timing */
void* ts_ctx_stream(ts_ctx* ctx);
/* per-stage timers (HIP events on the context's stream); names follow the reference's tracing
 * spans (uni-stark/src/prover.rs:53,82,121; fri/src/two_adic_pcs.rs:355-374; fri/src/prover.rs:18,45,92) */
ts_status ts_ctx_set_timing(ts_ctx* ctx, int enabled);
/* writes "name=ms;name=ms;..." of the stages recorded since the last call */
ts_status ts_ctx_take_timings(ts_ctx* ctx, char* buf, size_t cap);

/* MEASUREMENT AID: the ceiling of a "zero-host-sync" proof.  mode 1: the next ts_prove records the bytes the
 * host reads at each of its mid-proof synchronisations (two commitment roots, the opened-value sums, the FRI
 * block); mode 2: a ts_prove of the SAME trace, AIR and configuration skips those synchronisations and is
 * handed the recorded bytes at once -- as if the challenges cost nothing -- and must return the same proof;
 * mode 0: off.  Call it before EVERY proof it should apply to (it rewinds the log).  Not for production: with a
 * different trace a mode-2 proof is garbage. */
ts_status ts_ctx_set_replay(ts_ctx* ctx, int mode);
/* per-kernel timers: HIP events recorded on the context's stream around EVERY kernel launch
 * (resolved lazily, no sync per kernel); take writes "kernel=launches:total_ms;..." */
ts_status ts_ctx_set_kernel_timing(ts_ctx* ctx, int enabled);
ts_status ts_ctx_take_kernel_timings(ts_ctx* ctx, char* buf, size_t cap);
/* out[3] = bytes the context's device pool holds.  out[0..2] counted the FRI commit phase's replays
 * from a hipGraph, a measurement option that has been retired: they are always 0, kept so that the
 * layout does not change.  Diagnostics only. */
ts_status ts_ctx_graph_stats(ts_ctx* ctx, uint64_t out[4]);
/* One diagnostic counter of the context by index: 0-3 as ts_ctx_graph_stats; 4 = always 0 (it counted
 * refused reservations of the retired graph replay); 5 = ts_prove_sharded calls whose local quotient
 * (ts_shard_options.local_quotient) was redone through the broadcast path because FRI's final
 * polynomial was not constant, i.e. the trace was invalid (fri/src/prover.rs:129-134).
 * 6 / 7 / 8 = proof-of-work witnesses (fri/src/prover.rs:43) taken from the device search after the
 * host's one-step check_witness / device candidates the host refused (never expected) / searches the
 * host ran itself (no device candidate below 2^12, or TS_HOST_GRIND=1).
 * 9 = device blocks filled with the test pattern since the context was created; 0 unless the TEST KNOB
 * TS_POOL_POISON=<32-bit word, as strtoul(.., 0) reads it> was set when ts_ctx_create ran.  The context then
 * fills every block its pool hands out (the whole rounded block, recycled ones too) and every table it allocates
 * (twiddles, coset scales, selectors) with that word and waits for the fill, so that nothing can pass by reading
 * what an earlier use left behind; proofs are the same, only slower.  Unset or empty: off, at the cost of one
 * branch per block.  A value that is no 32-bit word makes ts_ctx_create return TS_ERR_INVALID.
 * 11 = pool blocks handed out and not yet given back (matrices, commitments and the temporaries of a call in
 * progress): a call that is refused leaves it where it was.  10 is not used.
 * TS_ERR_INVALID for an unknown index. */
ts_status ts_ctx_stat(ts_ctx* ctx, int which, uint64_t* out);

/* ------------------------------------------------------------------ matrices */
/* RowMajorMatrix<Val>::new(values, width): host row-major canonical values -> device */
ts_status ts_matrix_upload(ts_ctx* ctx, const uint32_t* host_row_major, uint64_t height,
                           uint32_t width, ts_matrix** out);
/* same from a device pointer (e.g. a torch tensor's data_ptr); the data is copied */
/* The same without waiting for the copy: `host_pinned` must come from ts_host_alloc (page-locked:
 * the copy then runs at the full PCIe rate, asynchronously on the context's stream) and must stay
 * untouched until the next ts_ctx_synchronize / blocking call on this context. */
ts_status ts_matrix_upload_async(ts_ctx* ctx, const uint32_t* host_pinned, uint64_t height,
                                 uint32_t width, ts_matrix** out);
ts_status ts_host_alloc(size_t bytes, void** out);
void ts_host_free(void* p);
ts_status ts_matrix_from_device(ts_ctx* ctx, const uint32_t* dev_row_major, uint64_t height,
                                uint32_t width, ts_matrix** out);
/* Traces generated on the device (no H2D).  ts_trace_fibonacci = generate_trace_rows(a, b, n) of
 * uni-stark/tests/fib_air.rs:59-78 (n x 2: row 0 = (a, b), then (l, r) -> (r, l + r));
 * ts_trace_synth_mul = the build-defined SynthMulAir-`width` trace of BASELINE configs 3/4
 * (SplitMix64 stream `seed`, tap-stark_amd/airs.py generate_synth_mul_trace);
 * ts_trace_synth_ext = the SynthExt-`width` trace of config 5's stand-in (generate_synth_ext_trace). */
ts_status ts_trace_fibonacci(ts_ctx* ctx, uint32_t a, uint32_t b, uint64_t n, ts_matrix** out);
ts_status ts_trace_synth_mul(ts_ctx* ctx, uint64_t n, uint32_t width, uint64_t seed, ts_matrix** out);
ts_status ts_trace_synth_ext(ts_ctx* ctx, uint64_t n, uint32_t width, uint64_t seed, ts_matrix** out);
ts_status ts_matrix_dims(const ts_matrix* m, uint64_t* height, uint32_t* width);
/* row-major, natural row order */
ts_status ts_matrix_download(ts_ctx* ctx, const ts_matrix* m, uint32_t* host_row_major);
void ts_matrix_free(ts_ctx* ctx, ts_matrix* m);

/* The row-major device pointer of a matrix (natural rows, canonical words), for a caller's own kernels --
 * their quotient, a lookup argument -- to read what the calls below return; ts_matrix_from_device is the
 * opposite direction.  Valid until the matrix is freed or consumed; ordered on the context's stream
 * (ts_ctx_stream): work enqueued there, or after ts_ctx_synchronize, sees the values.  Read-only. */
ts_status ts_matrix_device_ptr(ts_ctx* ctx, ts_matrix* m, const uint32_t** ptr);

/* ---- traces in the host's own form: packed columns, Montgomery words ----
 * RowMajorMatrix::new(values, width) for a host that does not hold canonical words: the calls below take the
 * trace as the host stores it and do the widening and the conversion in HBM, instead of the host's own pass
 * in front of ts_matrix_upload (reference `as_u32_vec`, basic/src/field/mod.rs:48-63; on a Plonky3 host the
 * `as_canonical_u32` map over RowMajorMatrix<BabyBear>::values, whose memory is Montgomery words).  Byte,
 * flag and 16-bit limb columns cross the link at their own size.  The result is an ordinary row-major
 * canonical ts_matrix; nothing downstream changes.
 *   TS_LAYOUT_ROWS    row r starts at byte r * stride (row_stride_bytes, 0 = the bytes of a row); its columns
 *                     follow one another at their own sizes with no padding, so a 4-byte column may sit at
 *                     any byte offset.  The buffer is height * stride bytes.
 *   TS_LAYOUT_PLANAR  column c is `height` elements of its size, contiguous; each column starts at the next
 *                     multiple of 16 bytes.  row_stride_bytes must be 0.
 * Any 32-bit word is accepted for the two Montgomery kinds and the result is canonical; TS_COL_U32 is not
 * range-checked, exactly as ts_matrix_upload.  Which radix a p3-baby-bear revision uses must be confirmed
 * with one known value. */
enum { TS_COL_U32 = 0,      /* canonical word, copied as ts_matrix_upload copies it */
       TS_COL_U16 = 1, TS_COL_U8 = 2,   /* unsigned little-endian, zero-extended */
       TS_COL_MONTY32 = 3,  /* word x stands for x * 2^-32 mod p */
       TS_COL_MONTY31 = 4 };/* word x stands for x * 2^-31 mod p */
enum { TS_LAYOUT_ROWS = 0, TS_LAYOUT_PLANAR = 1 };
typedef struct {
    uint32_t struct_size;      /* sizeof(ts_trace_format), else TS_ERR_INVALID */
    uint32_t layout;
    uint64_t row_stride_bytes; /* ROWS only; 0 = tight */
    uint32_t n_kinds;          /* 1 = every column has kinds[0]; else must equal width */
    uint32_t reserved;         /* 0 */
    const uint8_t* kinds;
} ts_trace_format;
/* Bytes of a height x width trace in this format: the one place the size is computed.  Host only, no context.
 * It makes every check of the format the upload calls make (text in ts_last_error(NULL)). */
ts_status ts_trace_format_bytes(const ts_trace_format* format, uint64_t height, uint32_t width, uint64_t* bytes);
/* ts_matrix_upload / ts_matrix_upload_async / ts_matrix_from_device for such a buffer (`host_pinned` from
 * ts_host_alloc, under the ordering contract of ts_matrix_upload_async; `dev`: a device pointer, e.g. a
 * torch uint8 tensor's).  The copy and the decode run on the context's stream; the device staging buffer comes
 * from the context's pool and is released in stream order.  TS_ERR_INVALID, with text in ts_last_error and
 * before anything touches a device, for a null context (checked first), a null format, a wrong struct_size, a
 * non-zero reserved, an unknown kind or layout, n_kinds neither 1 nor width, a stride below the row's bytes,
 * a base pointer that is not 16-byte aligned, a height that is no power of two or above 2^27.
 * ts_batch_item.host_trace stays canonical-only (that struct is frozen by its struct_size): a packed trace
 * enters ts_prove_batch as a device `trace` made with ts_matrix_upload_packed_async on the lane's context. */
ts_status ts_matrix_upload_packed(ts_ctx* ctx, const void* host, const ts_trace_format* format, uint64_t height,
                                  uint32_t width, ts_matrix** out);
ts_status ts_matrix_upload_packed_async(ts_ctx* ctx, const void* host_pinned, const ts_trace_format* format,
                                        uint64_t height, uint32_t width, ts_matrix** out);
ts_status ts_matrix_from_device_packed(ts_ctx* ctx, const void* dev, const ts_trace_format* format,
                                       uint64_t height, uint32_t width, ts_matrix** out);
/* ts_matrix_download as Montgomery words, for a host whose field type stores them (instead of its
 * `from_canonical_u32` pass): word = value * 2^monty_bits mod p, monty_bits 31 or 32, else TS_ERR_INVALID. */
ts_status ts_matrix_download_monty(ts_ctx* ctx, const ts_matrix* m, uint32_t monty_bits, uint32_t* host_row_major);

/* ------------------------------------------------------------------ Dft (TwoAdicSubgroupDft) */
/* The `Dft` of TwoAdicFriPcs::new(log_n, dft, mmcs, fri_config) (fri/src/two_adic_pcs.rs:38-55;
 * Radix2DitParallel in uni-stark/tests/fib_air.rs:113-115), the Plonky3 p3-dft trait of SURVEY.md App. A.5,
 * on device matrices.  Every call runs on the context's stream, only READS `in` (it is not consumed) and
 * returns a new matrix: row-major, natural rows unless stated, canonical values.  Heights are powers of
 * two; height 1 is the identity.  TS_ERR_INVALID (text in ts_last_error) for shift == 0 or shift >= p, a
 * height that is no power of two, a ts_dft_batch input above 2^26 rows or a ts_coset_lde_batch result above
 * 2^27 rows (the tallest input / LDE of ts_pcs_commit).
 * ts_dft_batch: inverse = 0 is coset_dft_batch -- per column, out row k = sum_j in[j] (shift w_n^k)^j
 *   (shift = 1: dft_batch); inverse = 1 is coset_idft_batch -- the coefficients of the interpolant of `in`
 *   over shift * H_n, 1/n included (shift = 1: idft_batch). */
ts_status ts_dft_batch(ts_ctx* ctx, const ts_matrix* in, int inverse, uint32_t shift, ts_matrix** out);
/* coset_lde_batch (App. A.5; what Pcs::commit calls, fri/src/two_adic_pcs.rs:233-241): `in` holds
 * evaluations over H_n; out is (n << added_bits) x width, row j = the interpolant at shift * w_N^j, or row
 * bitrev(j) with bit_reversed = 1 (`.bit_reverse_rows()`: then word for word the ts_pcs_data_lde of a
 * ts_pcs_commit with domain shift 31 / shift, :235).  shift = 1 is lde_batch; added_bits = 0 is allowed. */
ts_status ts_coset_lde_batch(ts_ctx* ctx, const ts_matrix* in, uint32_t added_bits, uint32_t shift,
                             int bit_reversed, ts_matrix** out);
/* Matrix::bit_reverse_rows().to_row_major_matrix() (p3-matrix, used at fri/src/two_adic_pcs.rs:239,257) */
ts_status ts_matrix_bit_reverse_rows(ts_ctx* ctx, const ts_matrix* in, ts_matrix** out);

/* ------------------------------------------------------------------ AIR */
/* Tape = serialised result of get_symbolic_constraints (uni-stark/src/symbolic_builder.rs:52-64):
 *   [0]=0x54415354 [1]=1 [2]=width [3]=n_public [4]=n_nodes [5]=n_constraints,
 *   n_nodes x {op,a,b}, n_constraints node ids in assert_zero order.
 * ops (symbolic_expression.rs:12-37): 0 CONST(a=value) 1 MAIN(a=offset 0|1,b=column)
 *   2 PUBLIC(a=index) 3 IS_FIRST_ROW 4 IS_LAST_ROW 5 IS_TRANSITION 6 ADD(a,b) 7 SUB(a,b) 8 NEG(a)
 *   9 MUL(a,b)
 * Version 2, for an AIR with preprocessed (fixed) columns -- the PairBuilder::preprocessed() of
 * uni-stark/src/symbolic_builder.rs:68-99,144-148 and Entry::Preprocessed { offset } of
 * symbolic_variable.rs:9-15,34-39 (degree multiple 1, like a main variable):
 *   [0]=0x54415354 [1]=2 [2]=width [3]=n_public [4]=n_nodes [5]=n_constraints [6]=preprocessed_width,
 *   then nodes and constraints as in version 1, with one more op:
 *   10 PREP(a=offset 0|1, b=column < preprocessed_width).
 * Version 1 is accepted and lowered exactly as before; a version-2 tape with preprocessed_width 0 behaves in
 * every call as the version-1 tape with the same nodes.  TS_ERR_INVALID: PREP in a version-1 tape, a column >=
 * preprocessed_width, an offset > 1, a word count that does not match the header, width 0.
 * Version 3 (build-defined; the reference has one trace phase), for an AIR with challenge-phase (aux) columns --
 * columns that depend on verifier challenges drawn after the main trace is committed (LogUp and its relatives):
 *   [0]=0x54415354 [1]=3 [2]=width [3]=n_public [4]=n_nodes [5]=n_constraints [6]=preprocessed_width
 *   [7]=aux_width [8]=n_challenges [9]=n_exposed, then nodes and constraints, with three more ops:
 *   11 AUX(a=offset 0|1, b=column < aux_width)   degree multiple 1, like a main variable
 *   12 CHALLENGE(a=word index < 4 n_challenges)  degree multiple 0, like a public value
 *   13 EXPOSED(a=index < n_exposed)              degree multiple 0
 * aux_width counts base-field columns, n_challenges extension elements (four words each), n_exposed base words.
 * An extension-valued constraint is four base constraints (tapstark_air.hpp ExtExpr).  TS_ERR_INVALID: one of
 * these ops in a version-1 or version-2 tape, an index out of range, an offset > 1.  Lowering: AUX takes the
 * LOAD operands PREP takes (a = 2, 3), CHALLENGE k the public slot n_public + k, EXPOSED e the slot n_public +
 * 4 n_challenges + e; the kernels see (aux LDE, trace LDE) where they see (key LDE, trace LDE), and the vector
 * public values ++ challenges ++ exposed.  A tape with preprocessed_width > 0 AND aux_width > 0 reads three
 * matrices: PREP keeps a = 2, 3 and AUX takes a = 4, 5, the local and next row of a THIRD matrix; the public slots
 * are unchanged.  Only the ts_*_pre_aux calls below prove, check and verify such an AIR; every other proving call
 * returns TS_ERR_UNSUPPORTED for it, before anything is consumed.
 * The library has a second node tape, the ROW PROGRAM of ts_matrix_derive ("TDER", at the end of this header): ops 0 to 9
 * keep their numbers and meaning there where they coincide (1 reads a column of the source matrix, 2 does not exist). */
/* ctx == NULL builds a host-only AIR (degree rules + verifier use; no kernels) */
ts_status ts_air_compile(ts_ctx* ctx, const uint32_t* tape, size_t n_words, ts_air** out);
/* get_log_quotient_degree, uni-stark/src/symbolic_builder.rs:15-32 */
ts_status ts_air_info(const ts_air* air, uint32_t* width, uint32_t* n_public,
                      uint32_t* max_constraint_degree, uint32_t* log_quotient_degree);
/* the preprocessed_width that get_log_quotient_degree / get_symbolic_constraints take
 * (symbolic_builder.rs:15-21,52-58): 0 for a version-1 tape */
ts_status ts_air_preprocessed_width(const ts_air* air, uint32_t* preprocessed_width);
/* 1 if the quotient kernel was specialised for this AIR with hiprtc, 0 if the generic on-device
 * interpreter is used (hiprtc missing, TS_NO_JIT set in the environment, the program is above the
 * compile budget, or a background compilation has not finished yet).
 * Compile budget (hiprtc's time grows faster than the program): up to TS_JIT_SYNC_INSTR (default 2048)
 * lowered instructions the kernel is compiled inside ts_air_compile; up to TS_JIT_MAX_INSTR (default
 * 32768) by a child process (the helper `ts_jitc` beside the library; TS_JITC_PATH overrides; without it
 * such programs stay on the interpreter) while proofs already run on the interpreter -- the first use after
 * it finishes switches over, the proof words are the same either way; larger programs stay on the
 * interpreter, which has no limit on program size or live values.  TS_JIT_CACHE_DIR (an existing
 * directory) keeps the code objects across processes: a later ts_air_compile of the same AIR loads
 * instead of compiling. */
int ts_air_is_jit(const ts_air* air);
/* joins a background compilation (every child of a segmented AIR); state: 0 none, 3 specialised kernel(s)
 * loaded, 4 compilation failed */
ts_status ts_air_jit_wait(ts_ctx* ctx, ts_air* air, int* state, double* compile_seconds);
void ts_air_free(ts_ctx* ctx, ts_air* air);
/* Inspection of what the tape was lowered to (none of these needs a GPU; `air` may be host-only).
 * The reference's counterpart is the monomorphised `Air::eval` inside quotient_values
 * (uni-stark/src/prover.rs:170-181): user code compiled into the prover.  Here the tape is lowered
 * to a register program (csrc/air.cpp) that the on-device interpreter runs, and that program to
 * straight-line HIP source compiled with hiprtc (csrc/jit.cpp); tests interpret the former and
 * compile the latter against the oracle's direct evaluation of the tape.
 * ts_air_program: out = [n_regs, n_instr, n_consts, n_instr x {op,dst,a,b}, n_consts x canonical
 *   value, n_consts x (public-value index or 0xffffffff)]; ops: 0 LOAD(a=row offset + 2 * matrix,
 *   b=column): a = 0 / 1 the main trace's local / next row, a = 2 / 3 the second matrix's (the preprocessed columns
 *   of a version-2 tape, or the aux columns of a version-3 tape without preprocessed columns), a = 4 / 5 the
 *   third's (the aux columns of a version-3 tape that has preprocessed columns too)
 *   1 CONST(a=const index) 2 SEL(a=0 first|1 last|2 transition) 3 ADD 4 SUB 5 NEG 6 MUL
 *   7 ASSERT(a=register, b=constraint index).  TS_ERR_BUFFER (with *n_words set) if cap is short.
 * ts_air_jit_source: the HIP source (not NUL-terminated; *n_bytes set even on TS_ERR_BUFFER).
 * ts_air_jit_compile: that source through hiprtc for `arch` ("gfx950"); the code object and the
 *   compile time.  TS_ERR_UNSUPPORTED if hiprtc is missing or the compilation fails. */
/* Segmented specialisation (opt-in).  A program longer than segment_instr lowered instructions is cut into
 * segments of at most that many, each its own straight-line kernel; a computed value that crosses a cut goes
 * through an explicit slab in device memory, the constraint sum as 8 more words.  Compile time grows with the
 * program, not faster, and no kernel spills: each stays within 128 VGPRs.  Such an AIR is always compiled in
 * the background by up to jit_jobs ts_jitc children (0 = up to 4; at most 8), one module each, while proofs
 * run on the interpreter; ts_air_jit_wait joins them all, ts_air_free kills those still running, and
 * TS_JIT_CACHE_DIR keeps every module under its own key.  It has no TS_JIT_MAX_INSTR ceiling but a cap of
 * 2^20 lowered instructions (TS_ERR_INVALID above).  opt == NULL or segment_instr == 0 is ts_air_compile, and
 * so is a program of at most segment_instr instructions.  struct_size must be sizeof(ts_air_options) and
 * reserved 0 (else TS_ERR_INVALID).  ts_air_jit_source / ts_air_jit_compile of a segmented AIR give all its
 * kernels in one module. */
typedef struct ts_air_options {
    uint32_t struct_size;   /* sizeof(ts_air_options) */
    uint32_t segment_instr; /* 0 = as ts_air_compile; S > 0: programs longer than S are segmented */
    uint32_t jit_jobs;      /* compiler children for one AIR; 0 = default */
    uint32_t reserved;      /* must be 0 */
} ts_air_options;
ts_status ts_air_compile_opts(ts_ctx* ctx, const uint32_t* tape, size_t n_words, const ts_air_options* opt,
                              ts_air** out);
/* The plan of a segmented AIR: out = [slab_width, n_segments, then per segment: begin, end (lowered
 * instructions, [begin, end)), n_in, n_out, pressure (most values its kernel holds at once), n_in x (defining
 * instruction, slot), n_out x (defining instruction, slot)].  slab_width counts value slots only (the most
 * values live across one cut).  TS_ERR_BUFFER with *n_words set if cap is short; TS_ERR_INVALID for an AIR
 * that is not segmented. */
ts_status ts_air_segment_plan(const ts_air* air, uint32_t* out, size_t cap_words, size_t* n_words);
ts_status ts_air_program(const ts_air* air, uint32_t* out, size_t cap_words, size_t* n_words);
ts_status ts_air_jit_source(const ts_air* air, char* buf, size_t cap, size_t* n_bytes);
ts_status ts_air_jit_compile(const ts_air* air, const char* arch, void* code_out, size_t cap,
                             size_t* n_bytes, double* seconds);

/* ------------------------------------------------------------------ PCS */
/* Pcs::commit, fri/src/two_adic_pcs.rs:227-245: for each (domain, evals): coset LDE with shift
 * 31/domain.shift, bit-reversed rows, then mmcs.commit.  The matrices may have different
 * (power-of-two) heights: a shorter one's row digests are injected at the tree layer of its
 * height and open_batch reduces the index (bf_mmcs.rs:10-15, tcs/mod.rs:339-378).  The matrices are consumed (like the moved
 * `RowMajorMatrix` arguments).  root_out = commitment. */
ts_status ts_pcs_commit(ts_ctx* ctx, const ts_fri_config* cfg, uint32_t n_mats,
                        ts_matrix* const* evals, const uint32_t* domain_shifts,
                        uint32_t root_out[8], ts_pcs_data** out);
/* BFMmcs::commit, basic/src/mmcs/bf_mmcs.rs:22-35 (reference impl taptree_mmcs.rs:101-114): commit
 * to the given matrices as they are (no LDE, rows in the given order), any widths -- rows wider
 * than 256 elements hash as multi-chunk Blake3 -- and power-of-two heights.  The result is a
 * ts_pcs_data: ts_pcs_open_batch, ts_pcs_data_digests, ts_pcs_data_lde (= get_matrices) apply.
 * The matrices are consumed. */
ts_status ts_mmcs_commit(ts_ctx* ctx, uint32_t n_mats, ts_matrix* const* mats, uint32_t root_out[8],
                         ts_pcs_data** out);
/* BFMmcs::get_matrices (basic/src/mmcs/bf_mmcs.rs:52): committed LDE `idx`, row-major,
 * bit-reversed row order, N x width */
ts_status ts_pcs_data_lde(ts_ctx* ctx, const ts_pcs_data* d, uint32_t idx, uint32_t* host_row_major);
/* Pcs::get_evaluations_on_domain (fri/src/two_adic_pcs.rs:247-258) kept on the device: the first
 * 2^log_size rows of committed LDE `idx`, un-bit-reversed (:257), as a row-major 2^log_size x width matrix --
 * the evaluations on the coset 31 * H_{2^log_size} for a matrix committed on its natural domain.  Works
 * for the shorter matrices of a mixed-height batch.  TS_ERR_INVALID if 2^log_size exceeds that matrix's
 * LDE height (:256 asserts) or idx is out of range. */
ts_status ts_pcs_data_evaluations_on_domain(ts_ctx* ctx, const ts_pcs_data* d, uint32_t idx, uint32_t log_size,
                                            ts_matrix** out);
ts_status ts_pcs_data_info(const ts_pcs_data* d, uint32_t* n_mats, uint32_t* log_height);
/* height (LDE rows) and width of committed matrix `idx`; log_height above is the tallest one's */
ts_status ts_pcs_data_matrix_info(const ts_pcs_data* d, uint32_t idx, uint64_t* height, uint32_t* width);
/* Merkle digest layer `level` (0 = leaves), (N >> level) x 8 words */
ts_status ts_pcs_data_digests(ts_ctx* ctx, const ts_pcs_data* d, uint32_t level, uint32_t* host_out);
/* BFMmcs::open_batch (bf_mmcs.rs:37-42; taptree_mmcs.rs:46-63): rows of every matrix at `index`
 * (concatenated) and the sibling path (log_height x 8 words, leaf level first) */
ts_status ts_pcs_open_batch(ts_ctx* ctx, const ts_pcs_data* d, uint64_t index, uint32_t* rows_out,
                            uint32_t* path_out);
void ts_pcs_data_free(ts_ctx* ctx, ts_pcs_data* d);

/* get_evaluations_on_domain + quotient_values + flatten_to_base + split_evals
 * (two_adic_pcs.rs:247-258; uni-stark/src/prover.rs:68-80,122-194): quotient_degree matrices of
 * n x 4, ready for ts_pcs_commit with domain shifts 31 * w_{n*qd}^c.
 * chunks_out must have room for 2^log_quotient_degree handles. */
ts_status ts_quotient_chunks(ts_ctx* ctx, const ts_pcs_data* trace_data, uint32_t log_blowup,
                             const ts_air* air, const uint32_t* public_values, uint32_t n_public,
                             const uint32_t alpha[4], ts_matrix** chunks_out);

/* Pcs::open up to the FRI input (two_adic_pcs.rs:312-389) for the prove() shape: round 0 = trace
 * data opened at {zeta, zeta*w_n}, round 1 = quotient data (qd matrices) opened at {zeta}.
 * opened_out: (2*w + 4*qd) EF4 in proof order (trace_local, trace_next, chunks);
 * reduced_out: N EF4 (the single FRI input vector), or NULL. */
ts_status ts_pcs_open_reduce(ts_ctx* ctx, const ts_fri_config* cfg, const ts_pcs_data* trace_data,
                             const ts_pcs_data* quotient_data, const uint32_t zeta[4],
                             const uint32_t batch_alpha[4], uint32_t* opened_out,
                             uint32_t* reduced_out);

/* Pcs::open, fri/src/two_adic_pcs.rs:260-419, for any rounds x matrices x points (the shapes of
 * fri/tests/pcs.rs:62-90 and uni-stark/src/prover.rs:94-104 alike; matrices of different heights in
 * one batch and several batches are allowed).  Samples the batch challenge from `chal`, computes the
 * opened values and runs bf_prove (fri/src/prover.rs:19-63) on the reduced openings.
 *   rounds[r]   committed batches (Pcs::ProverData), in the order the verifier will list them
 *   n_points[k] number of opening points of matrix k, k running over (round, matrix)
 *   points      4 canonical words per point, in the same order
 *   opened_out  EF4 values in (round, matrix, point, column) order
 *   proof_out   the FriProof in TSPF v1 words (commit-phase round count first; DESIGN.md "Proof
 *               format"); per query the input proof holds one BatchOpening per round
 * TS_ERR_BUFFER if a buffer is too small (the needed sizes are still written). */
ts_status ts_pcs_open(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal, uint32_t n_rounds,
                      const ts_pcs_data* const* rounds, const uint32_t* n_points,
                      const uint32_t* points, uint32_t* opened_out, size_t opened_cap_words,
                      size_t* n_opened_words, uint32_t* proof_out, size_t proof_cap_words,
                      size_t* n_proof_words);

/* bf_prove (fri/src/prover.rs:19-63) on its own, as fri/tests/fri.rs:51-147 drives it: `n_inputs`
 * host vectors of EF4 (4 words per element; BabyBear values are embedded as (v, 0, 0, 0)) of
 * strictly descending power-of-two lengths 2^log_lens[k]; the "input opening proof" of a query is
 * the literal reduced openings [(log_height, value)] (fri.rs:109-118).  Any challenger kind
 * (ts_chal_new: Blake3 or the test permutation, EF4 or BabyBear samples).  The proof is the FriProof
 * in TSPF v1 words with that input-proof shape.  ts_fri_verify = verify_shape_and_sample_challenges
 * + verify_challenges (fri/src/verifier.rs:20-98) for such a proof; verdict codes as ts_verify. */
ts_status ts_fri_prove(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal, uint32_t n_inputs,
                       const uint32_t* log_lens, const uint32_t* const* inputs, uint32_t* proof_out,
                       size_t cap_words, size_t* n_words_out);
ts_status ts_fri_verify(const ts_fri_config* cfg, ts_challenger* chal, const uint32_t* proof,
                        size_t n_words, int* verdict);

/* FriGenericConfig::fold_matrix, two_adic_pcs.rs:116-147 (host in, host out; 2h EF4 -> h EF4) */
ts_status ts_fri_fold(ts_ctx* ctx, const uint32_t* in, uint64_t h, const uint32_t beta[4],
                      uint32_t* out);
/* The same on DEVICE vectors (16-byte aligned), enqueued on the context's stream: what a caller that
 * keeps its FRI vectors in HBM binds, and what `bench.py --workload fold` times against the reference's only
 * benchmark (fri/benches/fold_even_odd.rs:14-46). */
ts_status ts_fri_fold_device(ts_ctx* ctx, const uint32_t* in_dev, uint64_t h, const uint32_t beta[4],
                             uint32_t* out_dev);

/* ------------------------------------------------------------------ challenger */
/* BfChallenger::new, basic/src/challenger/mod.rs:122-137.  permutation: 0 = Blake3Permutation
 * (mod.rs:23-49), 1 = reverse-the-state test permutation (fri/tests/fri.rs:35-48).
 * sample_ext: 1 = F is EF4 (as in uni-stark/tests/fib_air.rs:108), 0 = BabyBear. */
ts_status ts_chal_new(int permutation, int sample_ext, ts_challenger** out);
ts_status ts_chal_clone(const ts_challenger* c, ts_challenger** out);
void ts_chal_free(ts_challenger* c);
void ts_chal_observe(ts_challenger* c, uint32_t word);                   /* mod.rs:183-194 */
void ts_chal_observe_commitment(ts_challenger* c, const uint32_t d[8]);  /* mod.rs:197-223 */
void ts_chal_sample(ts_challenger* c, uint32_t out[4]);                  /* mod.rs:261-313 */
uint64_t ts_chal_sample_bits(ts_challenger* c, uint32_t bits);           /* mod.rs:341-348 */
int ts_chal_check_witness(ts_challenger* c, uint32_t bits, uint32_t witness); /* mod.rs:108-114 */
/* mod.rs:95-105; TS_ERR_INVARIANT when no witness in [0, 4096) ("failed to find witness") */
ts_status ts_chal_grind(ts_challenger* c, uint32_t bits, uint32_t* witness);
/* state export for tests: state[16], n_in, in[8], n_out, out[8] (34 words) */
void ts_chal_state(const ts_challenger* c, uint32_t out[34]);

/* ------------------------------------------------------------------ prove */
/* uni_stark::prove(config, air, challenger, trace, public_values) -> Proof
 * (uni-stark/src/prover.rs:25-119).  `trace` is consumed.  The proof is written in the TSPF v1
 * wire format: header, commitments, opened_values, opening_proof.  Like a release
 * build of the reference, it does not run check_constraints (prover.rs:40-41 is debug-only). */
ts_status ts_prove(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                   ts_matrix* trace, const uint32_t* public_values, uint32_t n_public,
                   uint32_t* proof_out, size_t cap_words, size_t* n_words_out);

/* ---- one proof over the GPUs of a node (BASELINE config 4) ----
 * The library does no networking of its own: the host hands it the collectives (RCCL through
 * torch.distributed in tap-stark_amd/dist.py; any MPI-like layer can stand in).  Buffers are DEVICE
 * pointers of the calling rank's GPU.  A callback is ordered on `hip_stream` (the context's
 * stream): it either enqueues its work there or synchronises the stream first, and when it returns
 * later work on that stream sees the result.  Return 0 on success. */
typedef struct {
    int rank, world;
    void* user;
    /* recv_dev receives world * bytes_per_rank bytes, the contributions in rank order */
    int (*all_gather)(void* user, const void* send_dev, void* recv_dev, size_t bytes_per_rank,
                      void* hip_stream);
    int (*broadcast)(void* user, void* buf_dev, size_t bytes, int root, void* hip_stream);
    /* optional (may be NULL): called on a rank whose ts_prove_sharded fails, so that its peers'
     * pending collectives fail too instead of waiting for ever */
    void (*abort)(void* user);
} ts_comm;

/* Native communicators (csrc/comm.cpp) for hosts without Python.
 * RCCL over xGMI, one process or thread per GPU: rank 0 calls ts_rccl_unique_id and passes the 128
 * bytes to its peers by any channel; every rank then calls ts_comm_rccl_create with its context
 * (the communicator binds to the context's device; collectives are enqueued on the context's
 * stream, no host synchronisation).  librccl is bound at run time; TS_ERR_UNSUPPORTED if absent. */
typedef struct ts_rccl_comm ts_rccl_comm;
int ts_rccl_available(void);
ts_status ts_rccl_unique_id(uint8_t out[128]);
ts_status ts_comm_rccl_create(ts_ctx* ctx, const uint8_t unique_id[128], int rank, int world,
                              ts_comm* out, ts_rccl_comm** handle);
void ts_comm_rccl_destroy(ts_rccl_comm* handle);
/* What RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice /
 * ncclGetVersion; -1 where the symbol is missing or the communicator was aborted) beside what it was
 * created with.  ts_comm_rccl_create already refuses (TS_ERR_COMM) a communicator whose count or rank
 * differ from the arguments; this is for launchers that want to print them. */
typedef struct {
    int rank, world;                 /* as passed to ts_comm_rccl_create */
    int comm_count, comm_user_rank;  /* as RCCL reports them */
    int comm_device, rccl_version, aborted;
    int checked;  /* 1: ts_comm_rccl_create confirmed rank / world with ncclCommUserRank / ncclCommCount;
                   * 0: this librccl lacks them, the check could not run */
} ts_rccl_info;
ts_status ts_comm_rccl_info(const ts_rccl_comm* handle, ts_rccl_info* out);
/* In-process group: `world` ranks = `world` host threads of one process, each with its own
 * context (same device or one device each: copies go device to device, peer to peer over xGMI).
 * Every rank's thread takes its ts_comm with ts_comm_local_get. */
typedef struct ts_comm_group ts_comm_group;
ts_status ts_comm_local_group_create(int world, ts_comm_group** out);
ts_status ts_comm_local_get(ts_comm_group* group, int rank, ts_comm* out);
void ts_comm_local_group_destroy(ts_comm_group* group);
/* A group is ONE-SHOT with respect to failure: after ts_comm.abort on any rank, or after a rendezvous
 * timed out (a peer died silently; 600 s unless TS_COMM_TIMEOUT_S or ..._set_timeout says otherwise),
 * every collective on it returns an error.  ts_comm_local_group_reset makes it usable again; call it
 * only once EVERY rank's ts_prove_sharded has returned (no thread may still be inside a collective). */
ts_status ts_comm_local_group_reset(ts_comm_group* group);
ts_status ts_comm_local_group_set_timeout(ts_comm_group* group, int seconds);

/* Throughput mode in one call: n_proofs independent proofs (uni-stark/src/prover.rs:25-35, one trace each, a
 * fresh BfChallenger each) of one AIR on n_lanes contexts of ONE device, one host thread per lane inside
 * the call; proof i runs on lane lane_of[i] (< n_lanes) with traces[i] (consumed; it must have been created
 * on that lane's context) and airs[lane_of[i]] (compiled on that context).  No two proofs start within
 * gate_ms of each other (0 = no gate; a quarter of one proof's solo time keeps the lanes in complementary
 * phases).  last_proof_out receives the proof of the highest index; start_ms_out / wall_ms_out (n_proofs each,
 * may be NULL): when each ts_prove-equivalent started, relative to the call's start, and how long it took.
 * The start is stamped inside the gate's critical section, so sorted starts are >= gate_ms apart.
 * Null arrays, n_lanes of 0 or > 64, one context on two lanes, lane_of[i] >= n_lanes or an invalid cfg
 * return TS_ERR_INVALID before any lane starts.  A trace made on another context, or of another width than
 * the lane's AIR, fails its lane with TS_ERR_INVALID and is not consumed.  A failing lane stops the others;
 * the call returns the status of the lowest-index failed lane.
 * What a host with cheap threads does itself (examples/prove_stream.cpp); a host behind an interpreter
 * lock gets the loop without paying its lock per proof. */
ts_status ts_prove_stream(ts_ctx* const* ctxs, const ts_air* const* airs, uint32_t n_lanes,
                          const ts_fri_config* cfg, ts_matrix* const* traces, const uint32_t* lane_of,
                          uint32_t n_proofs, const uint32_t* public_values, uint32_t n_public, double gate_ms,
                          uint32_t* last_proof_out, size_t cap_words, size_t* n_words_out,
                          double* start_ms_out, double* wall_ms_out);

/* Many statements in one call, every proof returned: n_items independent uni_stark::prove calls
 * (uni-stark/src/prover.rs:25-39: each with its own trace, public values and challenger, each returning its
 * proof) on n_lanes contexts of ONE device, one host thread per lane inside the call, as ts_prove_stream.
 * Item i runs on lane items[i].lane with airs[lane] (lanes may carry different AIRs); a lane takes its
 * items in index order.  Item i's proof words and final challenger state are those ts_prove gives for the
 * same context, AIR, trace, public values and a clone of the same challenger.
 *   trace / host_trace  exactly one is set.  `trace` must have been made on the lane's context and is
 *                       consumed (each handle in at most one item).  `host_trace` (height x width canonical
 *                       row-major values; height a power of two) is uploaded on the lane's own stream just
 *                       before its proof, so that one lane's upload overlaps the others' proofs; pinned
 *                       memory (ts_host_alloc) gets the full link rate.  THE HOST BUFFER MUST STAY UNTOUCHED
 *                       UNTIL THE CALL RETURNS.
 *   public_values       n_public values; n_public and the trace width must match airs[lane] (ts_air_info).
 *   challenger          NULL = a fresh BfChallenger(Blake3, sample_ext) as ts_prove_stream uses; otherwise
 *                       a CLONE of it is used and the caller's object is never modified (one object may
 *                       serve several items; it must not change during the call).
 *   proof_out           cap_words words; a finished proof is copied there at once (the library keeps at
 *                       most one proof per lane).
 * Outputs: status (-1 = not attempted), n_words (also on TS_ERR_BUFFER: the size needed), final_state (the
 * ts_chal_state layout of the challenger after the proof), start_ms / wall_ms (relative to the call's
 * start; the start is stamped inside the gate's critical section, so sorted starts are >= gate_ms apart),
 * proof_blake3 (Blake3 of the proof words as little-endian bytes, computed on the lane thread, only with
 * TS_BATCH_DIGEST in flags).
 * Failures: a bad item (width or n_public not the AIR's, a consumed or repeated trace, both or neither
 * trace source, lane >= n_lanes, a null buffer, a proof buffer too small) fails in its own status and the
 * other items still run; TS_ERR_HIP / TS_ERR_OOM / TS_ERR_INVARIANT stop that item's lane (its later items
 * stay at -1).  Returns TS_OK if every item is TS_OK, else the status of the lowest-index failed item;
 * ts_last_error of the item's lane context holds the text.  Null arrays, n_lanes of 0 or > 64, an invalid
 * cfg or any struct_size != sizeof(ts_batch_item) return TS_ERR_INVALID before any trace is consumed or any
 * item written. */
typedef struct {
    uint32_t struct_size;            /* = sizeof(ts_batch_item): another layout refuses the whole call */
    uint32_t lane;                   /* < n_lanes */
    ts_matrix* trace;                /* device trace made on the lane's context (consumed) ... */
    const uint32_t* host_trace;      /* ... OR canonical row-major host values, height x width */
    uint64_t height;                 /* of host_trace */
    uint32_t width;                  /* of host_trace */
    uint32_t n_public;
    const uint32_t* public_values;
    const ts_challenger* challenger; /* NULL = fresh; else cloned, never modified */
    uint32_t* proof_out;
    size_t cap_words;
    /* outputs */
    ts_status status;
    size_t n_words;
    uint32_t proof_blake3[8];
    uint32_t final_state[34];
    double start_ms, wall_ms;
} ts_batch_item;
#define TS_BATCH_DIGEST 1u
ts_status ts_prove_batch(ts_ctx* const* ctxs, const ts_air* const* airs, uint32_t n_lanes,
                         const ts_fri_config* cfg, ts_batch_item* items, uint32_t n_items, double gate_ms,
                         uint32_t flags);

/* prove() with the work of ONE proof split over comm->world ranks, one GPU each: rank g owns the
 * bit-reversed LDE rows [g N/G, (g+1) N/G) -- whole cosets, so world must be a power of two
 * <= 2^log_blowup (TS_ERR_UNSUPPORTED otherwise) -- with their Merkle sub-trees, FRI slabs and
 * queries.  `trace_rows` holds natural rows [g n/G, (g+1) n/G) of the trace and is consumed.
 * Every rank must pass a challenger in the same state; every rank receives the whole proof, which
 * is bit-identical to ts_prove's on the whole trace.  FRI rounds stay sharded while a rank holds
 * >= 2^min_local_log values. */
typedef struct {
    uint32_t struct_size;      /* = sizeof(ts_shard_options): a caller built against another layout of this
                                  struct (ABI 4 had a field here that did nothing) is refused with
                                  TS_ERR_INVALID instead of having its fields read as something else */
    uint32_t min_local_log;    /* 0 = default (12) */
    uint32_t trace_replicated; /* 1: `trace_rows` is the WHOLE trace on every rank (e.g. made by
                                  ts_trace_* on each device); the trace all-gather is skipped */
    uint32_t local_quotient;   /* 1: every rank evaluates the quotient (uni-stark/src/prover.rs:65-80) on
                                  its OWN cosets and derives its slab of the chunk LDEs from that: no rank
                                  waits for the owner of the quotient domain, no chunk broadcast.  Needs
                                  2^log_blowup / world >= quotient degree (else ignored).  The same proof as
                                  ts_prove for EVERY trace: for one that violates its constraints (ts_prove,
                                  like a release build of the reference, still hands out a proof, which the
                                  verifier rejects) constraints / Z_H is no polynomial, the mixed chunks are
                                  not low-degree, FRI's final polynomial is not constant
                                  (fri/src/prover.rs:129-134) -- on every rank alike -- and all ranks redo the
                                  quotient through the broadcast path (ts_ctx_stat 5 counts it) */
} ts_shard_options;
ts_status ts_prove_sharded(ts_ctx* ctx, const ts_fri_config* cfg, const ts_comm* comm,
                           const ts_air* air, ts_challenger* chal, ts_matrix* trace_rows,
                           const uint32_t* public_values, uint32_t n_public,
                           const ts_shard_options* options /* NULL = defaults */,
                           uint32_t* proof_out, size_t cap_words, size_t* n_words_out);

/* check_constraints (uni-stark/src/check_constraints.rs:11-39; what a debug build of prove() runs
 * first, prover.rs:40-41) on the GPU.  `trace` is NOT consumed.  *first_violation = -1 if every
 * constraint holds on every row, else row * 65536 + constraint index of the first failure. */
ts_status ts_check_constraints(ts_ctx* ctx, const ts_air* air, const ts_matrix* trace,
                               const uint32_t* public_values, uint32_t n_public,
                               int64_t* first_violation);

/* The same for an AIR with preprocessed columns (check_constraints.rs:11-39 with the PairBuilder's second
 * matrix): `preprocessed` is the uploaded height x preprocessed_width matrix, NOT consumed; NULL exactly for an
 * AIR with preprocessed_width == 0, where the answer is ts_check_constraints'. */
ts_status ts_check_constraints_pre(ts_ctx* ctx, const ts_air* air, const ts_matrix* preprocessed,
                                   const ts_matrix* trace, const uint32_t* public_values, uint32_t n_public,
                                   int64_t* first_violation);

/* ------------------------------------------------------------------ preprocessed columns */
/* An AIR with preprocessed columns (tape version 2) is proved against a KEY: the ordinary ts_pcs_data of
 *   ts_pcs_commit(ctx, cfg, 1, {the height x preprocessed_width matrix}, {1}, root, &key)
 * made once, never consumed, reusable by any number of proofs on its context; the verifier holds `root`.
 * The reference's AIR language has such columns but its prove / verify pass preprocessed_width 0
 * (uni-stark/src/prover.rs:46, verifier.rs:40), so the transcript is build-defined (DESIGN.md "Preprocessed
 * columns"): observe(key root); commit + observe the trace; alpha; quotient over (key LDE, trace LDE); commit +
 * observe the chunks; zeta; Pcs::open of three rounds -- key at {zeta, zeta w_n}, trace at {zeta, zeta w_n},
 * chunks at {zeta} -- with the round order and num_reduced offsets of ts_pcs_open for that argument list
 * (fri/src/two_adic_pcs.rs:371,383).  Proof: TSPF v3.
 *
 * ts_quotient_chunks_pre extends ts_quotient_chunks (prover.rs:122-194), ts_prove_pre extends ts_prove
 * (prover.rs:25-119; `trace` consumed as there), ts_verify_pre extends ts_verify (verifier.rs:19-161; host only,
 * verdict codes as ts_verify).
 * TS_ERR_INVALID, with text in ts_last_error and before any device work (the trace is then treated as ts_prove
 * treats its trace on that status): a null argument; a key that does not hold exactly one matrix, whose width is
 * not the AIR's preprocessed_width, whose LDE height is not trace height << log_blowup, or that was made on
 * another context; for ts_verify_pre a proof whose header version is not 3 (*verdict = 9) or whose
 * preprocessed_width word is not the AIR's (*verdict = 1).
 * For an AIR with preprocessed_width == 0 the key / root / matrix argument must be NULL and every call gives what
 * its unsuffixed counterpart gives (the proof differs in its v3 header alone).
 * The calls that take no key -- ts_prove, ts_quotient_chunks, ts_check_constraints, ts_verify, ts_prove_stream,
 * ts_prove_batch (in the item's status), ts_prove_sharded, ts_prove_tap, ts_prove_tap_sharded, ts_verify_tap --
 * return TS_ERR_UNSUPPORTED for an AIR with preprocessed_width > 0, and ts_proof_to_postcard does for a v3
 * proof (the reference's OpenedValues, uni-stark/src/proof.rs, has no preprocessed fields). */
ts_status ts_quotient_chunks_pre(ts_ctx* ctx, const ts_pcs_data* preprocessed, const ts_pcs_data* trace_data,
                                 uint32_t log_blowup, const ts_air* air, const uint32_t* public_values,
                                 uint32_t n_public, const uint32_t alpha[4], ts_matrix** chunks_out);
ts_status ts_prove_pre(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                       const ts_pcs_data* preprocessed /* not consumed */, ts_matrix* trace /* consumed */,
                       const uint32_t* public_values, uint32_t n_public, uint32_t* proof_out, size_t cap_words,
                       size_t* n_words_out);
ts_status ts_verify_pre(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                        const uint32_t preprocessed_root[8], const uint32_t* proof, size_t n_words,
                        const uint32_t* public_values, uint32_t n_public, int* verdict);

/* ------------------------------------------------------------------ verify (host only) */
/* uni_stark::verify (uni-stark/src/verifier.rs:19-25; pcs.verify fri/src/two_adic_pcs.rs:421-534;
 * fri/src/verifier.rs:20-165).  Needs no GPU: `air` may come from ts_air_compile(NULL, ...).
 * *verdict: 0 accept, 1 InvalidProofShape, 2 InvalidOpeningArgument (FRI shape), 3 InvalidPowWitness,
 * 4 input-MMCS error, 5 commit-phase MMCS error, 6 FinalPolyMismatch, 7 OodEvaluationMismatch,
 * 8 folded-evaluation mismatch (the reference asserts), 9 malformed proof buffer. */
ts_status ts_verify(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                    const uint32_t* proof, size_t n_words, const uint32_t* public_values,
                    uint32_t n_public, int* verdict);

/* Pcs::verify (fri/src/two_adic_pcs.rs:421-534 with fri/src/verifier.rs:20-165) for any rounds x
 * matrices x points: the counterpart of ts_pcs_open, host only.  Arguments follow ts_pcs_open:
 *   commitments   n_rounds x 8 words
 *   mats_per_round[r], then per matrix k in (round, matrix) order: log_degrees[k] (log2 of the
 *   committed matrix's height), widths[k], n_points[k]; points: 4 words each; opened_values: EF4 in
 *   (round, matrix, point, column) order; fri_proof: what ts_pcs_open wrote.
 * The challenger must be in the state the prover's had when ts_pcs_open was called.
 * *verdict as for ts_verify (0 accept, 1 shape, 2 FRI shape, 3 PoW, 4 input MMCS, 5 commit-phase
 * MMCS, 6 final poly, 8 folded evaluation, 9 malformed). */
ts_status ts_pcs_verify(const ts_fri_config* cfg, ts_challenger* chal, uint32_t n_rounds,
                        const uint32_t* commitments, const uint32_t* mats_per_round,
                        const uint32_t* log_degrees, const uint32_t* widths, const uint32_t* n_points,
                        const uint32_t* points, const uint32_t* opened_values,
                        const uint32_t* fri_proof, size_t n_words, int* verdict);

/* ------------------------------------------------------------------ proof wire format (host only) */
/* TSPF v1 words <-> the postcard encoding of the reference's serde proof types
 * (uni-stark/src/proof.rs:17-38, fri/src/proof.rs:8-33, fri/src/two_adic_pcs.rs:63-68; postcard is
 * the carrier the reference names: uni-stark/Cargo.toml:44, uni-stark/tests/mul_air.rs:133-137).
 * Field order and element encodings are the reference's; the commitment (one 32-byte root) and the
 * MMCS opening proof (sibling path) are this build's Merkle types.
 * TS_ERR_INVALID for a malformed input, TS_ERR_BUFFER if the output does not fit (size still set). */
ts_status ts_proof_to_postcard(const uint32_t* proof, size_t n_words, uint8_t* out, size_t cap_bytes,
                               size_t* n_bytes_out);
ts_status ts_proof_from_postcard(const uint8_t* bytes, size_t n_bytes, uint32_t* proof_out,
                                 size_t cap_words, size_t* n_words_out);
/* The postcard bytes do not record which MMCS produced them.  ts_proof_from_postcard infers the TSPF
 * version from the number of roots per commitment (one -> v1, several -> v2), which is wrong for the
 * one case of a proof over taptrees (v2) made with num_queries = 1.  tspf_version = 1 or 2 asks for
 * that framing explicitly (1 refuses several roots; 2 always writes the num_queries header word);
 * 0 infers as above. */
ts_status ts_proof_from_postcard_v(const uint8_t* bytes, size_t n_bytes, int tspf_version,
                                   uint32_t* proof_out, size_t cap_words, size_t* n_words_out);

/* ------------------------------------------------------------------ taptree-compatible MMCS
 * The reference's real BFMmcs (basic/src/mmcs/taptree_mmcs.rs:24-119) commits to Bitcoin taptrees:
 * tagged SHA-256 (BIP-341 TapLeaf / TapBranch with lexicographically sorted children), a complete
 * binary tree over one script leaf per row (basic/src/tcs/builder.rs:38-93), one tree per query.
 * Digests cross the ABI as 32 bytes (the byte string Bitcoin hashes), not as words.
 *
 * The lock scripts inside a leaf script come from un-vendored crates (bitcomm / primitives) and are
 * therefore SUPPLIED BY THE CALLER as bytes; ts_tap_winternitz_lock_script is a stand-in built from
 * the reference's local copy of the construction (scripts/src/bit_comm/winternitz.rs:171-274,
 * bit_comm_u32.rs:80-85, u32/u32_std.rs:122-173).  Script execution against a witness
 * (tcs/mod.rs:143-147) is out of scope. */
typedef struct ts_taptree ts_taptree;
typedef struct ts_tap_mmcs_data ts_tap_mmcs_data;
/* TapLeaf hash of a script (NodeInfo::new_leaf_with_ver(script, TapScript), builder.rs:24-29), host */
ts_status ts_tapleaf_hash(const uint8_t* script, size_t len, uint8_t out[32]);
/* TapNodeHash::from_node_hashes(a, b) (complete_taptree.rs:57-60), host */
ts_status ts_tapbranch_hash(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]);
/* lock script of a bit commitment over u32_count limbs (1 = BabyBear, 4 = EF4), host */
ts_status ts_tap_winternitz_lock_script(const uint8_t* secret, size_t secret_len, uint32_t u32_count,
                                        uint8_t* out, size_t cap, size_t* len_out);
/* CommitedLeaf::generate_script (tcs/mod.rs:197-225), host: lock_offsets has n_evals + 2 entries
 * (index lock, then one lock per evaluation); values = n_evals * u32_size canonical limbs */
ts_status ts_tap_leaf_script(const uint8_t* lock_scripts, const uint64_t* lock_offsets, uint32_t n_evals,
                             uint32_t u32_size, uint64_t index, const uint32_t* values, uint8_t* out,
                             size_t cap, size_t* len_out);
/* CompleteTaptree::new_with_scripts (complete_taptree.rs:67-75): script i = bytes
 * [offsets[i], offsets[i+1]); n_leaves must be a power of two (builder.rs:40).  Hashed on the device. */
ts_status ts_taptree_from_scripts(ts_ctx* ctx, const uint8_t* scripts, const uint64_t* offsets,
                                  uint64_t n_leaves, ts_taptree** out);
/* CompleteTaptree::combine (complete_taptree.rs:90-133): leaves of `a` keep their indices, those of
 * `b` follow; the inputs stay valid */
ts_status ts_taptree_combine(const ts_taptree* a, const ts_taptree* b, ts_taptree** out);
ts_status ts_taptree_info(const ts_taptree* t, uint64_t* leaf_count, uint8_t root[32]);
/* get_leaf_proof (complete_taptree.rs:155-159): leaf hash + sibling path, leaf-most first */
ts_status ts_taptree_leaf_proof(const ts_taptree* t, uint64_t index, uint8_t leaf_hash[32],
                                uint8_t* path, uint32_t cap_nodes, uint32_t* depth);
/* verify_inclusion (complete_taptree.rs:53-64), host; 1 = included */
int ts_taptree_verify_inclusion(const uint8_t root[32], const uint8_t leaf_hash[32], const uint8_t* path,
                                uint32_t depth);
void ts_taptree_free(ts_taptree* t);
/* TapTreeMmcs::commit (taptree_mmcs.rs:101-114 -> tcs/mod.rs:284-292,238-282,339-378): num_queries
 * trees over the rows of the matrices (tallest first, power-of-two heights, consumed).  u32_size =
 * F::U32_SIZE (1 or 4): an evaluation is u32_size consecutive columns.  Tree q uses lock scripts
 * [q (1 + n_evals), (q + 1)(1 + n_evals)) of `lock_offsets` (num_queries (1 + n_evals) + 1 entries,
 * n_evals = total width / u32_size).  The leaf scripts are assembled and hashed on the device.
 * roots_out: num_queries x 32 bytes (Commitment = Vec<TreeRoot>). */
ts_status ts_tap_mmcs_commit(ts_ctx* ctx, uint32_t n_mats, ts_matrix* const* mats, uint32_t u32_size,
                             uint32_t num_queries, const uint8_t* lock_scripts,
                             const uint64_t* lock_offsets, uint8_t* roots_out, ts_tap_mmcs_data** out);
ts_status ts_tap_mmcs_info(const ts_tap_mmcs_data* d, uint32_t* n_mats, uint32_t* log_max_height,
                           uint32_t* n_evals, uint32_t* num_queries);
/* open_batch (taptree_mmcs.rs:46-75): rows of every matrix at index >> bits_reduced (concatenated),
 * the sibling path in tree query_times_index (log_max_height x 32 bytes) and, if script_len is not
 * NULL, the opened leaf's script (CommitedProof.leaf, tcs/mod.rs:103-108) */
ts_status ts_tap_mmcs_open_batch(const ts_tap_mmcs_data* d, uint32_t query_times_index, uint64_t index,
                                 uint32_t* rows_out, uint8_t* path_out, uint8_t* script_out,
                                 size_t script_cap, size_t* script_len);
/* verify_batch (taptree_mmcs.rs:77-99), host: rebuilds the leaf from the tree's lock scripts
 * (n_evals + 2 offsets), the index and the opened values, and checks its inclusion under `root` */
ts_status ts_tap_mmcs_verify_batch(const uint8_t* lock_scripts, const uint64_t* lock_offsets,
                                   uint32_t n_evals, uint32_t u32_size, uint64_t index,
                                   const uint32_t* opened_values, const uint8_t* path, uint32_t depth,
                                   const uint8_t root[32], int* ok);
void ts_tap_mmcs_free(ts_tap_mmcs_data* d);

/* uni_stark::prove / verify with TapTreeMmcs as the MMCS of the PCS and of FRI -- the reference's
 * own configuration (uni-stark/tests/fib_air.rs:117-131): every commitment is cfg->num_queries
 * taptrees, the challenger observes all their roots (basic/src/challenger/mod.rs:211-223), query q
 * opens in tree q (fri/src/prover.rs:50-56).  The lock scripts are one flat table in the order the
 * reference's bit-commitment manager hands them out (tcs/mod.rs:251-260), i.e. commit order:
 *   trace: Q (1 + width); quotient chunks: Q (1 + 4 quotient_degree); each of the log2(n) FRI rounds:
 *   Q (1 + 2)  -- per tree: the index lock first, then one lock per evaluation
 * (n_scripts entries, n_scripts + 1 offsets).  Proof = TSPF v2: v1 with a sixth header word
 * (num_queries) and num_queries x 8 words per commitment, a digest being its 32 bytes read as
 * little-endian words.  ts_verify_tap is host only; verdict codes as ts_verify. */
ts_status ts_prove_tap(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                       ts_matrix* trace, const uint32_t* public_values, uint32_t n_public,
                       const uint8_t* lock_scripts, const uint64_t* lock_offsets, size_t n_scripts,
                       uint32_t* proof_out, size_t cap_words, size_t* n_words_out);
/* ts_prove_tap with the commitments of ONE proof split over comm->world GPUs BY TREE (the
 * reference clones the tree per query, tcs/mod.rs:284-292: the trees of a commitment are independent).
 * Every rank passes the WHOLE trace and a challenger in the same state and repeats the numeric
 * pipeline (milliseconds); rank g builds trees [g per, (g+1) per), per = ceil(num_queries / world), of
 * every commitment -- the SHA-256 of kilobyte leaf scripts, which is where the seconds go -- the roots
 * are all-gathered (32 bytes per tree), and query q is answered by the rank that owns tree q.  Every
 * rank receives the whole proof, identical to ts_prove_tap's.  Only comm->all_gather is used. */
ts_status ts_prove_tap_sharded(ts_ctx* ctx, const ts_fri_config* cfg, const ts_comm* comm, const ts_air* air,
                               ts_challenger* chal, ts_matrix* trace, const uint32_t* public_values,
                               uint32_t n_public, const uint8_t* lock_scripts, const uint64_t* lock_offsets,
                               size_t n_scripts, uint32_t* proof_out, size_t cap_words, size_t* n_words_out);
ts_status ts_verify_tap(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                        const uint32_t* proof, size_t n_words, const uint32_t* public_values,
                        uint32_t n_public, const uint8_t* lock_scripts, const uint64_t* lock_offsets,
                        size_t n_scripts, int* verdict);

/* Measurement aid: the whole-chip rate of NTT butterflies (kind 0), Blake3 compressions (kind 1) or
 * SHA-256 compressions (kind 2) with no memory traffic -- kinds 3 / 4: the butterflies with the LDS traffic
 * of a contiguous NTT pass added (4-byte / 16-byte accesses; measurement of what LDS costs in power), kind 5: the
 * butterflies on a Plantard-form twiddle (8 instructions instead of 10) --, using the library's own arithmetic -- the integer-ALU ceiling bench.py
 * reports beside the achieved rates. */
ts_status ts_bench_alu(ts_ctx* ctx, int kind, double* units_per_second);

/* Measurement aid: one stage of the path in a sustained loop on resident, arbitrary data, mean
 * milliseconds per repetition (HIP events on the context's stream).  stage 0: the coset LDE of a
 * 2^log_n x width matrix (fri/src/two_adic_pcs.rs:233-241: all NTT passes, every coset); stage 1: the
 * hashing of BFMmcs::commit (basic/src/mmcs/bf_mmcs.rs:22-35) over a 2^(log_n + log_blowup) x width
 * matrix; stages 2, 3, 4: one pass of that LDE alone (inverse contiguous stages / strided middle /
 * forward contiguous stages; log_n > 12).  What tools/power_per_stage.py samples clock and power over, per kernel family and per
 * working-set size. */
ts_status ts_bench_stage(ts_ctx* ctx, int stage, unsigned log_n, uint32_t width, unsigned log_blowup,
                         uint32_t reps, double* ms_per_rep);

/* ------------------------------------------------------------------ challenge-phase (aux) columns
 * An AIR of tape version 3 is proved in two phases (build-defined like the preprocessed prove; reference
 * prover.rs:46 stops at one).  ts_prove_aux: (1) commit the trace, observe its root; (2) sample n_challenges
 * extension elements as alpha is sampled; (3) call `aux_fn` with the still-live trace and the challenge words;
 * it returns the height x aux_width aux matrix (row-major, made on `ctx`; consumed) and n_exposed words;
 * (4) commit the aux matrix (natural domain), observe its root, then each exposed word; (5) alpha, the quotient
 * over (aux LDE, trace LDE) with public values ++ challenges ++ exposed; (6) zeta; (7) open three rounds: aux at
 * {zeta, zeta omega}, trace at {zeta, zeta omega}, chunks at {zeta}.  Proof = TSPF v4; it
 * has no postcard form (TS_ERR_UNSUPPORTED).
 * A non-zero status from the callback ends the call with that status, and the last error names the callback.
 * An aux matrix of another shape or context: TS_ERR_INVALID.  The trace is consumed as by ts_prove.
 * For an AIR with aux_width 0, aux_fn must be NULL and the proof is that of ts_prove but for the header.
 * ts_verify_aux (host only) checks the proof and hands back the exposed words; the STATEMENT about them (for
 * LogUp: "the sum is zero") is the caller's to check afterwards.  A proof of another TSPF version (*verdict = 9)
 * or with other header words than the AIR's (*verdict = 1) is refused as an argument, TS_ERR_INVALID.
 * Every call that takes no aux source returns TS_ERR_UNSUPPORTED for an AIR with aux_width > 0. */
typedef ts_status (*ts_aux_fn)(void* user, ts_ctx* ctx, const ts_matrix* trace /* not consumed */,
                               const uint32_t* challenges /* 4*n_challenges canonical words */, uint32_t n_challenges,
                               ts_matrix** aux_out /* consumed by the prover */, uint32_t* exposed_out);
ts_status ts_air_aux_info(const ts_air* air, uint32_t* aux_width, uint32_t* n_challenges, uint32_t* n_exposed);
/* aux_data: the committed aux trace (one matrix, ts_pcs_commit on the natural domain); NULL iff aux_width 0 */
ts_status ts_quotient_chunks_aux(ts_ctx* ctx, const ts_pcs_data* aux_data, const ts_pcs_data* trace_data,
                                 uint32_t log_blowup, const ts_air* air, const uint32_t* public_values,
                                 uint32_t n_public, const uint32_t* challenges, const uint32_t* exposed,
                                 const uint32_t alpha[4], ts_matrix** chunks_out);
/* aux: the uploaded row-major aux matrix of the trace's height; NULL iff aux_width 0 */
ts_status ts_check_constraints_aux(ts_ctx* ctx, const ts_air* air, const ts_matrix* aux, const ts_matrix* trace,
                                   const uint32_t* public_values, uint32_t n_public, const uint32_t* challenges,
                                   const uint32_t* exposed, int64_t* first_violation);
ts_status ts_prove_aux(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                       ts_matrix* trace /* consumed */, const uint32_t* public_values, uint32_t n_public,
                       ts_aux_fn aux_fn, void* user, uint32_t* proof_out, size_t cap_words, size_t* n_words_out);
ts_status ts_verify_aux(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal, const uint32_t* proof,
                        size_t n_words, const uint32_t* public_values, uint32_t n_public, uint32_t* exposed_out,
                        uint32_t cap_exposed, int* verdict);

/* LogUp aux columns built on the device (csrc/logup.hip).  Two challenges gamma, beta.  Interaction i on row r
 * has the denominator d_i = gamma + sum_j beta^j v_ij(r) and the fraction m_i(r) / d_i.  Interactions are paired:
 * group g holds 2g and 2g+1 (the last group one if K is odd).  Aux columns 4g .. 4g+3 hold h_g(r), the group's
 * sum; the last four hold phi(r) = sum_{r' < r} sum_g h_g(r'), phi(0) = 0; the four exposed words are
 * S = phi(n-1) + sum_g h_g(n-1).  Limits (TS_ERR_INVALID): 1 <= K <= 16 interactions, 1 <= n_values <= 8, columns
 * inside the trace, canonical constants.  A zero denominator gives TS_ERR_INVARIANT with the first row and
 * interaction in the last error, and no output.  TS_LOGUP_BLOCK_ROWS (1 .. 1024, read on every call) shrinks the
 * rows one workgroup owns: a test knob. */
typedef struct { uint32_t kind /* 0 constant (canonical), 1 main column, local row; 2 preprocessed column, local
                                  row: ts_logup_aux_build_pre only */; uint32_t value; } ts_logup_term;
typedef struct { ts_logup_term multiplicity; uint32_t n_values; const ts_logup_term* values; } ts_logup_interaction;
typedef struct { uint32_t struct_size, n_interactions; const ts_logup_interaction* interactions; } ts_logup_spec;
ts_status ts_logup_aux_width(const ts_logup_spec* spec, uint32_t* aux_width);  /* 4 * (ceil(K/2) + 1) */
ts_status ts_logup_aux_build(ts_ctx* ctx, const ts_logup_spec* spec, const ts_matrix* trace,
                             const uint32_t challenges[8], ts_matrix** aux_out, uint32_t exposed_out[4]);
/* The same with terms of kind 2: column `value` of the PREPROCESSED matrix, local row -- a lookup against a fixed
 * table.  `preprocessed` is the row-major n x preprocessed_width matrix of the key's values on this context (not
 * consumed; ts_pcs_commit consumes the matrix a key is made from, so the caller keeps a second upload or a
 * ts_matrix_from_device copy of ts_matrix_device_ptr for this call); NULL is allowed for a spec without kind-2
 * terms.  TS_ERR_INVALID with nothing consumed: a table of another height or context, a column >= its width.
 * Same launches, batching, knob and zero-denominator report as ts_logup_aux_build, which keeps refusing kind 2
 * (as does ts_logup_aux_width: the width is 4 * (ceil(K/2) + 1) whatever the kinds). */
ts_status ts_logup_aux_build_pre(ts_ctx* ctx, const ts_logup_spec* spec, const ts_matrix* preprocessed,
                                 const ts_matrix* trace, const uint32_t challenges[8], ts_matrix** aux_out,
                                 uint32_t exposed_out[4]);

/* The multiplicity column of one table, built in place in the resident main trace (csrc/logup_mult.hip).  Table
 * rows with equal tuples form a class whose representative is its lowest row.  For every row r and lookup l with
 * weight w != 0 whose tuple equals a class's tuple, w is added (in the field) to the representative; afterwards
 * trace[t][out_column] holds that sum mod p -- (p - sum) mod p with `negate` -- on a representative row and 0 on
 * every other row; no other word of the trace changes.  A lookup of weight 0 is skipped.  A lookup of non-zero
 * weight whose tuple is in no table row is a MISS: *n_missing counts them, *first_missing is the least
 * r * n_lookups + l among them (~0 when there are none), the status is TS_OK and the column holds the sums of the
 * lookups that did hit; with n_missing == NULL any miss gives TS_ERR_INVARIANT with the row and the lookup in the
 * last error.  Terms: kind 0 a canonical constant, 1 a main column, 2 a preprocessed column (needs `preprocessed`,
 * row-major, the trace's height, this context, not consumed), all on the local row.  Column words are matched as
 * they are stored; a weight is reduced mod p.  The result is the same words on every run.
 * TS_ERR_INVALID before any device work, nothing written: a wrong struct_size, n_values outside 1 .. 8, n_lookups
 * outside 1 .. 16, negate above 1, a term kind above 2, a column outside its matrix, a non-canonical constant, a
 * kind-2 term without `preprocessed`, a table of another height or context, a trace that is not row-major, is
 * consumed or is from another context, a height outside [1, 2^27], and out_column among the main columns any term
 * reads.  A slot table with no free slot cannot happen (it is half empty) and is reported as TS_ERR_INVARIANT too, the
 * ABI having no status for an internal error: the last error's text ("internal error") tells it from a miss.
 * TS_LOGUP_HASH_BITS (0 .. 32, read on every call, unset = 32) keeps that many low bits of the private hash: a test
 * knob that lengthens probe chains and changes no output. */
typedef struct {
    uint32_t struct_size;
    uint32_t n_values;             /* tuple width, 1 .. 8 */
    const ts_logup_term* table;    /* n_values terms: the table's tuple on row t */
    uint32_t n_lookups;            /* 1 .. 16 */
    const ts_logup_term* lookups;  /* n_lookups * n_values terms: lookup l's tuple on row r */
    const ts_logup_term* weights;  /* n_lookups terms: lookup l's weight on row r (a field element;
                                      constant 1 for a plain lookup, a 0/1 selector column, ...) */
    uint32_t out_column;           /* the MAIN column that receives the result */
    uint32_t negate;               /* 1: store p - sum (what a LogUp table interaction wants), 0: the sum */
} ts_logup_mult_spec;
ts_status ts_logup_multiplicities(ts_ctx* ctx, const ts_logup_mult_spec* spec,
                                  const ts_matrix* preprocessed /* may be NULL */,
                                  ts_matrix* trace /* not consumed; out_column overwritten */,
                                  uint64_t* n_missing, uint64_t* first_missing /* both may be NULL */);

/* ------------------------------------------------------------------ preprocessed AND aux columns together
 * An AIR with preprocessed_width > 0 and aux_width > 0 (a lookup against a FIXED table: the table is in a key
 * the verifier holds the root of).  These four calls extend their _pre and _aux parents and keep their contracts.
 * ts_prove_pre_aux extends ts_prove_pre (the key: committed once, observed first, not consumed, not in the proof)
 * and ts_prove_aux (the challenges, the callback, the aux commit, the exposed words).  Transcript: (1) observe the
 * key's root; (2) commit the trace, observe its root; (3) sample n_challenges; (4) call aux_fn with the live
 * row-major trace; (5) commit the aux matrix, observe its root and each exposed word; (6) alpha; (7) the quotient
 * over (key LDE, aux LDE, trace LDE); (8) commit the chunks; (9) zeta; (10) the batch challenge; (11) open four
 * rounds: key at {zeta, zeta omega}, aux at {zeta, zeta omega}, trace at {zeta, zeta omega}, chunks at {zeta}.
 * Proof = TSPF v5: the v4 header followed by the preprocessed width; opened values
 * preprocessed_local, preprocessed_next, aux_local, aux_next, trace_local, trace_next, chunks; four BatchOpenings
 * per query.  No postcard form (TS_ERR_UNSUPPORTED).
 * TS_ERR_INVALID with the last error set, before any device work and with the trace not consumed: a null
 * argument, a key of another width, height or context.  An aux matrix of another shape or context: TS_ERR_INVALID.
 * With preprocessed_width 0 the key (and the root) must be NULL and the result is that of the _aux call but for the
 * header; with aux_width 0 aux_fn must be NULL and the result is that of the _pre call but for the header.
 * ts_aux_fn is unchanged: a callback that reads the table carries its own row-major copy behind `user`
 * (ts_logup_aux_build_pre above).
 * ts_verify_pre_aux extends ts_verify_pre (preprocessed_root) and ts_verify_aux (exposed_out); host only.  A proof
 * of another TSPF version (*verdict = 9) or with other header words than the AIR's (*verdict = 1) is refused as an
 * argument, TS_ERR_INVALID; every other verify call answers a v5 proof with verdict 9.
 * ts_quotient_chunks_pre_aux extends ts_quotient_chunks_pre / _aux: key and aux_data are each one committed
 * matrix on the natural domain (NULL iff the width is 0).  ts_check_constraints_pre_aux extends
 * ts_check_constraints_pre / _aux: three row-major matrices of one height. */
ts_status ts_prove_pre_aux(ts_ctx* ctx, const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                           const ts_pcs_data* key /* not consumed */, ts_matrix* trace /* consumed */,
                           const uint32_t* public_values, uint32_t n_public, ts_aux_fn aux_fn, void* user,
                           uint32_t* proof_out, size_t cap_words, size_t* n_words_out);
ts_status ts_verify_pre_aux(const ts_fri_config* cfg, const ts_air* air, ts_challenger* chal,
                            const uint32_t preprocessed_root[8], const uint32_t* proof, size_t n_words,
                            const uint32_t* public_values, uint32_t n_public, uint32_t* exposed_out,
                            uint32_t cap_exposed, int* verdict);
ts_status ts_quotient_chunks_pre_aux(ts_ctx* ctx, const ts_pcs_data* key, const ts_pcs_data* aux_data,
                                     const ts_pcs_data* trace_data, uint32_t log_blowup, const ts_air* air,
                                     const uint32_t* public_values, uint32_t n_public, const uint32_t* challenges,
                                     const uint32_t* exposed, const uint32_t alpha[4], ts_matrix** chunks_out);
ts_status ts_check_constraints_pre_aux(ts_ctx* ctx, const ts_air* air, const ts_matrix* preprocessed,
                                       const ts_matrix* aux, const ts_matrix* trace, const uint32_t* public_values,
                                       uint32_t n_public, const uint32_t* challenges, const uint32_t* exposed,
                                       int64_t* first_violation);

/* ------------------------------------------------------------------ lookup AIRs in batch lanes
 * ts_prove_batch for AIRs with preprocessed columns, challenge-phase columns or both: the same lanes (one context
 * and one host thread each, a lane takes its items in index order), the same gate, stamps, digest flag and return
 * value, and per item the device work of ts_prove_pre_aux.  The key belongs to the LANE (lanes[l] goes with
 * ctxs[l] and airs[l]; `lanes` may be NULL when no lane's AIR has preprocessed columns), the aux source to the
 * ITEM, and it may be declarative: a ts_logup_spec the library runs itself on the lane's stream, so that
 * neither a C host nor a host behind an interpreter lock needs a callback per proof.
 * Equality: item i's proof words, exposed words and final challenger state are those of ts_prove_pre_aux for the
 * same context, AIR, key, public values and a clone of the challenger, the trace as it stands after the item's
 * multiplicity fills, and an aux source that returns what the item's source returns.  Hence TSPF v5 for every
 * item, whatever the widths: an AIR with neither width gets what ts_prove_pre_aux gives it with a null key and a
 * null source.
 *   lane, trace | host_trace, height, width, n_public, public_values, challenger, proof_out, cap_words
 *                       as in ts_batch_item.  A device trace must be ROW-MAJOR whenever aux_width > 0 or
 *                       n_mult > 0 (as ts_prove_aux requires).
 *   logup | aux_fn      the aux source: exactly one of them for an AIR with aux_width > 0, both NULL for
 *                       aux_width == 0.  `logup`: the library calls the builder of ts_logup_aux_build_pre with
 *                       (spec, the lane's key_values, the live trace, the challenges); the AIR must have 2
 *                       challenges and 4 exposed words and the spec's aux width must be the AIR's; a kind-2 term
 *                       needs the lane's key_values.  `aux_fn`: called on the LANE's thread with the lane's
 *                       context and aux_user; a non-zero status fails the item with that status.
 *   n_mult, mult        0 .. 8 multiplicity fills of the resident row-major trace (the device handle's, or the
 *                       host trace once uploaded), in order, after the upload and before the commit: each is
 *                       ts_logup_multiplicities with the lane's key_values.
 *   exposed_out         cap_exposed words, or NULL / 0: the exposed words of a finished proof.
 * Outputs: status, n_words, proof_blake3, final_state, start_ms, wall_ms as in ts_batch_item; n_exposed (the
 * AIR's); n_missing / first_missing: those of the first fill that misses (0 / ~0 when none does).
 * Whole-call refusals (TS_ERR_INVALID before any trace is consumed or any item written): those of ts_prove_batch,
 * any struct_size other than sizeof(ts_batch_lookup_item) in an item or sizeof(ts_batch_lane) in a lane, and
 * lanes == NULL while some lane's AIR has preprocessed columns.
 * Item refusals (TS_ERR_INVALID in the item's status, its trace NOT consumed, the other items still run): those
 * of ts_prove_batch; both aux sources, or none for an AIR with aux columns, or one for an AIR without; a spec
 * that does not fit the AIR; a kind-2 term (in `logup` or a fill) on a lane without key_values; n_mult > 8 or
 * a null `mult`; a column-major device trace where a row-major one is needed; a non-null exposed_out shorter
 * than the AIR's exposed words; a key that is null for an AIR with preprocessed columns (or given for one
 * without), or a key or key_values of another width, height or context than the item's trace needs.  A proof
 * buffer too small is TS_ERR_BUFFER with n_words set, as in ts_prove_batch.
 * Data errors do not stop a lane: a lookup in no table row (a fill's miss) or a zero denominator reported by the
 * builder is a statement about the item's data, raised after the kernels finished normally.  The item gets
 * TS_ERR_INVARIANT with the text ts_logup_multiplicities / ts_logup_aux_build_pre give, its trace is consumed,
 * and the lane goes on to its next item; so it does after a non-zero callback status.  TS_ERR_HIP, TS_ERR_OOM and
 * any other TS_ERR_INVARIANT stop the lane, as in ts_prove_batch.
 * ts_prove_batch and ts_prove_stream keep refusing these AIRs with TS_ERR_UNSUPPORTED. */
typedef struct {
    uint32_t struct_size;          /* = sizeof(ts_batch_lane) */
    const ts_pcs_data* key;        /* the lane AIR's committed key, made on the lane's context; NULL iff
                                      preprocessed_width == 0; never consumed, serves every item of the lane */
    const ts_matrix* key_values;   /* row-major n x preprocessed_width values on the lane's context, read by
                                      kind-2 terms of `logup` / `mult`; may be NULL; never consumed */
} ts_batch_lane;
typedef struct {
    uint32_t struct_size;            /* = sizeof(ts_batch_lookup_item): another layout refuses the whole call */
    uint32_t lane;                   /* < n_lanes */
    ts_matrix* trace;                /* device trace made on the lane's context (consumed) ... */
    const uint32_t* host_trace;      /* ... OR canonical row-major host values, height x width */
    uint64_t height;                 /* of host_trace */
    uint32_t width;                  /* of host_trace */
    uint32_t n_public;
    const uint32_t* public_values;
    const ts_challenger* challenger; /* NULL = fresh; else cloned, never modified */
    uint32_t* proof_out;
    size_t cap_words;
    const ts_logup_spec* logup;      /* aux source, declarative ... */
    ts_aux_fn aux_fn;                /* ... OR a callback, run on the lane's thread */
    void* aux_user;
    const ts_logup_mult_spec* mult;  /* n_mult fills, in order */
    uint32_t n_mult;                 /* 0 .. 8 */
    uint32_t cap_exposed;
    uint32_t* exposed_out;           /* may be NULL */
    /* outputs */
    ts_status status;
    uint32_t n_exposed;
    size_t n_words;
    uint64_t n_missing, first_missing;
    uint32_t proof_blake3[8];
    uint32_t final_state[34];
    double start_ms, wall_ms;
} ts_batch_lookup_item;
ts_status ts_prove_batch_lookup(ts_ctx* const* ctxs, const ts_air* const* airs, const ts_batch_lane* lanes,
                                uint32_t n_lanes, const ts_fri_config* cfg, ts_batch_lookup_item* items,
                                uint32_t n_items, double gate_ms, uint32_t flags);

/* ---- several AIR tables of mixed heights in ONE proof ---------------------------------------------------
 * A statement made of T chips of different heights (a CPU table, a memory table, a byte table ...) proved with one
 * FRI commit phase, one proof-of-work grind and one set of queries instead of T of each.  Plain AIRs only: tape
 * version 1, or a later version with preprocessed width 0 and aux width 0.  Build-defined (the reference proves
 * one table).  Transcript:
 *   1. observe the word T = n_tables, then log_degree_t for t = 0 .. T-1, as base words (ts_chal_observe): the
 *      heights are bound before anything is committed;
 *   2. ONE commit of all T traces on their natural domains, in table order (heights in any order, repeats
 *      allowed); observe the root; sample alpha;
 *   3. the quotient chunks of every table over that table's LDE in the batch, with its own public values and its
 *      constraints folded from alpha^0: chunk c of table t is what ts_quotient_chunks gives for that trace
 *      committed alone;
 *   4. ONE commit of all chunks of all tables, table-major and chunk-minor, chunk c of table t on the coset of
 *      its own split domain (as ts_prove shifts the chunks of one table); observe the root; sample zeta;
 *   5. two rounds opened as ts_pcs_open opens them (the batch challenge is sampled first): trace matrix t at
 *      {zeta, zeta * omega_{n_t}}, every chunk at {zeta};
 *   6. the FriProof, exactly as ts_pcs_open writes it for those two rounds.
 * Proof = TSPF v6: [magic, 6, T], T x [log_degree, width, qd], trace root, quotient root, the opened values in
 * ts_pcs_open's (round, matrix, point, column) order, the FriProof words.  v6 has no postcard form
 * (TS_ERR_UNSUPPORTED), and every other verify call answers a v6 proof with verdict 9.
 * Refusals, all before any trace is consumed and each with a text in ts_last_error:
 *   TS_ERR_INVALID      a null argument; n_tables 0 or above 64; a struct_size other than sizeof(ts_multi_table);
 *                       a trace or AIR of another context; a consumed trace; a width or n_public that is not the
 *                       AIR's; one trace handle in two tables; more than 64 quotient chunks over all tables
 *   TS_ERR_UNSUPPORTED  a table whose AIR has preprocessed or aux columns
 *   TS_ERR_INVARIANT    log_quotient_degree > log_blowup for some table
 * TS_ERR_BUFFER sets *n_words_out to the size needed, as ts_prove does (the traces are consumed then).  A trace
 * that violates its constraints gets the status ts_prove gives that table alone.
 * TS_MULTI_OPEN_GENERIC=1 in the environment (read on every call; a test and measurement knob) routes step 5
 * through the generic opening of ts_pcs_open instead of the one-pass-per-height kernels; the proof is the same. */
typedef struct {
    uint32_t struct_size;          /* = sizeof(ts_multi_table), else the whole call is TS_ERR_INVALID */
    uint32_t n_public;
    const ts_air* air;             /* compiled on ctx; preprocessed_width == 0 and aux_width == 0 */
    ts_matrix* trace;              /* made on ctx; consumed */
    const uint32_t* public_values;
} ts_multi_table;
ts_status ts_prove_multi(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal,
                         ts_multi_table* tables, uint32_t n_tables,
                         uint32_t* proof_out, size_t cap_words, size_t* n_words_out);
/* host only (AIRs compiled with a NULL context serve).  Parses TSPF v6, replays the transcript above, runs per
 * table the out-of-domain check of ts_verify on that table's domain (selectors at zeta, the quotient recomposed
 * from its chunks), then ts_pcs_verify over the two rounds.  Verdict codes as ts_verify: a header that disagrees
 * with the AIRs in T, a width or a qd is 1, a truncated or over-long buffer 9.  public_values[t] may be NULL
 * where n_public[t] == 0.  Reads nothing outside proof[0 .. n_words). */
ts_status ts_verify_multi(const ts_fri_config* cfg, ts_challenger* chal,
                          const ts_air* const* airs, uint32_t n_tables,
                          const uint32_t* const* public_values, const uint32_t* n_public,
                          const uint32_t* proof, size_t n_words, int* verdict);   /* host only */

/* ---- the tables of a multi-table proof connected: a LogUp bus across heights ----------------------------------
 * ts_prove_multi with a challenge phase ACROSS the tables: every table may carry LogUp aux columns (ts_logup_spec
 * over its own trace, terms of kind 0 and 1), all of them built from ONE gamma and ONE beta, so that the sends of
 * one table and the receives of another -- of any heights -- cancel in the sum of the exposed words.  Plain tables
 * may sit beside them.  ts_prove_multi itself keeps refusing aux AIRs.  Build-defined.  Transcript:
 *   1. observe T and every log_degree, as TSPF v6 does;
 *   2. ONE commit of all traces; observe the root;
 *   3. sample gamma, then beta, ONCE: one bus has one tuple encoding gamma + sum_j beta^j v_j.  Several buses in
 *      one statement are told apart by a constant first value of the tuple (("const", TAG), ...): tuples of
 *      different tags never meet in a denominator, so each bus balances on its own inside the one sum;
 *   4. the aux matrix of every table that has aux columns (ts_logup_aux_build_multi below: what
 *      ts_logup_aux_build gives for that trace and those challenges); ONE commit of them in table order, on their
 *      natural domains; observe the aux root, then the exposed words, four per aux table, in table order;
 *   5. sample alpha;
 *   6. per table the chunks over (aux LDE, trace LDE) with the public vector pis ++ gamma ++ beta ++ its four
 *      exposed words: chunk c of table t is what ts_quotient_chunks_aux gives for that trace and aux matrix
 *      committed alone; a table without aux columns as in v6;
 *   7. ONE commit of all chunks; observe the root; sample zeta;
 *   8. sample the batch challenge;
 *   9. three rounds in the order of TSPF v4: the aux matrices at {zeta, zeta * omega_{n_t}}, the traces at the
 *      same points, every chunk at {zeta}.
 * Proof = TSPF v7: [magic, 7, T], T x [log_degree, width, qd, aux_width, n_exposed], trace root, aux root, the
 * exposed words in table order, quotient root, the opened values in ts_pcs_open's (round, matrix, point, column)
 * order, the FriProof with three BatchOpenings per query.  v7 has no postcard form, and every other verify call
 * answers a v7 proof with verdict 9.  With T = 1 the words behind the header are those of ts_prove_aux with
 * ts_logup_aux_build as its source, for a challenger that has observed (1, log_degree).
 * Refusals, all before any trace is consumed and each with a text in ts_last_error:
 *   TS_ERR_INVALID      whatever ts_prove_multi refuses with TS_ERR_INVALID; no table with aux columns (the text
 *                       points at ts_prove_multi); a spec that is missing for an aux AIR, given for a plain one, of
 *                       another aux width than the AIR's, with a term of kind 2, a column outside the trace or a
 *                       non-canonical constant; an aux AIR without exactly 2 challenges and 4 exposed words; a
 *                       column-major trace under an aux table
 *   TS_ERR_UNSUPPORTED  a table whose AIR has preprocessed columns
 *   TS_ERR_INVARIANT    log_quotient_degree > log_blowup for some table
 * After the traces are consumed: TS_ERR_INVARIANT "logup: zero denominator at table t, row r, interaction i" (the
 * least such triple), TS_ERR_BUFFER with the size needed.
 * Memory: the row-major traces stay alive through their commit (the LDE stage only reads them) and are released
 * once the aux matrices exist.
 * TS_MULTI_OPEN_GENERIC=1 routes step 9 through the generic opening, TS_MULTI_LOGUP_PER_TABLE=1 step 4 through one
 * ts_logup_aux_build per table (both read on every call; test and measurement knobs); the proof is the same. */
typedef struct {
    uint32_t struct_size;          /* = sizeof(ts_multi_bus_table), else the whole call is TS_ERR_INVALID */
    uint32_t n_public;
    const ts_air* air;             /* preprocessed_width == 0; aux_width == 0, or n_challenges == 2 && n_exposed == 4 */
    ts_matrix* trace;              /* consumed; row-major where aux_width > 0 */
    const uint32_t* public_values;
    const ts_logup_spec* logup;    /* NULL iff aux_width == 0; kinds 0 and 1 only; its aux width = the AIR's */
} ts_multi_bus_table;
ts_status ts_prove_multi_bus(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal,
                             ts_multi_bus_table* tables, uint32_t n_tables,
                             uint32_t* proof_out, size_t cap_words, size_t* n_words_out);
/* host only.  ts_verify_multi extended with the two samples, the aux root and the exposed words, the per-table
 * out-of-domain check with the aux values, and ts_pcs_verify over the three rounds.  On verdict 0 exposed_out
 * (cap_exposed >= 4 per table with aux columns) holds the exposed words in table order and bus_sum their EF4 sum
 * over the tables.  "The bus balances" -- bus_sum == 0 -- is the caller's statement to check, as ts_verify_aux
 * leaves the exposed sum to its caller. */
ts_status ts_verify_multi_bus(const ts_fri_config* cfg, ts_challenger* chal,
                              const ts_air* const* airs, uint32_t n_tables,
                              const uint32_t* const* public_values, const uint32_t* n_public,
                              const uint32_t* proof, size_t n_words,
                              uint32_t* exposed_out, uint32_t cap_exposed, uint32_t bus_sum[4], int* verdict);
/* The LogUp columns of n traces for ONE set of challenges: the work of n ts_logup_aux_build calls in three launches
 * over the workgroups of all tables, one upload (the specs travel in a job table in device memory instead of the
 * launch argument) and one copy back.  aux_out[k] and exposed_out[4k .. 4k+3] are word for word what
 * ts_logup_aux_build(specs[k], traces[k], challenges) gives (extension addition is exact).  1 <= n <= 64; refusals
 * as the single call's, for any k, with nothing allocated and every aux_out[k] NULL.  A zero denominator is
 * TS_ERR_INVARIANT "logup: zero denominator at table k, row r, interaction i" for the least such triple, and no
 * output.  TS_LOGUP_BLOCK_ROWS applies as in the single call. */
ts_status ts_logup_aux_build_multi(ts_ctx* ctx, uint32_t n, const ts_logup_spec* const* specs,
                                   const ts_matrix* const* traces, const uint32_t challenges[8],
                                   ts_matrix** aux_out /* n */, uint32_t* exposed_out /* 4 n */);

/* The multiplicity column of a table whose lookups live in OTHER traces: the table side of a LogUp bus, filled in
 * HBM.  ts_logup_multiplicities counts lookups on the rows of the trace that holds the table; here the table's
 * tuple (`table`, n_values terms of kind 0 or 1) is read on the rows of `table_trace`, and every looker k brings
 * its own row-major trace lookers[k] (any height; read, not consumed; it may be table_trace itself) with 1 to 16
 * lookups (n_values terms each) and their weights, terms of kind 0 or 1 over THAT looker's row.  Semantics as
 * ts_logup_multiplicities: rows with equal tuples form a class and the class's lowest row receives the field sum
 * of the weights (p minus it with negate) while the others receive 0; a weight of 0 is skipped; the same words on
 * every run; TS_LOGUP_HASH_BITS honoured.  A lookup of non-zero weight whose tuple is in no table row is a miss:
 * *n_missing counts them and first_missing[3] = (looker, row, lookup) of the least one in that lexicographic order
 * (~0 each when there is none); with n_missing NULL a miss is TS_ERR_INVARIANT.  Launches: one insert over the
 * table, one count per looker, one write; one copy back.  With one looker that is table_trace the column is
 * exactly ts_logup_multiplicities'.
 * TS_ERR_INVALID before any device work: what the single-trace call refuses, per matrix (not row-major, consumed,
 * another context -- a looker's too --, height outside [1, 2^27], a column outside its trace, a non-canonical
 * constant, a term kind above 1, negate above 1, counts outside their limits, struct_size); out_column outside
 * table_trace or among the table_trace columns that any term reads, the table's or those of a looker that is
 * table_trace. */
typedef struct {
    uint32_t n_lookups;                 /* 1 .. 16 */
    uint32_t pad;
    const ts_logup_term* lookups;       /* n_lookups * n_values, lookup-major, over this looker's row */
    const ts_logup_term* weights;       /* n_lookups */
} ts_logup_bus_looker;
typedef struct {
    uint32_t struct_size;               /* = sizeof(ts_logup_mult_bus_spec) */
    uint32_t n_values;                  /* 1 .. 8 */
    const ts_logup_term* table;         /* n_values terms over table_trace's row */
    uint32_t n_lookers;                 /* 1 .. 16 */
    uint32_t out_column;                /* the column of table_trace that is overwritten */
    const ts_logup_bus_looker* lookers;
    uint32_t negate;                    /* 0 | 1 */
    uint32_t pad;
} ts_logup_mult_bus_spec;
ts_status ts_logup_multiplicities_bus(ts_ctx* ctx, const ts_logup_mult_bus_spec* spec, ts_matrix* table_trace,
                                      const ts_matrix* const* lookers /* n_lookers */, uint64_t* n_missing,
                                      uint64_t first_missing[3]);

/* ---- a multi-table proof against a commit-once key: fixed tables on the bus -------------------------------------
 * The tables a bus needs beyond a range -- byte operations (a, b, a xor b), a program ROM, a decode table -- are not
 * pinned by a transition constraint: they are preprocessed columns whose commitment the verifier holds.  A
 * ts_multi_key is ONE committed batch of 1 .. 64 preprocessed matrices of mixed power-of-two heights on their natural
 * domains (shift 1): its root is what ts_pcs_commit gives for the same list.  It is made once on a context, consumed
 * by no proof, and serves any number of them; the matrices' LDE and leaf hashing leave every proof.
 * keep_values = 1 (row-major matrices only) keeps the inputs alive inside the key, with no second copy (the LDE stage
 * only reads them): ts_multi_key_values lends matrix idx as a handle for ts_logup_aux_build_multi_pre,
 * ts_logup_multiplicities_bus_pre and for kind-2 terms inside ts_prove_multi_key; the handle lives as long as the key
 * and must not be freed or consumed.  Without kept values ts_multi_key_values is TS_ERR_INVALID.  `mats` are consumed.
 * ts_multi_key_info gives the natural height and the width of matrix idx. */
typedef struct ts_multi_key ts_multi_key;
ts_status ts_multi_key_commit(ts_ctx* ctx, const ts_fri_config* cfg, uint32_t n_mats, ts_matrix* const* mats /*consumed*/,
                              int keep_values, uint32_t root_out[8], ts_multi_key** out);
ts_status ts_multi_key_info(const ts_multi_key* key, uint32_t idx, uint64_t* height, uint32_t* width);
ts_status ts_multi_key_values(const ts_multi_key* key, uint32_t idx, const ts_matrix** out /* borrowed */);
ts_status ts_multi_key_free(ts_ctx* ctx, ts_multi_key* key);

/* ts_prove_multi_bus against a key.  The i-th table with preprocessed_width > 0, in table order, reads key matrix i,
 * which must have the table's height and the AIR's preprocessed width; the key holds exactly as many matrices as
 * there are such tables and was committed with cfg's log_blowup.  A table is plain, key-only, aux-only (the bus AIRs
 * of v7) or key and aux (a fixed table on the bus).  A table's ts_logup_spec may use terms of kind 2: column `value`
 * of that table's key matrix on the local row; the key must then have been made with keep_values = 1.
 * Build-defined.  Transcript (v7's, with the key):
 *   1. observe T and every log_degree;
 *   2. observe the key root, as ts_prove_pre does first;
 *   3. ONE commit of all traces; observe the root;
 *   4. if at least one table has aux columns (A > 0): sample gamma, then beta; the aux matrices
 *      (ts_logup_aux_build_multi_pre below: what ts_logup_aux_build_pre gives per table); ONE commit of them in table
 *      order; observe the aux root, then the exposed words in table order.  With A = 0 this step is skipped whole:
 *      no samples, no aux commitment, no aux root and no exposed words in the proof;
 *   5. sample alpha;
 *   6. per table the chunks over the side list (key LDE, aux LDE), each where present, in the order of
 *      ts_quotient_chunks_pre_aux; the public vector is v7's;
 *   7. ONE commit of all chunks; observe the root; sample zeta, then the batch challenge;
 *   8. the rounds in the order of TSPF v5: the key matrices at {zeta, zeta * omega_{n_t}}, the aux matrices at the
 *      same points if A > 0, the traces at the same points, every chunk at {zeta}.
 * Proof = TSPF v8: [magic, 8, T], T x [log_degree, width, qd, aux_width, n_exposed, preprocessed_width], trace root,
 * aux root and exposed words only if A > 0, quotient root, the opened values in ts_pcs_open's (round, matrix, point,
 * column) order, the FriProof with one BatchOpening per round per query.  The key root is NOT in the proof, as in v3
 * and v5.  v8 has no postcard form; every other verify call answers a v8 proof with verdict 9 and
 * ts_verify_multi_key answers any other version with 9.  With T = 1 the words behind the header are those of
 * ts_prove_pre_aux for a challenger that has observed (1, log_degree).
 * Refusals, all before any trace is consumed and each with a text in ts_last_error:
 *   what ts_prove_multi_bus refuses, with the same status, except preprocessed columns and a statement without aux
 *   tables; TS_ERR_INVALID for a NULL key or a key that no table uses (the text points at ts_prove_multi_bus), a key
 *   of another context, of another log_blowup, of another matrix count, or with a matrix of another height or width
 *   than its table's; a kind-2 term on a table without preprocessed columns or outside its key matrix, or against a
 *   key without kept values.
 * TS_MULTI_OPEN_GENERIC and TS_MULTI_LOGUP_PER_TABLE apply as in v7 (the per-table builder is
 * ts_logup_aux_build_pre); the proof is the same.  A height class of the opening may hold 64 key + 64 aux + 64 trace
 * + 64 chunk matrices: the per-class kernels read their jobs from device memory and have no bound of their own. */
typedef ts_multi_bus_table ts_multi_key_table;   /* air: any preprocessed_width; logup: kinds 0, 1 and 2 */
ts_status ts_prove_multi_key(ts_ctx* ctx, const ts_fri_config* cfg, ts_challenger* chal, const ts_multi_key* key,
                             ts_multi_key_table* tables, uint32_t n_tables,
                             uint32_t* proof_out, size_t cap_words, size_t* n_words_out);
/* host only.  ts_verify_multi_bus extended by the key root observation, the preprocessed opened values in each
 * table's out-of-domain check, and ts_pcs_verify over three or four rounds with key_root as the first commitment.
 * Verdict codes as ts_verify.  Reads nothing outside proof[0 .. n_words).  With A = 0 exposed_out may be NULL and
 * bus_sum is zero. */
ts_status ts_verify_multi_key(const ts_fri_config* cfg, ts_challenger* chal, const uint32_t key_root[8],
                              const ts_air* const* airs, uint32_t n_tables,
                              const uint32_t* const* public_values, const uint32_t* n_public,
                              const uint32_t* proof, size_t n_words,
                              uint32_t* exposed_out, uint32_t cap_exposed, uint32_t bus_sum[4], int* verdict);
/* ts_logup_aux_build_multi whose specs may use terms of kind 2: table k's read preprocessed[k], the row-major values
 * of its preprocessed columns (the trace's height, this context, not consumed; NULL for a table without such terms).
 * Every aux word and every S equals ts_logup_aux_build_pre(specs[k], preprocessed[k], traces[k]) word for word; a job
 * without a table runs the code it runs in ts_logup_aux_build_multi.  Refusals and the zero-denominator report as
 * there. */
ts_status ts_logup_aux_build_multi_pre(ts_ctx* ctx, uint32_t n, const ts_logup_spec* const* specs,
                                       const ts_matrix* const* preprocessed /* n, entries may be NULL */,
                                       const ts_matrix* const* traces, const uint32_t challenges[8],
                                       ts_matrix** aux_out /* n */, uint32_t* exposed_out /* 4 n */);
/* ts_logup_multiplicities_bus whose `table` terms may be of kind 2: a column of table_preprocessed (row-major,
 * table_trace's height, same context, not consumed; NULL without such terms).  The lookers keep kinds 0 and 1 and
 * out_column stays a main column of table_trace.  Classes, the lowest row as representative, misses, negate and
 * TS_LOGUP_HASH_BITS as there; with no kind-2 term and a NULL matrix the column is exactly
 * ts_logup_multiplicities_bus's. */
ts_status ts_logup_multiplicities_bus_pre(ts_ctx* ctx, const ts_logup_mult_bus_spec* spec,
                                          const ts_matrix* table_preprocessed, ts_matrix* table_trace,
                                          const ts_matrix* const* lookers /* n_lookers */, uint64_t* n_missing,
                                          uint64_t first_missing[3]);

/* ---- before you prove: the exact balance of a bus, and the debug counterpart of the bus proofs -----------------------
 * ts_verify_multi_bus and ts_verify_multi_key answer an unbalanced bus with bus_sum != 0 after a whole proof, and
 * bus_sum does not say which tuple is out of balance.  ts_bus_check says it from the resident traces, without a
 * challenge and exactly: a hash join in HBM over every table of the bus.
 *   A CONTRIBUTION is a triple (table k, row r, interaction i of specs[k]) whose multiplicity term, reduced mod p, is
 *   non-zero (a word of 0 or of p is none; p + 1 counts as 1).  Terms of kinds 0, 1 and 2 are read exactly as
 *   ts_logup_aux_build_multi_pre reads them.
 *   The TUPLE of a contribution is its value terms ZERO-PADDED to 8 words; words are compared as stored, as the
 *   multiplicity calls do.  The padding is what the argument means: gamma + sum_j beta^j v_j cannot tell (a, b) from
 *   (a, b, 0), so they are the same tuple on the bus.
 *   The bus is BALANCED iff every tuple's multiplicities sum to 0 mod p.
 *   first_table, first_row, first_interaction: the least contribution, in (table, row, interaction) order, over all
 *   contributions to unbalanced tuples; n_values, tuple and sum describe that contribution's tuple.
 *   shares[k] (if given) describes table k's part of that tuple: the number of its contributions, their multiplicity
 *   sum mod p, and the least (row, interaction) among them, ~0 each when table k has none.  When the bus is balanced
 *   shares is all zero with ~0 rows and interactions.
 * Every output is a count, a minimum or an integer sum: the same on every run.  No trace is written or consumed.
 * specs[k] == NULL: table k is not on the bus and traces[k] is not looked at.  preprocessed may be NULL (no kind-2
 * term anywhere), as may any entry.  TS_LOGUP_HASH_BITS is honoured as in ts_logup_multiplicities.
 * TS_ERR_INVALID, with a text, before any device work: what ts_logup_aux_build_multi_pre refuses for any k (a trace
 * that is not row-major, consumed or of another context, a height outside [1, 2^27], counts outside their limits, a
 * kind-2 term without its matrix, a column outside its matrix, a non-canonical constant); n outside 1 .. 64; every spec
 * NULL; the sum over k of height_k * K_k above 2^30 (which also keeps the 64-bit sums below 2^61); a struct_size that
 * is not sizeof the report.  A full slot table is TS_ERR_INVARIANT "internal error", as in the multiplicity calls.
 * Launches: one insert over the rows of all tables (the specs travel in a job table in device memory), one over the
 * slots, one copy back; only if unbalanced one more launch over the rows for the shares, and a second copy back. */
typedef struct { uint64_t count; uint32_t sum, first_row, first_interaction, pad; } ts_bus_share;
typedef struct {
    uint32_t struct_size, pad;      /* in: sizeof(ts_bus_report), else TS_ERR_INVALID */
    uint64_t n_contributions;       /* (table, row, interaction) with multiplicity != 0 mod p */
    uint64_t n_tuples;              /* distinct tuples among them */
    uint64_t n_unbalanced;          /* tuples whose multiplicities do not sum to 0 mod p */
    uint32_t first_table, first_row, first_interaction;  /* ~0 each when balanced */
    uint32_t n_values;              /* of that contribution's interaction */
    uint32_t tuple[8];              /* its values, zero-padded */
    uint32_t sum, pad2;             /* its multiplicity sum, canonical, != 0 */
} ts_bus_report;
ts_status ts_bus_check(ts_ctx* ctx, uint32_t n, const ts_logup_spec* const* specs /* entries may be NULL */,
                       const ts_matrix* const* preprocessed /* may be NULL; entries may be NULL */,
                       const ts_matrix* const* traces, ts_bus_report* report, ts_bus_share* shares /* n, may be NULL */);
/* The debug counterpart of ts_prove_multi_bus and ts_prove_multi_key, as ts_check_constraints is of ts_prove: the
 * statement's tables with their traces NOT consumed, and any gamma and beta (challenges: eight canonical words, the
 * caller's choice).  `key`: NULL iff no table has preprocessed columns, else made with keep_values = 1; the i-th table
 * with preprocessed columns reads key matrix i.  A host composition, no kernel of its own:
 *   1. the argument checks of ts_prove_multi_key that need no FRI configuration: struct_size, handles, contexts, one
 *      trace handle twice, specs against AIRs and traces, the key's count, heights and widths; every trace row-major;
 *   2. ts_logup_aux_build_multi_pre over the tables with aux columns: a zero denominator at these challenges is
 *      TS_ERR_INVARIANT as there;
 *   3. per table, in order, ts_check_constraints_pre_aux with that table's key matrix, aux matrix and exposed words:
 *      *bad_table is the first table with a violation and *first_violation that call's answer, both -1 when all hold
 *      (the later tables are then not checked);
 *   4. ts_bus_check over the same specs into report and shares (n_tables of them, may be NULL); without any table
 *      that has aux columns the report is the balanced one with zero counts;
 *   5. the aux matrices are freed. */
ts_status ts_check_multi(ts_ctx* ctx, const ts_multi_key* key, const ts_multi_key_table* tables, uint32_t n_tables,
                         const uint32_t challenges[8], int32_t* bad_table, int64_t* first_violation,
                         ts_bus_report* report, ts_bus_share* shares);

/* ---- rows in sorted order: a memory table, or any table whose constraints compare neighbours of a sorted order ----
 * ts_logup_multiplicities closed the host round trip for multiplicity columns; these two close it for ROW ORDER.  They
 * replace: ts_matrix_download, a stable host sort (np.lexsort), indexing, ts_matrix_upload.
 * ts_matrix_sort_rows: `src` is row-major, on ctx, neither consumed nor written.  *out is a new row-major matrix of
 * src's height and of src's width plus one column per set flag bit, the source-row column first, then group-start.
 *   Order: the rows [0, n_live) are ordered lexicographically by the words of key_columns AS STORED, compared as
 *   unsigned 32-bit words (a non-canonical word is not reduced: as the multiplicity calls compare words).  The sort is
 *   STABLE -- rows with equal keys keep their source order --, so the result is unique and the same on every run.  Rows
 *   [n_live, height) keep place and content.  n_live == 0 is a plain copy.
 *   Source-row column: the row of src that the output row came from (its own index at or beyond n_live).
 *   Group-start column: 1 on live row i if i == 0 or if one of its first group_keys key words differs from those of
 *   live row i - 1; 0 on every other row, every row at or beyond n_live included.  With group_keys == 0 it is 1 on
 *   live row 0 only.
 * TS_ERR_INVALID, each with a text in ts_last_error, before any device work: a NULL argument; struct_size; n_keys
 * outside 1 .. 4; a key column outside src; a key column named twice; group_keys > n_keys; a flag bit above 1;
 * n_live > height; a matrix that is not row-major, is consumed or belongs to another context; a height outside
 * [1, 2^27] (any value inside is taken, not only powers of two); an output wider than 2^16 columns, the widest matrix
 * these calls make; TS_SORT_BLOCK_ROWS outside [1, 2048].
 * Launches: one histogram over the live rows for all 4 * n_keys byte digits and ONE copy back of its table -- the
 * call's only host wait (none with n_live < 2) --; then per byte digit that moves anything (a digit on which every
 * live row agrees is skipped: canonical words never fill more than two bins of the top byte, 16-bit addresses skip
 * two passes of four) one count, one, three or five scan launches and one scatter of a uint32 row permutation with
 * the key word carried beside it, plus one key load per key column that has such a pass; one gather.  Temporaries
 * come from ctx's pool.
 * TS_SORT_BLOCK_ROWS (1 .. 2048, read on every call; a test knob): the positions one workgroup owns; the matrix is the
 * same for every value. */
typedef struct {
    uint32_t struct_size;      /* = sizeof(ts_sort_spec), else TS_ERR_INVALID */
    uint32_t n_keys;           /* 1 .. 4 */
    uint32_t key_columns[4];   /* most significant first; columns of src; no column twice */
    uint32_t group_keys;       /* 0 .. n_keys: the leading keys that define a group (see flags) */
    uint32_t flags;            /* bit 0: append a source-row column; bit 1: append a group-start column */
    uint64_t n_live;           /* rows [0, n_live) are sorted; rows [n_live, height) keep place and content */
} ts_sort_spec;
enum { TS_SORT_SOURCE_ROW = 1, TS_SORT_GROUP_START = 2 };
ts_status ts_matrix_sort_rows(ts_ctx* ctx, const ts_sort_spec* spec, const ts_matrix* src, ts_matrix** out);
/* out[i] = src[index[i][index_column]]: the sort's own last kernel over a caller's index, so that the source-row
 * column of a narrow key matrix reorders a wide payload matrix.  *out has index's height and src's width; both inputs
 * are row-major, on ctx, read and not consumed.  TS_ERR_INVALID before any device work: a NULL argument, a matrix as
 * ts_matrix_sort_rows refuses it, index_column outside index, src wider than 2^16 columns.  An index word >= src's
 * height is TS_ERR_INVALID "gather: row index r at row i outside the source" for the least such i (recorded by the
 * kernel with a 64-bit integer minimum), and there is no output.  One launch, one copy back. */
ts_status ts_matrix_gather_rows(ts_ctx* ctx, const ts_matrix* src, const ts_matrix* index, uint32_t index_column,
                                ts_matrix** out);

/* ---- derived columns: a row program evaluated in HBM ----
 * The sort closed the host round trip for row order; this closes it for every witness column that is a function of its
 * own row and its two neighbours: limb decompositions, is-zero inverses, comparison bits, a xor b, negated selectors,
 * the index column of a range table, the `gap` of a memory table.  It replaces: ts_matrix_download, a host loop,
 * ts_matrix_upload.
 * The program is a word tape, written as the AIR tape is:
 *   [0]=0x52454454 ("TDER") [1]=1 [2]=src_width [3]=n_nodes [4]=n_outputs,
 *   n_nodes x {op,a,b}       operands that are nodes name EARLIER nodes only
 *   n_outputs x {node, dst_column}
 * Every node's value is a canonical BabyBear element in [0, p), p = 0x78000001.  Ops:
 *    0 CONST(a=value < p)
 *    1 COL(a=row offset: 0 this row, 1 next row, 2 previous row; b=column < src_width): the word AS STORED, reduced
 *      mod p -- 0xFFFFFFFF gives 268435453 and p gives 0.  Rows are cyclic, as an AIR's next row is: next of row h-1 is
 *      row 0, previous of row 0 is row h-1
 *    3 IS_FIRST_ROW (1 on row 0)  4 IS_LAST_ROW (1 on row h-1)  5 IS_TRANSITION (1 - IS_LAST_ROW)
 *    6 ADD(a,b)  7 SUB(a,b)  8 NEG(a)  9 MUL(a,b): field operations
 *   32 ROW: the row index (< 2^27 < p)
 *   33 INV(a): the field inverse, INV(0) = 0 (the is-zero witness convention)
 *   34 IS_ZERO(a): 1 if a == 0, else 0
 *   35 LT(a,b): 1 if a < b as integers in [0, p), else 0
 *   36 BITS(a, b = shift | nbits << 8): (a >> shift) & (2^nbits - 1) on the canonical integer; nbits >= 1, shift +
 *      nbits <= 31
 *   37 AND(a,b)  38 XOR(a,b): bitwise on the canonical integers, the result reduced mod p (a result in [p, 2^31) becomes
 *      result - p)
 * Op 2 and every other number are TS_ERR_INVALID.
 * Output: *out is a NEW row-major matrix of src's height and of width W_out = max(src_width, 1 + max dst_column).  A
 * column named by an output holds that node's value, canonical.  Every other column must be < src_width and is copied
 * from src as stored (not reduced); every column >= src_width must be named, and no column may be named twice (one node
 * may go to several columns).  All reads see src: an output that overwrites column c does not change what COL of c
 * reads.  src is neither consumed nor written.  Every output word is a pure function of src, so the result is the same
 * on every run.
 * Lowering (ts_derive_check reports it): nodes no output reaches are dropped (they are still checked); one instruction
 * per remaining node, in tape order; a value lives in one slot from its instruction to its last use, and an
 * instruction's destination may take the slot of an operand whose last use it is; an output is stored when its node is
 * computed.  n_live is the most slots held at once.
 * TS_ERR_INVALID, each with a text in ts_last_error, before any device work: a NULL argument; a wrong magic or version,
 * or a word count that does not match the header; [2] != src's width; an unknown op; an operand >= the node's own
 * index; a COL offset > 2 or a column outside src; CONST >= p; BITS with nbits = 0 or shift + nbits > 31; n_nodes = 0 or
 * n_outputs = 0, or either above its limit; an output node >= n_nodes; a broken rule on destination columns; W_out >
 * 2^16; n_live > TS_DERIVE_MAX_LIVE (the text names both numbers); a matrix that is not row-major, is consumed or
 * belongs to another context; a height outside [1, 2^27] (any value inside is taken).  A refused call leaves *out NULL.
 * Launches: the lowered list goes to the device in one asynchronous copy through the context's page-locked staging
 * arena, then ONE kernel, one lane per row: a workgroup copies the untouched columns of its 256 rows with coalesced
 * accesses and interprets the list (scalar instruction fetch, the slot file in LDS).  The call makes no host wait of
 * its own (the arena waits once when it wraps, as for every small upload).  Temporaries come from ctx's pool.
 * The interpreter is the only form: a program is not specialised into a kernel of its own.
 * Out of scope: more than one source matrix; parameters other than constants; extension-field values; use inside batch
 * lanes.  A TDER program is row-local; rows that depend on derived values of other rows are the other program kind of
 * these three entry points, "iterated columns" below (a first-order linear recurrence down the rows is cheaper as
 * ts_matrix_scan further below; or chain two calls). */
enum { TS_DERIVE_MAX_NODES = 4096, TS_DERIVE_MAX_OUTPUTS = 256, TS_DERIVE_MAX_LIVE = 48 };
ts_status ts_matrix_derive(ts_ctx* ctx, const uint32_t* program, size_t n_words, const ts_matrix* src, ts_matrix** out);
/* Host only, no context: every check above that needs no matrix, against a source of src_width columns; the text of a
 * refusal is what ts_last_error returns for a NULL context.  out_width = W_out, n_instructions = the nodes kept,
 * n_live as above; each of the three may be NULL. */
ts_status ts_derive_check(const uint32_t* program, size_t n_words, uint32_t src_width, uint32_t* out_width,
                          uint32_t* n_instructions, uint32_t* n_live);
/* Host only: THE SAME lowered instruction list and slot allocation the device gets, over `height` host rows of
 * src_width words; out_row_major receives height * W_out words (TS_ERR_BUFFER if out_cap_words is less).  A reference
 * for tests and for callers without a device, not a fast path. */
ts_status ts_derive_rows_host(const uint32_t* program, size_t n_words, const uint32_t* src_row_major, uint64_t height,
                              uint32_t src_width, uint32_t* out_row_major, size_t out_cap_words);

/* ---- iterated columns: a row program with carried state, per group, in HBM ----
 * A TDER program is row-local and the scan below runs first-order LINEAR recurrences.  Everything else that is
 * sequential -- the state column of a hash or sponge chip, the rounds of a block cipher laid out one per row, a
 * division or square-root loop, a Fibonacci-style pair, a small state machine -- is a row program whose registers are
 * carried from one row to the next inside a group of rows: one call, one hash invocation, one address.  The recurrence
 * is sequential inside a group and a trace has thousands of groups, so the device walks the groups side by side.  It
 * replaces: ts_matrix_download, a host loop down the rows, ts_matrix_upload.
 * No entry point is added: the iterate form is a SECOND PROGRAM KIND of ts_matrix_derive, ts_derive_check and
 * ts_derive_rows_host, chosen by the tape's magic.  A "TDER" tape behaves as written above, word for word.
 * The program, a "TITR" tape of 32-bit words:
 *   [0]=0x52544954 ("TITR")  [1]=1  [2]=src_width  [3]=n_nodes  [4]=n_outputs
 *   [5]=n_carries (1 .. TS_ITERATE_MAX_CARRIES)  [6]=reset_column (a column of src, or 0xFFFFFFFF: none)
 *   [7]=max_group_rows (>= 1)
 *   n_nodes   x {op, a, b}          as TDER: operands name EARLIER nodes only
 *   n_outputs x {node, dst_column}  as TDER, the same rules on destination columns
 *   n_carries x {node, init}        carry k's value after a row is `node` of that row; init < p, canonical
 * Groups: row 0 starts a group, and so does every row whose reset_column word, reduced mod p, is != 0 -- the rule of the
 * scan's reset column and of the collect's selectors: 0, p and 2p do not fire, 1 and 0xFFFFFFFF do.  Without a reset
 * column the whole matrix is one group.  A group ends before the next start or at row h-1; groups are not cyclic.
 * Ops: every TDER op keeps its meaning, COL with its cyclic neighbour rows of the whole matrix included.  Four more:
 *   40 CARRY(a = k < n_carries): the value of carry k's node on the previous row of this group, init_k on the group's
 *      first row.  A CARRY always reads the value from BEFORE this row: a, b <- b, a + b with two carries needs no
 *      temporary
 *   41 STEP: the row minus the group's first row
 *   42 IS_GROUP_FIRST   43 IS_GROUP_LAST (1 when the next row starts a group, or on row h-1)
 * In a TDER tape 40 .. 43 stay unknown ops.
 * Output: as for a TDER program -- a NEW row-major matrix of src's height, named columns canonical, the others copied
 * as stored, all reads see src, src untouched, the result a pure function of src and the same on every run and for
 * every value of the knob below.
 * Lowering (ts_derive_check reports it): as above, and carry k owns slot k for the whole walk; a CARRY is an instruction
 * that copies its carry into a slot of its own; the nodes of the carries are always kept and hold their slots to the end
 * of the list, where one latch per carry moves the new value into the carry's slot, after every CARRY has been read.
 * n_live counts the carry slots and the temporaries together, against the same TS_DERIVE_MAX_LIVE; n_instructions is
 * the nodes kept.
 * TS_ERR_INVALID, each with a text ("iterate: ...") before any device work, on top of the TDER refusals: n_carries
 * outside 1 .. 16; a carry node >= n_nodes; init >= p; a CARRY index >= n_carries; reset_column outside src;
 * max_group_rows = 0; max_group_rows x (the length of the lowered list, stores and latches included) above
 * TS_ITERATE_MAX_WORK (the text names both factors) -- a condition, not a measurement: it bounds what one lane can be
 * asked to run on a machine it shares; a word count that does not match the header; TS_ITERATE_BLOCK_ROWS outside its
 * range.
 * A group longer than max_group_rows refuses the call after its one host wait, TS_ERR_INVARIANT "iterate: the group
 * that starts at row R has N rows, max_group_rows is M", R the least such start row; *out stays NULL, every pool block
 * goes back and the kernel that walks the groups is never launched.  The host evaluator refuses with the same text
 * before it writes a word.
 * Launches: FOUR kernels (csrc/iterate.hip), no workgroup waits for another.  (1) count: per block of
 * TS_ITERATE_BLOCK_ROWS rows the number of group starts and the last of them, from the reset column alone; (2) offsets,
 * one workgroup: the exclusive scan of the counts and the last start before every block; (3) starts: the row every
 * group starts at, and -- since a start knows the start before it -- the least over-long group, with its length;
 * (4) walk: workgroups of one wave, one lane per group; the workgroup copies the untouched columns of its rows with
 * coalesced accesses, then walks its longest group's rows with the interpreter of a TDER program (scalar instruction
 * fetch, the slot file in LDS), a lane past its group's end idle.  Every out word is written exactly once.
 * Waits: exactly ONE, between (3) and (4), for 16 bytes: the number of groups, which sizes (4), and the over-long
 * group, which refuses the call.  Temporaries come from ctx's pool: 4 bytes per row, 8 per block.
 * TS_ITERATE_BLOCK_ROWS (1 .. 1024, default 1024, read on every call) is a test knob: the rows of a count block.  No
 * output word depends on it; a value so small that a grid would pass 2^24 workgroups is TS_ERR_INVALID.
 * Out of scope: suffix (reverse) walks; extension-field state; more than one source; groups longer than the work
 * limit allows; use inside batch lanes; a program specialised into its own kernel. */
enum { TS_ITERATE_MAX_CARRIES = 16, TS_ITERATE_MAX_WORK = 1 << 20 };

/* ---- scanned columns: linear recurrences down the rows, in HBM ----
 * The derive closed the host round trip for columns that are a function of their own row and its neighbours; this closes
 * it for the columns a sequential machine's trace is made of: the value a read returns (the last value written to its
 * address), a running count, sum or balance inside a group, a byte-to-word Horner accumulator, the running product of a
 * permutation argument, a running random linear combination.  Each is a first-order linear recurrence over BabyBear,
 *   y[i] = a[i] * y[i-1] + b[i],   y[-1] = init,
 * optionally started over where a group starts.  It replaces: ts_matrix_download, a sequential host loop,
 * ts_matrix_upload.
 * A spec holds 1 to TS_SCAN_MAX_COLUMNS scans over the same source; each names its a and b (a constant < p, or a column
 * of src whose word is read AS STORED and reduced mod p -- 0xFFFFFFFF gives 268435453 and p gives 0), init (canonical),
 * a reset column or TS_SCAN_NO_RESET (where that column's word, reduced mod p, is != 0, row i starts over:
 * y[i] = a[i] * init + b[i]), its dst column and flags.  TS_SCAN_EXCLUSIVE: dst[i] is the state BEFORE row i -- y[i-1],
 * init on row 0 and on a reset row -- instead of y[i].
 * Output: *out is a NEW row-major matrix of src's height.  Its width is W = max(src_width, 1 + max dst_column) when
 * out_width is 0; else out_width, with 1 + max dst_column <= out_width <= W: the result keeps columns [0, out_width)
 * only, so helper columns at the tail of src (an `a` and a `b` made by ts_matrix_derive) are dropped.  Every dst word is
 * canonical.  Every other kept column must be < src_width and is copied from src as stored (not reduced); every kept
 * column >= src_width must be a dst, and no column may be dst twice.  All reads see src: a scan that overwrites column c
 * does not change what another scan reads from c.  src is neither consumed nor written.  The result is a pure function
 * of src: field arithmetic is exact and the composition of the maps x -> a x + b associative, so it is the same on every
 * run and for every value of the knob below.  finals, if not NULL, receives n_columns words: y[h-1] of each scan,
 * canonical (for an exclusive scan too: the state AFTER the last row).
 * TS_ERR_INVALID, each with a text in ts_last_error, before any device work: a NULL argument (finals may be NULL); a
 * wrong struct_size; n_columns outside 1..8; a term kind above 1; a constant or init that is not below p; a column
 * outside src; a flag bit above 0; a broken rule on dst columns or out_width; a width above 2^16; a height outside
 * [1, 2^27] (any value inside is taken); a matrix that is not row-major, is consumed or belongs to another context;
 * TS_SCAN_BLOCK_ROWS outside its range.  A refused call leaves *out NULL.
 * Launches: THREE kernels, reduce-then-scan, no workgroup waits for another.  (1) one workgroup per block of rows
 * composes the maps of its rows, every scan at once, into one map per scan; (2) one workgroup scans the block maps and
 * applies them to init: the state each block starts from, and y[h-1]; (3) the first grid again recomputes its in-block
 * scan from that state, writes the dst words and copies the untouched kept columns with coalesced accesses.  The spec
 * travels in the launch arguments; one bit per column goes to the device in one asynchronous copy through the context's
 * page-locked staging arena.  Waits: with finals == NULL the call makes no host wait of its own (the arena waits once
 * when it wraps, as for every small upload); with finals exactly one, for the copy back of n_columns words.
 * Temporaries come from ctx's pool.
 * TS_SCAN_BLOCK_ROWS (1 .. 1024, default 1024, read on every call) sets the rows one workgroup owns: a test knob that
 * makes small matrices cross the wave, the workgroup and several trips of launch 2's loop.  No output depends on it.
 * Out of scope: suffix (reverse) scans; extension-field state; more than one source matrix; second-order recurrences
 * (y[i] from y[i-1] AND y[i-2]); a or b that depend on a scanned value (chain two calls); use inside batch lanes. */
typedef struct { uint32_t kind, value; } ts_scan_term;      /* 0: constant, value < p;  1: column `value` of src */
typedef struct {
    ts_scan_term a, b;       /* y[i] = a[i] * y[i-1] + b[i] in BabyBear; a column word is read AS STORED and reduced mod p */
    uint32_t init;           /* y[-1], canonical, < p */
    uint32_t reset_column;   /* TS_SCAN_NO_RESET or a column of src: where its word, reduced mod p, is != 0, row i
                                starts over: y[i] = a[i] * init + b[i] */
    uint32_t dst_column;
    uint32_t flags;          /* bit 0 TS_SCAN_EXCLUSIVE */
} ts_scan_column;
enum { TS_SCAN_MAX_COLUMNS = 8, TS_SCAN_EXCLUSIVE = 1 };
#define TS_SCAN_NO_RESET 0xFFFFFFFFu
typedef struct {
    uint32_t struct_size, n_columns;            /* sizeof(ts_scan_spec); 1 .. 8 */
    ts_scan_column columns[TS_SCAN_MAX_COLUMNS];
    uint32_t out_width;      /* 0: W; else the result keeps columns [0, out_width) only */
    uint32_t pad;
} ts_scan_spec;
ts_status ts_matrix_scan(ts_ctx* ctx, const ts_scan_spec* spec, const ts_matrix* src, ts_matrix** out,
                         uint32_t* finals /* n_columns words: y[h-1] of each, canonical; may be NULL */);
/* Host only, no context: every check above that needs no matrix (the text of a refusal is what ts_last_error returns
 * for a NULL context), then the plain sequential loop over `height` host rows of src_width words.  out_row_major
 * receives height * out-width words (TS_ERR_BUFFER if out_cap_words is less; nothing is written then, nor by a refused
 * call).  A reference for tests and for callers without a device, not a fast path. */
ts_status ts_scan_rows_host(const ts_scan_spec* spec, const uint32_t* src_row_major, uint64_t height, uint32_t src_width,
                            uint32_t* out_row_major, size_t out_cap_words, uint32_t* finals /* may be NULL */);

/* ---- collected rows: the selected rows of resident traces as one table, in HBM ----
 * Every call above keeps the height of its source and reads one matrix.  A machine's execution trace has one row per
 * step and several access slots per row, some of them conditional; the table the sort and the scan work on has one row
 * per ACCESS.  Getting from the one to the other is a stream compaction: select the slots, reshape each to a common
 * tuple, stack them in execution order, pad to a power of two.  This call does that in HBM.  It replaces:
 * ts_matrix_download, a concatenation of masked slices on the host, ts_matrix_upload.
 * The spec is a word tape, written as the derive program is:
 *   [0]=0x4C4F4354 ("TCOL") [1]=1 [2]=n_sources (1..4) [3]=n_emitters (1..16) [4]=out_width (1..64),
 *   n_sources x src_width[s]          the width of source s, 1 .. 2^16
 *   out_width x pad word              the pad row, each word < p = 0x78000001
 *   n_emitters x {source, sel_kind, sel_value, out_width x {kind, value}}
 * Selector: sel_kind 0 is the constant 1 (sel_value must be 1: any other constant is refused) -- the emitter fires on
 * every row of its source; sel_kind 1 is column sel_value of the emitter's source -- the emitter fires on a row where
 * that word, reduced mod p, is != 0.  This is the rule of the scan's reset column: 0, p and 2p do not fire, 1 and
 * 0xFFFFFFFF do.
 * Terms, one per output column: kind 0 a constant < p; kind 1 column `value` of the emitter's source, copied AS STORED
 * (not reduced, like an untouched column of derive); kind 2 the index of the source row (value must be 0).
 * Order: the output rows are the fired (source, row, emitter) triples in lexicographic order of (source index, row,
 * emitter index in the spec): a source's rows in execution order, a row's slots in spec order, the sources stacked.
 * The result is unique, the same on every run and for every value of the knob below.
 * Height: *n_live is the number of triples that fired.  out_height is 0 or a power of two in [1, 2^27]; 0 means the
 * least power of two >= max(n_live, 1).  *out is a NEW row-major matrix of that height and out_width columns; rows
 * [n_live, height) hold the pad row.  n_live above a given out_height is TS_ERR_INVALID "collect: N rows selected,
 * out_height H"; n_live above 2^27 is TS_ERR_INVALID too.  In both cases there is no output, *n_live is 0 and every
 * pool block the call took is returned.
 * Sources: n_sources handles, row-major, on ctx, neither consumed nor written, each of any height in [1, 2^27].  One
 * handle may appear as several sources.
 * TS_ERR_INVALID, each with a text in ts_last_error, before any device work, leaving *out NULL: a NULL argument; a
 * wrong magic or version, or a word count that does not match the header; a count outside its range; src_width[s] that
 * differs from the matrix's width; a source index, column, kind, constant or pad word out of range; a matrix that is
 * not row-major, is consumed or belongs to another context; an out_height that is not 0 or a power of two in range;
 * TS_COLLECT_BLOCK_ROWS outside its range.
 * Launches: THREE kernels, reduce-then-scan, no workgroup waits for another.  The blocks of all sources form one job
 * grid; a block is a run of at most min(TS_COLLECT_BLOCK_ROWS, 4096 / E_s) consecutive rows of ONE source (E_s: the
 * emitters of that source).  (1) one workgroup per block counts what fires in it, reading the selector columns only;
 * (2) one workgroup makes the exclusive scan of the block counts, the carry in 64 bits: where each block's rows start
 * in the result, and the total; (3) the job grid again lists its fired (row, emitter) pairs in LDS and writes its rows,
 * one contiguous word range per block, with coalesced stores and reads gathered inside the block's own rows; the
 * workgroups behind the job grid in the same launch fill the pad rows.  Selectors, pad row and term table go to the
 * device in one asynchronous copy through the context's page-locked staging arena.  Every output word is written
 * exactly once and nothing reads the output.
 * Waits: exactly ONE, between launches 2 and 3, for the copy back of the total (8 bytes): it sizes the result when
 * out_height is 0 and decides the overflow refusal in every case.  Temporaries come from ctx's pool.
 * TS_COLLECT_BLOCK_ROWS (1 .. 1024, default 1024, read on every call) caps the rows one workgroup owns: a test knob
 * that makes small matrices cross the wave, the workgroup and several trips of launch 2's loop.  No output word depends
 * on it.  A value so small that the job grid would pass 2^24 workgroups is refused.
 * Out of scope: use inside batch lanes; a predicate other than one column (derive it first); any reordering (sort
 * afterwards); more than 4 sources, 16 emitters or 64 output columns; extension-field words; a kernel specialised per
 * spec.  Removal of duplicates is the group form of this call ("grouped rows" below). */
enum { TS_COLLECT_MAX_SOURCES = 4, TS_COLLECT_MAX_EMITTERS = 16, TS_COLLECT_MAX_WIDTH = 64 };
ts_status ts_matrix_collect_rows(ts_ctx* ctx, const uint32_t* spec, size_t n_words,
                                 const ts_matrix* const* sources /* n_sources */, uint64_t out_height,
                                 ts_matrix** out, uint64_t* n_live);
/* Host only, no context: every check above that needs no matrix; the text of a refusal is what ts_last_error returns
 * for a NULL context.  n_sources and out_width are the header's; each may be NULL. */
ts_status ts_collect_check(const uint32_t* spec, size_t n_words, uint32_t* n_sources, uint32_t* out_width);
/* Host only: the same checks, then the plain sequential loop over host rows: source s is heights[s] rows (1 .. 2^27)
 * of src_width[s] words at src_row_major[s].  out_row_major receives *out_height_used * out_width words, pad rows
 * included (TS_ERR_BUFFER if out_cap_words is less; nothing is written then, nor by a refused call).  The height rules
 * and the overflow refusal are those above.  A reference for tests and for callers without a device, not a fast
 * path. */
ts_status ts_collect_rows_host(const uint32_t* spec, size_t n_words, const uint32_t* const* src_row_major,
                               const uint64_t* heights, uint64_t out_height, uint32_t* out_row_major,
                               size_t out_cap_words, uint64_t* out_height_used, uint64_t* n_live);

/* ---- grouped rows: one row per distinct key tuple, in HBM ----
 * The collect stacks rows; nothing above makes ONE ROW PER DISTINCT KEY: the table of touched addresses of a memory
 * trace with each address's final value and the clock of its last access (what a continuation hands to the next
 * segment), the distinct (opcode, a, b) tuples a trace looked up with their multiplicities, per-call totals of a chip
 * table, per-page access counts.  That is a GROUP BY, and it is a second tape form of the three collect calls above,
 * told apart by its magic: no entry point of its own.  It replaces: ts_matrix_download, np.unique / np.lexsort and
 * reduceat on the host, ts_matrix_upload -- or, on sorted input only, sort, derive, scan and collect with four
 * output-sized matrices and two waits.
 *   [0]=0x50524754 ("TGRP") [1]=1 [2]=src_width (1..2^16) [3]=out_width (1..64) [4]=n_keys (1..8)
 *   [5]=sel_kind [6]=sel_value       the expand's rule: 0/1 every row; 1/c column c, the row takes part iff word mod p != 0
 *   n_keys x {kind, value}           key terms: kind 0 a constant < p, kind 1 a column of the row
 *   out_width x pad word             each < p
 *   out_width x {kind, value}        one term per output column
 * 7 + 2 n_keys + 3 out_width words.  Exactly ONE source: sources[0], or src_row_major[0] and heights[0] on the host;
 * the check call reports n_sources = 1.
 * Groups: the rows that take part and carry equal key tuples form a group.  Key words are compared AS STORED, the rule
 * of the join and of the multiplicity fill: p + 1 does not match 1.  A row that takes no part belongs to no group and
 * feeds no aggregate.
 * Order: one output row per group, in ascending order of the group's LEAST source row -- first appearance.  On a
 * source sorted by its key (the sort is stable) that is key order.
 * Terms, for the group with least row f, greatest row l and n rows:
 *   0 CONST      the constant (value < p)          5 COUNT  n (value 0)
 *   1 FIRST      column `value` of row f, as stored  6 SUM    the sum over the group of (word mod p), mod p, canonical
 *   2 LAST       column `value` of row l, as stored  7 MIN    the least (word mod p) of the group
 *   3 FIRST_ROW  f (value 0)                        8 MAX    the greatest (word mod p)
 *   4 LAST_ROW   l (value 0)                        9 INDEX  the group's own output row index (value 0)
 * At most 16 terms of kinds 6 to 8.  Sums are exact: integer sums of canonical words, below 2^58 at 2^27 rows, reduced
 * once.  Every aggregate is order-independent, so the result is the same words on every run and for every value of the
 * two knobs below.
 * Height: *n_live is the number of groups; out_height and the pad rows follow the collect's rule; a call where no row
 * takes part gives n_live = 0 and one pad row.  More groups than a given out_height is refused after the wait with
 * TS_ERR_INVALID "group: N groups, out_height H": *out is NULL, *n_live is 0 and every pool block the call took is back
 * in the pool.
 * TS_ERR_INVALID before any device work, each matrix-free one with a text of its own prefixed "group:" (the check call
 * makes them, the host loop makes them first): a count outside its range; a word count that does not match the header;
 * the selector rules; a key or term kind out of range; a column outside the source; a constant or pad word not below
 * p; a non-zero value word where the table says 0; more than 16 aggregates.  Those that need a matrix are the
 * collect's: wrong width, not row-major, consumed, another context, height outside [1, 2^27], out_height, a knob
 * outside its range.
 * Launches: plain ones, no cooperative launch, no workgroup waits for another, every probe loop bounded by the
 * capacity of the slot table (the power of two at or above 2 x height).  (1) insert: one lane per row evaluates the
 * selector, builds the tuple and runs the join's atomicCAS / atomicMin protocol, after which each class owns one slot
 * that holds its least row; the row keeps its class's slot index, so no later pass probes again; (2) per block of at
 * most TS_COLLECT_BLOCK_ROWS rows the leaders (rows their class's slot holds) are counted; (3) the collect's scan of
 * the block counts; then the one wait; (4) the groups' records are filled with their identities; (5) leaders take
 * index = block offset + rank and write it where the rows of their class find it; (6) every row that takes part adds
 * into its group's record: COUNT and the sums by 64-bit atomicAdd, LAST_ROW by atomicMax, MIN / MAX by 32-bit atomicMin
 * / atomicMax -- a wave whose rows all go to one group (a sorted source) combines with shuffles first and issues one
 * atomic per accumulator; (7) the result is written as one word range with consecutive lanes on consecutive words,
 * FIRST and LAST words gathered from the source, the pad rows by the workgroups behind the grid.  Every output word is
 * written exactly once and nothing reads the output; everything a kernel reads was written by a fill or a kernel of
 * this call.
 * Waits: exactly ONE, for the copy back of the number of groups (16 bytes), which sizes the result and the records.
 * Temporaries, all from ctx's pool: the slot table (4 bytes x capacity: 8 to 16 bytes per source row), the class word
 * (4 bytes per source row), the block counts and offsets (12 bytes per block), and, sized after the wait, the records:
 * 8 bytes x (3 + aggregates) per GROUP.  No table of capacity x aggregates.
 * Knobs, both read on every call, no output word depends on either: TS_COLLECT_BLOCK_ROWS (1 .. 1024) caps the rows of
 * a count block, with the meaning and the refusals it has above; TS_LOGUP_HASH_BITS (0 .. 32) lengthens the probe
 * chains.
 * Out of scope: several sources; a group id per SOURCE row (join the source against the result by key with
 * TS_JOIN_TABLE_ROW, or fetch INDEX); keys compared mod p (derive a canonical column first); products, or aggregates
 * over extension-field words; more than 8 key words, 16 aggregates or 64 columns; use inside batch lanes; a kernel
 * specialised per spec. */
enum { TS_GROUP_MAX_KEYS = 8, TS_GROUP_MAX_AGGREGATES = 16, TS_GROUP_MAX_WIDTH = 64 };

/* ---- joined rows: columns of another table, fetched by key, in HBM ----
 * Every call above reads the rows of its own sources.  A column whose value is DEFINED BY ANOTHER TABLE -- the
 * instruction a machine row fetched from a program ROM (pc -> opcode, operands), the flags an opcode decodes to, an
 * S-box entry given by its key tuple, a value read from a snapshot keyed by (segment, address) -- is a keyed fetch: for
 * every row of `src` find the row of `table` with the same key tuple and write chosen columns of that row into the
 * source's row.  This call does that in HBM.  It replaces: ts_matrix_download, a dictionary or sort-and-search join on
 * the host, ts_matrix_upload.
 * Keys: n_keys (1 .. 8) terms on each side, ts_logup_term of kind 0 (a canonical constant) or 1 (a column of the
 * side's own row); kind 2 is refused.  Matching is the rule of ts_logup_multiplicities: key words are compared AS
 * STORED, with no reduction (p + 1 does not match 1).  Only the table's rows [0, table_rows) are entered (0 = all of
 * them: a padded table gives the number of its real rows).  Entered rows with equal tuples form a class; the class's
 * LOWEST row is the match.  The result is the same words on every run and for every value of the knob below.
 * Taking part: `when` is a term on src's row; the row takes part iff the word, reduced mod p, is != 0 -- the selector
 * rule of ts_matrix_collect_rows: 0, p and 2p do not fire, 1 and 0xFFFFFFFF do.  The constant 1 is "every row".
 * What a row receives: for f < n_fetch, a matched row gets table[match][table_columns[f]], as stored, in column
 * dst_columns[f]; a row that takes no part, or that finds no match, gets defaults[f] (canonical).  With TS_JOIN_KEEP
 * such a row instead keeps src's own word where the dst column lies inside src (a dst column behind src still gets its
 * default): several joins can be chained, each filling the rows its `when` selects.
 * Misses: a miss is a row that takes part and finds no table row.  *n_missing counts them, *first_missing is the least
 * such source row (~0 when there is none); the status is TS_OK and the result is complete.  With n_missing == NULL any
 * miss is TS_ERR_INVARIANT with the row in the last error; *out is NULL then and every pool block the call took is
 * returned.  first_missing may be NULL in either case.
 * Shape of the result, as ts_matrix_derive: *out is a NEW row-major matrix of src's height.  Its width is
 * max(src_width, 1 + max dst_columns), then one more column for TS_JOIN_TABLE_ROW (the matched row's index, 0 without
 * a match) and one more for TS_JOIN_HIT (1 on a matched row, 0 elsewhere), in that order.  Every column at or beyond
 * src's width must be named by dst_columns; no dst column appears twice; every other column is copied as stored.  All
 * reads see src, so a dst column may overwrite a key column or the `when` column.  src and table may be the same
 * handle; neither is consumed or written.
 * TS_ERR_INVALID, each with a text in ts_last_error, before any device work, leaving *out NULL: a NULL argument; a
 * wrong struct_size; n_keys outside 1 .. 8 or n_fetch outside 0 .. 32; n_fetch == 0 with neither TS_JOIN_TABLE_ROW nor
 * TS_JOIN_HIT; an unknown flag; a term kind above 1; a column outside its matrix; a non-canonical constant or default;
 * a dst column named twice or a column behind src that is not named; table_rows above the table's height; a result
 * wider than 2^16; a height outside [1, 2^27]; a matrix that is not row-major, is consumed or is from another context;
 * TS_LOGUP_HASH_BITS outside its range.
 * Launches: TWO kernels (csrc/join.hip) behind the fills of the slot table and of the report, no workgroup waits for
 * another.  (1) insert, the protocol of the multiplicity fill: one table row per lane, atomicCAS / atomicMin on a slot
 * table of the power of two at or above 2 * table_rows; (2) fetch: a workgroup owns 256 source rows; one lane per row
 * evaluates `when`, builds the tuple, probes and leaves the matched row in LDS (the misses of a wave are one add); then
 * all lanes write the block's rows as one contiguous word range with coalesced stores, choosing per word the source
 * word, a table word through the LDS match, or a default.  Every result word is written exactly once.
 * Waits: exactly ONE, after launch 2, for the copy back of the miss report (32 bytes).  Temporaries come from ctx's
 * pool.  TS_LOGUP_HASH_BITS (0 .. 32, read on every call) lengthens the probe chains here too and changes no output.
 * A full slot table cannot happen and is TS_ERR_INVARIANT "internal error", as in the multiplicity calls.
 * Out of scope: a table index kept between calls (a handle built once for a ROM and probed by many traces); more than
 * one match per row; preprocessed-kind (kind 2) terms -- pass ts_multi_key_values(key, i) as the table instead;
 * extension-field words; use inside batch lanes. */
#define TS_JOIN_MAX_KEYS   8u      /* = the LogUp tuple width */
#define TS_JOIN_MAX_FETCH  32u
#define TS_JOIN_TABLE_ROW  1u      /* append the matched table row's index (0 on a row without a match) */
#define TS_JOIN_HIT        2u      /* append 1 on a matched row, 0 elsewhere */
#define TS_JOIN_KEEP       4u      /* a row without a match keeps src's word in a dst column inside src */
typedef struct {
    uint32_t struct_size;             /* = sizeof(ts_join_spec), else TS_ERR_INVALID */
    uint32_t n_keys;                  /* 1 .. 8 */
    const ts_logup_term* src_keys;    /* n_keys terms on src's row: kind 0 constant, 1 column */
    const ts_logup_term* table_keys;  /* n_keys terms on the table's row, same kinds */
    ts_logup_term when;               /* src's row takes part iff this word mod p != 0; constant 1 = every row */
    uint32_t n_fetch;                 /* 0 .. 32 */
    const uint32_t* table_columns;    /* n_fetch columns of the table ... */
    const uint32_t* dst_columns;      /* ... written to these columns of the result */
    const uint32_t* defaults;         /* n_fetch canonical words for rows without a match */
    uint32_t flags;
    uint64_t table_rows;              /* only rows [0, table_rows) of the table are entered; 0 = all */
} ts_join_spec;
ts_status ts_matrix_join_rows(ts_ctx* ctx, const ts_join_spec* spec, const ts_matrix* src, const ts_matrix* table,
                              ts_matrix** out, uint64_t* n_missing, uint64_t* first_missing);
/* Host only, no context: every check above that needs no matrix but the two widths; the text of a refusal is what
 * ts_last_error returns for a NULL context.  out_width (may be NULL) is the width of the result. */
ts_status ts_join_check(const ts_join_spec* spec, uint32_t src_width, uint32_t table_width, uint32_t* out_width);
/* Host only: the same checks, then the plain sequential loop: src is src_height rows of src_width words, table is
 * table_height rows of table_width words, both row-major; they may be one buffer.  out receives src_height * out_width
 * words (TS_ERR_BUFFER if out_words is less; nothing is written then, nor by a refused call, nor by a miss with
 * n_missing == NULL).  A reference for tests and for callers without a device, not a fast path. */
ts_status ts_join_rows_host(const ts_join_spec* spec, const uint32_t* src, uint64_t src_height, uint32_t src_width,
                            const uint32_t* table, uint64_t table_height, uint32_t table_width, uint32_t* out,
                            uint64_t out_words, uint64_t* n_missing, uint64_t* first_missing);

/* ---- expanded rows: a data-dependent number of rows per source row, in HBM ----
 * The collect selects rows: its output has at most 16 rows per source row, each written out in the spec.  A table with
 * a DATA-DEPENDENT number of rows per source row -- the elements of a block instruction (memcpy or memset of `len`
 * words, load or store multiple), the R rounds of a precompile call, the `cycles` rows a chip spends on an instruction,
 * a run-length-encoded trace unrolled -- is the inverse: a load-balanced expansion.  This call does that in HBM.  It
 * replaces: ts_matrix_download, a repeat of every row by its count and an index ramp on the host, ts_matrix_upload.
 * The spec is a word tape, written as the collect's is:
 *   [0]=0x50584554 ("TEXP") [1]=1 [2]=src_width (1..2^16) [3]=out_width (1..64)
 *   [4]=sel_kind [5]=sel_value        0/1: every row (the collect's rule: the value must be 1);
 *                                     1/c: column c, the row takes part iff the word, reduced mod p, is != 0
 *   [6]=count_kind [7]=count_value    0/c: the constant c, 1 <= c <= max_count (0 is refused);
 *                                     1/c: column c
 *   [8]=max_count                     1 .. 2^27
 *   out_width x pad word              the pad row, each word < p = 0x78000001
 *   out_width x {kind, value, step}   one term per output column
 * Count: a row that takes part asks for cnt = its count word reduced mod p (p asks for 0 rows, p + 3 for 3), or the
 * constant; a row that takes no part asks for 0.  cnt = 0 is allowed and emits nothing.  cnt > max_count on a row that
 * takes part is a data error (below).
 * Terms, for output row (source row r, inner index j, 0 <= j < cnt):
 *   kind 0  a constant `value` < p
 *   kind 1  column `value` of row r, copied AS STORED (not reduced, like the collect's kind 1)
 *   kind 2  the row index r
 *   kind 3  the inner index j
 *   kind 4  what remains, cnt - 1 - j
 *   kind 5  1 if j == 0, else 0
 *   kind 6  1 if j == cnt - 1, else 0
 *   kind 7  the stepped word (word mod p + j * step) mod p, canonical, over column `value`, with `step` < p: the
 *           address of element j of a span
 * `step` must be 0 for every kind but 7; `value` must be 0 for kinds 2 to 6.
 * Order: the output rows are the (r, j) pairs in lexicographic order.  The result is unique, the same on every run and
 * for every value of the knob below.
 * Height: *n_live is the sum of all cnt.  out_height is 0 or a power of two in [1, 2^27]; 0 means the least power of
 * two >= max(n_live, 1).  *out is a NEW row-major matrix of that height and out_width columns; rows [n_live, height)
 * hold the pad row.  src is neither consumed nor written.
 * TS_ERR_INVALID, each with a text in ts_last_error, before any device work, leaving *out NULL: a NULL argument; a
 * wrong magic or version, or a word count that does not match the header; a width, max_count, selector, count, column,
 * kind, constant, pad word, step or value word that breaks a rule above; src_width that differs from the matrix's
 * width; a matrix that is not row-major, is consumed or belongs to another context; a height outside [1, 2^27]; an
 * out_height that is not 0 or a power of two in range; TS_EXPAND_BLOCK_ROWS outside its range.
 * Refused after the one wait, in this order when both hold; there is no output then, *n_live is 0, *out is NULL and
 * every pool block the call took is returned:
 *   1. TS_ERR_INVARIANT "expand: row R asks for C rows, max_count M": R is the LEAST row over max_count, C its count;
 *   2. TS_ERR_INVALID "expand: N rows asked for, out_height H" (H = 2^27 when out_height is 0).  N is exact for any
 *      input, up to 2^27 rows of 2^27 each: every sum that feeds it is 64-bit.
 * Launches: THREE kernels (csrc/expand.hip), reduce-then-scan, no workgroup waits for another.  (1) one workgroup per
 * block of at most TS_EXPAND_BLOCK_ROWS source rows reads the selector and count columns only and leaves every row's
 * position inside its block, the block's sum and the block's least row over max_count; (2) one workgroup makes the
 * exclusive scan of the block sums, the carry in 64 bits, and leaves the total and the least offending row with its
 * count behind them; (3) the grid is partitioned by OUTPUT rows: a workgroup owns a tile of consecutive output rows,
 * finds the source row of each by binary search (the largest row whose offset is at or below it, so rows asking for
 * nothing lose), and writes the tile as one contiguous word range with coalesced stores and reads gathered in the
 * source rows; the workgroups behind the tiles in the same launch fill the pad rows.  One row asking for 2^22 rows
 * costs what 2^22 rows asking for one do.  Pad row and term table go to the device in one asynchronous copy through the
 * context's page-locked staging arena.  Every output word is written exactly once and nothing reads the output.
 * Waits: exactly ONE, between launches 2 and 3, for the copy back of the total, the least offending row and its count
 * (24 bytes).  Temporaries come from ctx's pool: 4 bytes per source row and 16 per block.
 * TS_EXPAND_BLOCK_ROWS (1 .. 1024, default 1024, read on every call) caps the source rows of a block of launch 1 and
 * the output rows of a tile of launch 3: a test knob that makes small matrices cross the lane, the wave, the workgroup,
 * several trips of launch 2's loop and tiles that straddle blocks.  No output word depends on it.  A value so small
 * that a grid would pass 2^24 workgroups is refused (for launch 3 this is known only after the wait).
 * Out of scope: several sources, or several output forms per element (stack with the collect or sort afterwards); use
 * inside batch lanes; extension-field words; a kernel specialised per spec. */
enum { TS_EXPAND_MAX_WIDTH = 64, TS_EXPAND_MAX_COUNT = 1 << 27 };
ts_status ts_matrix_expand_rows(ts_ctx* ctx, const uint32_t* spec, size_t n_words, const ts_matrix* src,
                                uint64_t out_height, ts_matrix** out, uint64_t* n_live);
/* Host only, no context: every check above that needs no matrix; the text of a refusal is what ts_last_error returns
 * for a NULL context.  src_width and out_width are the header's; each may be NULL. */
ts_status ts_expand_check(const uint32_t* spec, size_t n_words, uint32_t* src_width, uint32_t* out_width);
/* Host only: the same checks, then the plain sequential loop over `height` (1 .. 2^27) host rows of src_width words.
 * out_row_major receives *out_height_used * out_width words, pad rows included (TS_ERR_BUFFER if out_cap_words is less;
 * nothing is written then, nor by a refused call).  The height rules and the two late refusals are those above.  A
 * reference for tests and for callers without a device, not a fast path. */
ts_status ts_expand_rows_host(const uint32_t* spec, size_t n_words, const uint32_t* src_row_major, uint64_t height,
                              uint64_t out_height, uint32_t* out_row_major, size_t out_cap_words,
                              uint64_t* out_height_used, uint64_t* n_live);

/* library/ABI version (bumped on any incompatible change) */
uint32_t ts_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
