//! `prove_gpu`: the reference's `prove` (uni-stark/src/prover.rs:25-119) with the same arguments,
//! in two forms: (1) one call, `ts_prove` -- the whole transcript runs inside the library;
//! (2) step by step through `impl Pcs for GpuFriPcs`, line for line the reference's body, for
//! callers that interleave their own logic.  Both give the same bytes.
use std::ptr;

use p3_air::Air;
use p3_challenger::{CanObserve, CanSample};
use p3_commit::PolynomialSpace;
use p3_field::{AbstractField, PrimeField32};
use p3_matrix::dense::RowMajorMatrix;
use p3_matrix::Matrix;
use uni_stark::SymbolicAirBuilder;

use basic::bf_pcs::Pcs;

use crate::air::{serialize_constraints, LogUp, LogUpTerm};
use crate::context::{DeviceMatrix, GpuChallenger, GpuContext, PinnedTrace};
use crate::ffi::*;
use crate::pcs::{FriConfig, GpuFriPcs, GpuProverData};
use crate::proof::{Challenge, Commitments, OpenedValues, Proof, Val};

/// An AIR registered with the library (tape uploaded, quotient kernel specialised with hiprtc)
pub struct CompiledAir<'c> {
    ctx: &'c GpuContext,
    pub(crate) raw: *mut ts_air,
    pub log_quotient_degree: usize,
}
impl<'c> CompiledAir<'c> {
    pub fn new<A: Air<SymbolicAirBuilder<Val>>>(ctx: &'c GpuContext, air: &A, num_public_values: usize) -> Self {
        let tape = serialize_constraints::<Val, A>(air, num_public_values);
        let mut raw = ptr::null_mut();
        ctx.check(unsafe { ts_air_compile(ctx.raw, tape.as_ptr(), tape.len(), &mut raw) }, "ts_air_compile");
        let mut lqd = 0u32;
        unsafe { ts_air_info(raw, ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), &mut lqd) };
        Self { ctx, raw, log_quotient_degree: lqd as usize }
    }

    /// An AIR from its tape: what `AuxAirBuilder::tape()` gives for an AIR with preprocessed or aux columns.
    pub fn from_tape(ctx: &'c GpuContext, tape: &[u32]) -> Self {
        let mut raw = ptr::null_mut();
        ctx.check(unsafe { ts_air_compile(ctx.raw, tape.as_ptr(), tape.len(), &mut raw) }, "ts_air_compile");
        let mut lqd = 0u32;
        unsafe { ts_air_info(raw, ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), &mut lqd) };
        Self { ctx, raw, log_quotient_degree: lqd as usize }
    }
}
impl Drop for CompiledAir<'_> {
    fn drop(&mut self) {
        unsafe { ts_air_free(self.ctx.raw, self.raw) }
    }
}

fn proof_capacity(fri: &FriConfig, degree: usize, width: usize, qd: usize) -> usize {
    let log_n = degree.trailing_zeros() as usize + fri.log_blowup;
    let r = log_n - fri.log_blowup;
    64 + 8 * width + 16 * qd + 8 * r + fri.num_queries * (16 + width + 5 * qd + 16 * log_n + r * (9 + 8 * log_n))
}

/// Form 1.  `challenger` is left in the state the reference's `&mut Challenger` would be in.
pub fn prove_gpu<A>(pcs: &GpuFriPcs<'_>, air: &A, challenger: &mut GpuChallenger, trace: RowMajorMatrix<Val>,
                    public_values: &Vec<Val>) -> Proof
where
    A: Air<SymbolicAirBuilder<Val>>,
{
    let ctx = pcs.ctx;
    let cair = CompiledAir::new(ctx, air, public_values.len());
    let pis: Vec<u32> = public_values.iter().map(|v| v.as_canonical_u32()).collect();
    let m = DeviceMatrix::upload_monty(ctx, &trace.values, trace.height(), trace.width());
    let cfg = pcs.fri.raw();
    let mut out = vec![0u32; proof_capacity(&pcs.fri, trace.height(), trace.width(), 1 << cair.log_quotient_degree)];
    let mut n = 0usize;
    let raw_m = m.into_raw();
    ctx.check(
        unsafe {
            ts_prove(ctx.raw, &cfg, cair.raw, challenger.raw, raw_m,
                     if pis.is_empty() { ptr::null() } else { pis.as_ptr() }, pis.len() as u32, out.as_mut_ptr(),
                     out.len(), &mut n)
        },
        "ts_prove",
    );
    unsafe { ts_matrix_free(ctx.raw, raw_m) };
    Proof::from_tspf(&out[..n])
}

/// One table of `prove_gpu_multi`: a compiled plain AIR (no preprocessed, no aux columns), its trace on the AIR's
/// context (consumed) and its public values as canonical words.
pub struct MultiTable<'a> {
    pub air: &'a CompiledAir<'a>,
    pub trace: DeviceMatrix<'a>,
    pub public_values: Vec<u32>,
}

/// Several AIR tables of mixed heights in ONE proof (`ts_prove_multi`): the TSPF v6 words, for
/// `verify_gpu_multi`.  The challenger observes the table count and every log-degree first, so it ends where the
/// verifier's will.
pub fn prove_gpu_multi(pcs: &GpuFriPcs<'_>, challenger: &mut GpuChallenger, tables: Vec<MultiTable<'_>>) -> Vec<u32> {
    let ctx = pcs.ctx;
    let cfg = pcs.fri.raw();
    let pis: Vec<Vec<u32>> = tables.iter().map(|t| t.public_values.clone()).collect();
    let airs: Vec<*const ts_air> = tables.iter().map(|t| t.air.raw as *const ts_air).collect();
    let raws: Vec<*mut ts_matrix> = tables.into_iter().map(|t| t.trace.into_raw()).collect();
    let mut raw_tables: Vec<ts_multi_table> = (0..raws.len())
        .map(|t| ts_multi_table {
            struct_size: core::mem::size_of::<ts_multi_table>() as u32,
            n_public: pis[t].len() as u32,
            air: airs[t],
            trace: raws[t],
            public_values: if pis[t].is_empty() { ptr::null() } else { pis[t].as_ptr() },
        })
        .collect();
    // the call consumes the traces, so the buffer is sized generously rather than asked for in a first call
    // (TS_ERR_BUFFER would report the size, with the traces gone)
    let mut out = vec![0u32; 1 << 22];
    let mut n = 0usize;
    let rc = unsafe {
        ts_prove_multi(ctx.raw, &cfg, challenger.raw, raw_tables.as_mut_ptr(), raw_tables.len() as u32,
                       out.as_mut_ptr(), out.len(), &mut n)
    };
    for m in raws {
        unsafe { ts_matrix_free(ctx.raw, m) };
    }
    ctx.check(rc, "ts_prove_multi");
    out.truncate(n);
    out
}

/// `ts_verify_multi` (host only): the verdict, 0 = accepted, codes as `ts_verify`.
pub fn verify_gpu_multi(fri: FriConfig, challenger: &mut GpuChallenger, airs: &[&CompiledAir<'_>],
                        public_values: &[Vec<u32>], proof: &[u32]) -> i32 {
    let cfg = fri.raw();
    let raw_airs: Vec<*const ts_air> = airs.iter().map(|a| a.raw as *const ts_air).collect();
    let ptrs: Vec<*const u32> =
        public_values.iter().map(|p| if p.is_empty() { ptr::null() } else { p.as_ptr() }).collect();
    let counts: Vec<u32> = public_values.iter().map(|p| p.len() as u32).collect();
    let mut verdict: std::os::raw::c_int = -1;
    let rc = unsafe {
        ts_verify_multi(&cfg, challenger.raw, raw_airs.as_ptr(), raw_airs.len() as u32, ptrs.as_ptr(),
                        counts.as_ptr(), proof.as_ptr(), proof.len(), &mut verdict)
    };
    if rc != 0 { -1 } else { verdict as i32 }
}

/// One table of `prove_gpu_multi_bus`: a `MultiTable` whose AIR may have LogUp aux columns; `logup` is the
/// `ts_logup_spec` of those columns (the caller keeps what it points into alive), `None` for a plain AIR.
pub struct MultiBusTable<'a> {
    pub air: &'a CompiledAir<'a>,
    pub trace: DeviceMatrix<'a>,
    pub public_values: Vec<u32>,
    pub logup: Option<&'a ts_logup_spec>,
}

/// Several AIR tables of mixed heights tied by a LogUp bus in ONE proof (`ts_prove_multi_bus`): the TSPF v7 words,
/// for `verify_gpu_multi_bus`.
pub fn prove_gpu_multi_bus(pcs: &GpuFriPcs<'_>, challenger: &mut GpuChallenger, tables: Vec<MultiBusTable<'_>>) -> Vec<u32> {
    let ctx = pcs.ctx;
    let cfg = pcs.fri.raw();
    let pis: Vec<Vec<u32>> = tables.iter().map(|t| t.public_values.clone()).collect();
    let airs: Vec<*const ts_air> = tables.iter().map(|t| t.air.raw as *const ts_air).collect();
    let specs: Vec<*const ts_logup_spec> =
        tables.iter().map(|t| t.logup.map_or(ptr::null(), |s| s as *const ts_logup_spec)).collect();
    let raws: Vec<*mut ts_matrix> = tables.into_iter().map(|t| t.trace.into_raw()).collect();
    let mut raw_tables: Vec<ts_multi_bus_table> = (0..raws.len())
        .map(|t| ts_multi_bus_table {
            struct_size: core::mem::size_of::<ts_multi_bus_table>() as u32,
            n_public: pis[t].len() as u32,
            air: airs[t],
            trace: raws[t],
            public_values: if pis[t].is_empty() { ptr::null() } else { pis[t].as_ptr() },
            logup: specs[t],
        })
        .collect();
    let mut out = vec![0u32; 1 << 22];  // (sized generously: the call consumes the traces, as prove_gpu_multi)
    let mut n = 0usize;
    let rc = unsafe {
        ts_prove_multi_bus(ctx.raw, &cfg, challenger.raw, raw_tables.as_mut_ptr(), raw_tables.len() as u32,
                           out.as_mut_ptr(), out.len(), &mut n)
    };
    for m in raws {
        unsafe { ts_matrix_free(ctx.raw, m) };
    }
    ctx.check(rc, "ts_prove_multi_bus");
    out.truncate(n);
    out
}

/// `ts_verify_multi_bus` (host only): the verdict (0 = accepted, codes as `ts_verify`), the exposed words (four per
/// table with aux columns) and their EF4 sum over the tables.  The bus balances exactly when the sum is zero; that
/// check is the caller's.
pub fn verify_gpu_multi_bus(fri: FriConfig, challenger: &mut GpuChallenger, airs: &[&CompiledAir<'_>],
                            public_values: &[Vec<u32>], proof: &[u32]) -> (i32, Vec<u32>, [u32; 4]) {
    let cfg = fri.raw();
    let raw_airs: Vec<*const ts_air> = airs.iter().map(|a| a.raw as *const ts_air).collect();
    let ptrs: Vec<*const u32> =
        public_values.iter().map(|p| if p.is_empty() { ptr::null() } else { p.as_ptr() }).collect();
    let counts: Vec<u32> = public_values.iter().map(|p| p.len() as u32).collect();
    let mut verdict: std::os::raw::c_int = -1;
    let mut exposed = vec![0u32; 4 * airs.len().max(1)];
    let mut bus_sum = [0u32; 4];
    let rc = unsafe {
        ts_verify_multi_bus(&cfg, challenger.raw, raw_airs.as_ptr(), raw_airs.len() as u32, ptrs.as_ptr(),
                            counts.as_ptr(), proof.as_ptr(), proof.len(), exposed.as_mut_ptr(), exposed.len() as u32,
                            bus_sum.as_mut_ptr(), &mut verdict)
    };
    (if rc != 0 { -1 } else { verdict as i32 }, exposed, bus_sum)
}

/// `ts_logup_aux_build_multi`: the LogUp matrices of `traces` under `specs` for one pair of challenges, in three
/// launches; returns the aux matrices and the exposed sums (four words per table).
pub fn logup_aux_build_multi<'a>(ctx: &'a GpuContext, specs: &[&ts_logup_spec], traces: &[&DeviceMatrix<'a>],
                                 challenges: &[u32; 8]) -> (Vec<DeviceMatrix<'a>>, Vec<u32>) {
    assert_eq!(specs.len(), traces.len());
    let sp: Vec<*const ts_logup_spec> = specs.iter().map(|s| *s as *const ts_logup_spec).collect();
    let tr: Vec<*const ts_matrix> = traces.iter().map(|t| t.raw as *const ts_matrix).collect();
    let mut out: Vec<*mut ts_matrix> = vec![ptr::null_mut(); specs.len()];
    let mut exposed = vec![0u32; 4 * specs.len()];
    ctx.check(
        unsafe {
            ts_logup_aux_build_multi(ctx.raw, specs.len() as u32, sp.as_ptr(), tr.as_ptr(), challenges.as_ptr(),
                                     out.as_mut_ptr(), exposed.as_mut_ptr())
        },
        "ts_logup_aux_build_multi",
    );
    (out.into_iter().map(|raw| DeviceMatrix { ctx, raw }).collect(), exposed)
}

/// `ts_logup_multiplicities_bus`: fills `spec.out_column` of the resident `table_trace` from the lookups on the
/// rows of `lookers`; returns (n_missing, [looker, row, lookup] of the least miss).
pub fn logup_multiplicities_bus<'a>(ctx: &'a GpuContext, spec: &ts_logup_mult_bus_spec, table_trace: &mut DeviceMatrix<'a>,
                                    lookers: &[&DeviceMatrix<'a>]) -> (u64, [u64; 3]) {
    let lk: Vec<*const ts_matrix> = lookers.iter().map(|t| t.raw as *const ts_matrix).collect();
    let (mut n_missing, mut first) = (0u64, [u64::MAX; 3]);
    ctx.check(
        unsafe {
            ts_logup_multiplicities_bus(ctx.raw, spec, table_trace.raw, lk.as_ptr(), &mut n_missing, first.as_mut_ptr())
        },
        "ts_logup_multiplicities_bus",
    );
    (n_missing, first)
}

/// `ts_multi_key`: the preprocessed matrices of a multi-table proof committed once in one batch (mixed heights); never
/// consumed, so one key serves any number of `prove_gpu_multi_key` calls.  `root` is what the verifier holds.
pub struct MultiKey<'a> {
    ctx: &'a GpuContext,
    pub(crate) raw: *mut ts_multi_key,
    pub root: [u32; 8],
}

impl<'a> MultiKey<'a> {
    /// `ts_multi_key_commit`: consumes `matrices`; with `keep_values` their rows stay alive inside the key.
    pub fn commit(pcs: &GpuFriPcs<'a>, matrices: Vec<DeviceMatrix<'a>>, keep_values: bool) -> Self {
        let ctx = pcs.ctx;
        let cfg = pcs.fri.raw();
        let raws: Vec<*mut ts_matrix> = matrices.into_iter().map(|m| m.into_raw()).collect();
        let (mut raw, mut root) = (ptr::null_mut(), [0u32; 8]);
        let rc = unsafe {
            ts_multi_key_commit(ctx.raw, &cfg, raws.len() as u32, raws.as_ptr(), keep_values as std::os::raw::c_int,
                                root.as_mut_ptr(), &mut raw)
        };
        for m in raws {
            unsafe { ts_matrix_free(ctx.raw, m) };
        }
        ctx.check(rc, "ts_multi_key_commit");
        MultiKey { ctx, raw, root }
    }

    /// `ts_multi_key_values`: the row-major values of matrix `idx`, borrowed from the key; `None` without kept values.
    pub fn values(&self, idx: u32) -> Option<*const ts_matrix> {
        let mut out: *const ts_matrix = ptr::null();
        let rc = unsafe { ts_multi_key_values(self.raw, idx, &mut out) };
        if rc != 0 { None } else { Some(out) }
    }
}

impl Drop for MultiKey<'_> {
    fn drop(&mut self) {
        unsafe { ts_multi_key_free(self.ctx.raw, self.raw) };
    }
}

/// `ts_prove_multi_key`: `prove_gpu_multi_bus` against a commit-once key (TSPF v8).  The i-th table whose AIR has
/// preprocessed columns reads matrix i of `key`; a `logup` may use kind-2 terms over it.
pub fn prove_gpu_multi_key(pcs: &GpuFriPcs<'_>, challenger: &mut GpuChallenger, key: &MultiKey<'_>,
                           tables: Vec<MultiBusTable<'_>>) -> Vec<u32> {
    let ctx = pcs.ctx;
    let cfg = pcs.fri.raw();
    let pis: Vec<Vec<u32>> = tables.iter().map(|t| t.public_values.clone()).collect();
    let airs: Vec<*const ts_air> = tables.iter().map(|t| t.air.raw as *const ts_air).collect();
    let specs: Vec<*const ts_logup_spec> =
        tables.iter().map(|t| t.logup.map_or(ptr::null(), |s| s as *const ts_logup_spec)).collect();
    let raws: Vec<*mut ts_matrix> = tables.into_iter().map(|t| t.trace.into_raw()).collect();
    let mut raw_tables: Vec<ts_multi_bus_table> = (0..raws.len())
        .map(|t| ts_multi_bus_table {
            struct_size: core::mem::size_of::<ts_multi_bus_table>() as u32,
            n_public: pis[t].len() as u32,
            air: airs[t],
            trace: raws[t],
            public_values: if pis[t].is_empty() { ptr::null() } else { pis[t].as_ptr() },
            logup: specs[t],
        })
        .collect();
    let mut out = vec![0u32; 1 << 22];
    let mut n = 0usize;
    let rc = unsafe {
        ts_prove_multi_key(ctx.raw, &cfg, challenger.raw, key.raw, raw_tables.as_mut_ptr(), raw_tables.len() as u32,
                           out.as_mut_ptr(), out.len(), &mut n)
    };
    for m in raws {
        unsafe { ts_matrix_free(ctx.raw, m) };
    }
    ctx.check(rc, "ts_prove_multi_key");
    out.truncate(n);
    out
}

/// `ts_verify_multi_key` (host only): as `verify_gpu_multi_bus`, against the key's root.
pub fn verify_gpu_multi_key(fri: FriConfig, challenger: &mut GpuChallenger, key_root: &[u32; 8], airs: &[&CompiledAir<'_>],
                            public_values: &[Vec<u32>], proof: &[u32]) -> (i32, Vec<u32>, [u32; 4]) {
    let cfg = fri.raw();
    let raw_airs: Vec<*const ts_air> = airs.iter().map(|a| a.raw as *const ts_air).collect();
    let ptrs: Vec<*const u32> =
        public_values.iter().map(|p| if p.is_empty() { ptr::null() } else { p.as_ptr() }).collect();
    let counts: Vec<u32> = public_values.iter().map(|p| p.len() as u32).collect();
    let mut verdict: std::os::raw::c_int = -1;
    let mut exposed = vec![0u32; 4 * airs.len().max(1)];
    let mut bus_sum = [0u32; 4];
    let rc = unsafe {
        ts_verify_multi_key(&cfg, challenger.raw, key_root.as_ptr(), raw_airs.as_ptr(), raw_airs.len() as u32,
                            ptrs.as_ptr(), counts.as_ptr(), proof.as_ptr(), proof.len(), exposed.as_mut_ptr(),
                            exposed.len() as u32, bus_sum.as_mut_ptr(), &mut verdict)
    };
    (if rc != 0 { -1 } else { verdict as i32 }, exposed, bus_sum)
}

/// A stream of proofs from HOST traces at the PCIe-inclusive rate (INTEGRATION.md "Three rates").
///
/// `prove_gpu` above uploads synchronously from pageable memory: the GPU idles during the copy and
/// the copy runs at about half the link rate.  Here `lanes` contexts (2 is enough to hide the
/// upload; 4 also hides the latency-bound phases of a proof, as bench.py does) each own a pinned
/// buffer: `fill(i, buf)` writes trace `i` into the lane's buffer (canonical u32, row-major), the
/// upload is enqueued asynchronously on the lane's stream and `ts_prove` follows on the same
/// stream, so the upload of one lane overlaps the proofs of the others.  Mirrors bench.py's
/// `h2d_inclusive` leg (6.1-6.4 ms per 2^20 x 64 proof = the 43 GB/s the link gives; 2.8 ms when
/// the trace is born on the device).  One host thread per lane, as the library requires.
pub fn prove_gpu_stream<A, F>(device: i32, fri: FriConfig, air: &A, num_public_values: usize, height: usize,
                              width: usize, n_proofs: usize, lanes: usize, fill: F,
                              public_values: &(dyn Fn(usize) -> Vec<Val> + Sync)) -> Vec<Proof>
where
    A: Air<SymbolicAirBuilder<Val>> + Sync,
    F: Fn(usize, &mut [u32]) + Sync,
{
    use std::sync::atomic::{AtomicUsize, Ordering};
    use std::sync::Mutex;

    let next = AtomicUsize::new(0);
    let proofs: Mutex<Vec<Option<Proof>>> = Mutex::new((0..n_proofs).map(|_| None).collect());
    std::thread::scope(|s| {
        for _ in 0..lanes.max(1) {
            s.spawn(|| {
                let ctx = GpuContext::new(device);
                let pcs = GpuFriPcs { ctx: &ctx, fri };
                let cair = CompiledAir::new(&ctx, air, num_public_values);
                let mut buf = PinnedTrace::new(height, width);
                let cfg = fri.raw();
                let mut out = vec![0u32; proof_capacity(&pcs.fri, height, width, 1 << cair.log_quotient_degree)];
                loop {
                    let i = next.fetch_add(1, Ordering::Relaxed);
                    if i >= n_proofs {
                        break;
                    }
                    // the previous ts_prove on this context has returned (it blocks until the proof is on
                    // the host), so the lane's buffer is free to overwrite
                    fill(i, buf.as_mut_slice());
                    let pis: Vec<u32> = public_values(i).iter().map(|v| v.as_canonical_u32()).collect();
                    let raw_m = DeviceMatrix::upload_async(&ctx, &buf).into_raw();
                    let mut challenger = GpuChallenger::new();
                    let mut n = 0usize;
                    ctx.check(
                        unsafe {
                            ts_prove(ctx.raw, &cfg, cair.raw, challenger.raw, raw_m,
                                     if pis.is_empty() { ptr::null() } else { pis.as_ptr() }, pis.len() as u32,
                                     out.as_mut_ptr(), out.len(), &mut n)
                        },
                        "ts_prove",
                    );
                    unsafe { ts_matrix_free(ctx.raw, raw_m) };
                    proofs.lock().unwrap()[i] = Some(Proof::from_tspf(&out[..n]));
                    let _ = &mut challenger;
                }
            });
        }
    });
    proofs.into_inner().unwrap().into_iter().map(|p| p.expect("every proof index was taken")).collect()
}

/// One statement of `prove_gpu_batch`: the arguments of one reference `prove` call
/// (uni-stark/src/prover.rs:25-39) and the lane that proves it.
pub struct BatchStatement<'a> {
    pub lane: usize,
    pub trace: &'a RowMajorMatrix<Val>,
    pub public_values: &'a [Val],
    /// `None` = a fresh challenger; otherwise the library proves from a clone and leaves this one as it is
    pub challenger: Option<&'a GpuChallenger>,
}

/// Why one statement of a batch has no proof: the item's `ts_status` (-1: not attempted, an earlier
/// statement of its lane hit a device error), and the words it needed on `TS_ERR_BUFFER`.
#[derive(Debug, Clone, Copy)]
pub struct BatchError {
    pub status: ts_status,
    pub n_words: usize,
}

/// Many statements in ONE library call (`ts_prove_batch`): lane `l` is `lanes[l]` (its context and AIR; the AIRs
/// may differ), one host thread per lane inside the library, each trace uploaded on its lane's stream just
/// before its proof.  Every statement gets its own `Result`: a bad statement fails alone, a device error stops
/// only its lane.  What `prove_gpu_stream` does with Rust threads, for hosts that prefer one call.
pub fn prove_gpu_batch(fri: FriConfig, lanes: &[&CompiledAir<'_>], statements: &[BatchStatement<'_>],
                       gate_ms: f64) -> Vec<Result<Proof, BatchError>> {
    let ctxs: Vec<*mut ts_ctx> = lanes.iter().map(|a| a.ctx.raw).collect();
    let airs: Vec<*const ts_air> = lanes.iter().map(|a| a.raw as *const ts_air).collect();
    // the host buffers must stay untouched until the call returns: they live to the end of this function
    let words: Vec<Vec<u32>> =
        statements.iter().map(|s| s.trace.values.iter().map(|v| v.as_canonical_u32()).collect()).collect();
    let pis: Vec<Vec<u32>> =
        statements.iter().map(|s| s.public_values.iter().map(|v| v.as_canonical_u32()).collect()).collect();
    let mut outs: Vec<Vec<u32>> = statements
        .iter()
        .map(|s| {
            let lqd = lanes.get(s.lane).map_or(0, |a| a.log_quotient_degree);
            vec![0u32; proof_capacity(&fri, s.trace.height(), s.trace.width(), 1 << lqd)]
        })
        .collect();
    let mut items: Vec<ts_batch_item> = statements
        .iter()
        .enumerate()
        .map(|(i, s)| ts_batch_item {
            struct_size: core::mem::size_of::<ts_batch_item>() as u32,
            lane: s.lane as u32,
            trace: ptr::null_mut(),
            host_trace: words[i].as_ptr(),
            height: s.trace.height() as u64,
            width: s.trace.width() as u32,
            n_public: pis[i].len() as u32,
            public_values: if pis[i].is_empty() { ptr::null() } else { pis[i].as_ptr() },
            challenger: s.challenger.map_or(ptr::null(), |c| c.raw as *const ts_challenger),
            proof_out: outs[i].as_mut_ptr(),
            cap_words: outs[i].len(),
            status: -1,
            n_words: 0,
            proof_blake3: [0; 8],
            final_state: [0; 34],
            start_ms: 0.0,
            wall_ms: 0.0,
        })
        .collect();
    let cfg = fri.raw();
    let rc = unsafe {
        ts_prove_batch(ctxs.as_ptr(), airs.as_ptr(), ctxs.len() as u32, &cfg, items.as_mut_ptr(),
                       items.len() as u32, gate_ms, 0)
    };
    // a refused call (no lanes, an invalid FriConfig) writes no item: its status goes to every statement
    let refused = rc != TS_OK && items.iter().all(|it| it.status == -1);
    items
        .iter()
        .enumerate()
        .map(|(i, it)| match it.status {
            TS_OK => Ok(Proof::from_tspf(&outs[i][..it.n_words])),
            status => Err(BatchError { status: if refused { rc } else { status }, n_words: it.n_words }),
        })
        .collect()
}

/// One lane of `prove_gpu_batch_lookup`: its AIR, and what the lane owns for all of its statements.
pub struct LookupLane<'a> {
    pub air: &'a CompiledAir<'a>,
    /// the AIR's committed key (made on the lane's context); `None` exactly for an AIR without preprocessed columns
    pub key: Option<&'a GpuProverData<'a>>,
    /// the row-major table values `LogUpTerm::Prep` terms read (the key's commit consumed its own matrix)
    pub key_values: Option<&'a DeviceMatrix<'a>>,
    /// the aux source of every statement of the lane, run by the library on the lane's stream; `None` for an AIR
    /// without aux columns
    pub logup: Option<&'a LogUp>,
    /// multiplicity fills of every statement's trace, before its commit: (table interaction, lookup interactions)
    /// of `logup`, as `LogUp::fill_multiplicities` takes them
    pub fills: Vec<(usize, Vec<usize>)>,
}

/// A proved statement of `prove_gpu_batch_lookup`: the TSPF v5 words (`ts_verify_pre_aux` checks them) and the
/// exposed words, whose statement -- for LogUp: all zero -- is the caller's to check.
pub struct LookupProof {
    pub words: Vec<u32>,
    pub exposed: Vec<u32>,
}

/// Why a statement of `prove_gpu_batch_lookup` has no proof: `BatchError`, and for a multiplicity fill that found a
/// lookup in no table row (`TS_ERR_INVARIANT`; the lane goes on) the count and the first `row * lookups + lookup`.
#[derive(Debug, Clone, Copy)]
pub struct LookupBatchError {
    pub status: ts_status,
    pub n_words: usize,
    pub n_missing: u64,
    pub first_missing: u64,
}

/// `prove_gpu_batch` for AIRs with a preprocessed key, challenge-phase columns or both (`ts_prove_batch_lookup`):
/// the key per lane, the LogUp columns and multiplicity columns built by the library inside the lane, no callback
/// per proof.  Statement i's words are those of `ts_prove_pre_aux` on its lane's context.
pub fn prove_gpu_batch_lookup(fri: FriConfig, lanes: &[LookupLane<'_>], statements: &[BatchStatement<'_>],
                              gate_ms: f64) -> Vec<Result<LookupProof, LookupBatchError>> {
    let term = |t: LogUpTerm| {
        let (kind, value) = t.to_c();
        ts_logup_term { kind, value }
    };
    let ctxs: Vec<*mut ts_ctx> = lanes.iter().map(|l| l.air.ctx.raw).collect();
    let airs: Vec<*const ts_air> = lanes.iter().map(|l| l.air.raw as *const ts_air).collect();
    let raw_lanes: Vec<ts_batch_lane> = lanes
        .iter()
        .map(|l| ts_batch_lane {
            struct_size: core::mem::size_of::<ts_batch_lane>() as u32,
            key: l.key.map_or(ptr::null(), |k| k.raw as *const ts_pcs_data),
            key_values: l.key_values.map_or(ptr::null(), |m| m.raw as *const ts_matrix),
        })
        .collect();
    // per lane: the spec's terms, interactions and header, and the fills' terms and headers; all of it lives to the
    // end of this function, and no vector is touched after a pointer into it was taken
    let values: Vec<Vec<Vec<ts_logup_term>>> = lanes
        .iter()
        .map(|l| l.logup.map_or(Vec::new(), |u| {
            u.interactions.iter().map(|(_, v)| v.iter().map(|t| term(*t)).collect()).collect()
        }))
        .collect();
    let interactions: Vec<Vec<ts_logup_interaction>> = lanes
        .iter()
        .enumerate()
        .map(|(k, l)| l.logup.map_or(Vec::new(), |u| {
            u.interactions
                .iter()
                .enumerate()
                .map(|(i, (m, v))| ts_logup_interaction {
                    multiplicity: term(*m),
                    n_values: v.len() as u32,
                    values: values[k][i].as_ptr(),
                })
                .collect()
        }))
        .collect();
    let specs: Vec<ts_logup_spec> = interactions
        .iter()
        .map(|its| ts_logup_spec {
            struct_size: core::mem::size_of::<ts_logup_spec>() as u32,
            n_interactions: its.len() as u32,
            interactions: its.as_ptr(),
        })
        .collect();
    // (table tuple, lookups' tuples, weights) per fill
    let fill_terms: Vec<Vec<(Vec<ts_logup_term>, Vec<ts_logup_term>, Vec<ts_logup_term>, u32)>> = lanes
        .iter()
        .map(|l| {
            l.fills
                .iter()
                .map(|(table, lookups)| {
                    let u = l.logup.expect("prove_gpu_batch_lookup: fills need the lane's LogUp");
                    let (m, tuple) = &u.interactions[*table];
                    let out_column = match m {
                        LogUpTerm::Col(c) => *c,
                        _ => panic!("prove_gpu_batch_lookup: the table interaction's multiplicity must be a main column"),
                    };
                    let mut lookup_terms = Vec::new();
                    let mut weights = Vec::new();
                    for &i in lookups {
                        let (w, v) = &u.interactions[i];
                        assert_eq!(v.len(), tuple.len(), "prove_gpu_batch_lookup: interaction {i} has another number of values");
                        lookup_terms.extend(v.iter().map(|t| term(*t)));
                        weights.push(term(*w));
                    }
                    (tuple.iter().map(|t| term(*t)).collect(), lookup_terms, weights, out_column)
                })
                .collect()
        })
        .collect();
    let fill_specs: Vec<Vec<ts_logup_mult_spec>> = fill_terms
        .iter()
        .map(|fs| {
            fs.iter()
                .map(|(table, lookups, weights, out_column)| ts_logup_mult_spec {
                    struct_size: core::mem::size_of::<ts_logup_mult_spec>() as u32,
                    n_values: table.len() as u32,
                    table: table.as_ptr(),
                    n_lookups: weights.len() as u32,
                    lookups: lookups.as_ptr(),
                    weights: weights.as_ptr(),
                    out_column: *out_column,
                    negate: 1,
                })
                .collect()
        })
        .collect();

    let words: Vec<Vec<u32>> =
        statements.iter().map(|s| s.trace.values.iter().map(|v| v.as_canonical_u32()).collect()).collect();
    let pis: Vec<Vec<u32>> =
        statements.iter().map(|s| s.public_values.iter().map(|v| v.as_canonical_u32()).collect()).collect();
    // the widths beside the trace's and the exposed words, per lane
    let dims: Vec<(usize, usize)> = lanes
        .iter()
        .map(|l| {
            let (mut pw, mut aw, mut nc, mut ne) = (0u32, 0u32, 0u32, 0u32);
            unsafe {
                ts_air_preprocessed_width(l.air.raw, &mut pw);
                ts_air_aux_info(l.air.raw, &mut aw, &mut nc, &mut ne);
            }
            ((pw + aw) as usize, ne as usize)
        })
        .collect();
    let mut outs: Vec<Vec<u32>> = statements
        .iter()
        .map(|s| {
            let lqd = lanes.get(s.lane).map_or(0, |l| l.air.log_quotient_degree);
            let (extra, ne) = dims.get(s.lane).copied().unwrap_or((0, 0));
            let log_lde = s.trace.height().trailing_zeros() as usize + fri.log_blowup;
            // two more Merkle paths and batch headers per query than a plain proof of the joined width
            vec![0u32; proof_capacity(&fri, s.trace.height(), s.trace.width() + extra, 1 << lqd) + ne + 16
                       + 2 * fri.num_queries * (8 * log_lde + 8)]
        })
        .collect();
    let mut exposed: Vec<[u32; 4]> = vec![[0; 4]; statements.len()];
    let mut items: Vec<ts_batch_lookup_item> = statements
        .iter()
        .enumerate()
        .map(|(i, s)| {
            let l = s.lane;
            let has_spec = lanes.get(l).map_or(false, |lane| lane.logup.is_some());
            let fills = fill_specs.get(l).map_or(&[][..], |f| &f[..]);
            ts_batch_lookup_item {
                struct_size: core::mem::size_of::<ts_batch_lookup_item>() as u32,
                lane: l as u32,
                trace: ptr::null_mut(),
                host_trace: words[i].as_ptr(),
                height: s.trace.height() as u64,
                width: s.trace.width() as u32,
                n_public: pis[i].len() as u32,
                public_values: if pis[i].is_empty() { ptr::null() } else { pis[i].as_ptr() },
                challenger: s.challenger.map_or(ptr::null(), |c| c.raw as *const ts_challenger),
                proof_out: outs[i].as_mut_ptr(),
                cap_words: outs[i].len(),
                logup: if has_spec { &specs[l] } else { ptr::null() },
                aux_fn: None,
                aux_user: ptr::null_mut(),
                mult: if fills.is_empty() { ptr::null() } else { fills.as_ptr() },
                n_mult: fills.len() as u32,
                cap_exposed: 4,
                exposed_out: exposed[i].as_mut_ptr(),
                status: -1,
                n_exposed: 0,
                n_words: 0,
                n_missing: 0,
                first_missing: u64::MAX,
                proof_blake3: [0; 8],
                final_state: [0; 34],
                start_ms: 0.0,
                wall_ms: 0.0,
            }
        })
        .collect();
    let cfg = fri.raw();
    let rc = unsafe {
        ts_prove_batch_lookup(ctxs.as_ptr(), airs.as_ptr(), raw_lanes.as_ptr(), ctxs.len() as u32, &cfg,
                              items.as_mut_ptr(), items.len() as u32, gate_ms, 0)
    };
    let refused = rc != TS_OK && items.iter().all(|it| it.status == -1);
    items
        .iter()
        .enumerate()
        .map(|(i, it)| match it.status {
            TS_OK => Ok(LookupProof {
                words: outs[i][..it.n_words].to_vec(),
                exposed: exposed[i][..(it.n_exposed as usize).min(4)].to_vec(),
            }),
            status => Err(LookupBatchError {
                status: if refused { rc } else { status },
                n_words: it.n_words,
                n_missing: it.n_missing,
                first_missing: it.first_missing,
            }),
        })
        .collect()
}

/// Form 2: the body of uni-stark/src/prover.rs:40-118 over the `Pcs` trait.
pub fn prove_gpu_stepwise<A>(pcs: &GpuFriPcs<'_>, air: &A, challenger: &mut GpuChallenger,
                             trace: RowMajorMatrix<Val>, public_values: &Vec<Val>) -> Proof
where
    A: Air<SymbolicAirBuilder<Val>>,
{
    let degree = trace.height(); // :43
    let log_degree = degree.trailing_zeros() as usize;
    let cair = CompiledAir::new(pcs.ctx, air, public_values.len());
    let log_quotient_degree = cair.log_quotient_degree; // :46
    let quotient_degree = 1 << log_quotient_degree;
    let pis: Vec<u32> = public_values.iter().map(|v| v.as_canonical_u32()).collect();

    let trace_domain = pcs.natural_domain_for_degree(degree); // :50
    let (trace_commit, trace_data) = pcs.commit(vec![(trace_domain, trace)]); // :52-53
    challenger.observe(trace_commit.clone()); // :60
    let alpha: Challenge = challenger.sample(); // :63

    // :65-80 quotient domain, evaluations on it, quotient_values, flatten_to_base, split_evals:
    // one fused device call; chunk c lives on the domain {log_n, 31 * w_{n qd}^c} (split_domains)
    let chunks = pcs.quotient_chunks(&trace_data, cair.raw, quotient_degree, &pis, &alpha);
    let quotient_domain = trace_domain.create_disjoint_domain(1 << (log_degree + log_quotient_degree));
    let qc_domains = quotient_domain.split_domains(quotient_degree);
    // :82-83 commit to the chunks (already resident: no upload)
    let cfg = pcs.fri.raw();
    let shifts: Vec<u32> = qc_domains.iter().map(|d| d.shift.as_canonical_u32()).collect();
    let raws: Vec<*mut ts_matrix> = chunks.into_iter().map(DeviceMatrix::into_raw).collect();
    let (mut root, mut qraw) = ([0u32; 8], ptr::null_mut());
    pcs.ctx.check(
        unsafe {
            ts_pcs_commit(pcs.ctx.raw, &cfg, raws.len() as u32, raws.as_ptr(), shifts.as_ptr(), root.as_mut_ptr(),
                          &mut qraw)
        },
        "ts_pcs_commit (quotient chunks)",
    );
    for m in raws {
        unsafe { ts_matrix_free(pcs.ctx.raw, m) };
    }
    let quotient_commit = vec![root.map(u32::to_le_bytes)];
    let quotient_data = crate::pcs::GpuProverData {
        ctx: pcs.ctx,
        raw: qraw,
        dims: vec![(degree << pcs.fri.log_blowup, 4); quotient_degree],
    };
    challenger.observe(quotient_commit.clone()); // :84

    let zeta: Challenge = challenger.sample(); // :91
    let zeta_next = trace_domain.next_point(zeta).unwrap(); // :92
    let (opened_values, opening_proof) = pcs.open(
        vec![
            (&trace_data, vec![vec![zeta, zeta_next]]),
            (&quotient_data, (0..quotient_degree).map(|_| vec![zeta]).collect()),
        ],
        challenger,
    ); // :94-104
    let trace_local = opened_values[0][0][0].clone(); // :105-110
    let trace_next = opened_values[0][0][1].clone();
    let quotient_chunks = opened_values[1].iter().map(|v| v[0].clone()).collect();
    Proof {
        commitments: Commitments { trace: trace_commit, quotient_chunks: quotient_commit },
        opened_values: OpenedValues { trace_local, trace_next, quotient_chunks },
        opening_proof,
        degree_bits: log_degree,
    }
}
