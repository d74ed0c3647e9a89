//! AIR -> constraint tape (`ts_air_compile`, include/tapstark.h "AIR").
//!
//! `get_symbolic_constraints` (uni-stark/src/symbolic_builder.rs:52-64) runs `Air::eval` once on
//! symbolic variables; the resulting `Vec<SymbolicExpression<F>>` (symbolic_expression.rs:12-37) is
//! a DAG of `Rc` nodes.  The tape lists every distinct node once, operands before users
//! ({op, a, b} triples), then the constraint roots in `assert_zero` call order -- the order
//! `ProverConstraintFolder::assert_zero` folds them with alpha (folder.rs:60-64).
use std::collections::HashMap;
use std::rc::Rc;

use p3_air::Air;
use p3_field::{Field, PrimeField32};
// (uni-stark keeps its modules private and re-exports their items at the crate root, src/lib.rs:24-35)
use uni_stark::{get_symbolic_constraints, Entry, SymbolicAirBuilder, SymbolicExpression};

const TAPE_MAGIC: u32 = 0x5441_5354;
const OP_CONST: u32 = 0;
const OP_MAIN: u32 = 1;
const OP_PUBLIC: u32 = 2;
const OP_IS_FIRST_ROW: u32 = 3;
const OP_IS_LAST_ROW: u32 = 4;
const OP_IS_TRANSITION: u32 = 5;
const OP_ADD: u32 = 6;
const OP_SUB: u32 = 7;
const OP_NEG: u32 = 8;
const OP_MUL: u32 = 9;
const OP_PREP: u32 = 10; // version-2 tapes: Entry::Preprocessed { offset } (symbolic_variable.rs:9-15)

struct TapeBuilder<F: Field> {
    nodes: Vec<[u32; 3]>,
    by_ptr: HashMap<*const SymbolicExpression<F>, u32>, // shared sub-expressions (Rc) are emitted once
    by_leaf: HashMap<[u32; 3], u32>,
}

impl<F: PrimeField32> TapeBuilder<F> {
    fn push(&mut self, n: [u32; 3]) -> u32 {
        self.nodes.push(n);
        (self.nodes.len() - 1) as u32
    }
    fn leaf(&mut self, n: [u32; 3]) -> u32 {
        if let Some(&id) = self.by_leaf.get(&n) {
            return id;
        }
        let id = self.push(n);
        self.by_leaf.insert(n, id);
        id
    }
    fn rc(&mut self, e: &Rc<SymbolicExpression<F>>) -> u32 {
        let key = Rc::as_ptr(e);
        if let Some(&id) = self.by_ptr.get(&key) {
            return id;
        }
        let id = self.expr(e);
        self.by_ptr.insert(key, id);
        id
    }
    fn expr(&mut self, e: &SymbolicExpression<F>) -> u32 {
        match e {
            SymbolicExpression::Variable(v) => match v.entry {
                Entry::Main { offset } => self.leaf([OP_MAIN, offset as u32, v.index as u32]),
                Entry::Public => self.leaf([OP_PUBLIC, v.index as u32, 0]),
                // a preprocessed (fixed) column: proved against a commit-once key with `ts_prove_pre`
                // (uni-stark/src/prover.rs:46 itself passes preprocessed_width = 0)
                Entry::Preprocessed { offset } => self.leaf([OP_PREP, offset as u32, v.index as u32]),
                // no permutation / challenge columns on the hot path
                other => panic!("unsupported symbolic variable on the prover hot path: {other:?}"),
            },
            SymbolicExpression::IsFirstRow => self.leaf([OP_IS_FIRST_ROW, 0, 0]),
            SymbolicExpression::IsLastRow => self.leaf([OP_IS_LAST_ROW, 0, 0]),
            SymbolicExpression::IsTransition => self.leaf([OP_IS_TRANSITION, 0, 0]),
            SymbolicExpression::Constant(c) => self.leaf([OP_CONST, c.as_canonical_u32(), 0]),
            SymbolicExpression::Add { x, y, .. } => {
                let (a, b) = (self.rc(x), self.rc(y));
                self.push([OP_ADD, a, b])
            }
            SymbolicExpression::Sub { x, y, .. } => {
                let (a, b) = (self.rc(x), self.rc(y));
                self.push([OP_SUB, a, b])
            }
            SymbolicExpression::Neg { x, .. } => {
                let a = self.rc(x);
                self.push([OP_NEG, a, 0])
            }
            SymbolicExpression::Mul { x, y, .. } => {
                let (a, b) = (self.rc(x), self.rc(y));
                self.push([OP_MUL, a, b])
            }
        }
    }
}

/// The tape of `air` for `num_public_values` public inputs.  `get_log_quotient_degree`
/// (symbolic_builder.rs:15-32) is recomputed by the library from the tape with the same degree
/// rules (symbolic_expression.rs:41-61; `ts_air_info`).
pub fn serialize_constraints<F, A>(air: &A, num_public_values: usize) -> Vec<u32>
where
    F: PrimeField32,
    A: Air<SymbolicAirBuilder<F>>,
{
    serialize_constraints_pre(air, 0, num_public_values)
}

/// The same for an AIR that reads `preprocessed_width` preprocessed columns through
/// `PairBuilder::preprocessed()` (symbolic_builder.rs:144-148): a version-2 tape (one more header word, the
/// leaf `OP_PREP`), to be proved with `ts_prove_pre` against the committed key.  Width 0 gives the version-1
/// tape, word for word what `serialize_constraints` always gave.
pub fn serialize_constraints_pre<F, A>(air: &A, preprocessed_width: usize, num_public_values: usize) -> Vec<u32>
where
    F: PrimeField32,
    A: Air<SymbolicAirBuilder<F>>,
{
    let constraints: Vec<SymbolicExpression<F>> = get_symbolic_constraints(air, preprocessed_width, num_public_values);
    let mut tb = TapeBuilder::<F> { nodes: Vec::new(), by_ptr: HashMap::new(), by_leaf: HashMap::new() };
    let roots: Vec<u32> = constraints.iter().map(|c| tb.expr(c)).collect();
    let mut tape = Vec::with_capacity(7 + 3 * tb.nodes.len() + roots.len());
    tape.extend_from_slice(&[
        TAPE_MAGIC,
        if preprocessed_width == 0 { 1 } else { 2 },
        air.width() as u32,
        num_public_values as u32,
        tb.nodes.len() as u32,
        roots.len() as u32,
    ]);
    if preprocessed_width != 0 {
        tape.push(preprocessed_width as u32);
    }
    for n in &tb.nodes {
        tape.extend_from_slice(n);
    }
    tape.extend_from_slice(&roots);
    tape
}

// ---------------------------------------------------------------------------------------------------------------
// Challenge-phase (aux) columns: tape version 3 (include/tapstark.h).  uni-stark's `SymbolicAirBuilder` has one
// trace phase and no challenge entries, so an AIR with aux columns is captured with a builder of this crate's own:
// the mirror of `ts::air::Builder` in include/tapstark_air.hpp and of `SymbolicAirBuilder` in tap-stark_amd/air.py,
// node for node (hash-consed {op, a, b} triples; every operator builds its nodes in the same fixed order, so the
// three front ends give the same tape for the same `eval`).  Prove the tape with `ts_prove_aux`, or -- built with
// a `preprocessed_width` too, e.g. a `LogUp` with `LogUpTerm::Prep` terms -- with `ts_prove_pre_aux` against the key.
const OP_AUX: u32 = 11; // a = offset 0|1, b = column < aux_width; degree multiple 1
const OP_CHALLENGE: u32 = 12; // a = word index < 4 * n_challenges; degree multiple 0
const OP_EXPOSED: u32 = 13; // a = index < n_exposed; degree multiple 0
const BABYBEAR_P: u64 = 0x7800_0001;
const EF_W: u64 = 11; // EF4 = F[x] / (x^4 - 11)

/// A node id of an [`AuxAirBuilder`].
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Expr(pub u32);

/// An extension-field expression: four coefficients over x^4 - 11.  `assert_zero_ext` emits FOUR base
/// constraints, so an extension-valued constraint is an ordinary constraint of the tape language.
#[derive(Clone, Copy, Debug)]
pub struct ExtExpr(pub [Expr; 4]);

pub struct AuxAirBuilder {
    width: u32,
    n_public: u32,
    preprocessed_width: u32,
    aux_width: u32,
    n_challenges: u32,
    n_exposed: u32,
    nodes: Vec<[u32; 3]>,
    degs: Vec<u32>,
    cse: HashMap<[u32; 3], u32>,
    constraints: Vec<u32>,
}

impl AuxAirBuilder {
    /// Variables in the order of the other front ends: preprocessed, main, public, aux, challenge words, exposed.
    pub fn new(width: u32, n_public: u32, preprocessed_width: u32, aux_width: u32, n_challenges: u32, n_exposed: u32) -> Self {
        let mut b = AuxAirBuilder {
            width, n_public, preprocessed_width, aux_width, n_challenges, n_exposed,
            nodes: Vec::new(), degs: Vec::new(), cse: HashMap::new(), constraints: Vec::new(),
        };
        for off in 0..2 { for c in 0..preprocessed_width { b.node(OP_PREP, off, c, 1); } }
        for off in 0..2 { for c in 0..width { b.node(OP_MAIN, off, c, 1); } }
        for i in 0..n_public { b.node(OP_PUBLIC, i, 0, 0); }
        for off in 0..2 { for c in 0..aux_width { b.node(OP_AUX, off, c, 1); } }
        for k in 0..4 * n_challenges { b.node(OP_CHALLENGE, k, 0, 0); }
        for e in 0..n_exposed { b.node(OP_EXPOSED, e, 0, 0); }
        b
    }
    fn node(&mut self, op: u32, a: u32, b: u32, deg: u32) -> Expr {
        let key = [op, a, b];
        if let Some(&id) = self.cse.get(&key) {
            return Expr(id);
        }
        let id = self.nodes.len() as u32;
        self.nodes.push(key);
        self.degs.push(deg);
        self.cse.insert(key, id);
        Expr(id)
    }
    fn deg(&self, e: Expr) -> u32 { self.degs[e.0 as usize] }
    pub fn main(&mut self, offset: u32, column: u32) -> Expr { self.node(OP_MAIN, offset, column, 1) }
    pub fn preprocessed(&mut self, offset: u32, column: u32) -> Expr { self.node(OP_PREP, offset, column, 1) }
    pub fn public(&mut self, index: u32) -> Expr { self.node(OP_PUBLIC, index, 0, 0) }
    pub fn aux(&mut self, offset: u32, column: u32) -> Expr { self.node(OP_AUX, offset, column, 1) }
    pub fn exposed(&mut self, index: u32) -> Expr { self.node(OP_EXPOSED, index, 0, 0) }
    pub fn challenge(&mut self, k: u32) -> ExtExpr {
        ExtExpr([0, 1, 2, 3].map(|j| self.node(OP_CHALLENGE, 4 * k + j, 0, 0)))
    }
    pub fn constant(&mut self, v: u64) -> Expr { self.node(OP_CONST, (v % BABYBEAR_P) as u32, 0, 0) }
    pub fn is_first_row(&mut self) -> Expr { self.node(OP_IS_FIRST_ROW, 0, 0, 1) }
    pub fn is_last_row(&mut self) -> Expr { self.node(OP_IS_LAST_ROW, 0, 0, 1) }
    pub fn is_transition(&mut self) -> Expr { self.node(OP_IS_TRANSITION, 0, 0, 0) }
    pub fn add(&mut self, x: Expr, y: Expr) -> Expr {
        let d = self.deg(x).max(self.deg(y));
        self.node(OP_ADD, x.0, y.0, d)
    }
    pub fn sub(&mut self, x: Expr, y: Expr) -> Expr {
        let d = self.deg(x).max(self.deg(y));
        self.node(OP_SUB, x.0, y.0, d)
    }
    pub fn mul(&mut self, x: Expr, y: Expr) -> Expr {
        let d = self.deg(x) + self.deg(y);
        self.node(OP_MUL, x.0, y.0, d)
    }
    pub fn assert_zero(&mut self, x: Expr) { self.constraints.push(x.0); }
    /// `when(cond).assert_zero(x)`: assert_zero(cond * x)
    pub fn assert_zero_when(&mut self, cond: Expr, x: Expr) {
        let c = self.mul(cond, x);
        self.assert_zero(c);
    }

    // ---- ExtExpr: the node order of every operator is that of air.py's ExtExpr
    pub fn ext_from_base(&mut self, x: Expr) -> ExtExpr {
        let zero = self.constant(0);
        ExtExpr([x, zero, zero, zero])
    }
    pub fn ext_add(&mut self, x: ExtExpr, y: ExtExpr) -> ExtExpr { ExtExpr([0, 1, 2, 3].map(|k| self.add(x.0[k], y.0[k]))) }
    pub fn ext_sub(&mut self, x: ExtExpr, y: ExtExpr) -> ExtExpr { ExtExpr([0, 1, 2, 3].map(|k| self.sub(x.0[k], y.0[k]))) }
    pub fn ext_mul_base(&mut self, x: ExtExpr, y: Expr) -> ExtExpr { ExtExpr([0, 1, 2, 3].map(|k| self.mul(x.0[k], y))) }
    /// r_k = sum_{i+j=k} a_i b_j + 11 sum_{i+j=k+4} a_i b_j
    pub fn ext_mul(&mut self, x: ExtExpr, y: ExtExpr) -> ExtExpr {
        let mut out = [Expr(0); 4];
        for k in 0..4usize {
            let lo: Vec<Expr> = (0..=k).map(|i| self.mul(x.0[i], y.0[k - i])).collect();
            let hi: Vec<Expr> = (k + 1..4).map(|i| self.mul(x.0[i], y.0[k + 4 - i])).collect();
            let mut acc = lo[0];
            for &t in &lo[1..] {
                acc = self.add(acc, t);
            }
            if !hi.is_empty() {
                let mut h = hi[0];
                for &t in &hi[1..] {
                    h = self.add(h, t);
                }
                let w = self.constant(EF_W);
                let hw = self.mul(h, w);
                acc = self.add(acc, hw);
            }
            out[k] = acc;
        }
        ExtExpr(out)
    }
    pub fn assert_zero_ext(&mut self, x: ExtExpr) {
        for c in x.0 {
            self.assert_zero(c);
        }
    }
    pub fn assert_zero_ext_when(&mut self, cond: Expr, x: ExtExpr) {
        for c in x.0 {
            self.assert_zero_when(cond, c);
        }
    }

    pub fn max_constraint_degree(&self) -> u32 {
        self.constraints.iter().map(|&c| self.degs[c as usize]).max().unwrap_or(0)
    }
    /// Version 3 with aux columns, challenges or exposed words; else version 2 / 1 as `serialize_constraints_pre`.
    pub fn tape(&self) -> Vec<u32> {
        let v3 = self.aux_width != 0 || self.n_challenges != 0 || self.n_exposed != 0;
        let version = if v3 { 3 } else if self.preprocessed_width != 0 { 2 } else { 1 };
        let mut tape = vec![TAPE_MAGIC, version, self.width, self.n_public, self.nodes.len() as u32, self.constraints.len() as u32];
        if v3 {
            tape.extend_from_slice(&[self.preprocessed_width, self.aux_width, self.n_challenges, self.n_exposed]);
        } else if self.preprocessed_width != 0 {
            tape.push(self.preprocessed_width);
        }
        for n in &self.nodes {
            tape.extend_from_slice(n);
        }
        tape.extend_from_slice(&self.constraints);
        tape
    }
}

/// A term of a LogUp interaction: `Const(canonical value)`, `Col(main column)` or `Prep(preprocessed column)` (a
/// lookup against a fixed table: `ts_logup_term.kind = 2`, `ts_logup_aux_build_pre`), read on the local row.
#[derive(Clone, Copy, Debug)]
pub enum LogUpTerm {
    Const(u32),
    Col(u32),
    Prep(u32),
}

impl LogUpTerm {
    /// (kind, value) of the `ts_logup_term` this term is.
    pub fn to_c(self) -> (u32, u32) {
        match self {
            LogUpTerm::Const(v) => (0, v),
            LogUpTerm::Col(c) => (1, c),
            LogUpTerm::Prep(c) => (2, c),
        }
    }
}

/// LogUp over the main trace, from the spec `ts_logup_aux_build` takes: two challenges gamma, beta; interaction i
/// has d_i = gamma + sum_j beta^j v_ij and the fraction m_i / d_i; group g pairs interactions 2g and 2g+1; aux
/// columns 4g..4g+3 hold the group's sum h_g, the last four the exclusive running sum phi, the four exposed words
/// the total S.  `eval` emits `h_g d_a d_b - m_a d_b - m_b d_a = 0`, `is_first phi = 0`,
/// `is_transition (phi' - phi - sum h_g) = 0`, `is_last (phi + sum h_g - S) = 0`.  The statement S = 0 is the
/// caller's to check after `ts_verify_aux`.
pub struct LogUp {
    pub interactions: Vec<(LogUpTerm, Vec<LogUpTerm>)>,
}

impl LogUp {
    pub const N_CHALLENGES: u32 = 2;
    pub const N_EXPOSED: u32 = 4;
    pub fn n_groups(&self) -> u32 { (self.interactions.len() as u32 + 1) / 2 }
    pub fn aux_width(&self) -> u32 { 4 * (self.n_groups() + 1) }

    pub fn eval(&self, b: &mut AuxAirBuilder) {
        let (gamma, beta) = (b.challenge(0), b.challenge(1));
        let term = |b: &mut AuxAirBuilder, t: LogUpTerm| match t {
            LogUpTerm::Const(v) => b.constant(v as u64),
            LogUpTerm::Col(c) => b.main(0, c),
            LogUpTerm::Prep(c) => b.preprocessed(0, c),
        };
        let n_pow = self.interactions.iter().map(|(_, v)| v.len()).max().unwrap_or(1);
        let one = b.constant(1);
        let mut beta_pow = vec![b.ext_from_base(one)];
        for _ in 1..n_pow {
            let next = b.ext_mul(*beta_pow.last().unwrap(), beta);
            beta_pow.push(next);
        }
        let (mut dens, mut mults) = (Vec::new(), Vec::new());
        for (m, values) in &self.interactions {
            let mut d = gamma;
            for (j, v) in values.iter().enumerate() {
                let x = term(b, *v);
                let t = b.ext_mul_base(beta_pow[j], x);
                d = b.ext_add(d, t);
            }
            dens.push(d);
            mults.push(term(b, *m));
        }
        let g_count = self.n_groups();
        let ext_at = |b: &mut AuxAirBuilder, off: u32, first: u32| ExtExpr([0, 1, 2, 3].map(|k| b.aux(off, first + k)));
        let mut total: Option<ExtExpr> = None;
        for g in 0..g_count {
            let h = ext_at(b, 0, 4 * g);
            let (ia, ib) = (2 * g as usize, 2 * g as usize + 1);
            let hd = b.ext_mul(h, dens[ia]);
            if ib < dens.len() {
                let t1 = b.ext_mul(hd, dens[ib]);
                let t2 = b.ext_mul_base(dens[ib], mults[ia]);
                let t3 = b.ext_sub(t1, t2);
                let t4 = b.ext_mul_base(dens[ia], mults[ib]);
                let c = b.ext_sub(t3, t4);
                b.assert_zero_ext(c);
            } else {
                let m = b.ext_from_base(mults[ia]);
                let c = b.ext_sub(hd, m);
                b.assert_zero_ext(c);
            }
            total = Some(match total {
                None => h,
                Some(t) => b.ext_add(t, h),
            });
        }
        let total = total.expect("LogUp: no interactions");
        let phi = ext_at(b, 0, 4 * g_count);
        let phi_next = ext_at(b, 1, 4 * g_count);
        let s = ExtExpr([0, 1, 2, 3].map(|k| b.exposed(k)));
        let first = b.is_first_row();
        b.assert_zero_ext_when(first, phi);
        let transition = b.is_transition();
        let step = b.ext_sub(phi_next, phi);
        let c = b.ext_sub(step, total);
        b.assert_zero_ext_when(transition, c);
        let last = b.is_last_row();
        let end = b.ext_add(phi, total);
        let c = b.ext_sub(end, s);
        b.assert_zero_ext_when(last, c);
    }
}

impl LogUp {
    /// `ts_logup_multiplicities`: fills, in HBM, the multiplicity column of the table-side interaction `table` of
    /// the resident `trace` -- its multiplicity term must be `Col(c)`, and c receives the result; its values are
    /// the table's tuple -- from the interactions `lookups` (their multiplicity terms are the weights), negated so
    /// that the filled trace balances the argument.  `preprocessed`: the row-major values `Prep` terms read.
    /// Returns (n_missing, first_missing): the lookups of non-zero weight that are in no table row and the least
    /// `row * lookups.len() + lookup` among them (`u64::MAX` when none); panics on a miss unless `allow_missing`.
    /// Call it before `prove`, which consumes the trace.
    pub fn fill_multiplicities(&self, trace: &mut crate::context::DeviceMatrix<'_>, table: usize, lookups: &[usize],
                               preprocessed: Option<&crate::context::DeviceMatrix<'_>>, allow_missing: bool) -> (u64, u64) {
        use crate::ffi::{ts_logup_mult_spec, ts_logup_multiplicities, ts_logup_term};
        let c = |t: LogUpTerm| { let (kind, value) = t.to_c(); ts_logup_term { kind, value } };
        let (m, tuple) = &self.interactions[table];
        let out_column = match m {
            LogUpTerm::Col(col) => *col,
            _ => panic!("LogUp::fill_multiplicities: the table interaction's multiplicity must be a main column"),
        };
        assert!(!lookups.is_empty() && !lookups.contains(&table), "LogUp::fill_multiplicities: the lookups");
        let table_terms: Vec<ts_logup_term> = tuple.iter().map(|t| c(*t)).collect();
        let (mut lookup_terms, mut weights) = (Vec::new(), Vec::new());
        for &i in lookups {
            let (w, values) = &self.interactions[i];
            assert_eq!(values.len(), tuple.len(), "LogUp::fill_multiplicities: interaction {i} has another number of values");
            lookup_terms.extend(values.iter().map(|t| c(*t)));
            weights.push(c(*w));
        }
        let spec = ts_logup_mult_spec {
            struct_size: core::mem::size_of::<ts_logup_mult_spec>() as u32,
            n_values: table_terms.len() as u32,
            table: table_terms.as_ptr(),
            n_lookups: weights.len() as u32,
            lookups: lookup_terms.as_ptr(),
            weights: weights.as_ptr(),
            out_column,
            negate: 1,
        };
        let (mut n_missing, mut first_missing) = (0u64, u64::MAX);
        let rc = unsafe {
            ts_logup_multiplicities(trace.ctx.raw, &spec, preprocessed.map_or(core::ptr::null(), |p| p.raw as *const _),
                                    trace.raw, if allow_missing { &mut n_missing } else { core::ptr::null_mut() },
                                    &mut first_missing)
        };
        trace.ctx.check(rc, "ts_logup_multiplicities");
        (n_missing, first_missing)
    }
}

// ---- row programs with carried state for the iterate form of `ts_matrix_derive` (include/tapstark.h "iterated
// columns"): the constants and a mirror of `tap-stark_amd/iterate.py`'s builder.  Source only, never compiled, like
// the rest of the crate.  The tape goes to `ts_matrix_derive`, `ts_derive_check` and `ts_derive_rows_host` as it is.
pub const DERIVE_MAGIC: u32 = 0x5245_4454; // "TDER"
pub const ITERATE_MAGIC: u32 = 0x5254_4954; // "TITR"
pub const ITERATE_MAX_CARRIES: u32 = 16;
pub const ITERATE_MAX_WORK: u64 = 1 << 20;
pub const ITERATE_NO_RESET: u32 = 0xFFFF_FFFF;
pub const V_CONST: u32 = 0;
pub const V_COL: u32 = 1;
pub const V_ROW: u32 = 32;
pub const V_INV: u32 = 33;
pub const V_IS_ZERO: u32 = 34;
pub const V_LT: u32 = 35;
pub const V_BITS: u32 = 36;
pub const V_AND: u32 = 37;
pub const V_XOR: u32 = 38;
pub const V_CARRY: u32 = 40;
pub const V_STEP: u32 = 41;
pub const V_IS_GROUP_FIRST: u32 = 42;
pub const V_IS_GROUP_LAST: u32 = 43;

/// A node of an [`IterateBuilder`].
#[derive(Clone, Copy, Debug)]
pub struct IterNode(pub u32);

/// Collects the nodes, outputs and carries of a TITR program.  Nothing is checked here: `ts_derive_check` is the judge.
pub struct IterateBuilder {
    src_width: u32,
    reset_column: u32,
    max_group_rows: u32,
    nodes: Vec<[u32; 3]>,
    outputs: Vec<[u32; 2]>,
    carries: Vec<[u32; 2]>, // {node, init}
}

impl IterateBuilder {
    pub fn new(src_width: u32, reset_column: Option<u32>, max_group_rows: u32) -> Self {
        Self { src_width, reset_column: reset_column.unwrap_or(ITERATE_NO_RESET), max_group_rows, nodes: Vec::new(),
               outputs: Vec::new(), carries: Vec::new() }
    }
    pub fn node(&mut self, op: u32, a: u32, b: u32) -> IterNode {
        self.nodes.push([op, a, b]);
        IterNode(self.nodes.len() as u32 - 1)
    }
    pub fn constant(&mut self, v: u64) -> IterNode { self.node(V_CONST, (v % 0x7800_0001) as u32, 0) }
    pub fn col(&mut self, c: u32) -> IterNode { self.node(V_COL, 0, c) }
    pub fn next(&mut self, c: u32) -> IterNode { self.node(V_COL, 1, c) }
    pub fn prev(&mut self, c: u32) -> IterNode { self.node(V_COL, 2, c) }
    pub fn add(&mut self, x: IterNode, y: IterNode) -> IterNode { self.node(OP_ADD, x.0, y.0) }
    pub fn sub(&mut self, x: IterNode, y: IterNode) -> IterNode { self.node(OP_SUB, x.0, y.0) }
    pub fn mul(&mut self, x: IterNode, y: IterNode) -> IterNode { self.node(OP_MUL, x.0, y.0) }
    /// A new carry: the node reads its value from BEFORE this row, `init` on a group's first row.
    pub fn carry(&mut self, init: u64) -> IterNode {
        self.carries.push([u32::MAX, (init % 0x7800_0001) as u32]);
        self.node(V_CARRY, self.carries.len() as u32 - 1, 0)
    }
    /// After a row the carry (what `carry` returned) holds `x` of that row.
    pub fn set_carry(&mut self, carry: IterNode, x: IterNode) {
        let k = self.nodes[carry.0 as usize][1] as usize;
        self.carries[k][0] = x.0;
    }
    pub fn step(&mut self) -> IterNode { self.node(V_STEP, 0, 0) }
    pub fn is_group_first(&mut self) -> IterNode { self.node(V_IS_GROUP_FIRST, 0, 0) }
    pub fn is_group_last(&mut self) -> IterNode { self.node(V_IS_GROUP_LAST, 0, 0) }
    pub fn output(&mut self, x: IterNode, dst_column: u32) { self.outputs.push([x.0, dst_column]); }
    pub fn tape(&self) -> Vec<u32> {
        let mut t = vec![ITERATE_MAGIC, 1, self.src_width, self.nodes.len() as u32, self.outputs.len() as u32,
                         self.carries.len() as u32, self.reset_column, self.max_group_rows];
        t.extend(self.nodes.iter().flatten());
        t.extend(self.outputs.iter().flatten());
        t.extend(self.carries.iter().flatten());
        t
    }
}

// ---- the group form of the collect's spec (include/tapstark.h "grouped rows"): the counterpart of
// tap-stark_amd/group.py and of ts::air::Group, word for word.  Like the rest of this crate it has not been compiled.
pub const GROUP_MAGIC: u32 = 0x5052_4754; // "TGRP"
pub const G_CONST: u32 = 0;
pub const G_FIRST: u32 = 1;
pub const G_LAST: u32 = 2;
pub const G_FIRST_ROW: u32 = 3;
pub const G_LAST_ROW: u32 = 4;
pub const G_COUNT: u32 = 5;
pub const G_SUM: u32 = 6;
pub const G_MIN: u32 = 7;
pub const G_MAX: u32 = 8;
pub const G_INDEX: u32 = 9;

/// A key, the selector or an output term of a [`GroupSpec`]: `{kind, value}`.
#[derive(Clone, Copy, Debug)]
pub struct GroupTerm(pub u32, pub u32);

impl GroupTerm {
    pub fn constant(v: u64) -> Self { Self(G_CONST, (v % 0x7800_0001) as u32) }
    /// As a key or the selector: column `c`; as an output term: `first(c)`.
    pub fn col(c: u32) -> Self { Self(1, c) }
    pub fn always() -> Self { Self(0, 1) }
    pub fn first(c: u32) -> Self { Self(G_FIRST, c) }
    pub fn last(c: u32) -> Self { Self(G_LAST, c) }
    pub fn first_row() -> Self { Self(G_FIRST_ROW, 0) }
    pub fn last_row() -> Self { Self(G_LAST_ROW, 0) }
    pub fn count() -> Self { Self(G_COUNT, 0) }
    pub fn total(c: u32) -> Self { Self(G_SUM, c) }
    pub fn least(c: u32) -> Self { Self(G_MIN, c) }
    pub fn greatest(c: u32) -> Self { Self(G_MAX, c) }
    pub fn index() -> Self { Self(G_INDEX, 0) }
}

/// Collects the keys, the selector, the pad row and the terms of a TGRP tape.  Nothing is checked here:
/// `ts_collect_check` is the judge.
pub struct GroupSpec {
    pub src_width: u32,
    pub out_width: u32,
    pub keys: Vec<GroupTerm>,
    pub when: GroupTerm,
    pub pad: Vec<u32>, // shorter than out_width: filled with zeros
    pub terms: Vec<GroupTerm>,
}

impl GroupSpec {
    pub fn new(src_width: u32, out_width: u32, keys: Vec<GroupTerm>) -> Self {
        Self { src_width, out_width, keys, when: GroupTerm::always(), pad: Vec::new(), terms: Vec::new() }
    }
    pub fn tape(&self) -> Vec<u32> {
        let mut t = vec![GROUP_MAGIC, 1, self.src_width, self.out_width, self.keys.len() as u32, self.when.0, self.when.1];
        for k in &self.keys {
            t.extend([k.0, k.1]);
        }
        let mut pad = self.pad.clone();
        pad.resize(self.out_width as usize, 0);
        t.extend(pad);
        for k in &self.terms {
            t.extend([k.0, k.1]);
        }
        t
    }
}
