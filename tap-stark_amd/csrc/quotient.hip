// Quotient evaluation (reference uni-stark/src/prover.rs:122-194 `quotient_values` with
// ProverConstraintFolder, folder.rs:11-19,60-64; selectors: p3-commit selectors_on_coset,
// SURVEY.md App. A.4; chunking: prover.rs:78-80 flatten_to_base/split_evals).
//
// One thread per row of the quotient domain 31*H_{n*qd}, addressed in the LDE's own storage order
// (bit-reversed), so that `local` is a coalesced read and `next` (natural index + qd) is a second
// coalesced read for all but one wavefront in 2^(L-6).  The constraint program is interpreted with
// wave-uniform control flow; its register file lives in LDS ([reg][thread], conflict-free) or, for
// programs with more live registers than LDS holds, in a global slab per workgroup.
// folder.rs:60-64 accumulates acc = acc*alpha + c_i; here the same value is formed as
// sum_i c_i * alpha^(K-1-i) with precomputed powers (4 base multiplications per constraint instead
// of an EF4 x EF4 product) -- exact field arithmetic, identical result.
#include <stdlib.h>

#include <algorithm>

#include "air.hpp"
#include "kernels.hpp"

namespace ts {

// ------------------------------------------------------------------ selectors
// Storage index r <-> natural index i = bitrev_L(r); x_r = shift * omega_{2^L}^i (shift = 31, the
// quotient domain of prover.rs:65-66; a rank of the sharded prover that evaluates the quotient on its
// own cosets passes their shift, sharded.cpp "local quotient").
// W is the block-twiddle table: omega_{2^L}^bitrev_L(r) = (r odd ? -1 : 1) * W[2^(L-1) + (r >> 1)].
constexpr int SEL_BATCH = 8;

struct SelConsts {
    uint32_t zh_mont[MAX_QUOTIENT_CHUNKS];  // Z_H on the qd cosets: 31^n * omega_qd^c - 1  (Montgomery)
};

__global__ void __launch_bounds__(256)
k_selectors(unsigned L, unsigned log_qd, const uint32_t* __restrict__ W, uint32_t gen_mont,
            uint32_t gn_inv_mont, SelConsts sc, uint32_t* __restrict__ is_first,
            uint32_t* __restrict__ is_last, uint32_t* __restrict__ is_transition) {
    const uint64_t total = 1ull << L;
    const uint64_t r0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * SEL_BATCH;
    if (r0 >= total) return;
    const unsigned log_n = L - log_qd;
    uint32_t d[2 * SEL_BATCH];
    uint32_t pre[2 * SEL_BATCH];
    uint32_t run = R_MOD_P;
    const int cnt = (total - r0) < (uint64_t)SEL_BATCH ? (int)(total - r0) : SEL_BATCH;
#pragma unroll
    for (int k = 0; k < SEL_BATCH; k++) {
        if (k < cnt) {
            uint64_t r = r0 + k;
            uint32_t w = L == 0 ? R_MOD_P : W[(total >> 1) + (r >> 1)];
            if (r & 1) w = neg(w);
            uint32_t x = mont_mul(gen_mont, w);
            d[2 * k] = sub(x, R_MOD_P);         // x - 1
            d[2 * k + 1] = sub(x, gn_inv_mont);  // x - omega_n^-1
        } else {
            d[2 * k] = d[2 * k + 1] = R_MOD_P;
        }
        pre[2 * k] = run;
        run = mont_mul(run, d[2 * k]);
        pre[2 * k + 1] = run;
        run = mont_mul(run, d[2 * k + 1]);
    }
    uint32_t inv = mont_inv(run);
#pragma unroll
    for (int k = SEL_BATCH - 1; k >= 0; k--) {
        uint32_t inv_last = mont_mul(inv, pre[2 * k + 1]);
        inv = mont_mul(inv, d[2 * k + 1]);
        uint32_t inv_first = mont_mul(inv, pre[2 * k]);
        inv = mont_mul(inv, d[2 * k]);
        if (k < cnt) {
            uint64_t r = r0 + k;
            // coset index c = natural i mod qd = bitrev_lqd(r >> log_n)
            uint32_t c = bitrev32((uint32_t)(r >> log_n), log_qd);
            uint32_t zh = sc.zh_mont[c];
            is_first[r] = mont_mul(zh, inv_first);
            is_last[r] = mont_mul(zh, inv_last);
            is_transition[r] = d[2 * k + 1];
        }
    }
}

// Z_H on the qd cosets of the quotient domain, canonical: shift^n * omega_qd^c - 1.  The one place the stage
// works this out: the selectors multiply by it (Montgomery), the quotient divides by it.
static void coset_vanishing(uint32_t shift, unsigned log_n, unsigned log_qd, uint32_t zh[MAX_QUOTIENT_CHUNKS]) {
    TS_REQUIRE((1u << log_qd) <= (unsigned)MAX_QUOTIENT_CHUNKS, TS_ERR_UNSUPPORTED, "quotient degree > 64 not supported");
    const uint32_t s_pow_n = pow_canon(shift, 1ull << log_n);
    const uint32_t gqd = two_adic_generator(log_qd);
    for (uint32_t c = 0; c < (1u << log_qd); c++) zh[c] = sub(mul(s_pow_n, pow_canon(gqd, c)), 1);
}

static void launch_selectors(Context& ctx, unsigned log_n, unsigned log_qd, uint32_t* is_first,
                             uint32_t* is_last, uint32_t* is_transition, uint32_t shift) {
    const unsigned L = log_n + log_qd;
    ctx.ensure_twiddles(L == 0 ? 1 : L);
    SelConsts sc;
    coset_vanishing(shift, log_n, log_qd, sc.zh_mont);
    for (uint32_t c = 0; c < (1u << log_qd); c++) sc.zh_mont[c] = to_mont(sc.zh_mont[c]);
    const uint32_t gn_inv = inv_canon(two_adic_generator(log_n));
    const uint64_t threads = (((uint64_t)1 << L) + SEL_BATCH - 1) / SEL_BATCH;
    TS_LAUNCH(ctx, k_selectors, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, L, log_qd, ctx.d_twiddle_fwd, to_mont(shift), to_mont(gn_inv), sc, is_first,
                       is_last, is_transition);
    TS_HIP(hipGetLastError());
}

// Selectors depend on the shape and the shift only: kept in the context between proofs (Context::sel_tables,
// two entries, least recently used goes).
const uint32_t* selector_table(Context& ctx, unsigned log_n, unsigned log_qd, uint32_t shift) {
    Context::SelTable* st = nullptr;
    for (auto& t : ctx.sel_tables)
        if (t.d && t.log_n == log_n && t.log_qd == log_qd && t.shift == shift) st = &t;
    if (!st) {
        st = ctx.sel_tables[0].last_use <= ctx.sel_tables[1].last_use ? &ctx.sel_tables[0] : &ctx.sel_tables[1];
        if (st->d) {
            ctx.sync();  // an earlier launch may still read the old table
            (void)hipFree(st->d);
            *st = Context::SelTable{};  // matches nothing until the new table is built
        }
        const uint64_t qn = 1ull << (log_n + log_qd);
        TS_HIP(hipMalloc((void**)&st->d, 3 * qn * sizeof(uint32_t)));
        if (ctx.poison_on) ctx.poison(st->d, 3 * qn * sizeof(uint32_t));
        launch_selectors(ctx, log_n, log_qd, st->d, st->d + qn, st->d + 2 * qn, shift);
        st->log_n = log_n;
        st->log_qd = log_qd;
        st->shift = shift;
    }
    st->last_use = ++ctx.sel_clock;
    return st->d;
}

// ------------------------------------------------------------------ interpreter
struct QuotConsts {
    uint32_t inv_zh_canonical[MAX_QUOTIENT_CHUNKS];  // 1/Z_H per coset, CANONICAL: acc(Mont) * it -> canonical
};

// Register file of the interpreter: [reg][thread], in LDS while it fits (conflict-free, the common
// case), otherwise in a global scratch slab of the workgroup ([workgroup][reg][thread]: coalesced, L2
// resident for moderate programs) with a persistent grid walking the row tiles, so that the slab is
// sized by the grid and not by the domain.  There is no cap on live registers: a program the JIT
// declines (jit.cpp: instruction budget) still runs on the device.
struct RegFilePlan {
    int nthreads;
    bool global;
    size_t lds_bytes;
    unsigned grid;
    uint32_t n_tiles;  // of nthreads rows; more than `grid` where the slab caps a persistent grid
    size_t scratch_words;
};

// a measurement knob, read on every call (tests set them in-process); unset or empty: the default
static uint64_t env_u64(const char* name, uint64_t dflt) {
    const char* e = getenv(name);
    return e && *e ? (uint64_t)atoi(e) : dflt;
}

static RegFilePlan plan_reg_file(Context& ctx, uint32_t n_regs, uint64_t rows) {
    RegFilePlan pl;
    pl.nthreads = 256;
    while (pl.nthreads > 64 && (size_t)n_regs * pl.nthreads * 4 > 48 * 1024) pl.nthreads >>= 1;
    pl.lds_bytes = (size_t)n_regs * pl.nthreads * 4;
    // LDS only while a 256-lane workgroup's file stays small (several workgroups per CU); beyond that the
    // global slab is FASTER, not just possible: 424 registers in LDS leave one wave per CU (16.6 ms on a
    // 2^18-row domain against 3.9 from the slab, profiles/r06_quotient_paths.txt).  Knobs for measurements.
    const size_t lds_max_regs = env_u64("TS_INTERP_LDS_MAX_REGS", 48);
    const unsigned waves_per_cu = (unsigned)env_u64("TS_INTERP_WAVES_PER_CU", 16);
    pl.global = n_regs > lds_max_regs || pl.lds_bytes > ctx.max_lds_per_block || getenv("TS_INTERP_GLOBAL_REGS") != nullptr;
    if (pl.global) pl.nthreads = 64;
    pl.n_tiles = (uint32_t)((rows + pl.nthreads - 1) / pl.nthreads);
    if (pl.global) {
        pl.lds_bytes = 0;
        // a few waves per SIMD hide the slab's latency (16 per CU: 1.5x over 8, 32 adds nothing); the slab stays
        // below 4 GiB of the 288 (a smaller, cache-resident slab is slower: the grid is what matters)
        uint64_t grid = std::min<uint64_t>(pl.n_tiles, (uint64_t)ctx.num_cus * waves_per_cu);
        const uint64_t slab_mb = env_u64("TS_INTERP_SLAB_MB", 4096);
        const uint64_t cap = (slab_mb << 18) / ((uint64_t)n_regs * 64);
        grid = std::max<uint64_t>(1, std::min(grid, cap));
        pl.grid = (unsigned)grid;
    } else {
        pl.grid = pl.n_tiles;
    }
    pl.scratch_words = pl.global ? (size_t)pl.grid * n_regs * 64 : 0;
    return pl;
}

// This lane's column of the register file: element `reg` at my[reg * NTHREADS].
template <int NTHREADS, bool GLOBAL_REGS>
__device__ __forceinline__ uint32_t* lane_regs(uint32_t* reg_slabs, uint32_t n_regs) {
    extern __shared__ uint32_t lds_regs[];  // [n_regs][NTHREADS] unless GLOBAL_REGS
    return GLOBAL_REGS ? reg_slabs + (size_t)blockIdx.x * n_regs * NTHREADS + threadIdx.x : lds_regs + threadIdx.x;
}

// The program on one row, for one lane: what the eight instructions (air.hpp DevOp) mean.  `Row` is what a
// kernel knows about its row: load(a, b) = the canonical word of column b of the local (a = 0) or next row,
// sel(a) = selector a (Montgomery), on_assert(value, b) = what constraint b's value is used for.
//
// Wave-uniform instruction fetch (scalar loads), one instruction ahead.  The value an instruction
// produces stays in a VGPR for the next one (`fwd`): in a post-order evaluation the next instruction
// nearly always consumes it, and reading it back from the register file would put a memory round
// trip (LDS or, worse, the slab) on every link of the dependency chain.
template <int NTHREADS, class Row>
__device__ __forceinline__ void run_program(const uint32_t* code, uint32_t n_instr,
                                            const uint32_t* consts_mont, uint32_t* my, Row& row) {
    const uint4* code4 = reinterpret_cast<const uint4*>(code);
    uint4 ins = code4[0];
    uint32_t fwd_reg = ~0u, fwd_val = 0;
    auto rd = [&](uint32_t reg) { return reg == fwd_reg ? fwd_val : my[(size_t)reg * NTHREADS]; };
    for (uint32_t pc = 0; pc < n_instr; pc++) {
        const uint4 nxt = code4[pc + 1 < n_instr ? pc + 1 : pc];
        const uint32_t op = ins.x, dst = ins.y, a = ins.z, b = ins.w;
        ins = nxt;
        uint32_t v;
        switch (op) {
            case D_LOAD: v = to_mont(row.load(a, b)); break;
            case D_CONST: v = consts_mont[a]; break;
            case D_SEL: v = row.sel(a); break;
            case D_ADD: v = add(rd(a), rd(b)); break;
            case D_SUB: v = sub(rd(a), rd(b)); break;
            case D_NEG: v = neg(rd(a)); break;
            case D_MUL: v = mont_mul(rd(a), rd(b)); break;
            default: row.on_assert(rd(a), b); continue;  // D_ASSERT
        }
        my[(size_t)dst * NTHREADS] = v;
        fwd_reg = dst;
        fwd_val = v;
    }
}

// what both kernels' rows have in common: two row pointers and three selector words
struct RowBase {
    const uint32_t* row_local;
    const uint32_t* row_next;
    uint32_t sel0, sel1, sel2;
    __device__ __forceinline__ uint32_t sel(uint32_t a) const {
        // all three read first: a choice between the members themselves is compiled to an index into the
        // struct, which then stays in memory (scratch) instead of registers
        const uint32_t s0 = sel0, s1 = sel1, s2 = sel2;
        return a == 0 ? s0 : (a == 1 ? s1 : s2);
    }
};

// The side matrices as the quotient kernels take them, by value and as their LAST argument: base and column stride
// of the LDE of side matrix i < MATS - 1 (air.hpp AirProgram::n_side).  The other entries are not read; behind
// every other argument they do not move one either, so the MATS = 1 form is instruction for instruction the
// kernel that took no such argument.
struct SideCols {
    struct {
        const uint32_t* d;
        uint64_t stride;
    } m[MAX_SIDE_MATS];
};

// A row of the quotient domain in MATS column-major LDEs of one height with bit-reversed rows: the trace's and
// MATS - 1 side matrices', each with its own base and stride.  The constraints go into sum_i c_i alpha^(K-1-i).
// One struct, and the select chain written per MATS under `if constexpr`: the form that passed the scratch, VGPR
// and static-VALU gates (profiles/quotient_one_kernel_resources.txt).
template <int MATS>
struct QuotientRow : RowBase {
    uint64_t col_stride;
    const uint32_t* alpha_pows;
    uint32_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    // side matrix 0 (D_LOAD's a = 2, 3) and 1 (a = 4, 5); set for the matrices the kernel has.  Named members and
    // not arrays: load() chooses between them at run time
    const uint32_t *s0_local, *s0_next, *s1_local, *s1_next;
    uint64_t s0_stride, s1_stride;
    __device__ __forceinline__ uint32_t load(uint32_t a, uint32_t b) const {
        if constexpr (MATS == 1) {
            return (a ? row_next : row_local)[(uint64_t)b * col_stride];
        } else if constexpr (MATS == 2) {
            // all four read first and chosen with selects, as RowBase::sel: an index into the struct would put it
            // in scratch
            const uint32_t *p0 = row_local, *p1 = row_next, *p2 = s0_local, *p3 = s0_next;
            const uint64_t t0 = col_stride, t1 = s0_stride;
            const uint32_t* lo = (a & 1) ? p1 : p0;
            const uint32_t* hi = (a & 1) ? p3 : p2;
            return ((a & 2) ? hi : lo)[(uint64_t)b * ((a & 2) ? t1 : t0)];
        } else {
            // all six read first and chosen with selects
            const uint32_t *p0 = row_local, *p1 = row_next, *p2 = s0_local, *p3 = s0_next, *p4 = s1_local,
                           *p5 = s1_next;
            const uint64_t t0 = col_stride, t1 = s0_stride, t2 = s1_stride;
            const uint32_t* m0 = (a & 1) ? p1 : p0;
            const uint32_t* m1 = (a & 1) ? p3 : p2;
            const uint32_t* m2 = (a & 1) ? p5 : p4;
            const uint32_t* m = (a & 4) ? m2 : ((a & 2) ? m1 : m0);
            return m[(uint64_t)b * ((a & 4) ? t2 : ((a & 2) ? t1 : t0))];
        }
    }
    __device__ __forceinline__ void on_assert(uint32_t c, uint32_t b) {
        const uint32_t* ap = alpha_pows + 4 * b;
        acc0 = add(acc0, mont_mul(c, ap[0]));
        acc1 = add(acc1, mont_mul(c, ap[1]));
        acc2 = add(acc2, mont_mul(c, ap[2]));
        acc3 = add(acc3, mont_mul(c, ap[3]));
    }
};

// The interpreter over the trace LDE and MATS - 1 side LDEs; a workgroup walks its row tiles.  MATS = 1 is timed as
// k_quotient, 2 as k_quotient_pre, 3 as k_quotient_pre_aux (launch_quotient).
template <int NTHREADS, bool GLOBAL_REGS, int MATS>
__global__ void __launch_bounds__(NTHREADS)
k_quotient(const uint32_t* __restrict__ code, uint32_t n_instr, uint32_t n_regs,
           const uint32_t* __restrict__ lde, uint64_t col_stride, unsigned log_n, unsigned log_qd,
           const uint32_t* __restrict__ consts_mont, const uint32_t* __restrict__ alpha_pows,
           const uint32_t* __restrict__ is_first, const uint32_t* __restrict__ is_last,
           const uint32_t* __restrict__ is_transition, QuotConsts qc, QuotOut out,
           uint32_t row_begin, uint32_t row_end, uint32_t* __restrict__ reg_slabs, uint32_t n_tiles, SideCols side) {
    const unsigned L = log_n + log_qd;
    const uint32_t total = 1u << L;
    uint32_t* my = lane_regs<NTHREADS, GLOBAL_REGS>(reg_slabs, n_regs);
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t r = row_begin + tile * NTHREADS + threadIdx.x;
        const bool active = r < row_end;
        const uint32_t rr = active ? r : row_begin;
        const uint32_t i = bitrev32(rr, L);
        const uint32_t i_next = (i + (1u << log_qd)) & (total - 1);  // prover.rs:139-140,165
        const uint32_t r_next = bitrev32(i_next, L);
        QuotientRow<MATS> row{{lde + rr, lde + r_next, is_first[rr], is_last[rr], is_transition[rr]}, col_stride,
                              alpha_pows};
        if constexpr (MATS >= 2) {
            row.s0_local = side.m[0].d + rr;
            row.s0_next = side.m[0].d + r_next;
            row.s0_stride = side.m[0].stride;
        }
        if constexpr (MATS == 3) {
            row.s1_local = side.m[1].d + rr;
            row.s1_next = side.m[1].d + r_next;
            row.s1_stride = side.m[1].stride;
        }
        run_program<NTHREADS>(code, n_instr, consts_mont, my, row);
        if (!active) continue;
        // quotient(x) = constraints(x) / Z_H(x)  (prover.rs:183); flatten + split (prover.rs:78-80):
        // natural row i -> chunk i % qd, position i / qd; stored bit-reversed = r & (n-1)
        const uint32_t c = bitrev32(r >> log_n, log_qd);
        const uint32_t iz = qc.inv_zh_canonical[c];
        const uint64_t n = 1ull << log_n;
        uint32_t* o = out.chunk[c] + (r & (n - 1));
        o[0] = mont_mul(row.acc0, iz);
        o[n] = mont_mul(row.acc1, iz);
        o[2 * n] = mont_mul(row.acc2, iz);
        o[3 * n] = mont_mul(row.acc3, iz);
    }
}

// The four register-file forms of an interpreter kernel for one MATS (one function type for every MATS), and the
// name of its timer.  A launcher keeps one table per kernel family, indexed by the number of side matrices.
template <class F>
struct InterpKernels {
    const char* name;
    F global64, lds256, lds128, lds64;
};
#define TS_INTERP_KERNELS(name, K, MATS) \
    { name, K<64, true, MATS>, K<256, false, MATS>, K<128, false, MATS>, K<64, false, MATS> }

// Launches the instantiation that the register-file plan for `rows` rows asks for; `args` are the kernel's own,
// between the program and the register file, and `side` (the side matrices, by value) is its last.
template <class F, class Side, class... Args>
static void launch_interpreter(Context& ctx, const InterpKernels<F>& k, const AirProgram& air, uint64_t rows,
                               const Side& side, Args... args) {
    TS_REQUIRE(air.d_code != nullptr, TS_ERR_INVALID, "air program not uploaded");
    const RegFilePlan pl = plan_reg_file(ctx, air.n_regs, rows);
    DevBuf<uint32_t> slabs;
    if (pl.global) slabs = DevBuf<uint32_t>(&ctx, pl.scratch_words);
    const F kernel = pl.global ? k.global64 : pl.nthreads == 256 ? k.lds256 : pl.nthreads == 128 ? k.lds128 : k.lds64;
    // above 64 KiB the dynamic LDS size has to be granted per function (gfx950: 160 KiB per workgroup)
    if (pl.lds_bytes > 48 * 1024)
        TS_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
    TS_LAUNCH_NAMED(ctx, k.name, kernel, dim3(pl.grid), dim3(pl.nthreads), pl.lds_bytes, air.d_code,
                    (uint32_t)(air.code.size() / 4), air.n_regs, args..., slabs.p, pl.n_tiles, side);
    TS_HIP(hipGetLastError());
}

void launch_quotient(Context& ctx, const AirProgram& air, const ColMat& trace_lde, unsigned log_n,
                     unsigned log_qd, const uint32_t* d_consts_mont, const uint32_t* d_alpha_pows_mont,
                     const QuotOut& out, uint64_t row_begin, uint64_t row_end, uint32_t shift,
                     const SideLdes& side) {
    TS_REQUIRE(air.d_code != nullptr, TS_ERR_INVALID, "air program not uploaded");
    // a program with preprocessed or aux loads never runs without the matrices they read, and they cover the rows
    TS_REQUIRE(side.n == air.n_side(), TS_ERR_INVARIANT,
               "quotient: the preprocessed and aux LDEs given and the AIR's preprocessed and aux widths disagree");
    SideCols cols{};
    for (uint32_t i = 0; i < side.n; i++) {
        const ColMat* m = side.m[i];
        TS_REQUIRE(m && m->d && m->width == air.side_width(i) && m->height == trace_lde.height &&
                       m->col_stride >= m->height,
                   TS_ERR_INVALID, air.side_is_aux(i) ? "quotient: aux LDE shape" : "quotient: preprocessed LDE shape");
        cols.m[i].d = m->d;
        cols.m[i].stride = m->col_stride;
    }
    TS_REQUIRE(log_n + log_qd <= 31, TS_ERR_INVALID, "quotient domain too large");
    const uint64_t qn = 1ull << (log_n + log_qd);
    if (row_end == 0) row_end = qn;
    TS_REQUIRE(row_begin < row_end && row_end <= qn, TS_ERR_INVALID, "quotient: row range");
    // the selectors and 1/Z_H of this launch's own (shape, shift): they cannot disagree
    const uint32_t* is_first = selector_table(ctx, log_n, log_qd, shift);
    const uint32_t* is_last = is_first + qn;
    const uint32_t* is_transition = is_first + 2 * qn;
    QuotConsts qc;
    coset_vanishing(shift, log_n, log_qd, qc.inv_zh_canonical);
    for (uint32_t c = 0; c < (1u << log_qd); c++) qc.inv_zh_canonical[c] = inv_canon(qc.inv_zh_canonical[c]);
    const uint64_t total = row_end - row_begin;  // rows to do
    uint32_t rb = (uint32_t)row_begin, re = (uint32_t)row_end;
    const JitKernelSet* ks = air.jit.load();  // once per launch: published whole (air.hpp KernelSetRef)
    const uint32_t* lde_p = trace_lde.d;
    uint64_t stride = trace_lde.col_stride;
    QuotOut qo = out;
    if (ks) {
        // The specialised kernels (jit.cpp emit_head): the thirteen arguments every one takes, then (pointer,
        // stride) per side matrix, then the slab pair of a segmented kernel.  rb, re: the rows of one launch
        uint32_t* slab_p = nullptr;
        uint32_t slab_rows = 0;
        std::vector<void*> args = {&lde_p, &stride, &log_n, &log_qd, &d_consts_mont, &d_alpha_pows_mont, &is_first,
                                   &is_last, &is_transition, &qc, &qo, &rb, &re};
        for (uint32_t i = 0; i < side.n; i++) {
            args.push_back(&cols.m[i].d);
            args.push_back(&cols.m[i].stride);
        }
        if (!ks->seg) {
            // specialised straight-line kernel; same arguments, same results
            KernelTimer kt(&ctx, "k_quotient_jit");
            TS_HIP(hipModuleLaunchKernel((hipFunction_t)ks->fns[0], (unsigned)((total + 255) / 256), 1, 1,
                                         256, 1, 1, 0, ctx.stream, args.data(), nullptr));
            return;
        }
        // segmented kernels (jit.cpp jit_segment_sources): per tile of rows, segments 0..K-1 in stream order,
        // values crossing a cut in a slab of [slab_width + 8][tile_rows] words from the context's pool
        const uint64_t width = (uint64_t)ks->seg->slab_width + SEG_ACC_SLOTS;
        const uint64_t slab_mb = env_u64("TS_SEG_SLAB_MB", 4096);
        uint64_t tile = std::max<uint64_t>(256, ((slab_mb << 18) / width) & ~(uint64_t)255);
        tile = std::min<uint64_t>(tile, (total + 255) & ~(uint64_t)255);
        DevBuf<uint32_t> slab(&ctx, (size_t)(width * tile));
        slab_p = slab.p;
        slab_rows = (uint32_t)tile;
        args.push_back(&slab_p);
        args.push_back(&slab_rows);
        KernelTimer kt(&ctx, "k_quotient_seg");
        for (uint64_t t0 = row_begin; t0 < row_end; t0 += tile) {
            rb = (uint32_t)t0;
            re = (uint32_t)std::min<uint64_t>(row_end, t0 + tile);
            const unsigned grid = (unsigned)((re - rb + 255) / 256);
            for (void* fn : ks->fns)
                TS_HIP(hipModuleLaunchKernel((hipFunction_t)fn, grid, 1, 1, 256, 1, 1, 0, ctx.stream, args.data(),
                                             nullptr));
        }
        return;
    }
    static const InterpKernels<decltype(&k_quotient<64, true, 1>)> kernels[MAX_SIDE_MATS + 1] = {
        TS_INTERP_KERNELS("k_quotient", k_quotient, 1), TS_INTERP_KERNELS("k_quotient_pre", k_quotient, 2),
        TS_INTERP_KERNELS("k_quotient_pre_aux", k_quotient, 3)};
    launch_interpreter(ctx, kernels[side.n], air, total, cols, lde_p, stride, log_n, log_qd, d_consts_mont,
                       d_alpha_pows_mont, is_first, is_last, is_transition, qc, qo, rb, re);
}

// ------------------------------------------------------------------ chunk mix (sharded local quotient)
// One thread per (row, base column j < 4) of the slab: v[c'] = chunk c' column j at this row, then
// chunk c <- sum_c' mix[c][c'] v[c'].  Canonical values x Montgomery constants -> canonical.
template <int QD>
__global__ void __launch_bounds__(256)
k_chunk_mix(uint32_t* const* __restrict__ chunks, uint64_t rows, uint64_t col_stride,
            const uint32_t* __restrict__ mix) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 4 * rows) return;
    const uint64_t row = t % rows, j = t / rows;
    uint32_t v[QD];
#pragma unroll
    for (int c = 0; c < QD; c++) v[c] = chunks[c][j * col_stride + row];
#pragma unroll
    for (int c = 0; c < QD; c++) {
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < QD; k++) acc = add(acc, mont_mul(v[k], mix[c * QD + k]));
        chunks[c][j * col_stride + row] = acc;
    }
}

void launch_chunk_mix(Context& ctx, uint32_t* const* d_chunk_ptrs, uint32_t qd, uint64_t rows, uint64_t col_stride,
                      const uint32_t* d_mix_mont) {
    const dim3 grid((unsigned)((4 * rows + 255) / 256));
#define TS_MIX(Q) TS_LAUNCH(ctx, k_chunk_mix<Q>, grid, dim3(256), 0, d_chunk_ptrs, rows, col_stride, d_mix_mont)
    switch (qd) {
        case 2: TS_MIX(2); break;
        case 4: TS_MIX(4); break;
        case 8: TS_MIX(8); break;
        case 16: TS_MIX(16); break;
        case 32: TS_MIX(32); break;
        case 64: TS_MIX(64); break;
        default: TS_REQUIRE(false, TS_ERR_INVALID, "chunk mix: quotient degree must be 2 .. 64");
    }
#undef TS_MIX
    TS_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ check_constraints
// reference uni-stark/src/check_constraints.rs:11-39 (debug builds of prove(), prover.rs:40-41):
// every constraint must vanish on every row of the trace itself, with is_first_row = (i == 0),
// is_last_row = (i == h-1), is_transition = (i != h-1) and the next row wrapping around.
// One thread per row of the row-major trace; the first violation (row * 2^16 + constraint index,
// smallest wins) is left in *violation.
// A row of the row-major trace and of the MATS - 1 row-major side matrices of its height beside it (D_LOAD's
// a = 2, 3 and a = 4, 5); the first constraint that does not vanish goes into `bad`.  As QuotientRow: one struct,
// the select chain per MATS.
template <int MATS>
struct CheckRow : RowBase {
    uint64_t i;  // this row
    unsigned long long& bad;
    const uint32_t *s0_local, *s0_next, *s1_local, *s1_next;
    __device__ __forceinline__ uint32_t load(uint32_t a, uint32_t b) const {
        if constexpr (MATS == 1) {
            return (a ? row_next : row_local)[b];
        } else if constexpr (MATS == 2) {
            const uint32_t *p0 = row_local, *p1 = row_next, *p2 = s0_local, *p3 = s0_next;
            const uint32_t* lo = (a & 1) ? p1 : p0;
            const uint32_t* hi = (a & 1) ? p3 : p2;
            return ((a & 2) ? hi : lo)[b];
        } else {
            const uint32_t *p0 = row_local, *p1 = row_next, *p2 = s0_local, *p3 = s0_next, *p4 = s1_local,
                           *p5 = s1_next;
            const uint32_t* m0 = (a & 1) ? p1 : p0;
            const uint32_t* m1 = (a & 1) ? p3 : p2;
            const uint32_t* m2 = (a & 1) ? p5 : p4;
            return ((a & 4) ? m2 : ((a & 2) ? m1 : m0))[b];
        }
    }
    __device__ __forceinline__ void on_assert(uint32_t c, uint32_t b) {
        if (c != 0 && bad == ~0ull) bad = i * 65536ull + b;
    }
};

// MATS = 1 is timed as k_check_constraints, 2 as k_check_constraints_pre, 3 as k_check_pre_aux
template <int NTHREADS, bool GLOBAL_REGS, int MATS>
__global__ void __launch_bounds__(NTHREADS)
k_check_constraints(const uint32_t* __restrict__ code, uint32_t n_instr, uint32_t n_regs,
                    const uint32_t* __restrict__ trace, uint32_t width, uint64_t n,
                    const uint32_t* __restrict__ consts_mont, unsigned long long* __restrict__ violation,
                    uint32_t* __restrict__ reg_slabs, uint32_t n_tiles, SideRows side) {
    uint32_t* my = lane_regs<NTHREADS, GLOBAL_REGS>(reg_slabs, n_regs);
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = (uint64_t)tile * NTHREADS + threadIdx.x;
        const bool active = i < n;
        const uint64_t ii = active ? i : 0, nx = (ii + 1) % n;
        unsigned long long bad = ~0ull;
        CheckRow<MATS> row{{trace + ii * width, trace + nx * width, ii == 0 ? R_MOD_P : 0u, ii == n - 1 ? R_MOD_P : 0u,
                            ii != n - 1 ? R_MOD_P : 0u}, ii, bad};
        if constexpr (MATS >= 2) {
            row.s0_local = side.d[0] + ii * side.width[0];
            row.s0_next = side.d[0] + nx * side.width[0];
        }
        if constexpr (MATS == 3) {
            row.s1_local = side.d[1] + ii * side.width[1];
            row.s1_next = side.d[1] + nx * side.width[1];
        }
        run_program<NTHREADS>(code, n_instr, consts_mont, my, row);
        if (active && bad != ~0ull) atomicMin(violation, bad);
    }
}

void launch_check_constraints(Context& ctx, const AirProgram& air, const uint32_t* trace_row_major,
                              uint64_t n, const uint32_t* d_consts_mont,
                              unsigned long long* d_violation, const SideRows& side) {
    TS_REQUIRE(side.n == air.n_side(), TS_ERR_INVARIANT,
               "check_constraints: the preprocessed and aux matrices given and the AIR's preprocessed and aux widths "
               "disagree");
    for (uint32_t i = 0; i < side.n; i++)
        TS_REQUIRE(side.d[i] && side.width[i] == air.side_width(i), TS_ERR_INVALID,
                   air.side_is_aux(i) ? "check_constraints: aux matrix shape"
                                      : "check_constraints: preprocessed matrix shape");
    // the report is row * 2^16 + constraint index (the oracle's and stark.py's format)
    TS_REQUIRE(air.n_constraints <= 65536, TS_ERR_UNSUPPORTED, "check_constraints: more than 65536 constraints");
    static const InterpKernels<decltype(&k_check_constraints<64, true, 1>)> kernels[MAX_SIDE_MATS + 1] = {
        TS_INTERP_KERNELS("k_check_constraints", k_check_constraints, 1),
        TS_INTERP_KERNELS("k_check_constraints_pre", k_check_constraints, 2),
        TS_INTERP_KERNELS("k_check_pre_aux", k_check_constraints, 3)};
    launch_interpreter(ctx, kernels[side.n], air, n, side, trace_row_major, air.width, n, d_consts_mont, d_violation);
}
#undef TS_INTERP_KERNELS

}  // namespace ts
