// LogUp multiplicity column, built in HBM from the still-resident main trace: for every table row the (field)
// sum of the weights of the lookups whose tuple equals the row's tuple, stored in (or negated into) one main
// column.  Table rows with equal tuples form a class; the class's lowest row receives the sum, the others 0.
//
// Three plain launches and one small copy back; no grid barrier, no cooperative launch, no workgroup waits for
// another; every loop is bounded by `capacity` (the power of two >= 2 n), MULT_MAX_LOOKUPS or the wave size:
//   k_mult_insert  one table row per lane: hash the tuple, probe linearly; atomicCAS(slot, EMPTY, row) either
//                  inserts the row or returns the row that holds the slot; that row's tuple is read from the
//                  matrix (read-only for the launch) and compared: equal -> atomicMin(slot, row), else next slot.
//                  A slot's content is only ever taken from the value an atomic returned (a plain load of a word
//                  another XCD has just written can be stale); a slot never goes back to empty and never changes
//                  class, so each class ends in exactly one slot, holding its lowest row, whatever the order.
//   k_mult_count   one trace row per lane, looping over the lookups: weight 0 is skipped; otherwise probe with
//                  plain loads (the slots are final: an earlier launch wrote them); empty -> a miss (64-bit
//                  atomicAdd on the count, atomicMin on r * L + l); equal tuple -> no-return 64-bit
//                  atomicAdd(&sums[rep], w), w canonical.  Integer adds commute: the sums do not depend on order.
//                  They cannot wrap: 2^27 rows * 16 lookups * p < 2^62.
//   k_mult_write   one table row per lane: sums[t] % p, or p minus it, into trace[t][out_column].
// logup_multiplicities_bus (the lookups are rows of OTHER traces) launches k_mult_count_bus once per looker between
// the same insert and write: k_mult_count with the looker's rows apart from the table's.
// The hash (logup_hash.hpp, shared with bus_check.hip) changes no output; TS_LOGUP_HASH_BITS (0 .. 32, read on every call) masks
// it to that many low bits before it is reduced to a slot: a test knob that makes probe chains as long as the table.
// Contention: a wave whose hits all go to ONE representative (padding rows, a selector-heavy trace) sums their weights
// with shuffles and issues one add; every other wave issues one add per hit (DESIGN.md has the measurement: a ballot
// loop over every distinct destination of a wave lost on the byte-valued and the uniform inputs and was not kept).
#include <stdlib.h>
#include <string.h>

#include <string>

#include "logup_hash.hpp"

namespace ts {

constexpr int MULT_THREADS = 256;
constexpr uint32_t MULT_EMPTY = 0xFFFFFFFFu;

struct MultDev {
    uint32_t n_values, n_lookups, width, table_width, out_column, negate, hash_mask, cap_mask;
    uint32_t t_kind[LOGUP_MAX_VALUES], t_val[LOGUP_MAX_VALUES];
    uint32_t w_kind[LOGUP_MULT_MAX_LOOKUPS], w_val[LOGUP_MULT_MAX_LOOKUPS];
    uint32_t l_kind[LOGUP_MULT_MAX_LOOKUPS][LOGUP_MAX_VALUES], l_val[LOGUP_MULT_MAX_LOOKUPS][LOGUP_MAX_VALUES];
};

// what the one copy back holds (32 bytes)
struct MultBack {
    unsigned long long n_missing, first_missing;
    uint32_t error, pad[3];
};

// the table's tuple on row t
__device__ __forceinline__ MultTuple mult_table_tuple(const MultDev& s, const uint32_t* __restrict__ trace,
                                                      const uint32_t* __restrict__ pre, uint64_t t) {
    const uint32_t* row = trace + t * s.width;
    const uint32_t* pre_row = pre + t * s.table_width;
    MultTuple out;
#pragma unroll
    for (int q = 0; q < (int)LOGUP_MAX_VALUES; q++)
        out.v[q] = q < (int)s.n_values ? mult_term(s.t_kind[q], s.t_val[q], row, pre_row) : 0;
    return out;
}

__global__ void __launch_bounds__(MULT_THREADS)
k_mult_insert(const MultDev s, const uint32_t* __restrict__ trace, const uint32_t* __restrict__ pre, uint64_t n,
              uint32_t* __restrict__ slots, MultBack* __restrict__ back) {
    const uint64_t t = (uint64_t)blockIdx.x * MULT_THREADS + threadIdx.x;
    if (t >= n) return;
    const MultTuple mine = mult_table_tuple(s, trace, pre, t);
    const uint32_t h = mult_hash(mine, s.n_values) & s.hash_mask;
    for (uint64_t step = 0; step <= s.cap_mask; step++) {
        uint32_t* slot = slots + ((h + (uint32_t)step) & s.cap_mask);
        const uint32_t old = atomicCAS(slot, MULT_EMPTY, (uint32_t)t);
        if (old == MULT_EMPTY) return;
        if (mult_equal(mult_table_tuple(s, trace, pre, old), mine)) {
            atomicMin(slot, (uint32_t)t);
            return;
        }
    }
    atomicOr(&back->error, 1u);  // every slot holds another class: impossible at load <= 1/2
}

__device__ __forceinline__ unsigned long long mult_wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// the representative of `mine`'s class among the rows of `table` (plain loads: the slots are final), or MULT_EMPTY
__device__ __forceinline__ uint32_t mult_probe(const MultDev& s, const uint32_t* __restrict__ table,
                                               const uint32_t* __restrict__ pre, const uint32_t* __restrict__ slots,
                                               const MultTuple& mine) {
    const uint32_t h = mult_hash(mine, s.n_values) & s.hash_mask;
    for (uint64_t step = 0; step <= s.cap_mask; step++) {
        const uint32_t at = slots[(h + (uint32_t)step) & s.cap_mask];
        if (at == MULT_EMPTY) break;
        if (mult_equal(mult_table_tuple(s, table, pre, at), mine)) return at;
    }
    return MULT_EMPTY;  // (a full table of other classes is a miss too)
}

// sums[rep] += w on the lanes with `hit`; EVERY lane of the wave calls it (ballots), dead lanes with hit = false
__device__ __forceinline__ void mult_add_hits(bool hit, uint32_t rep, uint32_t w,
                                              unsigned long long* __restrict__ sums) {
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long hits = __ballot(hit);
    if (hits == 0) return;  // (wave-uniform)
    const int leader = __ffsll((long long)hits) - 1;
    const uint32_t dest = (uint32_t)__shfl((int)rep, leader, 64);
    if ((hits & (hits - 1)) && __ballot(hit && rep == dest) == hits) {
        // several hits, one representative: one add for the wave
        const unsigned long long sum = mult_wave_sum(hit ? (unsigned long long)w : 0ull);
        if (lane == (unsigned)leader) atomicAdd(sums + dest, sum);
    } else if (hit) {
        atomicAdd(sums + rep, (unsigned long long)w);
    }
}

__global__ void __launch_bounds__(MULT_THREADS)
k_mult_count(const MultDev s, const uint32_t* __restrict__ trace, const uint32_t* __restrict__ pre, uint64_t n,
             const uint32_t* __restrict__ slots, unsigned long long* __restrict__ sums, MultBack* __restrict__ back) {
    const uint64_t r = (uint64_t)blockIdx.x * MULT_THREADS + threadIdx.x;
    const bool live = r < n;  // (no early return: every lane of the wave takes part in the ballots of mult_add_hits)
    const uint32_t* row = trace + (live ? r : 0) * s.width;
    const uint32_t* pre_row = pre + (live ? r : 0) * s.table_width;
    for (uint32_t l = 0; l < s.n_lookups; l++) {
        uint32_t w = live ? mult_term(s.w_kind[l], s.w_val[l], row, pre_row) : 0;
        w = w >= P ? w - P : w;  // canonical, whatever word the column held (2^32 < 3 p)
        w = w >= P ? w - P : w;
        uint32_t rep = MULT_EMPTY;
        if (w != 0) {
            MultTuple mine;
#pragma unroll
            for (int q = 0; q < (int)LOGUP_MAX_VALUES; q++)
                mine.v[q] = q < (int)s.n_values ? mult_term(s.l_kind[l][q], s.l_val[l][q], row, pre_row) : 0;
            rep = mult_probe(s, trace, pre, slots, mine);
            if (rep == MULT_EMPTY) {
                atomicAdd(&back->n_missing, 1ull);
                atomicMin(&back->first_missing, (unsigned long long)r * s.n_lookups + l);
            }
        }
        mult_add_hits(rep != MULT_EMPTY, rep, w, sums);
    }
}

// ---- the lookups live in OTHER traces (logup_multiplicities_bus): one launch per looker.  k_mult_count with the
// looker's rows and terms apart from the table's: the lookup tuple and its weight are read from the looker's row,
// the probe compares against the TABLE's rows (`s`, `table`, and `pre` for its kind-2 terms: the table trace again
// where there are none).  A miss is keyed (looker, row, lookup).
struct MultLookerDev {
    uint32_t n_lookups, width, index, pad;
    uint32_t w_kind[LOGUP_MULT_MAX_LOOKUPS], w_val[LOGUP_MULT_MAX_LOOKUPS];
    uint32_t l_kind[LOGUP_MULT_MAX_LOOKUPS][LOGUP_MAX_VALUES], l_val[LOGUP_MULT_MAX_LOOKUPS][LOGUP_MAX_VALUES];
};

__global__ void __launch_bounds__(MULT_THREADS)
k_mult_count_bus(const MultDev s, const MultLookerDev k, const uint32_t* __restrict__ table,
                 const uint32_t* __restrict__ pre, const uint32_t* __restrict__ looker, uint64_t n_looker, const uint32_t* __restrict__ slots,
                 unsigned long long* __restrict__ sums, MultBack* __restrict__ back) {
    const uint64_t r = (uint64_t)blockIdx.x * MULT_THREADS + threadIdx.x;
    const bool live = r < n_looker;  // (no early return: the dead lanes of a short looker take part in the ballots)
    const uint32_t* row = looker + (live ? r : 0) * k.width;
    for (uint32_t l = 0; l < k.n_lookups; l++) {
        uint32_t w = live ? mult_term(k.w_kind[l], k.w_val[l], row, row) : 0;
        w = w >= P ? w - P : w;  // canonical, whatever word the column held (2^32 < 3 p)
        w = w >= P ? w - P : w;
        uint32_t rep = MULT_EMPTY;
        if (w != 0) {
            MultTuple mine;
#pragma unroll
            for (int q = 0; q < (int)LOGUP_MAX_VALUES; q++)
                mine.v[q] = q < (int)s.n_values ? mult_term(k.l_kind[l][q], k.l_val[l][q], row, row) : 0;
            rep = mult_probe(s, table, pre, slots, mine);
            if (rep == MULT_EMPTY) {
                atomicAdd(&back->n_missing, 1ull);
                atomicMin(&back->first_missing,
                          ((unsigned long long)k.index << 32) | (r * LOGUP_MULT_MAX_LOOKUPS + l));
            }
        }
        mult_add_hits(rep != MULT_EMPTY, rep, w, sums);
    }
}

__global__ void __launch_bounds__(MULT_THREADS)
k_mult_write(uint32_t width, uint32_t out_column, uint32_t negate, uint64_t n,
             const unsigned long long* __restrict__ sums, uint32_t* __restrict__ trace) {
    const uint64_t t = (uint64_t)blockIdx.x * MULT_THREADS + threadIdx.x;
    if (t >= n) return;
    const uint32_t v = (uint32_t)(sums[t] % P);
    trace[t * width + out_column] = negate && v ? P - v : v;
}

LogupMultResult logup_multiplicities(Context& ctx, const LogupMultSpec& spec, DeviceMatrix& trace,
                                     const DeviceMatrix* table) {
    StageTimer timer(&ctx, "logup multiplicities");
    MultDev s;
    memset(&s, 0, sizeof s);
    const size_t nv = spec.table.size(), nl = spec.weights.size();
    TS_REQUIRE(nv >= 1 && nv <= LOGUP_MAX_VALUES, TS_ERR_INVALID, "logup multiplicities: between 1 and 8 values");
    TS_REQUIRE(nl >= 1 && nl <= LOGUP_MULT_MAX_LOOKUPS && spec.lookups.size() == nl * nv, TS_ERR_INVALID,
               "logup multiplicities: between 1 and 16 lookups of n_values terms each");
    TS_REQUIRE(spec.negate <= 1, TS_ERR_INVALID, "logup multiplicities: negate must be 0 or 1");
    TS_REQUIRE(trace.buf.p && trace.layout == DeviceMatrix::ROW_MAJOR && trace.buf.ctx == &ctx, TS_ERR_INVALID,
               "logup multiplicities: needs a row-major, unconsumed trace made on this context");
    TS_REQUIRE(trace.height >= 1 && trace.height <= (1ull << 27) && trace.width >= 1, TS_ERR_INVALID,
               "logup multiplicities: trace height must be in [1, 2^27]");
    TS_REQUIRE(spec.out_column < trace.width, TS_ERR_INVALID, "logup multiplicities: out_column outside the trace");
    s.width = trace.width;
    if (table) {
        TS_REQUIRE(table->buf.p && table->layout == DeviceMatrix::ROW_MAJOR && table->buf.ctx == &ctx, TS_ERR_INVALID,
                   "logup multiplicities: the preprocessed table must be row-major, unconsumed and made on this context");
        TS_REQUIRE(table->height == trace.height && table->width >= 1, TS_ERR_INVALID,
                   "logup multiplicities: the preprocessed table must have the trace's height");
        s.table_width = table->width;
    }
    auto term = [&](const LogupTerm& tm, uint32_t& kind, uint32_t& val) {
        TS_REQUIRE(tm.kind <= 2, TS_ERR_INVALID,
                   "logup multiplicities: term kind must be 0 (constant), 1 (column) or 2 (preprocessed column)");
        TS_REQUIRE(tm.kind != 2 || table, TS_ERR_INVALID,
                   "logup multiplicities: a preprocessed-column term without a preprocessed table");
        TS_REQUIRE(tm.kind == 2 ? tm.value < s.table_width : tm.kind ? tm.value < trace.width : tm.value < P, TS_ERR_INVALID,
                   "logup multiplicities: a column outside the trace or the preprocessed table, or a non-canonical constant");
        TS_REQUIRE(tm.kind != 1 || tm.value != spec.out_column, TS_ERR_INVALID,
                   "logup multiplicities: out_column is among the main columns the spec reads");
        kind = tm.kind;
        val = tm.value;
    };
    for (size_t q = 0; q < nv; q++) term(spec.table[q], s.t_kind[q], s.t_val[q]);
    for (size_t l = 0; l < nl; l++) {
        term(spec.weights[l], s.w_kind[l], s.w_val[l]);
        for (size_t q = 0; q < nv; q++) term(spec.lookups[l * nv + q], s.l_kind[l][q], s.l_val[l][q]);
    }
    const long bits = mult_knob("TS_LOGUP_HASH_BITS", 0, 32, 32);
    s.n_values = (uint32_t)nv;
    s.n_lookups = (uint32_t)nl;
    s.out_column = spec.out_column;
    s.negate = spec.negate;
    s.hash_mask = bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1;

    const uint64_t n = trace.height;
    uint64_t capacity = 2;
    while (capacity < 2 * n) capacity <<= 1;  // <= 2^28
    s.cap_mask = (uint32_t)(capacity - 1);
    DevBuf<uint32_t> slots(&ctx, capacity);
    DevBuf<unsigned long long> sums(&ctx, n);
    DevBuf<MultBack> back(&ctx, 1);
    TS_HIP(hipMemsetAsync(slots.p, 0xff, capacity * sizeof(uint32_t), ctx.stream));
    TS_HIP(hipMemsetAsync(sums.p, 0, n * sizeof(unsigned long long), ctx.stream));
    TS_HIP(hipMemsetAsync(back.p, 0, sizeof(MultBack), ctx.stream));
    TS_HIP(hipMemsetAsync(&back.p->first_missing, 0xff, sizeof(unsigned long long), ctx.stream));
    const uint32_t* pre = table ? table->buf.p : trace.buf.p;  // (no kind-2 term gets here without a table)
    const dim3 grid((unsigned)((n + MULT_THREADS - 1) / MULT_THREADS)), block(MULT_THREADS);
    TS_LAUNCH(ctx, k_mult_insert, grid, block, 0, s, (const uint32_t*)trace.buf.p, pre, n, slots.p, back.p);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_mult_count, grid, block, 0, s, (const uint32_t*)trace.buf.p, pre, n, (const uint32_t*)slots.p, sums.p,
              back.p);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_mult_write, grid, block, 0, s.width, s.out_column, s.negate, n,
              (const unsigned long long*)sums.p, trace.buf.p);
    TS_HIP(hipGetLastError());
    MultBack host;
    d2h_sync(ctx, &host, back.p, sizeof host);
    if (host.error)
        throw Error(TS_ERR_INVARIANT, "logup multiplicities: internal error: the slot table was full");
    return LogupMultResult{host.n_missing, host.first_missing};
}

// ------------------------------------------------------------------ the table in one trace, the lookups in others
LogupMultBusResult logup_multiplicities_bus(Context& ctx, const LogupMultBusSpec& spec, DeviceMatrix& trace,
                                            const std::vector<const DeviceMatrix*>& lookers, const DeviceMatrix* table_pre,
                                            bool takes_pre) {
    StageTimer timer(&ctx, "logup multiplicities");
    MultDev s;
    memset(&s, 0, sizeof s);
    const size_t nv = spec.table.size(), nk = spec.lookers.size();
    TS_REQUIRE(nv >= 1 && nv <= LOGUP_MAX_VALUES, TS_ERR_INVALID, "logup multiplicities: between 1 and 8 values");
    TS_REQUIRE(nk >= 1 && nk <= LOGUP_MULT_MAX_LOOKERS && lookers.size() == nk, TS_ERR_INVALID,
               "logup multiplicities: between 1 and 16 lookers, one trace each");
    TS_REQUIRE(spec.negate <= 1, TS_ERR_INVALID, "logup multiplicities: negate must be 0 or 1");
    auto matrix = [&](const DeviceMatrix* m, const char* what) {
        TS_REQUIRE(m && m->buf.p && m->layout == DeviceMatrix::ROW_MAJOR && m->buf.ctx == &ctx, TS_ERR_INVALID,
                   std::string("logup multiplicities: ") + what + " must be a row-major, unconsumed matrix made on this context");
        TS_REQUIRE(m->height >= 1 && m->height <= (1ull << 27) && m->width >= 1, TS_ERR_INVALID,
                   std::string("logup multiplicities: the height of ") + what + " must be in [1, 2^27]");
    };
    matrix(&trace, "the table trace");
    TS_REQUIRE(spec.out_column < trace.width, TS_ERR_INVALID, "logup multiplicities: out_column outside the trace");
    s.width = trace.width;
    if (table_pre) {
        TS_REQUIRE(takes_pre, TS_ERR_INVALID, "logup multiplicities: this call takes no preprocessed table");
        matrix(table_pre, "the preprocessed table");
        TS_REQUIRE(table_pre->height == trace.height, TS_ERR_INVALID,
                   "logup multiplicities: the preprocessed table must have the table trace's height");
        s.table_width = table_pre->width;
    }
    // a term over matrix `m`; the table trace's out_column is read by no term of any side.  Kind 2 (the table's
    // terms of logup_multiplicities_bus_pre only) reads the preprocessed table.
    auto term = [&](const LogupTerm& tm, const DeviceMatrix& m, uint32_t& kind, uint32_t& val, bool table_side = false) {
        const bool pre_ok = takes_pre && table_side;
        TS_REQUIRE(tm.kind <= (pre_ok ? 2u : 1u), TS_ERR_INVALID,
                   pre_ok ? "logup multiplicities: term kind must be 0 (constant), 1 (column) or 2 (preprocessed column)"
                          : "logup multiplicities: term kind must be 0 (constant) or 1 (column)");
        TS_REQUIRE(tm.kind != 2 || table_pre, TS_ERR_INVALID,
                   "logup multiplicities: a preprocessed-column term without a preprocessed table");
        TS_REQUIRE(tm.kind == 2 ? tm.value < s.table_width : tm.kind ? tm.value < m.width : tm.value < P, TS_ERR_INVALID,
                   "logup multiplicities: a column outside its trace, or a non-canonical constant");
        TS_REQUIRE(tm.kind != 1 || m.buf.p != trace.buf.p || tm.value != spec.out_column, TS_ERR_INVALID,
                   "logup multiplicities: out_column is among the table-trace columns the spec reads");
        kind = tm.kind;
        val = tm.value;
    };
    for (size_t q = 0; q < nv; q++) term(spec.table[q], trace, s.t_kind[q], s.t_val[q], true);
    std::vector<MultLookerDev> lk(nk);
    for (size_t k = 0; k < nk; k++) {
        const LogupMultLooker& in = spec.lookers[k];
        matrix(lookers[k], "a looker");
        const size_t nl = in.weights.size();
        TS_REQUIRE(nl >= 1 && nl <= LOGUP_MULT_MAX_LOOKUPS && in.lookups.size() == nl * nv, TS_ERR_INVALID,
                   "logup multiplicities: between 1 and 16 lookups of n_values terms each per looker");
        MultLookerDev& d = lk[k];
        memset(&d, 0, sizeof d);
        d.n_lookups = (uint32_t)nl;
        d.width = lookers[k]->width;
        d.index = (uint32_t)k;
        for (size_t l = 0; l < nl; l++) {
            term(in.weights[l], *lookers[k], d.w_kind[l], d.w_val[l]);
            for (size_t q = 0; q < nv; q++) term(in.lookups[l * nv + q], *lookers[k], d.l_kind[l][q], d.l_val[l][q]);
        }
    }
    const long bits = mult_knob("TS_LOGUP_HASH_BITS", 0, 32, 32);
    s.n_values = (uint32_t)nv;
    s.out_column = spec.out_column;
    s.negate = spec.negate;
    s.hash_mask = bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1;

    const uint64_t n = trace.height;
    uint64_t capacity = 2;
    while (capacity < 2 * n) capacity <<= 1;  // <= 2^28
    s.cap_mask = (uint32_t)(capacity - 1);
    DevBuf<uint32_t> slots(&ctx, capacity);
    DevBuf<unsigned long long> sums(&ctx, n);
    DevBuf<MultBack> back(&ctx, 1);
    TS_HIP(hipMemsetAsync(slots.p, 0xff, capacity * sizeof(uint32_t), ctx.stream));
    TS_HIP(hipMemsetAsync(sums.p, 0, n * sizeof(unsigned long long), ctx.stream));
    TS_HIP(hipMemsetAsync(back.p, 0, sizeof(MultBack), ctx.stream));
    TS_HIP(hipMemsetAsync(&back.p->first_missing, 0xff, sizeof(unsigned long long), ctx.stream));
    const dim3 grid((unsigned)((n + MULT_THREADS - 1) / MULT_THREADS)), block(MULT_THREADS);
    const uint32_t* pre = table_pre ? table_pre->buf.p : trace.buf.p;  // (no kind-2 term gets here without a table)
    TS_LAUNCH(ctx, k_mult_insert, grid, block, 0, s, (const uint32_t*)trace.buf.p, pre, n, slots.p, back.p);
    TS_HIP(hipGetLastError());
    for (size_t k = 0; k < nk; k++) {
        const uint64_t nr = lookers[k]->height;
        TS_LAUNCH(ctx, k_mult_count_bus, dim3((unsigned)((nr + MULT_THREADS - 1) / MULT_THREADS)), block, 0, s, lk[k],
                  (const uint32_t*)trace.buf.p, pre, (const uint32_t*)lookers[k]->buf.p, nr, (const uint32_t*)slots.p, sums.p,
                  back.p);
        TS_HIP(hipGetLastError());
    }
    TS_LAUNCH(ctx, k_mult_write, grid, block, 0, s.width, s.out_column, s.negate, n,
              (const unsigned long long*)sums.p, trace.buf.p);
    TS_HIP(hipGetLastError());
    MultBack host;
    d2h_sync(ctx, &host, back.p, sizeof host);
    if (host.error)
        throw Error(TS_ERR_INVARIANT, "logup multiplicities: internal error: the slot table was full");
    LogupMultBusResult r{host.n_missing, ~0ull, ~0ull, ~0ull};
    if (host.n_missing) {
        const uint64_t low = host.first_missing & 0xFFFFFFFFull;
        r.looker = host.first_missing >> 32;
        r.row = low / LOGUP_MULT_MAX_LOOKUPS;
        r.lookup = low % LOGUP_MULT_MAX_LOOKUPS;
    }
    return r;
}

}  // namespace ts
