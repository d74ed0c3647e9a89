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
//   k_mult_count   one looker row per lane, looping over the lookups: weight 0 is skipped; otherwise probe with
//                  plain loads (the slots are final: an earlier launch wrote them); empty -> a miss (64-bit
//                  atomicAdd on the count, atomicMin on its key); equal tuple -> no-return 64-bit
//                  atomicAdd(&sums[rep], w), w canonical.  Integer adds commute: the sums do not depend on order.
//                  They cannot wrap: 2^27 rows * 16 lookups * p < 2^62.
//   k_mult_write   one table row per lane: sums[t] % p, or p minus it, into trace[t][out_column].
// A looker is a matrix whose rows carry lookups: the table trace itself (logup_multiplicities: one looker) or OTHER
// traces (logup_multiplicities_bus: one k_mult_count launch per looker between the same insert and write).
// The hash (logup_dev.hpp, shared with bus_check.hip) changes no output; TS_LOGUP_HASH_BITS (0 .. 32, read on every call) masks
// it to that many low bits before it is reduced to a slot: a test knob that makes probe chains as long as the table.
// Contention: a wave whose hits all go to ONE representative issues one add (add_hits, logup_dev.hpp).
#include <stdlib.h>
#include <string.h>

#include <string>

#include "logup_dev.hpp"

namespace ts {

constexpr int MULT_THREADS = 256;
constexpr uint32_t MULT_EMPTY = 0xFFFFFFFFu;

// the table side: its tuple's terms over the table trace (`width`) and its preprocessed matrix (`table_width`)
struct MultDev {
    uint32_t n_values, width, table_width, out_column, negate, hash_mask, cap_mask, pad;
    uint32_t t_kind[LOGUP_MAX_VALUES], t_val[LOGUP_MAX_VALUES];
};
// lookups and weights over the rows of one matrix (`width`) and of the matrix its kind-2 terms read (`pre_width`)
struct MultLookerDev {
    uint32_t n_lookups, width, pre_width, index;
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

// One launch per looker: the lookup tuple and its weight are read from the looker's row (and, for kind 2, from the
// same row of `looker_pre`: the table's preprocessed matrix where the looker is the table trace of the single-trace
// call, the looker again where it has no such terms); the probe compares against the TABLE's rows (`s`, `table`, and
// `pre` for its kind-2 terms: the table trace again where there are none).  A miss is keyed (looker, row, lookup).
__global__ void __launch_bounds__(MULT_THREADS)
k_mult_count(const MultDev s, const MultLookerDev k, const uint32_t* __restrict__ table,
             const uint32_t* __restrict__ pre, const uint32_t* __restrict__ looker,
             const uint32_t* __restrict__ looker_pre, uint64_t n_looker, const uint32_t* __restrict__ slots,
             unsigned long long* __restrict__ sums, MultBack* __restrict__ back) {
    const uint64_t r = (uint64_t)blockIdx.x * MULT_THREADS + threadIdx.x;
    const bool live = r < n_looker;  // (no early return: every lane of the wave, the dead lanes of a short looker
                                     // included, takes part in the ballots of add_hits)
    const uint32_t* row = looker + (live ? r : 0) * k.width;
    const uint32_t* pre_row = looker_pre + (live ? r : 0) * k.pre_width;
    for (uint32_t l = 0; l < k.n_lookups; l++) {
        const uint32_t w = live ? mult_canonical(mult_term(k.w_kind[l], k.w_val[l], row, pre_row)) : 0;
        uint32_t rep = MULT_EMPTY;
        if (w != 0) {
            MultTuple mine;
#pragma unroll
            for (int q = 0; q < (int)LOGUP_MAX_VALUES; q++)
                mine.v[q] = q < (int)s.n_values ? mult_term(k.l_kind[l][q], k.l_val[l][q], row, pre_row) : 0;
            rep = mult_probe(s, table, pre, slots, mine);
            if (rep == MULT_EMPTY) {
                atomicAdd(&back->n_missing, 1ull);
                atomicMin(&back->first_missing,
                          ((unsigned long long)k.index << 32) | (r * LOGUP_MULT_MAX_LOOKUPS + l));
            }
        }
        add_hits(rep != MULT_EMPTY, rep, w, sums);
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

namespace {

// one looker of a fill: its rows, the matrix its kind-2 terms read (null: it may have none), its spec
struct MultLooker {
    const DeviceMatrix* rows;
    const DeviceMatrix* pre;
    const std::vector<LogupTerm>*lookups, *weights;
};

// The fill both calls make: `table` (n_values terms of kind <= table_max_kind over `trace` and `table_pre`) against
// the lookups of `lookers`.  Every refusal comes before the first allocation.
LogupMultBusResult mult_fill(Context& ctx, const std::vector<LogupTerm>& table, uint32_t table_max_kind,
                             uint32_t out_column, uint32_t negate, DeviceMatrix& trace, const DeviceMatrix* table_pre,
                             const std::vector<MultLooker>& lookers) {
    StageTimer timer(&ctx, "logup multiplicities");
    const char* call = "logup multiplicities";
    MultDev s;
    memset(&s, 0, sizeof s);
    const size_t nv = table.size();
    TS_REQUIRE(nv >= 1 && nv <= LOGUP_MAX_VALUES, TS_ERR_INVALID, "logup multiplicities: between 1 and 8 values");
    TS_REQUIRE(negate <= 1, TS_ERR_INVALID, "logup multiplicities: negate must be 0 or 1");
    require_resident(ctx, trace, call, "the table trace");
    TS_REQUIRE(out_column < trace.width, TS_ERR_INVALID, "logup multiplicities: out_column outside the trace");
    if (table_pre) {
        require_resident(ctx, *table_pre, call, "the preprocessed table");
        TS_REQUIRE(table_pre->height == trace.height, TS_ERR_INVALID,
                   "logup multiplicities: the preprocessed table must have the table trace's height");
        s.table_width = table_pre->width;
    }
    // the table trace's out_column is read by no term of any side
    for (size_t q = 0; q < nv; q++) {
        require_term(call, table[q], table_max_kind, trace.width, table_pre, out_column);
        s.t_kind[q] = table[q].kind;
        s.t_val[q] = table[q].value;
    }
    std::vector<MultLookerDev> lk(lookers.size());
    for (size_t k = 0; k < lookers.size(); k++) {
        const MultLooker& in = lookers[k];
        require_resident(ctx, *in.rows, call, "a looker");
        const size_t nl = in.weights->size();
        TS_REQUIRE(nl >= 1 && nl <= LOGUP_MULT_MAX_LOOKUPS && in.lookups->size() == nl * nv, TS_ERR_INVALID,
                   "logup multiplicities: between 1 and 16 lookups of n_values terms each per looker");
        const uint32_t unread = in.rows->buf.p == trace.buf.p ? out_column : ~0u;
        auto term = [&](const LogupTerm& tm, uint32_t& kind, uint32_t& val) {
            require_term(call, tm, in.pre ? 2 : 1, in.rows->width, in.pre, unread);
            kind = tm.kind;
            val = tm.value;
        };
        MultLookerDev& d = lk[k];
        memset(&d, 0, sizeof d);
        d.n_lookups = (uint32_t)nl;
        d.width = in.rows->width;
        d.pre_width = in.pre ? in.pre->width : in.rows->width;
        d.index = (uint32_t)k;
        for (size_t l = 0; l < nl; l++) {
            term((*in.weights)[l], d.w_kind[l], d.w_val[l]);
            for (size_t q = 0; q < nv; q++) term((*in.lookups)[l * nv + q], d.l_kind[l][q], d.l_val[l][q]);
        }
    }
    s.n_values = (uint32_t)nv;
    s.width = trace.width;
    s.out_column = out_column;
    s.negate = negate;
    s.hash_mask = mult_hash_mask();

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
    for (size_t k = 0; k < lookers.size(); k++) {
        const DeviceMatrix& rows = *lookers[k].rows;
        const uint64_t nr = rows.height;
        TS_LAUNCH(ctx, k_mult_count, dim3((unsigned)((nr + MULT_THREADS - 1) / MULT_THREADS)), block, 0, s, lk[k],
                  (const uint32_t*)trace.buf.p, pre, (const uint32_t*)rows.buf.p,
                  (const uint32_t*)(lookers[k].pre ? lookers[k].pre->buf.p : rows.buf.p), nr, (const uint32_t*)slots.p,
                  sums.p, back.p);
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

}  // namespace

// the table trace is its own looker, and its kind-2 terms read the table's preprocessed matrix
LogupMultResult logup_multiplicities(Context& ctx, const LogupMultSpec& spec, DeviceMatrix& trace,
                                     const DeviceMatrix* table) {
    const LogupMultBusResult r = mult_fill(ctx, spec.table, 2, spec.out_column, spec.negate, trace, table,
                                           {MultLooker{&trace, table, &spec.lookups, &spec.weights}});
    return LogupMultResult{r.n_missing, r.n_missing ? r.row * spec.weights.size() + r.lookup : ~0ull};
}

// ------------------------------------------------------------------ the table in one trace, the lookups in others
LogupMultBusResult logup_multiplicities_bus(Context& ctx, const LogupMultBusSpec& spec, DeviceMatrix& trace,
                                            const std::vector<const DeviceMatrix*>& lookers, const DeviceMatrix* table_pre,
                                            bool takes_pre) {
    const size_t nk = spec.lookers.size();
    TS_REQUIRE(nk >= 1 && nk <= LOGUP_MULT_MAX_LOOKERS && lookers.size() == nk, TS_ERR_INVALID,
               "logup multiplicities: between 1 and 16 lookers, one trace each");
    TS_REQUIRE(!table_pre || takes_pre, TS_ERR_INVALID, "logup multiplicities: this call takes no preprocessed table");
    // kind 2 is the table's alone (logup_multiplicities_bus_pre): the lookers keep kinds 0 and 1
    std::vector<MultLooker> in(nk);
    for (size_t k = 0; k < nk; k++) {
        TS_REQUIRE(lookers[k], TS_ERR_INVALID, "logup multiplicities: null looker");
        in[k] = MultLooker{lookers[k], nullptr, &spec.lookers[k].lookups, &spec.lookers[k].weights};
    }
    return mult_fill(ctx, spec.table, takes_pre ? 2 : 1, spec.out_column, spec.negate, trace, table_pre, in);
}

}  // namespace ts
