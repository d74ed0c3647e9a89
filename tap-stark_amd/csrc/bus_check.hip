// The exact balance of a LogUp bus, checked in HBM over the still-resident traces and before any challenge: for every
// distinct tuple on the bus the field sum of its multiplicities over all tables, rows and interactions must be 0.
//
// A contribution is (table k, row r, interaction i of specs[k]) whose multiplicity term is non-zero mod p; its tuple is
// its value terms ZERO-PADDED to LOGUP_MAX_VALUES words and compared as stored (gamma + sum_j beta^j v_j cannot tell
// (a, b) from (a, b, 0): they are one tuple on the bus).  Contributions with equal tuples form a class.
//
// Plain launches and one small copy back (a second launch and copy only when the bus is unbalanced); no grid barrier,
// no cooperative launch, no workgroup waits for another; every loop is bounded by `capacity` (the power of two >= twice
// the possible contributions), LOGUP_MAX_INTERACTIONS or the wave size.  The specs and matrix pointers travel in a job
// table in device memory and the workgroups of all tables are laid out by first_block, as logup.hip's *_jobs kernels do:
//   k_bus_insert  one row per lane, looping over the interactions: hash the padded tuple, probe linearly with the
//                 discipline of k_mult_insert (logup_mult.hip): atomicCAS(slot, EMPTY, key) either inserts the
//                 contribution's key or returns a key of the class that holds the slot; that contribution's tuple is read
//                 from its trace (read-only for the launch) and compared: equal -> atomicMin(slot, key) where the key is
//                 lower than the one returned, else next slot.  A slot's content is only ever taken from the value an
//                 atomic returned (a plain load of a word another XCD has just written can be stale); a slot never
//                 goes back to empty and never changes class, so each class ends in exactly one slot holding its least
//                 key, whatever the order.  The key packs (table, row, interaction) in that order of significance.
//                 The slot's index is settled with its class, so the same lane then feeds sums[slot] with a no-return
//                 64-bit atomicAdd of the canonical multiplicity: integer adds commute, and 2^30 * p < 2^61.  A wave
//                 whose contributions of one interaction all carry ONE tuple sends its lowest lane alone through the
//                 probe and sums the multiplicities with shuffles into one add (the wave-level combine of
//                 add_hits, extended to the probe): 0.39 ms against 18.3 on 2^20 rows of one tuple, 12.3 with the
//                 add combined alone; no difference beyond the run-to-run spread on the bus statements
//                 (profiles/bus_check.json, profiles/bus_check_combine_experiment.json).
//   k_bus_scan    one slot per lane (plain loads: an earlier launch wrote them): the used slots, those whose sum is not
//                 0 mod p, and the least key among those -- which is the least contribution to any unbalanced tuple,
//                 since a slot holds the least key of its class.  One atomic per wave and counter.
//   k_bus_shares  (unbalanced only) one row per lane again: the reported contribution's key comes by value, its tuple is
//                 read once per lane with uniform loads, and every contribution of that tuple is counted per table:
//                 count, integer sum and least (row, interaction), combined inside the wave (a wave lies in one table)
//                 and added with one atomic each.
// Nothing is written to a trace.  TS_LOGUP_HASH_BITS is honoured as in logup_mult.hip (logup_dev.hpp).
#include <string.h>

#include <string>

#include "logup_dev.hpp"

namespace ts {

constexpr int BUS_THREADS = 256;
constexpr unsigned long long BUS_EMPTY = ~0ull;

// one per table, at the table's index; a table that is not on the bus has K = 0, no rows and no workgroups
struct BusJob {
    GlobalConstWords trace;
    GlobalConstWords pre;  // the row-major values of its preprocessed columns (kind-2 terms), or null
    uint64_t n;
    uint32_t first_block, K, width, pre_width;
    LogupInteractionDev it[LOGUP_MAX_INTERACTIONS];
};

// what the first copy back holds
struct BusBack {
    unsigned long long n_contributions, n_tuples, n_unbalanced, first_key;
    uint32_t error, pad[3];
};
// what the second holds: one BusShareDev per table, then the tuple
struct BusShareDev {
    unsigned long long count, sum, first;  // first: row << 4 | interaction, ~0 without a contribution
};
struct BusTupleBack {
    uint32_t tuple[LOGUP_MAX_VALUES];
    uint32_t n_values, pad[3];
};

// (table, row, interaction), most significant first: row < 2^27, interaction < 16, table < 64
__host__ __device__ __forceinline__ unsigned long long bus_key(uint32_t table, uint64_t row, uint32_t i) {
    return ((unsigned long long)table << 32) | (row << 4) | i;
}
__host__ __device__ __forceinline__ uint32_t bus_key_table(unsigned long long key) { return (uint32_t)(key >> 32); }
__host__ __device__ __forceinline__ uint32_t bus_key_row(unsigned long long key) { return (uint32_t)key >> 4; }
__host__ __device__ __forceinline__ uint32_t bus_key_interaction(unsigned long long key) { return (uint32_t)key & 15u; }

__device__ __forceinline__ const uint32_t* bus_row(const BusJob& j, uint64_t r) {
    return (const uint32_t*)j.trace + r * j.width;
}
__device__ __forceinline__ const uint32_t* bus_pre_row(const BusJob& j, uint64_t r, const uint32_t* row) {
    return j.pre ? (const uint32_t*)j.pre + r * j.pre_width : row;  // (no kind-2 term gets here without a table)
}

// the zero-padded tuple of interaction i on the row
__device__ __forceinline__ MultTuple bus_tuple(const LogupInteractionDev& it, const uint32_t* __restrict__ row,
                                               const uint32_t* __restrict__ pre_row) {
    MultTuple out;
#pragma unroll
    for (int q = 0; q < (int)LOGUP_MAX_VALUES; q++)
        out.v[q] = q < (int)it.n_values ? mult_term(it.kind[q], it.val[q], row, pre_row) : 0;
    return out;
}

// the tuple of the contribution a key names (a key some lane built from a live row: inside its trace)
__device__ __forceinline__ MultTuple bus_tuple_of_key(const BusJob* __restrict__ jobs, unsigned long long key) {
    const BusJob& j = jobs[bus_key_table(key)];
    const uint32_t* row = bus_row(j, bus_key_row(key));
    return bus_tuple(j.it[bus_key_interaction(key)], row, bus_pre_row(j, bus_key_row(key), row));
}

__global__ void __launch_bounds__(BUS_THREADS)
k_bus_insert(const BusJob* __restrict__ jobs, const uint32_t* __restrict__ first, uint32_t n_jobs, uint32_t hash_mask,
             uint32_t cap_mask, unsigned long long* __restrict__ slots, unsigned long long* __restrict__ sums,
             BusBack* __restrict__ back) {
    const uint32_t table = job_of_block(first, n_jobs);
    const BusJob& j = jobs[table];
    const uint64_t r = (uint64_t)(blockIdx.x - j.first_block) * BUS_THREADS + threadIdx.x;
    const bool live = r < j.n;  // (no early return: every lane of the wave takes part in the ballots and sums below)
    const uint32_t* row = bus_row(j, live ? r : 0);
    const uint32_t* pre_row = bus_pre_row(j, live ? r : 0, row);
    unsigned long long mine = 0;
    for (uint32_t i = 0; i < j.K; i++) {  // (K is the job's: the same trip count in every lane)
        const LogupInteractionDev& it = j.it[i];
        const uint32_t m = live ? mult_canonical(mult_term(it.m_kind, it.m_val, row, pre_row)) : 0;
        // a wave whose contributions of this interaction all carry ONE tuple sends its lowest lane alone through the
        // probe (lanes ascend with the rows, so that lane holds the wave's least key) and shares the slot it found
        const unsigned long long has = __ballot(m != 0);
        if (has == 0) continue;  // (wave-uniform)
        const int leader = __ffsll((long long)has) - 1;
        MultTuple tuple;
        bool same = m != 0;
        if (m != 0) tuple = bus_tuple(it, row, pre_row);
#pragma unroll
        for (int q = 0; q < (int)LOGUP_MAX_VALUES; q++) {
            const uint32_t w = m != 0 ? tuple.v[q] : 0;
            same = same && w == (uint32_t)__shfl((int)w, leader, 64);
        }
        const bool one_tuple = (has & (has - 1)) && __ballot(same) == has;
        bool placed = false;
        uint32_t at = 0;
        if (m != 0) mine++;
        if (m != 0 && (!one_tuple || (int)(threadIdx.x & 63) == leader)) {
            const unsigned long long key = bus_key(table, r, i);
            const uint32_t h = mult_hash(tuple, LOGUP_MAX_VALUES) & hash_mask;
            for (uint64_t step = 0; step <= cap_mask && !placed; step++) {
                at = (h + (uint32_t)step) & cap_mask;
                const unsigned long long old = atomicCAS(slots + at, BUS_EMPTY, key);
                if (old != BUS_EMPTY) {
                    if (!mult_equal(bus_tuple_of_key(jobs, old), tuple)) continue;
                    if (key < old) atomicMin(slots + at, key);  // (the slot only ever goes down: old <= key needs none)
                }
                placed = true;
            }
            if (!placed) atomicOr(&back->error, 1u);  // every slot holds another class: impossible at load <= 1/2
        }
        if (one_tuple) {  // (wave-uniform)
            at = (uint32_t)__shfl((int)at, leader, 64);
            placed = m != 0 && __shfl((int)placed, leader, 64) != 0;
        }
        add_hits(placed, at, m, sums);
    }
    const unsigned long long total = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && total) atomicAdd(&back->n_contributions, total);
}

__global__ void __launch_bounds__(BUS_THREADS)
k_bus_scan(const unsigned long long* __restrict__ slots, const unsigned long long* __restrict__ sums, uint64_t capacity,
           BusBack* __restrict__ back) {
    const uint64_t at = (uint64_t)blockIdx.x * BUS_THREADS + threadIdx.x;
    const unsigned long long key = at < capacity ? slots[at] : BUS_EMPTY;
    const bool used = key != BUS_EMPTY;
    const bool bad = used && sums[at] % P != 0;
    const unsigned long long n_used = __popcll(__ballot(used)), n_bad = __popcll(__ballot(bad));
    if (n_used == 0) return;  // (wave-uniform)
    const unsigned long long least = n_bad ? wave_min(bad ? key : BUS_EMPTY) : BUS_EMPTY;
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&back->n_tuples, n_used);
        if (n_bad) {
            atomicAdd(&back->n_unbalanced, n_bad);
            atomicMin(&back->first_key, least);
        }
    }
}

__global__ void __launch_bounds__(BUS_THREADS)
k_bus_shares(const BusJob* __restrict__ jobs, const uint32_t* __restrict__ first, uint32_t n_jobs,
             unsigned long long reported, BusShareDev* __restrict__ shares, BusTupleBack* __restrict__ tuple_back) {
    const uint32_t table = job_of_block(first, n_jobs);
    const BusJob& j = jobs[table];
    const MultTuple target = bus_tuple_of_key(jobs, reported);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < (int)LOGUP_MAX_VALUES; q++) tuple_back->tuple[q] = target.v[q];
        tuple_back->n_values = jobs[bus_key_table(reported)].it[bus_key_interaction(reported)].n_values;
    }
    const uint64_t r = (uint64_t)(blockIdx.x - j.first_block) * BUS_THREADS + threadIdx.x;
    unsigned long long count = 0, sum = 0, least = BUS_EMPTY;
    if (r < j.n) {
        const uint32_t* row = bus_row(j, r);
        const uint32_t* pre_row = bus_pre_row(j, r, row);
        for (uint32_t i = 0; i < j.K; i++) {
            const LogupInteractionDev& it = j.it[i];
            const uint32_t m = mult_canonical(mult_term(it.m_kind, it.m_val, row, pre_row));
            if (m == 0 || !mult_equal(bus_tuple(it, row, pre_row), target)) continue;
            count++;
            sum += m;
            const unsigned long long at = (r << 4) | i;
            least = at < least ? at : least;
        }
    }
    count = wave_sum(count);
    sum = wave_sum(sum);
    least = wave_min(least);
    if ((threadIdx.x & 63) == 0 && count) {
        atomicAdd(&shares[table].count, count);
        atomicAdd(&shares[table].sum, sum);
        atomicMin(&shares[table].first, least);
    }
}

BusReport bus_check(Context& ctx, const std::vector<const LogupSpec*>& specs,
                    const std::vector<const DeviceMatrix*>& traces, const std::vector<const DeviceMatrix*>& tables) {
    StageTimer timer(&ctx, "bus check");
    const size_t T = specs.size();
    TS_REQUIRE(T >= 1 && T <= LOGUP_MAX_TABLES && traces.size() == T && tables.size() == T, TS_ERR_INVALID,
               "bus check: between 1 and 64 tables, one trace per spec");
    // every refusal first: nothing is allocated before the last table passed
    std::vector<BusJob> jobs(T);
    std::vector<uint32_t> first(T + 1, 0);
    uint64_t n_blocks = 0, possible = 0;
    bool any = false;
    for (size_t k = 0; k < T; k++) {
        BusJob& j = jobs[k];
        memset((void*)&j, 0, sizeof j);
        j.first_block = first[k] = (uint32_t)n_blocks;
        if (!specs[k]) continue;
        any = true;
        TS_REQUIRE(traces[k], TS_ERR_INVALID, "bus check: a spec without a trace");
        logup_check_spec(ctx, *specs[k], *traces[k], tables[k]);
        const LogupSpec& spec = *specs[k];
        j.trace = (GlobalConstWords)traces[k]->buf.p;
        j.pre = tables[k] ? (GlobalConstWords)tables[k]->buf.p : nullptr;
        j.n = traces[k]->height;
        j.K = (uint32_t)spec.interactions.size();
        j.width = traces[k]->width;
        j.pre_width = tables[k] ? tables[k]->width : 0;
        load_interactions(spec, j.it);
        n_blocks += (j.n + BUS_THREADS - 1) / BUS_THREADS;
        possible += j.n * j.K;
    }
    first[T] = (uint32_t)n_blocks;
    TS_REQUIRE(any, TS_ERR_INVALID, "bus check: every spec is null: no table is on the bus");
    TS_REQUIRE(possible <= BUS_CHECK_MAX_CONTRIBUTIONS, TS_ERR_INVALID,
               "bus check: the sum over the tables of height * interactions is above 2^30");
    const uint32_t hash_mask = mult_hash_mask();

    uint64_t capacity = 2;
    while (capacity < 2 * possible) capacity <<= 1;  // <= 2^31
    const uint32_t cap_mask = (uint32_t)(capacity - 1);
    const JobTable<BusJob> d_tab = upload_jobs(ctx, jobs, first);
    const BusJob* d_jobs = d_tab.jobs;
    const uint32_t* d_first = d_tab.first;
    DevBuf<unsigned long long> slots(&ctx, capacity);
    DevBuf<unsigned long long> sums(&ctx, capacity);
    DevBuf<BusBack> back(&ctx, 1);
    TS_HIP(hipMemsetAsync(slots.p, 0xff, capacity * sizeof(unsigned long long), ctx.stream));
    TS_HIP(hipMemsetAsync(sums.p, 0, capacity * sizeof(unsigned long long), ctx.stream));
    TS_HIP(hipMemsetAsync(back.p, 0, sizeof(BusBack), ctx.stream));
    TS_HIP(hipMemsetAsync(&back.p->first_key, 0xff, sizeof(unsigned long long), ctx.stream));
    const dim3 block(BUS_THREADS);
    TS_LAUNCH(ctx, k_bus_insert, dim3((unsigned)n_blocks), block, 0, d_jobs, d_first, (uint32_t)T, hash_mask, cap_mask,
              slots.p, sums.p, back.p);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_bus_scan, dim3((unsigned)((capacity + BUS_THREADS - 1) / BUS_THREADS)), block, 0,
              (const unsigned long long*)slots.p, (const unsigned long long*)sums.p, capacity, back.p);
    TS_HIP(hipGetLastError());
    BusBack host;
    d2h_sync(ctx, &host, back.p, sizeof host);
    if (host.error) throw Error(TS_ERR_INVARIANT, "bus check: internal error: the slot table was full");

    BusReport rep;
    rep.n_contributions = host.n_contributions;
    rep.n_tuples = host.n_tuples;
    rep.n_unbalanced = host.n_unbalanced;
    rep.shares.assign(T, BusShare());
    if (!host.n_unbalanced) return rep;

    // the reported tuple's part per table: {T shares, the tuple} in one buffer, one copy back
    static_assert(sizeof(BusShareDev) == 24 && sizeof(BusTupleBack) % 8 == 0, "laid out in 64-bit words");
    const size_t share_words = T * sizeof(BusShareDev) / 8, back_words = share_words + sizeof(BusTupleBack) / 8;
    DevBuf<unsigned long long> d_shares(&ctx, back_words);
    std::vector<unsigned long long> init(back_words, 0);
    for (size_t k = 0; k < T; k++) init[3 * k + 2] = BUS_EMPTY;
    h2d(ctx, d_shares.p, init.data(), back_words * 8);
    TS_LAUNCH(ctx, k_bus_shares, dim3((unsigned)n_blocks), block, 0, d_jobs, d_first, (uint32_t)T,
              (unsigned long long)host.first_key, reinterpret_cast<BusShareDev*>(d_shares.p),
              reinterpret_cast<BusTupleBack*>(d_shares.p + share_words));
    TS_HIP(hipGetLastError());
    std::vector<unsigned long long> got(back_words);
    d2h_sync(ctx, got.data(), d_shares.p, back_words * 8);
    rep.first_table = bus_key_table(host.first_key);
    rep.first_row = bus_key_row(host.first_key);
    rep.first_interaction = bus_key_interaction(host.first_key);
    BusTupleBack tb;
    memcpy(&tb, got.data() + share_words, sizeof tb);
    rep.n_values = tb.n_values;
    memcpy(rep.tuple, tb.tuple, sizeof rep.tuple);
    uint64_t sum = 0;
    for (size_t k = 0; k < T; k++) {
        BusShare& s = rep.shares[k];
        s.count = got[3 * k];
        s.sum = (uint32_t)(got[3 * k + 1] % P);
        if (s.count) {
            s.first_row = (uint32_t)(got[3 * k + 2] >> 4);
            s.first_interaction = (uint32_t)(got[3 * k + 2] & 15u);
        }
        sum = (sum + s.sum) % P;
    }
    rep.sum = (uint32_t)sum;
    return rep;
}

}  // namespace ts
