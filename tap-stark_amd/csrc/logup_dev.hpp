// The device pieces the LogUp kernels over resident traces share (logup.hip: the aux columns; logup_mult.hip: one
// table's multiplicity column; bus_check.hip: the exact balance of a whole bus), one copy each: a spec term read on a
// row and its admission, an interaction's device form, the job table the workgroups of several tables find their work
// in, the tuple of up to LOGUP_MAX_VALUES words with its hash and comparison, the 64-bit wave sum and minimum, the
// wave-combined add, and the reader of the integer knobs.  The hash is private to these files and changes no output.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "logup.hpp"

namespace ts {

// kind 0: the constant; 1: column `val` of the trace's row; 2: column `val` of the preprocessed row
__device__ __forceinline__ uint32_t mult_term(uint32_t kind, uint32_t val, const uint32_t* __restrict__ row,
                                              const uint32_t* __restrict__ pre_row) {
    return kind == 0 ? val : (kind == 1 ? row : pre_row)[val];
}

// The admission of one spec term over a matrix `width` columns wide, before anything is allocated: its kind is at most
// max_kind, kind 2 has the matrix `pre` of preprocessed columns to read, a column lies inside its matrix, a constant is
// canonical, and no kind-1 term names column `unread` (the out_column of a multiplicity fill; ~0: nothing to keep off).
inline void require_term(const std::string& call, const LogupTerm& tm, uint32_t max_kind, uint32_t width,
                         const DeviceMatrix* pre, uint32_t unread = ~0u) {
    TS_REQUIRE(tm.kind <= max_kind, TS_ERR_INVALID,
               call + (max_kind >= 2 ? ": term kind must be 0 (constant), 1 (column) or 2 (preprocessed column)"
                                     : ": term kind must be 0 (constant) or 1 (column)"));
    TS_REQUIRE(tm.kind != 2 || pre, TS_ERR_INVALID, call + ": a preprocessed-column term without a preprocessed table");
    TS_REQUIRE(tm.kind == 2 ? tm.value < pre->width : tm.kind ? tm.value < width : tm.value < P, TS_ERR_INVALID,
               call + ": a column outside the trace or the preprocessed table, or a non-canonical constant");
    TS_REQUIRE(tm.kind != 1 || tm.value != unread, TS_ERR_INVALID,
               call + ": out_column is among the table-trace columns the spec reads");
}

// one interaction of a LogupSpec: its multiplicity term and its value terms
struct LogupInteractionDev {
    uint32_t m_kind, m_val, n_values, pad;
    uint32_t kind[LOGUP_MAX_VALUES], val[LOGUP_MAX_VALUES];
};
// (terms admitted already)
inline void load_interactions(const LogupSpec& spec, LogupInteractionDev* it) {
    for (size_t i = 0; i < spec.interactions.size(); i++) {
        const LogupInteraction& in = spec.interactions[i];
        it[i].m_kind = in.multiplicity.kind;
        it[i].m_val = in.multiplicity.value;
        it[i].n_values = (uint32_t)in.values.size();
        for (size_t q = 0; q < in.values.size(); q++) {
            it[i].kind[q] = in.values[q].kind;
            it[i].val[q] = in.values[q].value;
        }
    }
}

// ---- a job table in device memory: one job per table, the workgroups of all tables in one launch.  A workgroup finds
// its job from the first-workgroup prefix `first` (n_jobs + 1 ascending words, first[n_jobs] = the grid) with a search
// on blockIdx alone, so the job index is the same in every lane and the job's words are read with scalar loads.
// (a pointer read from memory is a generic one to the compiler and costs flat loads and stores; a job's pointers are
// device allocations and are typed so, which keeps the global accesses the by-value kernels have)
typedef const uint32_t __attribute__((address_space(1)))* GlobalConstWords;
typedef uint32_t __attribute__((address_space(1)))* GlobalWords;

// first[lo] <= blockIdx.x < first[lo + 1] (jobs without workgroups are stepped over)
__device__ __forceinline__ uint32_t job_of_block(const uint32_t* __restrict__ first, uint32_t n_jobs) {
    uint32_t lo = 0, hi = n_jobs;  // first[lo] <= blockIdx.x < first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (first[mid] <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the jobs and, behind them, the prefix (jobs.size() + 1 words): one upload
template <class Job>
struct JobTable {
    DevBuf<unsigned long long> buf;
    const Job* jobs;
    const uint32_t* first;
};
template <class Job>
JobTable<Job> upload_jobs(Context& ctx, const std::vector<Job>& jobs, const std::vector<uint32_t>& first) {
    static_assert(sizeof(Job) % 8 == 0, "the prefix follows the jobs, aligned");
    const size_t job_bytes = jobs.size() * sizeof(Job);
    std::vector<char> tab(job_bytes + first.size() * sizeof(uint32_t));
    memcpy(tab.data(), (const void*)jobs.data(), job_bytes);
    memcpy(tab.data() + job_bytes, first.data(), first.size() * sizeof(uint32_t));
    JobTable<Job> t{DevBuf<unsigned long long>(&ctx, (tab.size() + 7) / 8), nullptr, nullptr};
    h2d(ctx, t.buf.p, tab.data(), tab.size());
    t.jobs = reinterpret_cast<const Job*>(t.buf.p);
    t.first = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(t.buf.p) + job_bytes);
    return t;
}

// ---- tuples and their hash
struct MultTuple {
    uint32_t v[LOGUP_MAX_VALUES];
};

// over the first nv words (a caller that compares zero-padded tuples of mixed lengths passes LOGUP_MAX_VALUES)
__device__ __forceinline__ uint32_t mult_hash(const MultTuple& t, uint32_t nv) {
    uint32_t h = 0x9E3779B9u;
#pragma unroll
    for (int q = 0; q < (int)LOGUP_MAX_VALUES; q++)
        if (q < (int)nv) {
            h = (h ^ t.v[q]) * 0x85EBCA6Bu;
            h ^= h >> 13;
        }
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

__device__ __forceinline__ bool mult_equal(const MultTuple& a, const MultTuple& b) {
    bool eq = true;  // (the words past n_values are zero on both sides)
#pragma unroll
    for (int q = 0; q < (int)LOGUP_MAX_VALUES; q++) eq = eq && a.v[q] == b.v[q];
    return eq;
}

// canonical, whatever word the column held (2^32 < 3 p)
__device__ __forceinline__ uint32_t mult_canonical(uint32_t w) {
    w = w >= P ? w - P : w;
    return w >= P ? w - P : w;
}

// ---- over the wave; every lane calls them
__device__ __forceinline__ unsigned long long wave_shfl_xor(unsigned long long v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += wave_shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = wave_shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

// sums[at] += w on the lanes with `hit`; EVERY lane of the wave calls it (ballots), dead lanes with hit = false.  A
// wave whose hits all go to ONE destination (padding rows, a selector-heavy trace) sums their weights with shuffles
// and issues one add; every other wave issues one add per hit (DESIGN.md has the measurement: a ballot loop over
// every distinct destination of a wave lost on the byte-valued and the uniform inputs and was not kept).
__device__ __forceinline__ void add_hits(bool hit, uint32_t at, uint32_t w, unsigned long long* __restrict__ sums) {
    const unsigned long long hits = __ballot(hit);
    if (hits == 0) return;  // (wave-uniform)
    const int leader = __ffsll((long long)hits) - 1;
    const uint32_t dest = (uint32_t)__shfl((int)at, leader, 64);
    if ((hits & (hits - 1)) && __ballot(hit && at == dest) == hits) {
        const unsigned long long sum = wave_sum(hit ? (unsigned long long)w : 0ull);
        if ((threadIdx.x & 63) == (unsigned)leader) atomicAdd(sums + dest, sum);
    } else if (hit) {
        atomicAdd(sums + at, (unsigned long long)w);
    }
}

// ---- knobs
// an integer knob in [lo, hi], or `unset`
inline long mult_knob(const char* name, long lo, long hi, long unset) {
    const char* e = getenv(name);
    if (!e || !*e) return unset;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    TS_REQUIRE(end && !*end && v >= lo && v <= hi, TS_ERR_INVALID,
               (std::string(name) + " must be in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]").c_str());
    return v;
}

// TS_LOGUP_HASH_BITS (0 .. 32, read on every call): the hash is masked to that many low bits before it is reduced to
// a slot, a test knob that makes probe chains as long as the table
inline uint32_t mult_hash_mask() {
    const long bits = mult_knob("TS_LOGUP_HASH_BITS", 0, 32, 32);
    return bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1;
}

}  // namespace ts
