// What the hash joins over resident traces share (logup_mult.hip: one table's multiplicity column; bus_check.hip: the
// exact balance of a whole bus): a spec term read on a row, the tuple of up to LOGUP_MAX_VALUES words, its hash and
// comparison, and the reader of the integer knobs.  The hash is private to these files and changes no output.
#pragma once
#include <stdlib.h>

#include <string>

#include "logup.hpp"

namespace ts {

// kind 0: the constant; 1: column `val` of the trace's row; 2: column `val` of the preprocessed row
__device__ __forceinline__ uint32_t mult_term(uint32_t kind, uint32_t val, const uint32_t* __restrict__ row,
                                              const uint32_t* __restrict__ pre_row) {
    return kind == 0 ? val : (kind == 1 ? row : pre_row)[val];
}

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
