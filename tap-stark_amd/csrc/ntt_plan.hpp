// The pass plan of the NTT: how a transform of 2^log_n points is split into a strided (middle) pass and
// contiguous passes, and the shapes it is refused for.  The one place that decides it: coset_lde, the
// standalone transforms, the fused transpose and ts_bench_stage all ask here (ntt_lde.hip's header says
// why the plan is what it is).  Host only and free of HIP, so that a plain C++ compiler can build it
// (tests/test_ntt_plan_cpu.py prints the whole table).
#pragma once
#include <stdint.h>

#include "bb.hpp"

namespace ts {

constexpr int LOG_M = 12;          // default contiguous chunk = 4096 elements
constexpr int TILE_ELEMS = 8192;   // strided tile (generic and fixed plans)
constexpr uint32_t NTT_MAX_COLS = 65535;  // columns are a grid's y dimension

// chunk size of the contiguous passes: 2^12, or log_n - 8 for n = 2^21 / 2^22
inline unsigned lde_chunk_log(unsigned log_n) {
    return (log_n == 21 || log_n == 22) ? log_n - 8 : (unsigned)LOG_M;
}

enum class NttMid {
    GENERIC,     // run-time round plan on the 8192-element tile
    FIXED256,    // 256 rows x 32 slots: two radix-16 rounds at compile-time distances (n = 2^(LM + 8))
    TILE16384,   // run-time round plan on a 16384-element tile (68 KB of LDS): sA = 14, n = 2^26
};

struct NttPlan {
    unsigned log_n;
    unsigned LM;         // contiguous chunk = 2^LM elements
    bool two_pass;       // n > 2^LM; else the middle kernel does the whole column, one workgroup each
    unsigned sA;         // stages of the strided pass when two_pass (the contiguous passes do the other LM)
    unsigned log_T;      // a strided tile is 2^log_len rows x 2^log_T adjacent slots
    unsigned log_len;    // stages of the middle pass: sA, or log_n when it is the only one
    unsigned row_shift;  // rows of a tile are 2^row_shift elements apart: LM, or 0
    NttMid mid;
    bool fused_first_round;  // there is a contiguous inverse pass whose first round k_transpose_bitrev_r16 can take
    uint32_t chunks;     // contiguous chunks per column (2^sA)
    uint32_t tiles;      // strided tiles per column
};

inline NttPlan ntt_plan(unsigned log_n) {
    NttPlan p{};
    p.log_n = log_n;
    p.LM = lde_chunk_log(log_n);
    p.two_pass = log_n > p.LM;
    p.sA = p.two_pass ? log_n - p.LM : 0;
    if (p.sA > 14) return p;  // n > 2^26: refused (ntt_plan_refusal), nothing further is defined
    // sA <= 13 fits the 8192-element tile, as wide as it allows up to 64 slots (256 bytes a row); sA = 14
    // (n = 2^26, the longest trace a blowup of 2 leaves room for below the two-adicity 27) takes the
    // 16384-element tile, one slot wide
    if (p.two_pass && p.sA <= 13)
        while ((1u << (p.sA + p.log_T + 1)) <= (unsigned)TILE_ELEMS && p.log_T < 6) p.log_T++;
    p.log_len = p.two_pass ? p.sA : log_n;
    p.row_shift = p.two_pass ? p.LM : 0;
    p.mid = p.sA == 14 ? NttMid::TILE16384 : (p.sA == 8 && p.log_T == 5) ? NttMid::FIXED256 : NttMid::GENERIC;
    p.fused_first_round = p.two_pass;
    p.chunks = 1u << p.sA;
    p.tiles = p.two_pass ? 1u << (p.LM - p.log_T) : 1u;
    return p;
}

// The shape limits of a transform of `ncols` columns with the given strides (stride_b: the output of an LDE,
// else 0).  nullptr if the plan can run, else the message of the TS_ERR_INVALID the caller throws
// (kernels.hpp ntt_require_shape).  `lde`: the wording coset_lde has always used.
inline const char* ntt_plan_refusal(const NttPlan& p, uint32_t ncols, uint64_t stride_a, uint64_t stride_b, bool lde) {
    if (ncols > NTT_MAX_COLS) return lde ? "coset_lde: bad column count" : "dft: more than 65535 columns";
    if (p.sA > 14) return lde ? "coset_lde: log_n > 26" : "dft: height above 2^26";
    // the vectorised chunk loads need 16-byte aligned columns
    if (p.two_pass && (stride_a % 4 != 0 || stride_b % 4 != 0))
        return lde ? "coset_lde: column strides must be multiples of 4 elements"
                   : "dft: column stride must be a multiple of 4 elements";
    return nullptr;
}

// Which block of a whole coset LDE is its own input.  Block beta of coset_lde's output holds the values on the
// coset s_beta = shift * w_N^bitrev_b(beta) of H_n (N = n << log_blowup, b = log_blowup; ntt.hip
// k_build_shift_tables), in the row order of the input, and the input holds the values on H_n itself: where
// s_beta = 1 the inverse transform, the scaling and the forward transform compose to the identity and, the words
// in HBM being canonical, the block is the input word for word.  Returns that beta, or -1 if no coset is H_n
// (the trace commit's shift 31).  The one owner of the question: coset_lde and the callers that prepare its
// input ask here.  By the definition, over every beta, in the order of the exponent e = bitrev_b(beta).
inline int lde_own_coset(unsigned log_n, unsigned log_blowup, uint32_t shift) {
    const unsigned log_N = log_n + log_blowup;
    if (log_N > 27 || shift == 0 || shift >= P) return -1;
    // every s_beta lies in shift * H_N: outside the subgroup of order N none of them is 1
    if (pow_canon(shift, 1ull << log_N) != 1u) return -1;
    const uint32_t w = to_mont(two_adic_generator(log_N));
    uint32_t s = shift;  // shift * w_N^e
    for (uint32_t e = 0; e < (1u << log_blowup); e++, s = mont_mul(s, w))
        if (s == 1u) return (int)bitrev32(e, log_blowup);
    return -1;
}

}  // namespace ts
