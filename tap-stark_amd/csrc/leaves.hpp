// The leaf kinds of the Blake3 MMCS, each defined ONCE as a per-row functor: digest(row, cv) hashes leaf
// `row` (any side effect -- the FRI fold's store -- included).  The standalone leaf kernel (merkle.hip:
// k_leaf_hash), the leaf-tree kernel (leaf_tree.hpp) and the FRI round kernel (fri.hip) all hash through
// these.  The types stay directly in namespace ts under these names: the profile tools map the demangled
// k_leaf_tree<R, Leaf> to the kernel-timer names that Leaf::name(log2 R) gives.
// Device code; include from .hip files only.
#pragma once
#include "blake3.hpp"
#include "kernels.hpp"

namespace ts {

__device__ __forceinline__ Ef load_ef(const Ef* p) {
    uint4 v = *reinterpret_cast<const uint4*>(p);
    return Ef{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void store_ef(Ef* p, Ef e) {
    *reinterpret_cast<uint4*>(p) = make_uint4(e.c[0], e.c[1], e.c[2], e.c[3]);
}

#define TS_LEAF_TREE_NAMES(kind) \
    {"k_leaf_tree<0," kind ">", "k_leaf_tree<1," kind ">", "k_leaf_tree<2," kind ">", "k_leaf_tree<3," kind ">"}

// one matrix (width <= 256): column c of the row is base[c * stride + r] -- no pointer table, no
// per-word bounds checks; n_full whole 64-byte blocks, then (rem != 0) one short block of rem words.
// (Round 3: widths that are not multiples of 16 took the pointer-table hash before -- the 163-column
// trace of config 5 hashed at 0.74 of the Blake3 rate against 0.97 here.)
struct StridedLeaf {
    const uint32_t* base;
    uint64_t stride;
    uint32_t n_full, rem;
    static const char* name(int lr) {
        static const char* const N[4] = TS_LEAF_TREE_NAMES("strided");
        return N[lr];
    }
    __device__ __forceinline__ void digest(uint64_t r, uint32_t cv[8]) const {
        b3::iv(cv);
        const uint32_t* p = base + r;
        for (uint32_t blk = 0; blk < n_full; blk++) {
            uint32_t m[16];
#pragma unroll
            for (int j = 0; j < 16; j++) m[j] = p[(uint64_t)j * stride];
            p += 16 * stride;
            const uint32_t flags = (blk == 0 ? b3::CHUNK_START : 0u) |
                                   (blk + 1 == n_full && rem == 0 ? (b3::CHUNK_END | b3::ROOT) : 0u);
            b3::compress(cv, m, 64, flags);
        }
        if (rem != 0) {
            uint32_t m[16];
#pragma unroll
            for (int j = 0; j < 16; j++) m[j] = (uint32_t)j < rem ? p[(uint64_t)j * stride] : 0u;
            b3::compress(cv, m, rem * 4, (n_full == 0 ? b3::CHUNK_START : 0u) | b3::CHUNK_END | b3::ROOT);
        }
    }
};

// several matrices (total width <= 256): column c of the concatenated row through the pointer table,
// 16 words (one Blake3 block) at a time; the 16 loads of a block are independent and issue back to back
struct TableLeaf {
    const uint32_t* const* cols;
    uint32_t total;
    static const char* name(int lr) {
        static const char* const N[4] = TS_LEAF_TREE_NAMES("table");
        return N[lr];
    }
    __device__ __forceinline__ void digest(uint64_t r, uint32_t cv[8]) const {
        b3::iv(cv);
        const uint32_t n_blocks = total == 0 ? 1 : (total + 15) / 16;
        for (uint32_t blk = 0; blk < n_blocks; blk++) {
            uint32_t m[16];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t c = blk * 16 + j;
                // a pointer read from memory is a generic one to the compiler (flat_load: an aperture
                // check per access); these are device allocations: say so
                typedef const uint32_t __attribute__((address_space(1))) * gptr;
                m[j] = c < total ? ((gptr)cols[c])[r] : 0u;
            }
            const uint32_t words = total - blk * 16 < 16 ? total - blk * 16 : 16;
            const uint32_t flags = (blk == 0 ? b3::CHUNK_START : 0u) |
                                   (blk + 1 == n_blocks ? (b3::CHUNK_END | b3::ROOT) : 0u);
            b3::compress(cv, m, words * 4, flags);
        }
    }
};

// rows wider than one Blake3 chunk (256 elements): chunk chaining + parent tree per row
// (b3::hash_stream); the subtree stack is indexed by a wave-uniform depth and lives in scratch.
// Rare shape (bf_mmcs.rs:17-68 allows any width), kept simple; standalone leaf kernel only.
struct WideLeaf {
    const uint32_t* const* cols;
    uint32_t total;
    __device__ __forceinline__ void digest(uint64_t r, uint32_t cv[8]) const {
        const uint32_t* const* c = cols;
        b3::hash_stream([c, r](uint64_t k) { return c[k][r]; }, total, cv);
    }
};

// rows of two EF4 (32 bytes) of an array-of-EF4 vector -> one short block each
struct EfPairLeaf {
    const Ef* vec;
    static const char* name(int lr) {
        static const char* const N[4] = TS_LEAF_TREE_NAMES("ef_pairs");
        return N[lr];
    }
    __device__ __forceinline__ void digest(uint64_t r, uint32_t cv[8]) const {
        b3::hash_ef_pair(load_ef(vec + 2 * r), load_ef(vec + 2 * r + 1), cv);
    }
};

// ---- the FRI commit-phase leaf ------------------------------------------------------------------
constexpr uint32_t HALF_MONT = 0x07ffffffu;  // to_mont(2^-1)

// out = (lo + hi)/2 + (lo - hi) * w * (beta/2);  w = g^-bitrev(i) (Montgomery base)
__device__ __forceinline__ Ef fold_one(Ef lo, Ef hi, uint32_t w_mont, Ef half_beta_mont,
                                       uint32_t half_mont) {
    Ef s = ef_mul_base(ef_add(lo, hi), half_mont);
    Ef d = ef_mul_base(ef_sub(lo, hi), w_mont);
    return ef_add(s, ef_mul(d, half_beta_mont));
}
__device__ __forceinline__ Ef half_beta_mont_of(const Ef* beta) {
    return ef_mul_base(ef_to_mont(load_ef(beta)), HALF_MONT);
}

// leaf i of a round's matrix = (cur[2i], cur[2i+1]).  FOLD: cur is not in memory yet: it is the fold of
// the previous round's vector with that round's challenge (cur[k] = fold(prev[2k], prev[2k+1]); tw[k] =
// g^-bitrev(k), the twiddle of output k), computed, stored and hashed by the lane that owns the leaf.
template <bool FOLD>
__device__ __forceinline__ void fri_leaf_digest(const Ef* prev, const uint32_t* tw, Ef half_beta_mont, Ef* cur,
                                                uint64_t i, uint32_t cv[8]) {
    Ef a, b;
    if (FOLD) {
        a = fold_one(load_ef(prev + 4 * i), load_ef(prev + 4 * i + 1), tw[2 * i], half_beta_mont, HALF_MONT);
        b = fold_one(load_ef(prev + 4 * i + 2), load_ef(prev + 4 * i + 3), tw[2 * i + 1], half_beta_mont,
                     HALF_MONT);
        store_ef(cur + 2 * i, a);
        store_ef(cur + 2 * i + 1, b);
    } else {
        a = load_ef(cur + 2 * i);
        b = load_ef(cur + 2 * i + 1);
    }
    b3::hash_ef_pair(a, b, cv);
}

// the leaf-tree form: the challenge is read from where the previous round's kernel left it
template <bool FOLD>
struct FriLeaf {
    const Ef* prev;
    const uint32_t* tw;
    const Ef* beta_prev;
    Ef* cur;
    static const char* name(int lr) {
        static const char* const N[2][4] = {TS_LEAF_TREE_NAMES("fri_leaf"), TS_LEAF_TREE_NAMES("fri_fold")};
        return N[FOLD ? 1 : 0][lr];
    }
    __device__ __forceinline__ void digest(uint64_t i, uint32_t cv[8]) const {
        fri_leaf_digest<FOLD>(prev, tw, FOLD ? half_beta_mont_of(beta_prev) : ef_zero(), cur, i, cv);
    }
};

#undef TS_LEAF_TREE_NAMES

}  // namespace ts
