// Blake3 Merkle MMCS kernels (build-defined spec; there is no Merkle tree
// in the reference, whose BFMmcs is a Bitcoin taptree: basic/src/mmcs/taptree_mmcs.rs:101-114).
//   leaf  = Blake3(row of matrix 0 || row of matrix 1 || ...), elements as canonical u32 LE
//   node  = Blake3(left || right)
// Leaves: one thread per row; column-major matrices make every column read a coalesced 256 B
// per wavefront.  Digests are stored as 8 consecutive words per node, levels back to back.
#include <stdlib.h>

#include "blake3.hpp"
#include "blake3_quad.hpp"
#include "merkle_tree.hpp"
#include "leaf_tree.hpp"
#include "leaves.hpp"
#include "chal_dev.hpp"
#include "kernels.hpp"

namespace ts {

// The standalone leaf kernel: one thread per row, one instantiation per leaf kind (leaves.hpp).  It
// serves what the leaf-tree kernel does not take: trees below 2^8 leaves, rows wider than 256,
// mixed-height batches, short sharded slabs, TS_LEAF_TREE=0.
template <class Leaf>
__global__ void __launch_bounds__(256)
k_leaf_hash(Leaf leaf, uint64_t height, uint32_t* __restrict__ digests) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= height) return;
    uint32_t cv[8];
    leaf.digest(r, cv);
    b3::store_digest(digests + 8 * r, cv);
}

// `name`: the kernel-timer names keep one entry per leaf kind, as the profile tools know them
template <class Leaf>
static void launch_leaf_kernel(Context& ctx, const char* name, const Leaf& leaf, uint64_t height, uint32_t* digests) {
    TS_LAUNCH_NAMED(ctx, name, k_leaf_hash<Leaf>, dim3((unsigned)((height + 255) / 256)), dim3(256), 0, leaf, height,
                    digests);
    TS_HIP(hipGetLastError());
}

// single matrix: the strided hash; several: the pointer table
static bool strided(const LeafMats& mats) { return mats.n_mats == 1 && mats.d[0] != nullptr && mats.total_width >= 1; }
static StridedLeaf strided_leaf(const LeafMats& mats) {
    return StridedLeaf{mats.d[0], mats.col_stride[0], mats.total_width / 16, mats.total_width % 16};
}

void launch_leaf_hash(Context& ctx, const LeafMats& mats, uint64_t height, uint32_t* digests) {
    TS_REQUIRE(mats.total_width <= (1u << 20), TS_ERR_UNSUPPORTED,
               "leaf rows wider than 2^20 field elements are not supported");
    TS_REQUIRE(mats.cols != nullptr, TS_ERR_INVALID, "leaf_hash: column pointer table missing");
    if (mats.total_width > 256)
        launch_leaf_kernel(ctx, "k_leaf_hash_wide", WideLeaf{mats.cols, mats.total_width}, height, digests);
    else if (strided(mats))
        launch_leaf_kernel(ctx, "k_leaf_hash_strided", strided_leaf(mats), height, digests);
    else
        launch_leaf_kernel(ctx, "k_leaf_hash<1>", TableLeaf{mats.cols, mats.total_width}, height, digests);
}

void launch_leaf_hash_ef_pairs(Context& ctx, const uint32_t* vec, uint64_t n_rows, uint32_t* digests) {
    launch_leaf_kernel(ctx, "k_leaf_hash_ef_pairs", EfPairLeaf{reinterpret_cast<const Ef*>(vec)}, n_rows, digests);
}

// one level: parents[i] = Blake3(children[2i] || children[2i+1]), one parent per thread (two, as
// independent chains, measured no better inside whole proofs: 3.32 vs 3.27-3.33 ms/step)
__global__ void __launch_bounds__(256)
k_merkle_level(const uint4* __restrict__ children, uint32_t* __restrict__ parents, uint64_t n_parents) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parents) return;
    const uint4 a = children[4 * i], b = children[4 * i + 1], c = children[4 * i + 2], d = children[4 * i + 3];
    const uint32_t m[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    uint32_t cv[8];
    b3::hash64(m, cv);
    b3::store_digest(parents + 8 * i, cv);
}

// (A variant with fully coalesced traffic -- 16-byte loads at consecutive addresses into LDS, each
// thread then picking up its 64 bytes, digests leaving the same way -- measured 0.421 against 0.410 ms
// per C3 proof: the access pattern is not what holds these launches at 2.8 TB/s; most of the 27 per
// proof are short levels of 2^16..2^18 parents whose time is launch and tail latency.)
static void launch_level(Context& ctx, const uint32_t* children, uint32_t* parents, uint64_t n_parents) {
    TS_LAUNCH_NAMED(ctx, "k_merkle_level<1>", k_merkle_level, dim3((unsigned)((n_parents + 255) / 256)), dim3(256), 0,
                    reinterpret_cast<const uint4*>(children), parents, n_parents);
}

void launch_merkle_one_level(Context& ctx, const uint32_t* children, uint32_t* parents,
                             uint64_t n_parents) {
    launch_level(ctx, children, parents, n_parents);
    TS_HIP(hipGetLastError());
}

// mixed-height injection: nodes[i] = Blake3(nodes[i] || inj[i])
__global__ void __launch_bounds__(256)
k_merkle_inject(uint4* __restrict__ nodes, const uint4* __restrict__ inj, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint4 a = nodes[2 * i], b = nodes[2 * i + 1], c = inj[2 * i], d = inj[2 * i + 1];
    uint32_t m[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    uint32_t cv[8];
    b3::hash64(m, cv);
    b3::store_digest(reinterpret_cast<uint32_t*>(nodes + 2 * i), cv);
}
void launch_merkle_inject(Context& ctx, uint32_t* nodes, const uint32_t* inj, uint64_t n) {
    TS_LAUNCH(ctx, k_merkle_inject, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
              reinterpret_cast<uint4*>(nodes), reinterpret_cast<const uint4*>(inj), n);
    TS_HIP(hipGetLastError());
}

// Top of a sharded tree: level 0 = the G gathered sub-tree roots, then log2(G) levels; G is small
// (<= 64), so one wavefront does a level at a time.
__global__ void __launch_bounds__(64)
k_shard_top(const uint32_t* __restrict__ subroots, uint32_t G, uint32_t* __restrict__ top,
            DevChallenger* __restrict__ ch, uint32_t* __restrict__ root_out, Ef* __restrict__ beta_out) {
    for (uint32_t i = threadIdx.x; i < 8 * G; i += 64) top[i] = subroots[i];
    __threadfence_block();
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t cnt = G; cnt > 1; cnt >>= 1) {
        const uint32_t i = threadIdx.x;
        if (i < cnt / 2) {
            uint32_t m[16], cv[8];
            for (int k = 0; k < 16; k++) m[k] = top[8 * (off + 2 * i) + k];
            b3::hash64(m, cv);
            for (int k = 0; k < 8; k++) top[8 * (off + cnt + i) + k] = cv[k];
        }
        off += cnt;
        __threadfence_block();
        __syncthreads();
    }
    if (ch != nullptr && threadIdx.x == 0) dc_round_one_lane(ch, top + 8 * off, root_out, beta_out);
}
void launch_shard_top(Context& ctx, const uint32_t* subroots, uint32_t G, uint32_t* top,
                      DevChallenger* ch, uint32_t* root_out, Ef* beta_out) {
    TS_REQUIRE(G >= 1 && G <= 64 && (G & (G - 1)) == 0, TS_ERR_INVALID, "shard_top: G must be 2^k <= 64");
    TS_LAUNCH(ctx, k_shard_top, dim3(1), dim3(64), 0, subroots, G, top, ch, root_out, beta_out);
    TS_HIP(hipGetLastError());
}

// Up to 2^22 first-level nodes: the whole tree in ONE launch (merkle_tree.hpp).  Taller trees run
// their first levels one launch per level (bandwidth-bound there, ~3.7 TB/s of digest traffic).
__global__ void __launch_bounds__(mt::NTH)
k_merkle_tree(uint32_t* __restrict__ tree, unsigned log_leaves, unsigned first_level,
              uint32_t* __restrict__ ticket, DevChallenger* __restrict__ ch,
              uint32_t* __restrict__ root_out, Ef* __restrict__ beta_out) {
    __shared__ mt::Lds lds;
    __shared__ uint32_t s_last;
    uint64_t off = 0;
    for (unsigned l = 0; l < first_level; l++) off += (uint64_t)1 << (log_leaves - l);
    const unsigned remaining = log_leaves - first_level;
    const mt::Levels lv{tree, off, (uint64_t)1 << remaining};
    mt::T9::StagedNodes<false> prod{lv.at(0, 0)};
    mt::T9::tree_body(lds, s_last, prod, lv, remaining, ticket, ch, root_out, beta_out);
}

void launch_merkle_tree_from(Context& ctx, uint32_t* tree, unsigned log_leaves, unsigned first_level,
                             DevChallenger* ch, uint32_t* root_out, Ef* beta_out) {
    TS_REQUIRE(first_level < log_leaves && log_leaves - first_level <= mt::MAX_LOG_TREE, TS_ERR_INVALID,
               "merkle_tree_from: between 2 and 2^22 nodes in the first level");
    const unsigned remaining = log_leaves - first_level;
    TS_LAUNCH(ctx, k_merkle_tree, dim3(1u << (remaining - mt::block_log(remaining))), dim3(mt::NTH), 0, tree,
              log_leaves, first_level, ctx.ticket(), ch, root_out, beta_out);
    TS_HIP(hipGetLastError());
}

// ---- leaves + tree in one launch (leaf_tree.hpp) ---------------------------------------------------
bool leaf_tree_enabled(unsigned log_leaves) {
    static const int on = [] {
        const char* e = getenv("TS_LEAF_TREE");  // 0: the round-4 path (leaf launch, level launches, tree launch)
        return e ? atoi(e) : 1;
    }();
    return on != 0 && log_leaves >= mt::LEAF_TREE_MIN_LOG;
}

void launch_commit_tree(Context& ctx, const LeafMats& mats, unsigned log_leaves, uint32_t* tree,
                        uint32_t* root_out) {
    const uint64_t height = (uint64_t)1 << log_leaves;
    if (!leaf_tree_enabled(log_leaves) || mats.total_width > 256) {
        launch_leaf_hash(ctx, mats, height, tree);
        launch_merkle_levels(ctx, tree, log_leaves, nullptr, root_out, nullptr);
        return;
    }
    TS_REQUIRE(mats.cols != nullptr, TS_ERR_INVALID, "commit_tree: column pointer table missing");
    if (strided(mats))
        launch_leaf_tree(ctx, strided_leaf(mats), tree, log_leaves, nullptr, root_out, nullptr);
    else
        launch_leaf_tree(ctx, TableLeaf{mats.cols, mats.total_width}, tree, log_leaves, nullptr, root_out, nullptr);
}

// Measured (tools/time_tree.py, us per tree above the leaves, one launch / per-level launches down to
// 2^16): 2^17 34 / 33, 2^18 60 / 44, 2^20 89 / 71, 2^22 216 / 152.  In one launch the bulk levels run
// as four-lane compressions out of LDS between workgroup barriers at 3 workgroups per CU, ~19 G
// compressions/s; k_merkle_level streams them at ~34 G/s.  So the single launch takes over at 2^17.
static unsigned merkle_tree_max_log() {
    static const unsigned v = [] {
        const char* e = getenv("TS_TREE_MAX_LOG");  // up to 22, for A/B runs
        const int x = e ? atoi(e) : 17;
        return (unsigned)(x < 1 ? 1 : x > (int)mt::MAX_LOG_TREE ? (int)mt::MAX_LOG_TREE : x);
    }();
    return v;
}

bool launch_merkle_levels(Context& ctx, uint32_t* tree, unsigned log_leaves, DevChallenger* ch,
                          uint32_t* root_out, Ef* beta_out) {
    unsigned level = 0;
    uint64_t off = 0;
    while (log_leaves - level > merkle_tree_max_log()) {
        const uint64_t n_children = (uint64_t)1 << (log_leaves - level);
        const uint64_t n_parents = n_children / 2;
        launch_level(ctx, tree + 8 * off, tree + 8 * (off + n_children), n_parents);
        off += n_children;
        level++;
    }
    if (level == log_leaves) return false;
    launch_merkle_tree_from(ctx, tree, log_leaves, level, ch, root_out, beta_out);
    return ch != nullptr;
}

}  // namespace ts
