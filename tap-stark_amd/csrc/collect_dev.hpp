// The device pieces collect.hip and group.hip share, one copy each: the workgroup's exclusive scan in lane order and
// the launch of the scan over the block counts.
#pragma once
#include <stdint.h>

#include "context.hpp"

namespace ts {

constexpr int COLLECT_THREADS = 256;
constexpr int COLLECT_RPT = 4;  // rows per lane at most: a workgroup owns up to 1024 rows
constexpr int COLLECT_WAVES = COLLECT_THREADS / 64;
constexpr uint32_t COLLECT_PAD_TILE_ROWS = 256;
constexpr uint32_t COLLECT_PAD_BLOCKS = 1024;

// Over the workgroup's lanes in lane order: the sum of v over the lanes BEFORE this one; total <- over all lanes.
// Wave-64 shuffles inside a wave, LDS across the waves.  Every thread calls it.
__device__ __forceinline__ uint32_t collect_block_scan(uint32_t v, uint32_t (&wave_sums)[COLLECT_WAVES], uint32_t& total) {
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += up;
    }
    __syncthreads();  // (a second call reuses wave_sums)
    if (lane == 63) wave_sums[wv] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < COLLECT_WAVES; k++) {
        const uint32_t w = wave_sums[k];
        if (k < (int)wv) before += w;
        all += w;
    }
    total = all;
    return before + inc - v;
}

// k_collect_offsets (collect.hip) on ctx's stream: offsets[b] <- counts[0] + ... + counts[b-1], b < n_blocks;
// offsets[n_blocks] <- the sum of all.  One workgroup.
void collect_launch_offsets(Context& ctx, const uint32_t* counts, uint32_t n_blocks, uint64_t* offsets);

}  // namespace ts
