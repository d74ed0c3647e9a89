// Rows of a resident row-major matrix in sorted order, and rows gathered through an index column (sort.hip).
#pragma once
#include <vector>

#include "prover_internal.hpp"

namespace ts {

constexpr uint32_t SORT_MAX_KEYS = 4;
constexpr uint32_t SORT_MAX_WIDTH = 1u << 16;     // of a matrix these calls make: height * width stays below 2^43 words
constexpr uint32_t SORT_DEFAULT_BLOCK_ROWS = 2048;  // TS_SORT_BLOCK_ROWS (1 .. this, read on every call)

struct SortSpec {
    std::vector<uint32_t> key_columns;  // 1 .. 4 columns of src, most significant first, none twice
    uint32_t group_keys = 0;            // 0 .. n_keys
    uint32_t flags = 0;                 // bit 0: a source-row column; bit 1: a group-start column
    uint64_t n_live = 0;                // rows [0, n_live) are sorted, the others keep place and content
};
// A new row-major matrix of src's height: the live rows of `src` (row-major, this context; read only) in the unique
// stable order of their key words compared as stored, unsigned; then the columns the flags ask for.  Throws
// TS_ERR_INVALID before any device work on anything outside the limits; synchronises the stream once (the histogram's
// copy back), and not at all with n_live < 2.
DeviceMatrix sort_rows(Context& ctx, const SortSpec& spec, const DeviceMatrix& src);
// out[i] = src[index[i][index_column]]: the last kernel of sort_rows over a caller's index.  An index word outside
// src throws TS_ERR_INVALID naming the least such row; synchronises the stream once.
DeviceMatrix gather_rows(Context& ctx, const DeviceMatrix& src, const DeviceMatrix& index, uint32_t index_column);

}  // namespace ts
