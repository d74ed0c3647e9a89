// Scanned trace columns: first-order linear recurrences y[i] = a[i] y[i-1] + b[i] over BabyBear down the rows of a
// resident row-major matrix (include/tapstark.h "scanned columns"), optionally started over where a reset column is
// not zero.  The affine maps x -> a x + b compose associatively, so every scan of a call is one parallel scan over
// pairs of field elements: the operator is written once here, for the three kernels of scan.hip.  scan.cpp holds the
// checks and the plain sequential loop over host rows.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bb.hpp"

namespace ts {

constexpr uint32_t SCAN_MAX_COLUMNS = 8;
constexpr uint32_t SCAN_NO_RESET = 0xFFFFFFFFu;
constexpr uint32_t SCAN_EXCLUSIVE = 1;
constexpr uint32_t SCAN_MAX_WIDTH = 1u << 16;  // as derive and the sort: height * width stays below 2^43 words
constexpr uint64_t SCAN_MAX_HEIGHT = 1ull << 27;

// One scan, as the caller wrote it (ts_scan_column, field for field).
struct ScanColumn {
    uint32_t a_kind, a_value, b_kind, b_value;  // kind 0: the constant `value` < p; 1: column `value` of src
    uint32_t init, reset_column, dst_column, flags;
};

struct ScanSpec {
    std::vector<ScanColumn> columns;
    uint32_t out_width = 0;  // 0: max(src_width, 1 + max dst_column)
};

// What the checks leave: the width of the result and which of its columns a scan writes.
struct ScanPlan {
    uint32_t src_width = 0, out_width = 0;
    std::vector<uint32_t> named;  // bit c: out column c is a dst (else copied from src)
};

// Every rule that needs no matrix; throws TS_ERR_INVALID with a text.
ScanPlan scan_check(const ScanSpec& spec, uint32_t src_width);
// out (height x out_width, row-major) from src (height x src_width): the sequential loop, plain integers mod p.
// finals (spec.columns.size() words, y[h-1] of each) may be null.
void scan_rows_host(const ScanSpec& spec, const ScanPlan& plan, const uint32_t* src, uint64_t height, uint32_t* out,
                    uint32_t* finals);
// A new row-major matrix of src's height and the plan's out_width (scan.hip).  `src` is row-major, on ctx, read only.
// Throws TS_ERR_INVALID before any device work.  Three launches; no host wait unless `finals` is given, then one.
struct Context;
struct DeviceMatrix;
DeviceMatrix scan_matrix(Context& ctx, const ScanSpec& spec, const DeviceMatrix& src, uint32_t* finals);

// ---- the operator (host and device) -------------------------------------------------------------------------
// x -> a x + b, both in Montgomery form.
struct ScanMap {
    uint32_t a, b;
};
TS_HD ScanMap scan_identity() { return ScanMap{R_MOD_P, 0u}; }
// `later` after `earlier`: (a2, b2) o (a1, b1) = (a2 a1, a2 b1 + b2)
TS_HD ScanMap scan_compose(ScanMap later, ScanMap earlier) {
    return ScanMap{mont_mul(later.a, earlier.a), add(mont_mul(later.a, earlier.b), later.b)};
}
TS_HD uint32_t scan_apply(ScanMap m, uint32_t x) { return add(mont_mul(m.a, x), m.b); }
// The map of one row from its stored words (any 32-bit word: to_mont reduces it).  A reset row is the constant map
// (0, a init + b): what came before is multiplied away, so the scan itself has no branch for it.
TS_HD ScanMap scan_row_map(uint32_t a_m, uint32_t b_m, bool reset, uint32_t init_m) {
    return reset ? ScanMap{0u, add(mont_mul(a_m, init_m), b_m)} : ScanMap{a_m, b_m};
}

}  // namespace ts
