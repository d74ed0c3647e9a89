// Ingest of a trace in the form a host holds it (include/tapstark.h ts_trace_format): columns at their own
// size -- u8 / u16 / u32 -- and Montgomery words, in rows or planar, widened and reduced in HBM into the
// row-major canonical matrix everything downstream reads.  It replaces the host's pass over the trace in
// front of RowMajorMatrix::new (the `as_canonical_u32` map of a Plonky3 host; reference `as_u32_vec`,
// basic/src/field/mod.rs:48-63) and shrinks what crosses the link to the bytes the columns really have.
//
// k_ingest<PLANAR>: a workgroup takes a tile of rows (and, for very wide matrices, of columns).
//   stage   the tile's source bytes go to LDS with 16-byte loads over the raw byte range: in rows layout one
//           contiguous range per tile, rounded out to 16-byte boundaries (the base is 16-byte aligned; a
//           stride or a row size that is no multiple of 16 only moves where the rows sit in the tile);
//           planar, one range per column, each starting on a 16-byte boundary because columns do and tiles
//           begin at multiples of 16 rows.  Only the buffer's last 16 bytes can be partial: read bytewise.
//   decode  one lane per output word, consecutive lanes on consecutive words of the row-major result.  The
//           word is cut out of the two aligned LDS dwords it can straddle (a 4-byte column may sit at any
//           byte offset), masked to the column's size, Montgomery-reduced where the kind says so.
// LDS banking (ds_read_b32: bank = dword index mod 32 within 32 lanes): in rows layout consecutive lanes read
// consecutive bytes -- neighbouring or identical dwords, which broadcast.  Planar, consecutive lanes read
// columns planar_pitch() apart; the pitch keeps 16-byte alignment for the staging stores, which leaves a
// 4-way conflict on the decode reads -- an LDS rate still above what HBM takes, and this kernel is bound by
// HBM.
// A uniform 4-byte format in tight rows is the matrix word for word: the copy goes straight into the
// matrix and k_scale_words reduces it in place (nothing to stage, no second buffer).
#include <algorithm>

#include "kernels.hpp"

namespace ts {

namespace {

constexpr int INGEST_THREADS = 256;
constexpr uint32_t INGEST_TILE_BYTES = 32 * 1024;  // source bytes of one tile
constexpr uint32_t INGEST_LDS_BYTES = INGEST_TILE_BYTES + 64;  // + rounding to 16 at both ends + the straddle dword
constexpr uint32_t INGEST_TILE_COLS = 4096;        // rows layout: at most 16 KiB of one row per tile
constexpr uint32_t PLANAR_TILE_ROWS = 64;          // multiple of 16: a tile's column segments start 16-aligned

__host__ __device__ inline uint32_t kind_bytes(uint32_t kind) { return kind == COL_U8 ? 1u : kind == COL_U16 ? 2u : 4u; }
// LDS bytes from one planar column slot to the next: the column's tile rounded to 16, and 16 more for the straddle read
__host__ __device__ inline uint32_t planar_pitch(uint32_t tile_rows) { return ((4 * tile_rows + 15) & ~15u) + 16; }
// x * 2^-32 = mont_mul(x, 1), x * 2^-31 = mont_mul(x, 2): 2 x < p 2^32 for every 32-bit x
__host__ __device__ inline uint32_t monty_factor(uint32_t kind) { return kind == COL_MONTY31 ? 2u : 1u; }

struct IngestArgs {
    const uint8_t* src;
    uint64_t src_bytes;
    const uint64_t* table;  // IngestPlan::table
    uint32_t* out;
    uint64_t height;
    uint64_t stride;  // rows layout
    uint32_t width;
    uint32_t tile_rows, tile_cols;
};

// 16 bytes at src + b; past the end of the buffer (its last chunk only) byte by byte
__device__ __forceinline__ uint4 load_chunk(const uint8_t* __restrict__ src, uint64_t b, uint64_t src_bytes) {
    if (b + 16 <= src_bytes) return *reinterpret_cast<const uint4*>(src + b);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < 16 && b + k < src_bytes; k++) w[k >> 2] |= (uint32_t)src[b + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the column's value from the LDS bytes at `pos`
__device__ __forceinline__ uint32_t decode(const uint32_t* lds, uint32_t pos, uint32_t kind) {
    const uint32_t lo = lds[pos >> 2], hi = lds[(pos >> 2) + 1];
    uint32_t x = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (pos & 3)));
    if (kind == COL_U8) x &= 0xffu;
    if (kind == COL_U16) x &= 0xffffu;
    if (kind >= COL_MONTY32) x = mont_mul(x, monty_factor(kind));
    return x;
}

template <bool PLANAR>
__global__ void __launch_bounds__(INGEST_THREADS) k_ingest(IngestArgs a) {
    __shared__ uint4 lds4[INGEST_LDS_BYTES / 16];
    const uint32_t* lds = reinterpret_cast<const uint32_t*>(lds4);
    const uint32_t tid = threadIdx.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * a.tile_rows;
    const uint32_t nr = (uint32_t)(a.height - r0 < a.tile_rows ? a.height - r0 : a.tile_rows);
    const uint32_t c0 = blockIdx.y * a.tile_cols;
    const uint32_t nc = a.width - c0 < a.tile_cols ? a.width - c0 : a.tile_cols;

    uint32_t base = 0, row_step = 0;  // rows layout: LDS byte of (tile row rr, column c) = base + rr * row_step + offset(c)
    uint64_t off0 = 0;
    if (PLANAR) {
        const uint32_t per_col = (4 * a.tile_rows + 15) >> 4;  // chunk slots of one column
        const uint32_t pitch16 = planar_pitch(a.tile_rows) >> 4;
        for (uint32_t i = tid; i < nc * per_col; i += INGEST_THREADS) {
            const uint32_t j = i / per_col, k = i % per_col;
            const uint64_t e = a.table[c0 + j];
            const uint32_t s = kind_bytes((uint32_t)e & 7);
            if (16 * k < nr * s) lds4[j * pitch16 + k] = load_chunk(a.src, (e >> 3) + r0 * s + 16 * k, a.src_bytes);
        }
    } else {
        const uint64_t e_last = a.table[c0 + nc - 1];
        off0 = a.table[c0] >> 3;
        const uint64_t lo = r0 * a.stride + off0;
        const uint64_t hi = (r0 + nr - 1) * a.stride + (e_last >> 3) + kind_bytes((uint32_t)e_last & 7);
        const uint64_t alo = lo & ~(uint64_t)15;
        const uint32_t n_chunks = (uint32_t)((hi - alo + 15) >> 4);
        for (uint32_t i = tid; i < n_chunks; i += INGEST_THREADS)
            lds4[i] = load_chunk(a.src, alo + 16 * (uint64_t)i, a.src_bytes);
        base = (uint32_t)(lo - alo);
        row_step = nr > 1 ? (uint32_t)a.stride : 0;  // several rows in a tile: stride <= INGEST_TILE_BYTES
    }
    __syncthreads();

    // word i of the tile is (row i / nc, column i % nc); the lane walks i = tid, tid + 256, ... without dividing
    uint32_t rr = tid / nc, cc = tid % nc;
    const uint32_t dr = INGEST_THREADS / nc, dc = INGEST_THREADS % nc;
    while (rr < nr) {
        const uint64_t e = a.table[c0 + cc];
        const uint32_t kind = (uint32_t)e & 7;
        const uint32_t pos = PLANAR ? cc * planar_pitch(a.tile_rows) + rr * kind_bytes(kind)
                                    : base + rr * row_step + (uint32_t)((e >> 3) - off0);
        a.out[(r0 + rr) * a.width + c0 + cc] = decode(lds, pos, kind);
        rr += dr;
        cc += dc;
        if (cc >= nc) {
            cc -= nc;
            rr++;
        }
    }
}

// out[i] = in[i] * mult * 2^-32 mod p, canonical; in place allowed.  in[i] * mult < p 2^32 (mult <= 2, or mult < p).
__global__ void __launch_bounds__(256) k_scale_words(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t mult) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i = 4 * t;
    if (i + 4 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(in + i);
        *reinterpret_cast<uint4*>(out + i) =
            make_uint4(mont_mul(v.x, mult), mont_mul(v.y, mult), mont_mul(v.z, mult), mont_mul(v.w, mult));
    } else {
        for (uint64_t k = i; k < n; k++) out[k] = mont_mul(in[k], mult);
    }
}

}  // namespace

IngestPlan ingest_plan(const uint8_t* kinds, uint32_t n_kinds, bool planar, uint64_t row_stride, uint64_t height,
                       uint32_t width) {
    TS_REQUIRE(kinds != nullptr, TS_ERR_INVALID, "trace format: null kinds");
    TS_REQUIRE(width >= 1, TS_ERR_INVALID, "trace format: width 0");
    TS_REQUIRE(n_kinds == 1 || n_kinds == width, TS_ERR_INVALID, "trace format: n_kinds must be 1 or the width");
    TS_REQUIRE(height >= 1 && (height & (height - 1)) == 0, TS_ERR_INVALID,
               "trace format: height must be a power of two");
    TS_REQUIRE(height <= (1ull << 27), TS_ERR_INVALID, "trace format: height > 2^27");
    IngestPlan p;
    p.planar = planar;
    p.height = height;
    p.width = width;
    p.table.resize(width);
    bool uniform4 = true;
    uint64_t off = 0;
    for (uint32_t c = 0; c < width; c++) {
        const uint8_t kind = kinds[n_kinds == 1 ? 0 : c];
        TS_REQUIRE(kind <= COL_MONTY31, TS_ERR_INVALID, "trace format: unknown column kind");
        uniform4 = uniform4 && kind == kinds[0] && kind_bytes(kind) == 4;
        if (planar) off = (off + 15) & ~(uint64_t)15;
        p.table[c] = (off << 3) | kind;
        off += planar ? height * kind_bytes(kind) : kind_bytes(kind);
    }
    if (planar) {
        TS_REQUIRE(row_stride == 0, TS_ERR_INVALID, "trace format: row_stride is for the rows layout only");
        p.bytes = off;
    } else {
        p.stride = row_stride ? row_stride : off;
        TS_REQUIRE(p.stride >= off, TS_ERR_INVALID, "trace format: row_stride is below the bytes of a row");
        TS_REQUIRE(p.stride <= (1ull << 32), TS_ERR_INVALID, "trace format: row_stride > 2^32");
        p.bytes = height * p.stride;
        if (uniform4 && p.stride == off) p.uniform4 = kinds[0];
    }
    return p;
}

void launch_scale_words(Context& ctx, const uint32_t* in, uint32_t* out, uint64_t n, uint32_t mult) {
    if (!n) return;
    const uint64_t threads = (n + 3) / 4;
    TS_LAUNCH(ctx, k_scale_words, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, in, out, n, mult);
    TS_HIP(hipGetLastError());
}

uint32_t monty_ingest_factor(uint32_t kind) { return monty_factor(kind); }

void launch_ingest(Context& ctx, const IngestPlan& plan, const uint8_t* src, uint32_t* out) {
    IngestArgs a;
    a.src = src;
    a.src_bytes = plan.bytes;
    a.out = out;
    a.height = plan.height;
    a.stride = plan.stride;
    a.width = plan.width;
    if (plan.planar) {
        a.tile_rows = (uint32_t)std::min<uint64_t>(plan.height, PLANAR_TILE_ROWS);
        a.tile_cols = std::min(plan.width, INGEST_TILE_BYTES / planar_pitch(a.tile_rows));
    } else {
        a.tile_rows = (uint32_t)std::min<uint64_t>(plan.height, std::max<uint64_t>(1, INGEST_TILE_BYTES / plan.stride));
        a.tile_cols = std::min(plan.width, INGEST_TILE_COLS);
    }
    const uint64_t gx = (plan.height + a.tile_rows - 1) / a.tile_rows;
    const uint32_t gy = (plan.width + a.tile_cols - 1) / a.tile_cols;
    TS_REQUIRE(gy <= 65535, TS_ERR_INVALID, "packed trace: too wide");

    const size_t table_bytes = plan.table.size() * sizeof(uint64_t);
    DevBuf<uint64_t> d_table(&ctx, plan.table.size());
    // small tables go through the context's page-locked arena, so the copy never reads the caller's vector
    // late; a pageable source is copied out before hipMemcpyAsync returns
    const void* from = table_bytes <= (1u << 20) ? ctx.stage(plan.table.data(), table_bytes) : plan.table.data();
    TS_HIP(hipMemcpyAsync(d_table.p, from, table_bytes, hipMemcpyHostToDevice, ctx.stream));
    a.table = d_table.p;
    if (plan.planar)
        TS_LAUNCH(ctx, k_ingest<true>, dim3((unsigned)gx, gy), dim3(INGEST_THREADS), 0, a);
    else
        TS_LAUNCH(ctx, k_ingest<false>, dim3((unsigned)gx, gy), dim3(INGEST_THREADS), 0, a);
    TS_HIP(hipGetLastError());
}

}  // namespace ts
