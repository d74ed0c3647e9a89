// Derived trace columns in HBM: the instruction list of derive.hpp interpreted over a resident row-major matrix, one
// lane per row, one launch per call.
//
// The interpreter is quotient.hip's run_program over another instruction set: the code pointer and the program counter
// are wave-uniform, so an instruction is one scalar 16-byte load, fetched one ahead; the slot file is LDS laid out
// [slot][lane], so lane l of a wave is on bank l and nothing conflicts; the value an instruction produces stays in a
// VGPR for the next one, which nearly always reads it.  Values are field elements in Montgomery form (bb.hpp) from COL
// to the store; derive_value converts around the integer ops and nowhere else.
//
// A workgroup owns one tile of 256 consecutive rows.  It first copies the tile's untouched columns: the tile is one
// contiguous range of words in src and in out, walked word by word with consecutive lanes on consecutive words, a bit
// per out column saying whether a store owns it.  That pass also brings the tile's source lines into the cache the
// program's COL reads (one word per lane, a row apart) then hit.  Then the program runs; a store writes one word per
// lane into its column.  Neither pass reads out and both read only src, so no barrier stands between them, and every
// out word is written exactly once: by the copy if no output names its column, by one store otherwise.
// Addressing: row * width is 64-bit everywhere.
#include <string>

#include "derive.hpp"
#include "iterate.hpp"
#include "prover_internal.hpp"

namespace ts {

constexpr int DERIVE_THREADS = 256;

struct DeriveDev {
    uint64_t height;
    uint32_t src_width, out_width, n_instr;
};

__global__ void __launch_bounds__(DERIVE_THREADS)
k_derive(const uint4* __restrict__ code, const uint32_t* __restrict__ named, const DeriveDev d,
         const uint32_t* __restrict__ src, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t derive_slots[];  // [n_live][DERIVE_THREADS]
    const uint64_t r0 = (uint64_t)blockIdx.x * DERIVE_THREADS;
    const uint64_t left = d.height - r0;
    const uint32_t tile_rows = left < DERIVE_THREADS ? (uint32_t)left : DERIVE_THREADS;

    // the untouched columns, coalesced on both sides
    const uint32_t tile_words = tile_rows * d.out_width;  // <= 2^8 * 2^16
    for (uint32_t j = threadIdx.x; j < tile_words; j += DERIVE_THREADS) {
        const uint32_t lr = j / d.out_width, c = j - lr * d.out_width;
        if ((named[c >> 5] >> (c & 31)) & 1) continue;  // (a column at or beyond src_width always is)
        out[(r0 + lr) * d.out_width + c] = src[(r0 + lr) * d.src_width + c];
    }

    const bool active = threadIdx.x < tile_rows;
    const uint64_t row = active ? r0 + threadIdx.x : r0;  // an idle lane computes the tile's first row and stores nothing
    const uint32_t* rows0 = src + row * d.src_width;
    const uint32_t* rows1 = src + (row + 1 == d.height ? 0 : row + 1) * d.src_width;
    const uint32_t* rows2 = src + (row == 0 ? d.height - 1 : row - 1) * d.src_width;
    uint32_t* o = out + row * d.out_width;
    uint32_t* my = derive_slots + threadIdx.x;

    uint4 ins = code[0];
    uint32_t fwd_slot = ~0u, fwd_val = 0;
    auto rd = [&](uint32_t slot) { return slot == fwd_slot ? fwd_val : my[slot * DERIVE_THREADS]; };
    // all three row pointers read first and chosen with selects: an index into an array of them would go to scratch
    auto ld = [&](uint32_t offset, uint32_t column) {
        const uint32_t *p0 = rows0, *p1 = rows1, *p2 = rows2;
        return (offset == 0 ? p0 : offset == 1 ? p1 : p2)[column];
    };
    for (uint32_t pc = 0; pc < d.n_instr; pc++) {
        const uint4 nxt = code[pc + 1 < d.n_instr ? pc + 1 : pc];
        const uint32_t op = ins.x & 255, dst = (ins.x >> 8) & 255, stores = ins.x >> 16, y = ins.y, z = ins.z, w = ins.w;
        ins = nxt;
        if (op == V_STORE) {
            if (active) o[w] = from_mont(rd(y));
            continue;
        }
        const uint32_t v = derive_value(op, y, z, row, d.height, rd, ld);
        my[dst * DERIVE_THREADS] = v;
        fwd_slot = dst;
        fwd_val = v;
        if (stores && active) o[w] = from_mont(v);
    }
}

DeviceMatrix derive_matrix(Context& ctx, const uint32_t* program, size_t n_words, const DeviceMatrix& src) {
    const bool iterate = program && n_words && program[0] == ITERATE_MAGIC;
    StageTimer timer(&ctx, iterate ? "iterate" : "derive");
    require_resident(ctx, src, iterate ? "iterate" : "derive", "the source");
    const DeriveProgram prog = derive_lower(program, n_words, src.width);
    if (prog.iterate) return iterate_matrix(ctx, prog, src);  // the other program kind: iterate.hip

    DeviceMatrix out;
    out.buf = DevBuf<uint32_t>(&ctx, (size_t)src.height * prog.out_width);
    out.height = src.height;
    out.width = prog.out_width;
    out.layout = DeviceMatrix::ROW_MAJOR;

    // the list and the column bits in one upload through the context's page-locked arena: no wait of its own
    std::vector<uint32_t> image(prog.code);
    image.insert(image.end(), prog.named.begin(), prog.named.end());
    DevBuf<uint32_t> d_image(&ctx, image.size());
    h2d(ctx, d_image.p, image.data(), image.size() * 4);

    DeriveDev d;
    d.height = src.height;
    d.src_width = src.width;
    d.out_width = prog.out_width;
    d.n_instr = prog.n_instr();
    const dim3 grid((unsigned)((src.height + DERIVE_THREADS - 1) / DERIVE_THREADS)), block(DERIVE_THREADS);
    const size_t lds = (size_t)prog.n_live * DERIVE_THREADS * 4;  // <= 48 KiB
    TS_LAUNCH(ctx, k_derive, grid, block, lds, (const uint4*)d_image.p, (const uint32_t*)(d_image.p + prog.code.size()), d,
              (const uint32_t*)src.buf.p, out.buf.p);
    TS_HIP(hipGetLastError());
    return out;
}

}  // namespace ts
