// Field probe: every primitive of csrc/bb.hpp, and the register butterflies of csrc/ntt_rounds.hpp (on the
// Montgomery table type, ops 32-35, and on the Plantard one, ops 48-51: tests/_plantard_cases.py), applied to
// operands chosen by a test and written back word for word, so that tests/_field_cases.py can compare the
// host build (--host, no HIP call: runs without a GPU) and the device build of the SAME source with plain
// Python integer arithmetic.  Built beside the library by tapstark_amd.build (lib/field_probe).
//
//   field_probe [--host] <operands> <results>
//
// Operand file (u32 words): MAGIC, n_records, then per record  op, count, n_in, n_out, in[count * n_in].
// Result file:              MAGIC, n_records, then per record  op, count, n_out, out[count * n_out].
// One record per op; in device mode a record is ONE kernel launch (item i on thread i), then the program exits.
// Exit status: 0 done, 2 usage / file / malformed record, 3 no HIP device, 4 HIP error.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bb.hpp"
#include "ntt_rounds.hpp"

using namespace ts;

namespace {

constexpr uint32_t MAGIC = 0x42465042u;  // "BPFB"

enum Op : uint32_t {
    OP_CONSTS = 0,      // 1 -> 8   P, P_INV, P_NEG_INV, R_MOD_P, R2_MOD_P, GENERATOR, TWO_ADIC_GEN_27, EF_W
    OP_ADD = 1,         // 2 -> 1
    OP_SUB = 2,         // 2 -> 1
    OP_NEG = 3,         // 1 -> 1
    OP_RED2P = 4,       // 1 -> 1
    OP_MONT_REDUCE = 5, // lo, hi -> 1
    OP_MONT_MUL = 6,    // 2 -> 1
    OP_TO_MONT = 7,     // 1 -> 1
    OP_FROM_MONT = 8,   // 1 -> 1
    OP_MUL = 9,         // 2 -> 1
    OP_MONT_INV = 10,   // 1 -> 1
    OP_INV_CANON = 11,  // 1 -> 1
    OP_MONT_MUL_LAZY = 12,  // 2 -> 1
    // acc_lo, acc_hi, n (<= 8), fix_mask, (a, b) x 8  ->  acc_lo, acc_hi, lazy_finish(acc):
    // for i < n: acc = lazy_mac(acc, a_i, b_i); if fix_mask bit i: acc = lazy_fix(acc)
    OP_LAZY = 13,       // 20 -> 3
    OP_EF_ADD = 14,     // 8 -> 4
    OP_EF_SUB = 15,     // 8 -> 4
    OP_EF_NEG = 16,     // 4 -> 4
    OP_EF_MUL = 17,     // 8 -> 4
    OP_EF_MUL_BASE = 18,   // 5 -> 4
    OP_EF_INV_PARTS = 19,  // 4 -> 5  num[4], nrm
    OP_EF_INV = 20,     // 4 -> 4
    OP_EF_POW = 21,     // a[4], e_lo, e_hi -> 4
    OP_BITREV = 22,     // x, bits -> 1
    OP_TWO_ADIC_GEN = 23,  // bits -> 1
    OP_POW_CANON = 24,  // a, e_lo, e_hi -> 1
    OP_MONT_POW = 25,   // a, e_lo, e_hi -> 1
    N_SCALAR_OPS = 26,
    // device only: v[16], W[16] -> v[16]; radix_butterflies<4, INV, TOP>(v, 0, 0, 0, 0, W)
    OP_BFLY = 32,       // + (INV ? 1 : 0) + (TOP ? 2 : 0)
    OP_BFLY_END = 36,
    // the Plantard product (bb.hpp), host and device
    OP_PLANT_CONSTS = 40,  // 1 -> 2   P_INV64 lo, hi
    OP_PLANT_CONST = 41,   // w -> 2   plant_const(w) lo, hi
    OP_PLANT_MUL = 42,     // a, w -> 1   plant_mul(a, plant_const(w))
    // device only: v[16], W'[16] as {lo, hi} pairs -> v[16]; radix_butterflies<4, INV, TOP>(v, 0, 0, 0, 0, W') on the
    // Plantard table type
    OP_PLANT_BFLY = 48,    // + (INV ? 1 : 0) + (TOP ? 2 : 0)
    OP_PLANT_BFLY_END = 52,
};
constexpr bool device_only(uint32_t op) {
    return (op >= OP_BFLY && op < OP_BFLY_END) || (op >= OP_PLANT_BFLY && op < OP_PLANT_BFLY_END);
}

struct Shape {
    uint32_t n_in, n_out;
};
TS_HD Shape shape_of(uint32_t op) {
    switch (op) {
        case OP_CONSTS: return {1, 8};
        case OP_ADD: case OP_SUB: case OP_MONT_REDUCE: case OP_MONT_MUL: case OP_MUL: case OP_MONT_MUL_LAZY:
        case OP_BITREV: return {2, 1};
        case OP_NEG: case OP_RED2P: case OP_TO_MONT: case OP_FROM_MONT: case OP_MONT_INV: case OP_INV_CANON:
        case OP_TWO_ADIC_GEN: return {1, 1};
        case OP_LAZY: return {20, 3};
        case OP_EF_ADD: case OP_EF_SUB: case OP_EF_MUL: return {8, 4};
        case OP_EF_NEG: case OP_EF_INV: return {4, 4};
        case OP_EF_MUL_BASE: return {5, 4};
        case OP_EF_INV_PARTS: return {4, 5};
        case OP_EF_POW: return {6, 4};
        case OP_POW_CANON: case OP_MONT_POW: return {3, 1};
        case OP_PLANT_CONSTS: case OP_PLANT_CONST: return {1, 2};
        case OP_PLANT_MUL: return {2, 1};
        default:
            return (op >= OP_BFLY && op < OP_BFLY_END)               ? Shape{32, 16}
                   : (op >= OP_PLANT_BFLY && op < OP_PLANT_BFLY_END) ? Shape{48, 16}
                                                                     : Shape{0, 0};
    }
}

TS_HD Ef ef_at(const uint32_t* p) { return Ef{{p[0], p[1], p[2], p[3]}}; }
TS_HD void ef_put(uint32_t* p, Ef e) {
    for (int k = 0; k < 4; k++) p[k] = e.c[k];
}
TS_HD uint64_t u64_at(const uint32_t* p) { return (uint64_t)p[0] | ((uint64_t)p[1] << 32); }

// one item of a scalar op: the same text is the host and the device build of every primitive
TS_HD void apply(uint32_t op, const uint32_t* in, uint32_t* out) {
    switch (op) {
        case OP_CONSTS:
            out[0] = P; out[1] = P_INV; out[2] = P_NEG_INV; out[3] = R_MOD_P; out[4] = R2_MOD_P;
            out[5] = GENERATOR; out[6] = TWO_ADIC_GEN_27; out[7] = EF_W;
            break;
        case OP_ADD: out[0] = add(in[0], in[1]); break;
        case OP_SUB: out[0] = sub(in[0], in[1]); break;
        case OP_NEG: out[0] = neg(in[0]); break;
        case OP_RED2P: out[0] = red2p(in[0]); break;
        case OP_MONT_REDUCE: out[0] = mont_reduce(u64_at(in)); break;
        case OP_MONT_MUL: out[0] = mont_mul(in[0], in[1]); break;
        case OP_TO_MONT: out[0] = to_mont(in[0]); break;
        case OP_FROM_MONT: out[0] = from_mont(in[0]); break;
        case OP_MUL: out[0] = mul(in[0], in[1]); break;
        case OP_MONT_INV: out[0] = mont_inv(in[0]); break;
        case OP_INV_CANON: out[0] = inv_canon(in[0]); break;
        case OP_MONT_MUL_LAZY: out[0] = mont_mul_lazy(in[0], in[1]); break;
        case OP_LAZY: {
            uint64_t acc = u64_at(in);
            const uint32_t n = in[2] < 8 ? in[2] : 8, mask = in[3];
            for (uint32_t i = 0; i < n; i++) {
                acc = lazy_mac(acc, in[4 + 2 * i], in[5 + 2 * i]);
                if ((mask >> i) & 1u) acc = lazy_fix(acc);
            }
            out[0] = (uint32_t)acc;
            out[1] = (uint32_t)(acc >> 32);
            out[2] = lazy_finish(acc);
            break;
        }
        case OP_EF_ADD: ef_put(out, ef_add(ef_at(in), ef_at(in + 4))); break;
        case OP_EF_SUB: ef_put(out, ef_sub(ef_at(in), ef_at(in + 4))); break;
        case OP_EF_NEG: ef_put(out, ef_neg(ef_at(in))); break;
        case OP_EF_MUL: ef_put(out, ef_mul(ef_at(in), ef_at(in + 4))); break;
        case OP_EF_MUL_BASE: ef_put(out, ef_mul_base(ef_at(in), in[4])); break;
        case OP_EF_INV_PARTS: {
            Ef num;
            uint32_t nrm;
            ef_inv_parts(ef_at(in), num, nrm);
            ef_put(out, num);
            out[4] = nrm;
            break;
        }
        case OP_EF_INV: ef_put(out, ef_inv(ef_at(in))); break;
        case OP_EF_POW: ef_put(out, ef_pow(ef_at(in), u64_at(in + 4))); break;
        case OP_BITREV: out[0] = bitrev32(in[0], in[1]); break;
        case OP_TWO_ADIC_GEN: out[0] = two_adic_generator(in[0]); break;
        case OP_POW_CANON: out[0] = pow_canon(in[0], u64_at(in + 1)); break;
        case OP_MONT_POW: out[0] = mont_pow(in[0], u64_at(in + 1)); break;
        case OP_PLANT_CONSTS: out[0] = (uint32_t)P_INV64; out[1] = (uint32_t)(P_INV64 >> 32); break;
        case OP_PLANT_CONST: {
            const uint64_t w = plant_const(in[0]);
            out[0] = (uint32_t)w;
            out[1] = (uint32_t)(w >> 32);
            break;
        }
        case OP_PLANT_MUL: out[0] = plant_mul(in[0], plant_const(in[1])); break;
        default: break;
    }
}

__global__ void __launch_bounds__(256) k_probe(uint32_t op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                               uint32_t count, uint32_t n_in, uint32_t n_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    apply(op, in + (size_t)i * n_in, out + (size_t)i * n_out);
}

template <bool INV, bool TOP>
__global__ void __launch_bounds__(256) k_probe_bfly(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                    uint32_t count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    uint32_t v[16];
    for (int q = 0; q < 16; q++) v[q] = in[(size_t)i * 32 + q];
    radix_butterflies<4, INV, TOP>(v, 0, 0, 0, 0, in + (size_t)i * 32 + 16);
    for (int q = 0; q < 16; q++) out[(size_t)i * 16 + q] = v[q];
}

template <bool INV, bool TOP>
__global__ void __launch_bounds__(256) k_probe_plant_bfly(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                          uint32_t count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    uint32_t v[16];
    for (int q = 0; q < 16; q++) v[q] = in[(size_t)i * 48 + q];
    // 48 words an item, the table 16 words in: 8-byte aligned
    radix_butterflies<4, INV, TOP>(v, 0, 0, 0, 0, reinterpret_cast<const uint2*>(in + (size_t)i * 48 + 16));
    for (int q = 0; q < 16; q++) out[(size_t)i * 16 + q] = v[q];
}

bool read_words(const char* path, std::vector<uint32_t>& w) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (sz < 0 || sz % 4) {
        fclose(f);
        return false;
    }
    w.resize((size_t)sz / 4);
    const bool ok = fread(w.data(), 4, w.size(), f) == w.size();
    fclose(f);
    return ok;
}

#define HIP_OR_FAIL(call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "field_probe: %s: %s\n", #call, hipGetErrorString(e_));            \
            return 4;                                                                          \
        }                                                                                      \
    } while (0)

// one record on the device: upload, ONE launch, download
int run_device(uint32_t op, const uint32_t* in, uint32_t* out, uint32_t count, Shape sh) {
    uint32_t *d_in = nullptr, *d_out = nullptr;
    const size_t in_bytes = (size_t)count * sh.n_in * 4, out_bytes = (size_t)count * sh.n_out * 4;
    HIP_OR_FAIL(hipMalloc(&d_in, in_bytes));
    HIP_OR_FAIL(hipMalloc(&d_out, out_bytes));
    HIP_OR_FAIL(hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice));
    HIP_OR_FAIL(hipMemset(d_out, 0xff, out_bytes));
    const dim3 grid((count + 255) / 256), block(256);
    switch (op) {
        case OP_BFLY + 0: k_probe_bfly<false, false><<<grid, block>>>(d_in, d_out, count); break;
        case OP_BFLY + 1: k_probe_bfly<true, false><<<grid, block>>>(d_in, d_out, count); break;
        case OP_BFLY + 2: k_probe_bfly<false, true><<<grid, block>>>(d_in, d_out, count); break;
        case OP_BFLY + 3: k_probe_bfly<true, true><<<grid, block>>>(d_in, d_out, count); break;
        case OP_PLANT_BFLY + 0: k_probe_plant_bfly<false, false><<<grid, block>>>(d_in, d_out, count); break;
        case OP_PLANT_BFLY + 1: k_probe_plant_bfly<true, false><<<grid, block>>>(d_in, d_out, count); break;
        case OP_PLANT_BFLY + 2: k_probe_plant_bfly<false, true><<<grid, block>>>(d_in, d_out, count); break;
        case OP_PLANT_BFLY + 3: k_probe_plant_bfly<true, true><<<grid, block>>>(d_in, d_out, count); break;
        default: k_probe<<<grid, block>>>(op, d_in, d_out, count, sh.n_in, sh.n_out); break;
    }
    HIP_OR_FAIL(hipGetLastError());
    HIP_OR_FAIL(hipDeviceSynchronize());
    HIP_OR_FAIL(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    HIP_OR_FAIL(hipFree(d_in));
    HIP_OR_FAIL(hipFree(d_out));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    bool host = false;
    const char* paths[2] = {nullptr, nullptr};
    int n_paths = 0;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--host")) host = true;
        else if (n_paths < 2) paths[n_paths++] = argv[i];
        else n_paths = 3;
    }
    if (n_paths != 2) {
        fprintf(stderr, "usage: field_probe [--host] <operands> <results>\n");
        return 2;
    }
    std::vector<uint32_t> in;
    if (!read_words(paths[0], in) || in.size() < 2 || in[0] != MAGIC) {
        fprintf(stderr, "field_probe: cannot read operand file %s\n", paths[0]);
        return 2;
    }
    if (!host) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) {
            fprintf(stderr, "field_probe: no HIP device (use --host for the host build of the primitives)\n");
            return 3;
        }
        HIP_OR_FAIL(hipSetDevice(0));
    }
    std::vector<uint32_t> res{MAGIC, in[1]};
    size_t pos = 2;
    for (uint32_t r = 0; r < in[1]; r++) {
        if (pos + 4 > in.size()) {
            fprintf(stderr, "field_probe: record %u: truncated header\n", r);
            return 2;
        }
        const uint32_t op = in[pos], count = in[pos + 1];
        const Shape sh = shape_of(op);
        if (sh.n_in == 0 || in[pos + 2] != sh.n_in || in[pos + 3] != sh.n_out || count == 0 ||
            (size_t)count * sh.n_in > in.size() - (pos + 4)) {
            fprintf(stderr, "field_probe: record %u: op %u with %u x (%u -> %u) words is malformed\n", r, op, count,
                    in[pos + 2], in[pos + 3]);
            return 2;
        }
        if (host && device_only(op)) {
            fprintf(stderr, "field_probe: record %u: op %u exists in the device build only\n", r, op);
            return 2;
        }
        const uint32_t* src = &in[pos + 4];
        res.insert(res.end(), {op, count, sh.n_out});
        const size_t at = res.size();
        res.resize(at + (size_t)count * sh.n_out, 0xffffffffu);
        if (host) {
            for (uint32_t i = 0; i < count; i++) apply(op, src + (size_t)i * sh.n_in, &res[at + (size_t)i * sh.n_out]);
        } else if (int rc = run_device(op, src, &res[at], count, sh)) {
            return rc;
        }
        pos += 4 + (size_t)count * sh.n_in;
    }
    FILE* f = fopen(paths[1], "wb");
    if (!f || fwrite(res.data(), 4, res.size(), f) != res.size() || fclose(f) != 0) {
        fprintf(stderr, "field_probe: cannot write %s\n", paths[1]);
        return 2;
    }
    return 0;
}
