// Run-time specialisation of the quotient kernel for one AIR: the register program produced by
// compile_air (air.cpp) is translated 1:1 into straight-line HIP source and compiled with hiprtc
// for the local GPU, so the constraint evaluation runs out of VGPRs with no instruction decode.
// The AIR is user code in the reference too (a monomorphised `Air::eval`, uni-stark/src/prover.rs:180);
// this is the GPU analogue.  If hiprtc is unavailable the interpreter in quotient.hip is used
// (also a GPU path).  libhiprtc is loaded with dlopen so that the library itself has no hard
// dependency on it.
#include "jit.hpp"

#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <sstream>

namespace ts {

namespace {

typedef void* rtcProgram;
struct Rtc {
    void* lib = nullptr;
    int (*create)(rtcProgram*, const char*, const char*, int, const char**, const char**) = nullptr;
    int (*compile)(rtcProgram, int, const char**) = nullptr;
    int (*log_size)(rtcProgram, size_t*) = nullptr;
    int (*get_log)(rtcProgram, char*) = nullptr;
    int (*code_size)(rtcProgram, size_t*) = nullptr;
    int (*get_code)(rtcProgram, char*) = nullptr;
    int (*destroy)(rtcProgram*) = nullptr;
    bool ok = false;
};

Rtc load_rtc() {
    Rtc r;
    for (const char* name : {"libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"}) {
        r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (r.lib) break;
    }
    if (!r.lib) return r;
    r.create = (decltype(r.create))dlsym(r.lib, "hiprtcCreateProgram");
    r.compile = (decltype(r.compile))dlsym(r.lib, "hiprtcCompileProgram");
    r.log_size = (decltype(r.log_size))dlsym(r.lib, "hiprtcGetProgramLogSize");
    r.get_log = (decltype(r.get_log))dlsym(r.lib, "hiprtcGetProgramLog");
    r.code_size = (decltype(r.code_size))dlsym(r.lib, "hiprtcGetCodeSize");
    r.get_code = (decltype(r.get_code))dlsym(r.lib, "hiprtcGetCode");
    r.destroy = (decltype(r.destroy))dlsym(r.lib, "hiprtcDestroyProgram");
    r.ok = r.create && r.compile && r.log_size && r.get_log && r.code_size && r.get_code && r.destroy;
    return r;
}

Rtc& rtc() {
    static Rtc r = load_rtc();  // function-local static: initialised once, thread-safe
    return r;
}

// The generated text, by what it is: the helper functions with the two argument structs (the start of every
// module), the kernel head (signature and row addressing, one for both kernel forms) and the epilogue.
const char* kHelpers = R"SRC(
typedef unsigned int u32;
typedef unsigned long long u64;
#define P 0x78000001u
__device__ __forceinline__ u32 umin32(u32 a, u32 b) { return a < b ? a : b; }
__device__ __forceinline__ u32 add(u32 a, u32 b) { u32 s = a + b; return umin32(s, s - P); }
__device__ __forceinline__ u32 sub(u32 a, u32 b) { u32 d = a - b; return umin32(d, d + P); }
__device__ __forceinline__ u32 neg(u32 a) { return a ? P - a : 0u; }
// additive form, as bb.hpp: m = -t p^-1 mod 2^32, (t + m p) / 2^32 < 2p  (mul_lo, mad_u64, sub, min)
__device__ __forceinline__ u32 mont_reduce(u64 t) {
    u32 m = (u32)t * 0x77ffffffu;
    u32 r = (u32)((t + (u64)m * P) >> 32);
    return umin32(r, r - P);
}
__device__ __forceinline__ u32 mont_mul(u32 a, u32 b) { return mont_reduce((u64)a * b); }
__device__ __forceinline__ u32 to_mont(u32 a) { return mont_mul(a, 0x45dddde3u); }
typedef u32 v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u64 lazy_fix(u64 acc) {  // high word corrected in place (bb.hpp lazy_fix)
    v2u u = __builtin_bit_cast(v2u, acc);
    u.y = umin32(u.y, u.y - P);
    return __builtin_bit_cast(u64, u);
}
__device__ __forceinline__ u32 lazy_finish(u64 acc) { return mont_reduce(lazy_fix(acc)); }
struct QC { u32 inv_zh[64]; };  // = QuotConsts
struct QO { u32* chunk[64]; };  // = QuotOut, MAX_QUOTIENT_CHUNKS
)SRC";

// What differs between the heads of k_quotient_jit and k_quotient_seg<k>; the rest of the head is one text.
struct KernelHead {
    const char* launch_bounds;
    std::string name;
    const char* extra_params;  // after row_end: the slab of a segment
    const char* row_index;     // the statements that define the row r of this thread
};

// An AIR with preprocessed columns reads a second committed matrix: two more parameters right after row_end and
// two more row pointers (row2, row3: D_LOAD's a = 2, 3).  Any other AIR's source has neither.
const char* kPrepParams = ", const u32* __restrict__ prep, u64 prep_stride";
const char* kPrepRows = "    const u32* __restrict__ row2 = prep + r;\n    const u32* __restrict__ row3 = prep + r_next;\n";

// An AIR with preprocessed AND aux columns reads a third: one more pair after the prep pair, rows row4, row5.
const char* kAuxParams = ", const u32* __restrict__ aux, u64 aux_stride";
const char* kAuxRows = "    const u32* __restrict__ row4 = aux + r;\n    const u32* __restrict__ row5 = aux + r_next;\n";

void emit_head(std::ostream& s, const KernelHead& h, bool prep, bool aux) {
    s << "extern \"C\" __global__ void __launch_bounds__(" << h.launch_bounds << ")\n" << h.name;
    s << R"SRC((const u32* __restrict__ lde, u64 col_stride, unsigned log_n, unsigned log_qd,
               const u32* __restrict__ C, const u32* __restrict__ AP, const u32* __restrict__ isf,
               const u32* __restrict__ isl, const u32* __restrict__ ist, QC qc, QO out,
               u32 row_begin, u32 row_end)SRC" << (prep ? kPrepParams : "") << (aux ? kAuxParams : "") << h.extra_params << R"SRC() {
    const unsigned L = log_n + log_qd;
    const u32 total = 1u << L;
)SRC" << h.row_index << R"SRC(    if (r >= row_end) return;
    const u32 i = L ? (__brev(r) >> (32 - L)) : 0u;
    const u32 i_next = (i + (1u << log_qd)) & (total - 1u);
    const u32 r_next = L ? (__brev(i_next) >> (32 - L)) : 0u;
    const u32* __restrict__ row0 = lde + r;
    const u32* __restrict__ row1 = lde + r_next;
    const u32 sel0 = isf[r], sel1 = isl[r], sel2 = ist[r];
)SRC";
    if (prep) s << kPrepRows;
    if (aux) s << kAuxRows;
}

const char* kAccZero = "    u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;\n";
const char* kLazyFix = "    a0 = lazy_fix(a0); a1 = lazy_fix(a1); a2 = lazy_fix(a2); a3 = lazy_fix(a3);\n";

const char* kEpilogue = R"SRC(
    a0 = lazy_fix(a0); a1 = lazy_fix(a1); a2 = lazy_fix(a2); a3 = lazy_fix(a3);
    const u32 c = log_qd ? (__brev(r >> log_n) >> (32 - log_qd)) : 0u;
    const u32 iz = qc.inv_zh[c];
    const u64 n = 1ull << log_n;
    u32* o = out.chunk[c] + (r & (n - 1));
    o[0] = mont_mul(lazy_finish(a0), iz);
    o[n] = mont_mul(lazy_finish(a1), iz);
    o[2 * n] = mont_mul(lazy_finish(a2), iz);
    o[3 * n] = mont_mul(lazy_finish(a3), iz);
}
)SRC";

// How a kernel form names the values of the program: the monolithic kernel assigns its registers in place
// (r<reg>), a segment defines each value once (const u32 v<defining instruction>).
struct Naming {
    const char* def;  // what stands before the id of a result
    const char* use;  // what stands before the id of an operand
};
const Naming kRegisters{"    r", "r"};
const Naming kValues{"    const u32 v", "v"};

// a leaf (LOAD / CONST / SEL) as an expression: it has no register operands
std::string leaf_expr(const uint32_t* ins) {
    const std::string a = std::to_string(ins[2]);
    if (ins[0] == D_LOAD)  // the row pointer is known here: rows 2, 3 are the second matrix with its own stride,
                           // rows 4, 5 the third
        return "to_mont(row" + a + "[" + std::to_string(ins[3]) +
               (ins[2] >= 4 ? "ull * aux_stride])" : ins[2] >= 2 ? "ull * prep_stride])" : "ull * col_stride])");
    return (ins[0] == D_CONST ? "C[" + a + "]" : "sel" + a);
}

// D_ASSERT: acc += value * alpha_pow[b], the sums left lazy and their high words corrected after every
// second one (bb.hpp lazy_fix)
void emit_assert(std::ostream& s, const Naming& nm, uint32_t va, uint32_t b, uint32_t& n_assert) {
    for (uint32_t q = 0; q < 4; q++)
        s << (q ? " a" : "    a") << q << " += (u64)" << nm.use << va << " * AP[" << 4 * b + q << "];";
    s << "\n";
    if (++n_assert % 2 == 0) s << kLazyFix;
}

// One instruction {op, dst, a, b}: its result is named `dst`, its register operands `va`, `vb`.
void emit_instr(std::ostream& s, const Naming& nm, const uint32_t* ins, uint32_t dst, uint32_t va, uint32_t vb,
                uint32_t& n_assert) {
    auto binary = [&](const char* fn) {
        s << nm.def << dst << " = " << fn << "(" << nm.use << va << ", " << nm.use << vb << ");\n";
    };
    switch (ins[0]) {
        case D_LOAD: case D_CONST: case D_SEL: s << nm.def << dst << " = " << leaf_expr(ins) << ";\n"; break;
        case D_ADD: binary("add"); break;
        case D_SUB: binary("sub"); break;
        case D_NEG: s << nm.def << dst << " = neg(" << nm.use << va << ");\n"; break;
        case D_MUL: binary("mont_mul"); break;
        default: emit_assert(s, nm, va, ins[3], n_assert); break;
    }
}

}  // namespace

std::string jit_quotient_source(const AirProgram& air) {
    std::ostringstream s;
    s << kHelpers;
    emit_head(s, {"256", "k_quotient_jit", "", "    const u32 r = row_begin + blockIdx.x * 256u + threadIdx.x;\n"},
              air.n_side() >= 1, air.n_side() == 2);
    s << kAccZero;
    for (uint32_t r = 0; r < air.n_regs; r++) s << "    u32 r" << r << " = 0;\n";
    uint32_t n_assert = 0;
    for (size_t pc = 0; pc < air.code.size() / 4; pc++) {
        const uint32_t* ins = &air.code[4 * pc];
        emit_instr(s, kRegisters, ins, ins[1], ins[2], ins[3], n_assert);
    }
    s << kEpilogue;
    return s.str();
}

// ---- segmented form (air.hpp SegmentPlan): one kernel per segment, values crossing a cut go through the
// slab as S[slot * slab_rows] (one u32 per row of the tile: coalesced), the accumulators as 8 words after
// lazy_fix.  Values are named v<defining instruction>; a value from an earlier segment is materialised right
// before its first use here (a slab load, or the leaf itself re-emitted).
static std::string seg_kernel(const AirProgram& air, const SegmentPlan& plan, uint32_t k) {
    const SegmentPlan::Segment& sg = plan.segs[k];
    const bool last = k + 1 == plan.segs.size();
    const uint32_t W = plan.slab_width;
    std::ostringstream s;
    s << "\n";
    emit_head(s, {"256, 4", "k_quotient_seg" + std::to_string(k), ", u32* __restrict__ slab, u32 slab_rows",
                  "    const u32 t = blockIdx.x * 256u + threadIdx.x;\n    const u32 r = row_begin + t;\n"},
              air.n_side() >= 1, air.n_side() == 2);
    s << "    u32* __restrict__ S = slab + t;\n";
    auto sl = [&](uint32_t slot) { return "S[" + std::to_string(slot) + "ull * slab_rows]"; };
    if (k == 0) {
        s << kAccZero;
    } else {
        for (int q = 0; q < 4; q++)
            s << "    u64 a" << q << " = (u64)" << sl(W + 2 * q) << " | ((u64)" << sl(W + 2 * q + 1) << " << 32);\n";
    }
    std::vector<uint32_t> slot_in(air.code.size() / 4, ~0u);
    for (const auto& li : sg.live_in) slot_in[li.def] = li.slot;
    std::vector<std::vector<const SegmentPlan::Slot*>> stores(sg.end - sg.begin);
    for (const auto& lo : sg.live_out) stores[lo.at - sg.begin].push_back(&lo);
    std::vector<uint8_t> have(air.code.size() / 4, 0);
    uint32_t n_assert = 0;
    for (uint32_t pc = sg.begin; pc < sg.end; pc++) {
        const uint32_t va = plan.opdef[2 * (size_t)pc], vb = plan.opdef[2 * (size_t)pc + 1];
        for (uint32_t v : {va, vb}) {
            if (v == ~0u || v >= sg.begin || have[v]) continue;
            have[v] = 1;
            s << kValues.def << v << " = " << (slot_in[v] != ~0u ? sl(slot_in[v]) : leaf_expr(&air.code[4 * (size_t)v])) << ";\n";
        }
        emit_instr(s, kValues, &air.code[4 * (size_t)pc], pc, va, vb, n_assert);
        for (const SegmentPlan::Slot* st : stores[pc - sg.begin]) s << "    " << sl(st->slot) << " = v" << st->def << ";\n";
    }
    if (last) {
        s << kEpilogue;
    } else {  // lazy_fix first: the next segment starts from the overflow invariant of a fresh sum
        s << kLazyFix;
        for (int q = 0; q < 4; q++)
            s << "    " << sl(W + 2 * q) << " = (u32)a" << q << "; " << sl(W + 2 * q + 1) << " = (u32)(a" << q
              << " >> 32);\n";
        s << "}\n";
    }
    return s.str();
}

uint32_t jit_segment_module_first(const SegmentPlan& plan, uint32_t n_modules, uint32_t j) {
    const uint64_t K = plan.segs.size();
    return (uint32_t)(K * j / n_modules);
}

std::vector<std::string> jit_segment_sources(const AirProgram& air, const SegmentPlan& plan, uint32_t n_modules) {
    n_modules = std::max(1u, std::min<uint32_t>(n_modules, (uint32_t)plan.segs.size()));
    std::vector<std::string> out;
    for (uint32_t j = 0; j < n_modules; j++) {
        std::string src = kHelpers;
        for (uint32_t k = jit_segment_module_first(plan, n_modules, j); k < jit_segment_module_first(plan, n_modules, j + 1); k++)
            src += seg_kernel(air, plan, k);
        out.push_back(std::move(src));
    }
    return out;
}

// ---- optional on-disk cache of code objects (TS_JIT_CACHE_DIR): the reference pays for `Air::eval` once, at
// build time; a prover process that restarts should not pay hiprtc again for an AIR it has compiled before.
// Key: 128 bits of FNV-1a over (generator version, hiprtc version, arch, source).
static const char* kGeneratorVersion = "tapstark-jit-2";  // 2: a third matrix (aux beside preprocessed columns)

std::string jit_cache_path(const std::string& src, const char* arch) {
    const char* dir = getenv("TS_JIT_CACHE_DIR");
    if (!dir || !*dir) return "";
    int major = 0, minor = 0;
    if (void* lib = rtc().lib)
        if (auto ver = (int (*)(int*, int*))dlsym(lib, "hiprtcVersion")) (void)ver(&major, &minor);
    uint64_t h1 = 0xcbf29ce484222325ull, h2 = 0x84222325cbf29ce4ull;
    auto mix = [&](const void* p, size_t n) {
        const unsigned char* b = (const unsigned char*)p;
        for (size_t i = 0; i < n; i++) {
            h1 = (h1 ^ b[i]) * 0x100000001b3ull;
            h2 = (h2 ^ (b[i] + 0x9e)) * 0x100000001b3ull;
            h2 ^= h2 >> 29;
        }
    };
    mix(kGeneratorVersion, strlen(kGeneratorVersion));
    mix(&major, sizeof major);
    mix(&minor, sizeof minor);
    mix(arch, strlen(arch));
    mix(src.data(), src.size());
    char name[96];
    snprintf(name, sizeof name, "/q_%016llx%016llx_%s.co", (unsigned long long)h1, (unsigned long long)h2, arch);
    return std::string(dir) + name;
}
bool read_file(const std::string& path, std::vector<char>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}
bool jit_cache_load(const std::string& path, std::vector<char>& code) {
    return !path.empty() && read_file(path, code) && code.size() > 64 && memcmp(code.data(), "\177ELF", 4) == 0;
}
void jit_cache_store(const std::string& path, const std::vector<char>& code) {
    if (path.empty() || code.empty()) return;
    const std::string tmp = path + ".part" + std::to_string((long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return;  // the directory must exist; a cache that cannot be written is simply not used
    const bool ok = fwrite(code.data(), 1, code.size(), f) == code.size();
    fclose(f);
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) (void)unlink(tmp.c_str());
}

bool jit_compile_source(const std::string& src, const char* arch, std::vector<char>& code, std::string& log) {
    Rtc& r = rtc();
    if (!r.ok) {
        log = "libhiprtc not available";
        return false;
    }
    if (const char* dump = getenv("TS_JIT_DUMP")) {  // the generated source, for offline inspection (hipcc -S)
        if (FILE* f = fopen(dump, "w")) {
            fwrite(src.data(), 1, src.size(), f);
            fclose(f);
        }
    }
    const std::string cached = jit_cache_path(src, arch);
    if (jit_cache_load(cached, code)) {
        log = "code object from " + cached;
        return true;
    }
    rtcProgram prog = nullptr;
    if (r.create(&prog, src.c_str(), "quotient_jit.hip", 0, nullptr, nullptr) != 0) {
        log = "hiprtcCreateProgram failed";
        return false;
    }
    std::string arch_opt = std::string("--offload-arch=") + arch;
    const char* opts[] = {arch_opt.c_str(), "-O3"};
    const int rc = r.compile(prog, 2, opts);
    size_t sz = 0;
    r.log_size(prog, &sz);
    if (sz > 1) {
        log.resize(sz);
        r.get_log(prog, &log[0]);
    }
    if (rc != 0) {
        r.destroy(&prog);
        return false;
    }
    r.code_size(prog, &sz);
    code.resize(sz);
    r.get_code(prog, code.data());
    r.destroy(&prog);
    jit_cache_store(cached, code);
    return true;
}

bool jit_load_module(const std::vector<char>& code, const std::vector<std::string>& names, JitKernelSet& set,
                     std::string& log) {
    hipModule_t mod = nullptr;
    if (hipModuleLoadData(&mod, code.data()) != hipSuccess) {
        log += " hipModuleLoadData failed";
        return false;
    }
    set.modules.push_back(mod);
    for (const std::string& name : names) {
        hipFunction_t fn = nullptr;
        if (hipModuleGetFunction(&fn, mod, name.c_str()) != hipSuccess) {
            log += " hipModuleGetFunction(" + name + ") failed";
            return false;
        }
        set.fns.push_back(fn);
    }
    return true;
}

}  // namespace ts
