// Per-GPU context of the tap-stark HIP library: stream, caching device allocator, twiddle tables,
// error reporting.  One context is driven by one host thread (SURVEY.md section 8(b) Threading).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "bb.hpp"

namespace ts {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// fri/src/prover.rs:129-134 `assert_eq!(x, final_poly)`: its own type so that a caller that can take
// another route (prove_sharded's local quotient) can tell it from every other invariant
struct FinalPolyNotConstant : Error {
    explicit FinalPolyNotConstant(const std::string& m) : Error(5 /* TS_ERR_INVARIANT */, m) {}
};

// status codes of the C ABI (include/tapstark.h)
enum : int {
    TS_OK = 0,
    TS_ERR_INVALID = 1,    // bad argument / shape
    TS_ERR_HIP = 2,        // HIP runtime failure
    TS_ERR_OOM = 3,        // device allocation failed
    TS_ERR_UNSUPPORTED = 4,
    TS_ERR_INVARIANT = 5,  // the reference would have panicked (assert/expect)
    TS_ERR_BUFFER = 6,     // output buffer too small
    TS_ERR_COMM = 7,       // a communicator callback failed
};

#define TS_HIP(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            throw ts::Error(ts::TS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#define TS_REQUIRE(cond, code, msg)                   \
    do {                                              \
        if (!(cond)) throw ts::Error((code), (msg));  \
    } while (0)

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string last_error;
    int num_cus = 256;
    size_t max_lds_per_block = 64 * 1024;
    std::string arch_name;  // "gfx950"

    // caching allocator: blocks are rounded up and recycled by exact rounded size
    std::multimap<size_t, void*> free_blocks;
    std::map<void*, size_t> live_blocks;
    size_t bytes_reserved = 0;
    bool pool_debug = false;  // TS_POOL_DEBUG, read once by the constructor: alloc reads no environment
    // TEST KNOB TS_POOL_POISON=<32-bit word>, read once by the constructor: every block the pool hands out
    // (the whole rounded block) and every table allocated beside it is first filled with the word, so that a
    // kernel or driver that leaves something unwritten, or reads past what was written, can no longer find
    // the right words there from an earlier use (tests/test_gpu_pool_poison.py).  Off: one branch per block.
    bool poison_on = false;
    uint32_t poison_word = 0;
    uint64_t poison_fills = 0;  // blocks filled since creation (ts_ctx_stat 9)
    void poison(void* p, size_t bytes);

    // twiddle tables in bit-reversed block order (kernels_ntt.hip): W[m + i] = w_{2m}^bitrev(i),
    // Montgomery form; index 0 unused.  Grown on demand, never shrunk.
    uint32_t* d_twiddle_fwd = nullptr;
    uint32_t* d_twiddle_inv = nullptr;
    unsigned twiddle_log = 0;
    // the same twiddles as Plantard words {low, high} (bb.hpp plant_const), for the NTT passes alone
    // (ntt_rounds.hpp), each direction with a size of its own: the inverse table by the longest TRANSFORM asked
    // for (log_n), the forward one by the longest LDE (log_n + log_blowup: the forward passes of coset beta
    // take block beta's stages of the N-point transform, ntt_lde.hip) -- 8 MB and 32 MB at 2^20 x blowup 4
    uint2* d_plant_fwd = nullptr;
    uint2* d_plant_inv = nullptr;
    unsigned plant_fwd_log = 0, plant_inv_log = 0;

    // scale tables of the LDE (ntt_lde.hip): T[k] = shift^k / n for one (log_n, shift); a trace commit
    // asks for the same one every proof, so a few are kept
    struct ScaleTable {
        unsigned log_n;
        uint32_t shift;
        uint32_t* d;
        size_t words;
        uint64_t last_use;
    };
    std::vector<ScaleTable> scale_tables;
    uint64_t scale_clock = 0;
    // the last selector table (is_first | is_last | is_transition on the quotient domain,
    // quotient.hip): a function of (log_n, log_qd) only, so repeated proofs of one shape reuse it
    // selector tables (quotient.hip) by (log_n, log_qd, domain shift): two entries, so that a context
    // that alternates between the reference shift (prove, the broadcast path) and a rank's own
    // (local quotient) rebuilds neither -- a rebuild is a stream sync, a hipFree and a hipMalloc
    struct SelTable {
        uint32_t* d = nullptr;
        unsigned log_n = ~0u, log_qd = ~0u;
        uint32_t shift = 0;
        uint64_t last_use = 0;
    };
    SelTable sel_tables[2];
    uint64_t sel_clock = 0;

    // zero-initialised words (17 lines of 64 bytes) the "last workgroup done" kernels count in
    // (merkle.hip); each kernel leaves them at zero, and launches on the one stream run in order
    uint32_t* d_ticket = nullptr;
    uint32_t* ticket();

    // measurement only (ts_bench_stage): which of the three LDE passes coset_lde launches (bit 0 inverse
    // contiguous, 1 strided middle, 2 forward contiguous); 7 everywhere else
    unsigned lde_pass_mask = 7;

    // Mailbox: a page of page-locked host memory that kernels write small results into directly (a
    // Merkle root, the opened-value sums): the host reads them after a stream sync, with no copy
    // kernel in between (a D2H hipMemcpyAsync of 32 bytes is a launch of its own: ~7 us of a proof's
    // critical path each time).  Slots are handed out round-robin; a slot is only reused after the
    // sync that read it.
    uint32_t* h_mailbox = nullptr;
    size_t mailbox_off = 0;
    uint32_t* h_mailbox_big = nullptr;  // messages above a quarter of the page: one at a time
    size_t h_mailbox_big_words = 0;
    uint32_t* mailbox(size_t words);

    // pinned host staging
    void* h_pinned = nullptr;
    size_t h_pinned_bytes = 0;
    // page-locked bump arena for small host->device uploads (challenge powers, index lists,
    // pointer tables): the bytes are copied here first, so the async copy never reads a caller's
    // stack or vector and no sync is needed to protect them.  When full: one sync, then reuse.
    char* h_arena = nullptr;
    size_t h_arena_bytes = 0, h_arena_off = 0;
    const void* stage(const void* src, size_t bytes);

    // optional per-stage timing (bench.py): name -> accumulated ms, measured with HIP events on
    // `stream`
    bool timing = false;
    std::vector<std::pair<std::string, float>> stage_ms;

    // optional per-kernel timing: HIP events recorded on `stream` around every launch, resolved
    // lazily (no sync per kernel) by take_kernel_timings()
    struct KernelEvent {
        const char* name;
        hipEvent_t e0, e1;
    };
    bool kernel_timing = false;
    std::vector<KernelEvent> kernel_events;
    // name -> (launch count, total ms)
    std::map<std::string, std::pair<uint64_t, double>> take_kernel_timings();

    // fri_pow_witness (prover.cpp): witnesses taken from the device search after the host's one-step check,
    // device candidates the host refused (never expected), and searches run on the host
    uint64_t pow_hints_accepted = 0, pow_hints_rejected = 0, pow_host_grinds = 0;
    uint64_t local_quotient_fallbacks = 0;    // prove_sharded: local quotient -> broadcast path (invalid trace)

    explicit Context(int dev);
    ~Context();
    Context(const Context&) = delete;

    void* alloc(size_t bytes);
    void free(void* p);
    template <class T>
    T* alloc_n(size_t n) { return static_cast<T*>(alloc(n * sizeof(T))); }
    void release_cache();

    // MEASUREMENT AID (ts_ctx_set_replay, tools/latency_replay.py): what would a proof cost if the host never
    // had to wait for the device -- the ceiling of a "zero-host-sync" design?  Mode 1 records, at every point
    // where prove() synchronises to read a small device result (two commitment roots, the opened-value sums,
    // the FRI block), the bytes it read; mode 2 proves the SAME trace again without those synchronisations,
    // handing the host the recorded bytes at once (the device still computes and writes the same values).
    // The proof must come out identical; only the final gather still synchronises.
    int replay_mode = 0;
    size_t replay_pos = 0;
    std::vector<std::vector<char>> replay_log;
    void sync_point(void* host, size_t bytes);                        // host memory a kernel wrote (mailbox)
    void d2h_point(void* host_dst, const void* dev_src, size_t bytes);  // an async copy + sync
    void* pinned(size_t bytes);
    void ensure_twiddles(unsigned log_size);
    // forward table for 2^log_fwd points, inverse for 2^log_inv; 0 = that direction is not asked for
    void ensure_plant_twiddles(unsigned log_fwd, unsigned log_inv);
    // what a prover asks for once, before its first launch, so that no table is rebuilt between two launches
    // of a proof: the Montgomery tables and the Plantard forward table over the whole LDE domain
    void ensure_lde_twiddles(unsigned log_N) {
        ensure_twiddles(log_N);
        ensure_plant_twiddles(log_N, 0);
    }
    // (polling hipStreamQuery instead was measured and made no difference: profiles/r06_sync_spin_ab.txt)
    void sync() { TS_HIP(hipStreamSynchronize(stream)); }
};

// RAII device buffer from the context's pool
template <class T>
struct DevBuf {
    Context* ctx = nullptr;
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(Context* c, size_t count) : ctx(c), p(c->alloc_n<T>(count)), n(count) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : ctx(o.ctx), p(o.p), n(o.n) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            ctx = o.ctx; p = o.p; n = o.n; o.p = nullptr;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) ctx->free(p);
        p = nullptr;
    }
};

// Brackets one kernel launch with events when per-kernel timing is on (bench.py's roofline leg).
struct KernelTimer {
    Context* ctx;
    Context::KernelEvent ev;
    bool on;
    KernelTimer(Context* c, const char* name) : ctx(c), on(c->kernel_timing) {
        if (on) {
            ev.name = name;
            (void)hipEventCreate(&ev.e0);
            (void)hipEventCreate(&ev.e1);
            (void)hipEventRecord(ev.e0, ctx->stream);
        }
    }
    ~KernelTimer() {
        if (on) {
            (void)hipEventRecord(ev.e1, ctx->stream);
            ctx->kernel_events.push_back(ev);
        }
    }
};

// The timer's name is what bench.py and the profile tools look a kernel up by: the kernel as spelled at
// the launch, or `name` where a template argument would spell it differently (k_leaf_hash, k_leaf_tree).
#define TS_LAUNCH_NAMED(ctx, name, kernel, grid, block, lds, ...)                   \
    do {                                                                            \
        ts::KernelTimer _kt(&(ctx), name);                                          \
        hipLaunchKernelGGL(kernel, grid, block, lds, (ctx).stream, __VA_ARGS__);    \
    } while (0)
#define TS_LAUNCH(ctx, kernel, ...) TS_LAUNCH_NAMED(ctx, #kernel, kernel, __VA_ARGS__)

struct StageTimer {
    Context* ctx;
    const char* name;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    StageTimer(Context* c, const char* n) : ctx(c), name(n) {
        if (ctx->timing) {
            (void)hipEventCreate(&e0);
            (void)hipEventCreate(&e1);
            (void)hipEventRecord(e0, ctx->stream);
        }
    }
    ~StageTimer() {
        if (ctx->timing && e0) {
            (void)hipEventRecord(e1, ctx->stream);
            (void)hipEventSynchronize(e1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e0, e1);
            ctx->stage_ms.emplace_back(name, ms);
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
        }
    }
};

}  // namespace ts
