#include <errno.h>
#include <stdio.h>
#include <time.h>
#include <stdlib.h>
#include "context.hpp"

#include <string.h>

#include "kernels.hpp"

namespace ts {

// TS_POOL_POISON: unset or empty = off, else a 32-bit word in any base strtoul(.., 0) reads
static bool poison_knob(uint32_t* word) {
    const char* e = getenv("TS_POOL_POISON");
    if (!e || !*e) return false;
    char* end = nullptr;
    errno = 0;
    const unsigned long v = strtoul(e, &end, 0);
    TS_REQUIRE(errno == 0 && end != e && *end == 0 && e[0] != '-' && v <= 0xFFFFFFFFul, TS_ERR_INVALID,
               "TS_POOL_POISON is not a 32-bit word (decimal, 0x hex or 0 octal)");
    *word = (uint32_t)v;
    return true;
}

Context::Context(int dev) : device(dev) {
    pool_debug = getenv("TS_POOL_DEBUG") != nullptr;
    poison_on = poison_knob(&poison_word);  // before the device is touched: a bad value is refused anywhere
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        throw Error(TS_ERR_HIP, "no HIP device available: the tap-stark HIP path has no CPU fallback");
    TS_REQUIRE(dev >= 0 && dev < count, TS_ERR_INVALID, "device index out of range");
    TS_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop;
    TS_HIP(hipGetDeviceProperties(&prop, dev));
    num_cus = prop.multiProcessorCount;
    max_lds_per_block = prop.sharedMemPerBlock;  // gfx950: 160 KiB
    arch_name = prop.gcnArchName;
    arch_name = arch_name.substr(0, arch_name.find(':'));
    TS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
}

Context::~Context() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (d_twiddle_fwd) (void)hipFree(d_twiddle_fwd);
    if (d_twiddle_inv) (void)hipFree(d_twiddle_inv);
    if (d_plant_fwd) (void)hipFree(d_plant_fwd);
    if (d_plant_inv) (void)hipFree(d_plant_inv);
    for (auto& t : scale_tables) (void)hipFree(t.d);
    for (auto& t : sel_tables)
        if (t.d) (void)hipFree(t.d);
    if (d_ticket) (void)hipFree(d_ticket);
    for (auto& kv : free_blocks) (void)hipFree(kv.second);
    for (auto& kv : live_blocks) (void)hipFree(kv.first);
    if (h_pinned) (void)hipHostFree(h_pinned);
    if (h_mailbox) (void)hipHostFree(h_mailbox);
    if (h_mailbox_big) (void)hipHostFree(h_mailbox_big);
    if (h_arena) (void)hipHostFree(h_arena);
    if (stream) (void)hipStreamDestroy(stream);
}

static size_t round_block(size_t bytes) {
    if (bytes < 512) return 512;
    if (bytes < (1u << 20)) {  // next power of two
        size_t r = 512;
        while (r < bytes) r <<= 1;
        return r;
    }
    const size_t g = 1u << 20;  // 1 MiB granules
    return (bytes + g - 1) / g * g;
}

void* Context::alloc(size_t bytes) {
    const size_t sz = round_block(bytes);
    auto it = free_blocks.find(sz);
    void* p = nullptr;
    if (it != free_blocks.end()) {
        p = it->second;
        free_blocks.erase(it);
    } else {
        TS_HIP(hipSetDevice(device));
        if (pool_debug) {
            struct timespec ts_;
            clock_gettime(CLOCK_MONOTONIC, &ts_);
            fprintf(stderr, "[ts pool %p t=%.3f ms] hipMalloc %zu KiB (reserved %zu MiB)\n", (void*)this,
                    ts_.tv_sec * 1e3 + ts_.tv_nsec * 1e-6, sz >> 10, bytes_reserved >> 20);
        }
        hipError_t e = hipMalloc(&p, sz);
        if (e != hipSuccess) {
            // drop the cache and retry once
            release_cache();
            e = hipMalloc(&p, sz);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();  // the refusal must not surface again at the next launch check
            throw Error(TS_ERR_OOM, "device allocation failed");
        }
        bytes_reserved += sz;
    }
    live_blocks[p] = sz;
    if (poison_on) poison(p, sz);
    return p;
}

// The stream is non-blocking and a block may next be written from elsewhere (another rank's stream in the
// in-process collectives, a caller's own stream through ts_matrix_device_ptr): the fill must have landed
// before the block is handed out, so it is waited for.
void Context::poison(void* p, size_t bytes) {
    TS_HIP(hipSetDevice(device));
    TS_HIP(hipMemsetD32Async((hipDeviceptr_t)p, (int)poison_word, bytes / 4, stream));
    TS_HIP(hipStreamSynchronize(stream));
    poison_fills++;
}

void Context::free(void* p) {
    if (!p) return;
    auto it = live_blocks.find(p);
    if (it == live_blocks.end()) return;
    // All work is enqueued on the single stream, so a recycled block is only touched by kernels
    // that run after every earlier user of it.
    free_blocks.emplace(it->second, p);
    live_blocks.erase(it);
}

void Context::release_cache() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto& kv : free_blocks) {
        (void)hipFree(kv.second);
        bytes_reserved -= kv.first;
    }
    free_blocks.clear();
}

uint32_t* Context::ticket() {
    if (!d_ticket) {
        TS_HIP(hipMalloc((void**)&d_ticket, 64 * 17));  // the global word + 16 group words, a line each
        TS_HIP(hipMemsetAsync(d_ticket, 0, 64 * 17, stream));
    }
    return d_ticket;
}

const void* Context::stage(const void* src, size_t bytes) {
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (need > h_arena_bytes / 2) {  // (re)allocate: rare, at most a few times per context
        sync();
        if (h_arena) (void)hipHostFree(h_arena);
        h_arena = nullptr;
        size_t sz = 1 << 20;
        while (sz / 2 < need) sz <<= 1;
        TS_HIP(hipHostMalloc((void**)&h_arena, sz, hipHostMallocDefault));
        h_arena_bytes = sz;
        h_arena_off = 0;
    }
    if (h_arena_off + need > h_arena_bytes) {  // wrap: everything staged so far must have been consumed
        sync();
        h_arena_off = 0;
    }
    void* p = h_arena + h_arena_off;
    memcpy(p, src, bytes);
    h_arena_off += need;
    return p;
}

void Context::sync_point(void* host, size_t bytes) {
    if (replay_mode == 2 && replay_pos < replay_log.size() && replay_log[replay_pos].size() == bytes) {
        memcpy(host, replay_log[replay_pos++].data(), bytes);
        return;
    }
    sync();
    if (replay_mode == 1) replay_log.emplace_back((const char*)host, (const char*)host + bytes);
}
void Context::d2h_point(void* host_dst, const void* dev_src, size_t bytes) {
    if (replay_mode == 2 && replay_pos < replay_log.size() && replay_log[replay_pos].size() == bytes) {
        memcpy(host_dst, replay_log[replay_pos++].data(), bytes);  // no copy enqueued: host_dst may die before it ran
        return;
    }
    if (bytes) TS_HIP(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, stream));
    sync();
    if (replay_mode == 1) replay_log.emplace_back((const char*)host_dst, (const char*)host_dst + bytes);
}

uint32_t* Context::mailbox(size_t words) {
    constexpr size_t WORDS = 16384;  // 64 KiB
    if (words > WORDS / 4) {
        // a message of its own size class (the opened values of a trace wider than ~500 columns): one
        // page-locked buffer grown on demand; its previous reader has synced, and growing it syncs again
        if (words > h_mailbox_big_words) {
            sync();
            if (h_mailbox_big) (void)hipHostFree(h_mailbox_big);
            h_mailbox_big = nullptr;
            h_mailbox_big_words = 0;
            TS_HIP(hipHostMalloc((void**)&h_mailbox_big, words * 4, hipHostMallocDefault));
            h_mailbox_big_words = words;
        }
        return h_mailbox_big;
    }
    if (!h_mailbox) TS_HIP(hipHostMalloc((void**)&h_mailbox, WORDS * 4, hipHostMallocDefault));
    const size_t need = (words + 15) & ~(size_t)15;
    if (mailbox_off + need > WORDS) mailbox_off = 0;  // every earlier slot has been read: its reader synced
    uint32_t* p = h_mailbox + mailbox_off;
    mailbox_off += need;
    return p;
}

void* Context::pinned(size_t bytes) {
    if (bytes > h_pinned_bytes) {
        if (h_pinned) {
            sync();
            (void)hipHostFree(h_pinned);
        }
        size_t sz = 1 << 16;
        while (sz < bytes) sz <<= 1;
        TS_HIP(hipHostMalloc(&h_pinned, sz, hipHostMallocDefault));
        h_pinned_bytes = sz;
    }
    return h_pinned;
}

std::map<std::string, std::pair<uint64_t, double>> Context::take_kernel_timings() {
    std::map<std::string, std::pair<uint64_t, double>> out;
    sync();
    for (auto& ev : kernel_events) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev.e0, ev.e1);
        auto& slot = out[ev.name];
        slot.first += 1;
        slot.second += ms;
        (void)hipEventDestroy(ev.e0);
        (void)hipEventDestroy(ev.e1);
    }
    kernel_events.clear();
    return out;
}

void Context::ensure_twiddles(unsigned log_size) {
    if (log_size <= twiddle_log && d_twiddle_fwd) return;
    TS_REQUIRE(log_size <= 27, TS_ERR_INVALID, "two-adicity of BabyBear is 27");
    sync();
    if (d_twiddle_fwd) (void)hipFree(d_twiddle_fwd);
    if (d_twiddle_inv) (void)hipFree(d_twiddle_inv);
    d_twiddle_fwd = d_twiddle_inv = nullptr;
    const size_t n = (size_t)1 << log_size;
    TS_HIP(hipMalloc((void**)&d_twiddle_fwd, n * 4));
    TS_HIP(hipMalloc((void**)&d_twiddle_inv, n * 4));
    if (poison_on) {
        poison(d_twiddle_fwd, n * 4);
        poison(d_twiddle_inv, n * 4);
    }
    twiddle_log = log_size;
    launch_build_twiddles(*this, d_twiddle_fwd, d_twiddle_inv, log_size);
}

void Context::ensure_plant_twiddles(unsigned log_fwd, unsigned log_inv) {
    auto grow = [&](uint2*& d, unsigned& have, unsigned want, bool inverse) {
        if (want <= have && d) return;
        TS_REQUIRE(want <= 27, TS_ERR_INVALID, "two-adicity of BabyBear is 27");
        sync();
        if (d) (void)hipFree(d);
        d = nullptr;
        const size_t n = (size_t)1 << want;
        TS_HIP(hipMalloc((void**)&d, n * 8));
        if (poison_on) poison(d, n * 8);
        have = want;
        launch_build_plant_twiddles(*this, d, want, inverse);
    };
    if (log_fwd) grow(d_plant_fwd, plant_fwd_log, log_fwd, false);
    if (log_inv) grow(d_plant_inv, plant_inv_log, log_inv, true);
}

}  // namespace ts
