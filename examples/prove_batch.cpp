// examples/prove_batch.cpp -- the reference's fib_air test (uni-stark/tests/fib_air.rs:59-141) over MANY
// statements in one call of ts_prove_batch, against the public C ABI only:
//
//   generate_trace_rows(a, b, n)  fib_air.rs:59-78    N traces with different (a, b), made on the host into
//                                                     page-locked buffers (ts_host_alloc); each lane uploads
//                                                     its trace on its own stream just before the proof
//   public values [a, b, f_n]     fib_air.rs:133-139  one vector per statement
//   prove + verify                fib_air.rs:117-149  every proof verified against its own public values,
//                                                     and refused against its neighbour's
//
//   g++ -std=c++17 -pthread -I include examples/prove_batch.cpp -L tap-stark_amd/lib -ltapstark_hip -o prove_batch
//   ./prove_batch [N] [log_n] [lanes]     (defaults 16, 12, 4; exit status 0 only if every check holds)
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t P = 0x78000001u;

struct FibonacciAir {  // fib_air.rs:21-57 (the same capture as examples/fib_air.cpp)
    uint32_t width() const { return 2; }
    void eval(ts::air::Builder& builder) const {
        const auto& pis = builder.public_values();
        const auto a = pis[0], b = pis[1], x = pis[2];
        const auto &local = builder.local(), &next = builder.next();
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_eq(local[0], a);
        when_first_row.assert_eq(local[1], b);
        auto when_transition = builder.when_transition();
        when_transition.assert_eq(local[1], next[0]);
        when_transition.assert_eq(local[0] + local[1], next[1]);
        builder.when_last_row().assert_eq(local[1], x);
    }
};

}  // namespace

int main(int argc, char** argv) {
    const uint32_t N = argc > 1 ? (uint32_t)atoi(argv[1]) : 16;
    const unsigned log_n = argc > 2 ? (unsigned)atoi(argv[2]) : 12;
    const uint32_t lanes = argc > 3 ? (uint32_t)atoi(argv[3]) : 4;
    if (N < 2 || log_n < 1 || log_n > 24 || lanes < 1 || lanes > 64) {
        fprintf(stderr, "usage: prove_batch [N >= 2] [log_n in 1..24] [lanes in 1..64]\n");
        return 1;
    }
    const uint64_t n = 1ull << log_n;

    std::vector<ts_ctx*> ctxs(lanes, nullptr);
    for (uint32_t l = 0; l < lanes; l++)
        if (ts_ctx_create(0, &ctxs[l]) != TS_OK) {
            fprintf(stderr, "no MI355X context: %s\n", ts_last_error(nullptr));
            return 2;  // no fallback path exists
        }
    FibonacciAir fib;
    ts::air::Builder builder(fib.width(), 3);
    fib.eval(builder);
    const std::vector<uint32_t> tape = builder.tape();
    std::vector<ts_air*> airs(lanes, nullptr);
    for (uint32_t l = 0; l < lanes; l++)
        if (ts_air_compile(ctxs[l], tape.data(), tape.size(), &airs[l]) != TS_OK) {
            fprintf(stderr, "ts_air_compile: %s\n", ts_last_error(ctxs[l]));
            return 1;
        }
    ts_air* host_air = nullptr;  // verification needs no GPU
    if (ts_air_compile(nullptr, tape.data(), tape.size(), &host_air) != TS_OK) return 1;

    // N statements: trace i starts at (a, b) = (i, 3 i + 1); pis = [a, b, last row's right column]
    std::vector<uint32_t*> host(N, nullptr);
    std::vector<std::vector<uint32_t>> pis(N);
    for (uint32_t i = 0; i < N; i++) {
        void* p = nullptr;
        if (ts_host_alloc(n * 2 * 4, &p) != TS_OK) return 1;
        host[i] = (uint32_t*)p;
        uint32_t l = i % P, r = (3 * i + 1) % P;
        pis[i] = {l, r, 0};
        for (uint64_t k = 0; k < n; k++) {
            host[i][2 * k] = l;
            host[i][2 * k + 1] = r;
            const uint32_t nx = (uint32_t)(((uint64_t)l + r) % P);
            l = r;
            r = nx;
        }
        pis[i][2] = host[i][2 * (n - 1) + 1];
    }

    const ts_fri_config fri = {2, 28, 8};  // fib_air.rs:119-129
    const size_t cap = 1u << 20;           // far above any proof of a 2^24 x 2 trace at this configuration
    std::vector<std::vector<uint32_t>> proofs(N, std::vector<uint32_t>(cap));
    std::vector<ts_batch_item> items(N);
    for (uint32_t i = 0; i < N; i++) {
        ts_batch_item& it = items[i];
        it = ts_batch_item{};
        it.struct_size = sizeof(ts_batch_item);
        it.lane = i % lanes;
        it.host_trace = host[i];
        it.height = n;
        it.width = 2;
        it.n_public = 3;
        it.public_values = pis[i].data();
        it.proof_out = proofs[i].data();
        it.cap_words = cap;
    }
    const ts_status st = ts_prove_batch(ctxs.data(), airs.data(), lanes, &fri, items.data(), N, 0.0, TS_BATCH_DIGEST);
    bool ok = st == TS_OK;
    if (!ok) fprintf(stderr, "ts_prove_batch -> status %d\n", (int)st);

    int accepted = 0, refused = 0;
    double wall_sum = 0;
    for (uint32_t i = 0; i < N; i++) {
        const ts_batch_item& it = items[i];
        if (it.status != TS_OK) {
            fprintf(stderr, "item %u: status %d: %s\n", i, (int)it.status, ts_last_error(ctxs[it.lane]));
            ok = false;
            continue;
        }
        wall_sum += it.wall_ms;
        const std::vector<uint32_t>& other = pis[(i + 1) % N];
        int v_own = -1, v_other = -1;
        ts_challenger* c1 = nullptr;
        ts_challenger* c2 = nullptr;
        if (ts_chal_new(0, 1, &c1) != TS_OK || ts_chal_new(0, 1, &c2) != TS_OK) return 1;
        if (ts_verify(&fri, host_air, c1, proofs[i].data(), it.n_words, pis[i].data(), 3, &v_own) != TS_OK ||
            ts_verify(&fri, host_air, c2, proofs[i].data(), it.n_words, other.data(), 3, &v_other) != TS_OK)
            ok = false;
        ts_chal_free(c1);
        ts_chal_free(c2);
        accepted += v_own == 0;
        refused += v_other != 0;
        if (v_own != 0 || v_other == 0) {
            fprintf(stderr, "item %u: verify -> %d, with item %u's public values -> %d\n", i, v_own, (i + 1) % N,
                    v_other);
            ok = false;
        }
    }
    printf("prove_batch: %u statements of 2^%u rows on %u lanes, %d accepted with their own public values, "
           "%d refused with a neighbour's, mean %.3f ms per proof; proof 0: %zu words, blake3 %08x...\n",
           N, log_n, lanes, accepted, refused, wall_sum / N, items[0].n_words, items[0].proof_blake3[0]);

    for (uint32_t i = 0; i < N; i++) ts_host_free(host[i]);
    ts_air_free(nullptr, host_air);
    for (uint32_t l = 0; l < lanes; l++) {
        ts_air_free(ctxs[l], airs[l]);
        ts_ctx_destroy(ctxs[l]);
    }
    return ok ? 0 : 1;
}
