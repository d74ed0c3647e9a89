// examples/multi_table.cpp -- two AIR tables of different heights in ONE proof, against the public C ABI only
// (include/tapstark.h + the header-only AIR capture): a FibonacciAir table of 2^10 rows and a second one of 2^6
// rows share one trace commitment, one quotient commitment and one FRI proof (ts_prove_multi, TSPF v6).  The
// proof is verified with ts_verify_multi, then refused with one public value flipped.
//
//   g++ -std=c++17 -I include examples/multi_table.cpp -L tap-stark_amd/lib -ltapstark_hip -o multi_table
//   ./multi_table
#include <stdio.h>

#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t P = 0x78000001u;

struct FibonacciAir {  // uni-stark/tests/fib_air.rs:21-57
    uint32_t width() const { return 2; }
    void eval(ts::air::Builder& builder) const {
        const auto& pis = builder.public_values();
        const auto &local = builder.local(), &next = builder.next();
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_eq(local[0], pis[0]);
        when_first_row.assert_eq(local[1], pis[1]);
        auto when_transition = builder.when_transition();
        when_transition.assert_eq(local[1], next[0]);
        when_transition.assert_eq(local[0] + local[1], next[1]);
        builder.when_last_row().assert_eq(local[1], pis[2]);
    }
};

// public values [a, b, x] of the n-row table that starts with (a, b)
std::vector<uint32_t> fib_publics(uint32_t a, uint32_t b, uint64_t n) {
    uint32_t l = a, r = b;
    for (uint64_t i = 1; i < n; i++) {
        const uint32_t nx = (uint32_t)(((uint64_t)l + r) % P);
        l = r;
        r = nx;
    }
    return {a, b, r};
}

#define CHECK(call)                                                                      \
    do {                                                                                 \
        ts_status _s = (call);                                                           \
        if (_s != TS_OK) {                                                               \
            fprintf(stderr, "%s -> status %d: %s\n", #call, (int)_s, ts_last_error(ctx)); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

}  // namespace

int main() {
    ts_ctx* ctx = nullptr;
    if (ts_ctx_create(0, &ctx) != TS_OK) {
        fprintf(stderr, "no MI355X context: %s\n", ts_last_error(nullptr));
        return 2;  // no fallback path exists
    }
    FibonacciAir fib;
    ts::air::Builder builder(fib.width(), 3);
    fib.eval(builder);
    const std::vector<uint32_t> tape = builder.tape();
    ts_air* air = nullptr;
    CHECK(ts_air_compile(ctx, tape.data(), tape.size(), &air));

    const uint64_t heights[2] = {1ull << 10, 1ull << 6};
    const uint32_t starts[2][2] = {{0, 1}, {3, 4}};
    std::vector<uint32_t> pis[2];
    ts_multi_table tables[2];
    for (int t = 0; t < 2; t++) {
        pis[t] = fib_publics(starts[t][0], starts[t][1], heights[t]);
        tables[t].struct_size = sizeof(ts_multi_table);
        tables[t].n_public = (uint32_t)pis[t].size();
        tables[t].air = air;
        tables[t].trace = nullptr;
        tables[t].public_values = pis[t].data();
        CHECK(ts_trace_fibonacci(ctx, starts[t][0], starts[t][1], heights[t], &tables[t].trace));
    }

    const ts_fri_config fri = {2, 28, 8};
    ts_challenger* challenger = nullptr;
    CHECK(ts_chal_new(0, 1, &challenger));
    std::vector<uint32_t> proof(1u << 20);
    size_t n_words = 0;
    CHECK(ts_prove_multi(ctx, &fri, challenger, tables, 2, proof.data(), proof.size(), &n_words));
    proof.resize(n_words);

    const ts_air* airs[2] = {air, air};
    const uint32_t n_public[2] = {3, 3};
    const uint32_t* values[2] = {pis[0].data(), pis[1].data()};
    ts_challenger* fresh = nullptr;
    CHECK(ts_chal_new(0, 1, &fresh));
    int verdict = -1;
    CHECK(ts_verify_multi(&fri, fresh, airs, 2, values, n_public, proof.data(), proof.size(), &verdict));

    // the short table's last public value flipped: its out-of-domain check fails (OodEvaluationMismatch)
    std::vector<uint32_t> wrong = pis[1];
    wrong[2] ^= 1;
    values[1] = wrong.data();
    ts_challenger* fresh2 = nullptr;
    CHECK(ts_chal_new(0, 1, &fresh2));
    int verdict_wrong = -1;
    CHECK(ts_verify_multi(&fri, fresh2, airs, 2, values, n_public, proof.data(), proof.size(), &verdict_wrong));

    printf("multi_table: tables of 2^10 and 2^6 rows, TSPF v%u proof of %zu words, verify -> %d, "
           "flipped public value -> %d\n", proof[1], n_words, verdict, verdict_wrong);
    ts_chal_free(challenger);
    ts_chal_free(fresh);
    ts_chal_free(fresh2);
    for (int t = 0; t < 2; t++) ts_matrix_free(ctx, tables[t].trace);
    ts_air_free(ctx, air);
    ts_ctx_destroy(ctx);
    return verdict == 0 && verdict_wrong == 7 ? 0 : 1;
}
