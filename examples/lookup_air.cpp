// examples/lookup_air.cpp -- an AIR with challenge-phase columns, end to end over the public C ABI: the
// RangeLookupAir of tap-stark_amd/airs.py (a LogUp range check) captured with include/tapstark_air.hpp, proved
// with ts_prove_aux through a C callback that builds the LogUp columns on the device (ts_logup_aux_build),
// verified with a fresh challenger, and the statement about the exposed sum -- it is zero -- checked by the
// caller, whose job that is.
//
//   g++ -std=c++17 -I include examples/lookup_air.cpp -L tap-stark_amd/lib -ltapstark_hip -o lookup_air
//   ./lookup_air [log_n]  |  ./lookup_air --tape      (the version-3 tape, one word per line; needs no GPU)
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t P = 0x78000001u;

// main columns (value, table, mult): the table column is the row index, `mult` holds MINUS the number of rows that
// look the row's table entry up, and LogUp balances (+1, value) against (mult, table)
struct RangeLookupAir {
    ts::air::LogUp logup{{{{0, 1}, {{1, 0}}}, {{1, 2}, {{1, 1}}}}};
    uint32_t width() const { return 3; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(local[1]);
        auto when_transition = builder.when_transition();
        const ts::air::Expr step = local[1] + 1;
        when_transition.assert_eq(next[1], step);
        logup.eval(builder);
    }
};

// the aux source: the prover calls it once, after the trace is committed and the challenges are drawn
ts_status build_logup_columns(void* user, ts_ctx* ctx, const ts_matrix* trace, const uint32_t* challenges,
                              uint32_t n_challenges, ts_matrix** aux_out, uint32_t* exposed_out) {
    if (n_challenges != 2) return TS_ERR_INVALID;
    return ts_logup_aux_build(ctx, static_cast<const ts_logup_spec*>(user), trace, challenges, aux_out, exposed_out);
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

int main(int argc, char** argv) {
    RangeLookupAir lookup;
    ts::air::Builder builder(lookup.width(), 0, 0, lookup.logup.aux_width(), ts::air::LogUp::n_challenges,
                             ts::air::LogUp::n_exposed);
    lookup.eval(builder);
    const std::vector<uint32_t> tape = builder.tape();
    if (argc > 1 && std::string(argv[1]) == "--tape") {
        for (uint32_t w : tape) printf("%u\n", w);
        return 0;
    }
    const unsigned log_n = argc > 1 ? (unsigned)atoi(argv[1]) : 8;
    const uint64_t n = 1ull << log_n;
    ts_ctx* ctx = nullptr;
    if (ts_ctx_create(0, &ctx) != TS_OK) {
        fprintf(stderr, "no MI355X context: %s\n", ts_last_error(nullptr));
        return 2;  // no fallback path exists
    }
    ts_air* air = nullptr;
    CHECK(ts_air_compile(ctx, tape.data(), tape.size(), &air));

    // the same interactions for the device builder
    const ts_logup_term v0[] = {{1, 0}}, v1[] = {{1, 1}};
    const ts_logup_interaction interactions[] = {{{0, 1}, 1, v0}, {{1, 2}, 1, v1}};
    ts_logup_spec spec = {sizeof(ts_logup_spec), 2, interactions};
    uint32_t aux_width = 0;
    CHECK(ts_logup_aux_width(&spec, &aux_width));
    if (aux_width != lookup.logup.aux_width()) return 1;

    // a trace whose values all lie in the table 0 .. n-1
    std::vector<uint32_t> rows(3 * n), counts(n, 0);
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (uint64_t r = 0; r < n; r++) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t value = (uint32_t)((state >> 33) % n);
        rows[3 * r] = value;
        rows[3 * r + 1] = (uint32_t)r;
        counts[value]++;
    }
    for (uint64_t r = 0; r < n; r++) rows[3 * r + 2] = (P - counts[r]) % P;
    ts_matrix* trace = nullptr;
    CHECK(ts_matrix_upload(ctx, rows.data(), n, 3, &trace));

    const ts_fri_config fri = {2, 28, 8};
    ts_challenger* challenger = nullptr;
    CHECK(ts_chal_new(0, 1, &challenger));
    std::vector<uint32_t> proof(1u << 22);
    size_t n_words = 0;
    CHECK(ts_prove_aux(ctx, &fri, air, challenger, trace, nullptr, 0, build_logup_columns, &spec, proof.data(),
                       proof.size(), &n_words));
    proof.resize(n_words);

    ts_challenger* fresh = nullptr;
    CHECK(ts_chal_new(0, 1, &fresh));
    int verdict = -1;
    uint32_t sum[4] = {1, 1, 1, 1};
    CHECK(ts_verify_aux(&fri, air, fresh, proof.data(), proof.size(), nullptr, 0, sum, 4, &verdict));
    const bool zero = !(sum[0] | sum[1] | sum[2] | sum[3]);
    printf("lookup_air: n = 2^%u, proof %zu words (TSPF v%u), verify -> %d, the exposed sum is %s\n", log_n, n_words,
           proof[1], verdict, zero ? "zero" : "NOT zero");
    ts_chal_free(challenger);
    ts_chal_free(fresh);
    ts_matrix_free(ctx, trace);
    ts_air_free(ctx, air);
    ts_ctx_destroy(ctx);
    return verdict == 0 && zero ? 0 : 1;
}
