// examples/table_lookup_air.cpp -- a lookup against a FIXED table, end to end over the public C ABI: the
// TableLookupAir of tap-stark_amd/airs.py (value and multiplicity columns in the main trace, the table in a
// preprocessed column) captured with include/tapstark_air.hpp.  The table is committed ONCE as a key; the proof
// is made with ts_prove_pre_aux through a C callback that builds the LogUp columns on the device
// (ts_logup_aux_build_pre, which reads the table's row-major values), verified against the key's root with a fresh
// challenger, and the statement about the exposed sum -- it is zero -- checked by the caller, whose job that is.
//
//   g++ -std=c++17 -I include examples/table_lookup_air.cpp -L tap-stark_amd/lib -ltapstark_hip -o table_lookup_air
//   ./table_lookup_air [log_n]  |  ./table_lookup_air --tape   (the version-3 tape, one word per line; needs no GPU)
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t P = 0x78000001u;

// main columns (value, mult), preprocessed column (table): `mult` holds MINUS the number of rows that look the
// row's table entry up, and LogUp balances (+1, value) against (mult, table).  No other constraint: what the table
// holds is fixed by the key.
struct TableLookupAir {
    ts::air::LogUp logup{{{{0, 1}, {{1, 0}}}, {{1, 1}, {{2, 0}}}}};
    uint32_t width() const { return 2; }
    uint32_t preprocessed_width() const { return 1; }
    void eval(ts::air::Builder& builder) const { logup.eval(builder); }
};

// what the aux source needs beside the trace: the spec and the table's values, row-major on the prover's context
struct LookupUser {
    const ts_logup_spec* spec;
    const ts_matrix* table;
};

// the aux source: the prover calls it once, after the trace is committed and the challenges are drawn
ts_status build_logup_columns(void* user, ts_ctx* ctx, const ts_matrix* trace, const uint32_t* challenges,
                              uint32_t n_challenges, ts_matrix** aux_out, uint32_t* exposed_out) {
    if (n_challenges != 2) return TS_ERR_INVALID;
    const LookupUser* u = static_cast<const LookupUser*>(user);
    return ts_logup_aux_build_pre(ctx, u->spec, u->table, trace, challenges, aux_out, exposed_out);
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
    TableLookupAir lookup;
    ts::air::Builder builder(lookup.width(), 0, lookup.preprocessed_width(), lookup.logup.aux_width(),
                             ts::air::LogUp::n_challenges, ts::air::LogUp::n_exposed);
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
    const ts_fri_config fri = {2, 28, 8};

    // the key: the table 0 .. n-1, committed once on the natural domain.  The commit consumes its matrix, so the
    // values the LogUp builder reads are a second upload.
    std::vector<uint32_t> table(n);
    for (uint64_t r = 0; r < n; r++) table[r] = (uint32_t)r;
    ts_matrix *key_matrix = nullptr, *table_rows = nullptr;
    CHECK(ts_matrix_upload(ctx, table.data(), n, 1, &key_matrix));
    CHECK(ts_matrix_upload(ctx, table.data(), n, 1, &table_rows));
    const uint32_t shifts[1] = {1};
    uint32_t key_root[8];
    ts_pcs_data* key = nullptr;
    CHECK(ts_pcs_commit(ctx, &fri, 1, &key_matrix, shifts, key_root, &key));

    // the same interactions for the device builder: kind 2 is a column of the preprocessed matrix
    const ts_logup_term v0[] = {{1, 0}}, v1[] = {{2, 0}};
    const ts_logup_interaction interactions[] = {{{0, 1}, 1, v0}, {{1, 1}, 1, v1}};
    ts_logup_spec spec = {sizeof(ts_logup_spec), 2, interactions};
    LookupUser user = {&spec, table_rows};

    // two proofs against the one key, each of a trace whose values all lie in the table
    int verdict = -1;
    bool zero = false;
    size_t n_words = 0;
    std::vector<uint32_t> proof(1u << 22);
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 2; k++) {
        std::vector<uint32_t> rows(2 * n), counts(n, 0);
        for (uint64_t r = 0; r < n; r++) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const uint32_t value = (uint32_t)((state >> 33) % n);
            rows[2 * r] = value;
            counts[value]++;
        }
        for (uint64_t r = 0; r < n; r++) rows[2 * r + 1] = (P - counts[r]) % P;
        ts_matrix* trace = nullptr;
        CHECK(ts_matrix_upload(ctx, rows.data(), n, 2, &trace));
        ts_challenger* challenger = nullptr;
        CHECK(ts_chal_new(0, 1, &challenger));
        CHECK(ts_prove_pre_aux(ctx, &fri, air, challenger, key, trace, nullptr, 0, build_logup_columns, &user,
                               proof.data(), proof.size(), &n_words));
        ts_challenger* fresh = nullptr;
        CHECK(ts_chal_new(0, 1, &fresh));
        uint32_t sum[4] = {1, 1, 1, 1};
        CHECK(ts_verify_pre_aux(&fri, air, fresh, key_root, proof.data(), n_words, nullptr, 0, sum, 4, &verdict));
        zero = !(sum[0] | sum[1] | sum[2] | sum[3]);
        printf("table_lookup_air: n = 2^%u, proof %d: %zu words (TSPF v%u), verify -> %d, the exposed sum is %s\n",
               log_n, k, n_words, proof[1], verdict, zero ? "zero" : "NOT zero");
        ts_chal_free(challenger);
        ts_chal_free(fresh);
        ts_matrix_free(ctx, trace);
        if (verdict != 0 || !zero) break;
    }
    ts_matrix_free(ctx, table_rows);
    ts_matrix_free(ctx, key_matrix);
    ts_pcs_data_free(ctx, key);
    ts_air_free(ctx, air);
    ts_ctx_destroy(ctx);
    return verdict == 0 && zero ? 0 : 1;
}
