// examples/table_lookup_resident.cpp -- the lookup of examples/table_lookup_air.cpp for a trace that lives in HBM:
// the host uploads the VALUE column only (the multiplicity column is zero), ts_logup_multiplicities fills the
// multiplicity column on the device from the resident trace and the key's table, and the proof is made with
// ts_prove_pre_aux, verified against the key's root, and its exposed sum checked to be zero.  No histogram on the
// host, no download of the trace.
//
//   g++ -std=c++17 -I include examples/table_lookup_resident.cpp -L tap-stark_amd/lib -ltapstark_hip -o table_lookup_resident
//   ./table_lookup_resident [log_n]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

// main columns (value, mult), preprocessed column (table); LogUp balances (+1, value) against (mult, table)
struct TableLookupAir {
    ts::air::LogUp logup{{{{0, 1}, {{1, 0}}}, {{1, 1}, {{2, 0}}}}};
    uint32_t width() const { return 2; }
    uint32_t preprocessed_width() const { return 1; }
    void eval(ts::air::Builder& builder) const { logup.eval(builder); }
};

struct LookupUser {
    const ts_logup_spec* spec;
    const ts_matrix* table;
};

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

    // the key: the table 0 .. n-1 committed once; a second upload keeps its rows for the two LogUp calls
    std::vector<uint32_t> table(n);
    for (uint64_t r = 0; r < n; r++) table[r] = (uint32_t)r;
    ts_matrix *key_matrix = nullptr, *table_rows = nullptr;
    CHECK(ts_matrix_upload(ctx, table.data(), n, 1, &key_matrix));
    CHECK(ts_matrix_upload(ctx, table.data(), n, 1, &table_rows));
    const uint32_t shifts[1] = {1};
    uint32_t key_root[8];
    ts_pcs_data* key = nullptr;
    CHECK(ts_pcs_commit(ctx, &fri, 1, &key_matrix, shifts, key_root, &key));

    // the values, with the multiplicity column left zero (a trace generator on the device would write the same)
    std::vector<uint32_t> rows(2 * n, 0);
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (uint64_t r = 0; r < n; r++) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        rows[2 * r] = (uint32_t)((state >> 33) % n);
    }
    ts_matrix* trace = nullptr;
    CHECK(ts_matrix_upload(ctx, rows.data(), n, 2, &trace));

    // interaction 1 is the table side: its multiplicity column receives minus the counts of interaction 0's lookups
    const ts::air::LogUp::MultSpec mult = lookup.logup.mult_spec(1, {0});
    uint64_t n_missing = 0, first_missing = 0;
    CHECK(ts_logup_multiplicities(ctx, &mult.spec, table_rows, trace, &n_missing, &first_missing));

    const ts_logup_term v0[] = {{1, 0}}, v1[] = {{2, 0}};
    const ts_logup_interaction interactions[] = {{{0, 1}, 1, v0}, {{1, 1}, 1, v1}};
    ts_logup_spec spec = {sizeof(ts_logup_spec), 2, interactions};
    LookupUser user = {&spec, table_rows};
    std::vector<uint32_t> proof(1u << 22);
    size_t n_words = 0;
    ts_challenger *challenger = nullptr, *fresh = nullptr;
    CHECK(ts_chal_new(0, 1, &challenger));
    CHECK(ts_chal_new(0, 1, &fresh));
    CHECK(ts_prove_pre_aux(ctx, &fri, air, challenger, key, trace, nullptr, 0, build_logup_columns, &user, proof.data(),
                           proof.size(), &n_words));
    int verdict = -1;
    uint32_t sum[4] = {1, 1, 1, 1};
    CHECK(ts_verify_pre_aux(&fri, air, fresh, key_root, proof.data(), n_words, nullptr, 0, sum, 4, &verdict));
    const bool zero = !(sum[0] | sum[1] | sum[2] | sum[3]);
    printf("table_lookup_resident: n = 2^%u, multiplicities filled in HBM (%llu missing), proof %zu words (TSPF v%u), "
           "verify -> %d, the exposed sum is %s\n",
           log_n, (unsigned long long)n_missing, n_words, proof[1], verdict, zero ? "zero" : "NOT zero");
    ts_chal_free(challenger);
    ts_chal_free(fresh);
    ts_matrix_free(ctx, trace);
    ts_matrix_free(ctx, table_rows);
    ts_matrix_free(ctx, key_matrix);
    ts_pcs_data_free(ctx, key);
    ts_air_free(ctx, air);
    ts_ctx_destroy(ctx);
    return verdict == 0 && zero && n_missing == 0 ? 0 : 1;
}
