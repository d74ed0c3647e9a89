// examples/multi_key.cpp -- a FIXED table on the bus of a multi-table proof, against the public C ABI only
// (include/tapstark.h + the header-only AIR capture).  The 4-bit x 4-bit xor table (a, b, a xor b), 2^8 rows, is a
// preprocessed matrix in a key committed ONCE (ts_multi_key_commit); the verifier holds the key's root.  Two
// statements are proved against that one key (ts_prove_multi_key, TSPF v8): tuple senders of two heights put
// (TAG, a, b, c) on the bus, the table takes every tuple off as often as it was sent.  Its multiplicity column is
// filled in HBM from the resident sender traces against the key's own values (ts_logup_multiplicities_bus_pre).  Each
// proof is verified against the key root and the bus sum is checked to be zero.  Then the first proof is verified
// against the root of a key with ONE table entry changed: rejected.
//
//   g++ -std=c++17 -I include examples/multi_key.cpp -L tap-stark_amd/lib -ltapstark_hip -o multi_key
//   ./multi_key
#include <stdio.h>

#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t TAG = 11;  // the constant first value of this bus's tuples

// main columns (a, b, c, sel): the row sends (TAG, a, b, c) sel times, sel boolean
struct TupleSendAir {
    ts::air::LogUp logup{{{{1, 3}, {{0, TAG}, {1, 0}, {1, 1}, {1, 2}}}}};
    uint32_t width() const { return 4; }
    uint32_t preprocessed_width() const { return 0; }
    void eval(ts::air::Builder& builder) const {
        const ts::air::Expr sel = builder.local()[3];
        const ts::air::Expr sel_minus_one = sel - 1;
        builder.assert_zero(sel * sel_minus_one);
        logup.eval(builder);
    }
};

// preprocessed columns (a, b, a xor b) -- a matrix of the key --, one main column `mult` = MINUS the number of times
// the senders sent the row's tuple.  No other constraint: the key fixes what the table holds.
struct KeyTableAir {
    ts::air::LogUp logup{{{{1, 0}, {{0, TAG}, {2, 0}, {2, 1}, {2, 2}}}}};
    uint32_t width() const { return 1; }
    uint32_t preprocessed_width() const { return 3; }
    void eval(ts::air::Builder& builder) const { logup.eval(builder); }
};

template <class Air>
std::vector<uint32_t> tape_of(const Air& air) {
    ts::air::Builder builder(air.width(), 0, air.preprocessed_width(), air.logup.aux_width(),
                             ts::air::LogUp::n_challenges, ts::air::LogUp::n_exposed);
    air.eval(builder);
    return builder.tape();
}

// the ts_logup_spec of a ts::air::LogUp, and the arrays it points into
struct Spec {
    std::vector<std::vector<ts_logup_term>> values;
    std::vector<ts_logup_interaction> interactions;
    ts_logup_spec spec;
    explicit Spec(const ts::air::LogUp& logup) {
        for (auto& it : logup.interactions()) {
            values.emplace_back();
            for (auto& v : it.values) values.back().push_back({v.kind, v.value});
        }
        size_t i = 0;
        for (auto& it : logup.interactions()) {
            interactions.push_back({{it.multiplicity.kind, it.multiplicity.value}, (uint32_t)values[i].size(),
                                    values[i].data()});
            i++;
        }
        spec = {sizeof(ts_logup_spec), (uint32_t)interactions.size(), interactions.data()};
    }
    Spec(const Spec&) = delete;
};

std::vector<uint32_t> xor_table() {
    std::vector<uint32_t> rows(256 * 3);
    for (uint32_t a = 0; a < 16; a++)
        for (uint32_t b = 0; b < 16; b++) {
            uint32_t* row = &rows[(a * 16 + b) * 3];
            row[0] = a;
            row[1] = b;
            row[2] = a ^ b;
        }
    return rows;
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
    const TupleSendAir send;
    const KeyTableAir table;
    const std::vector<uint32_t> tapes[2] = {tape_of(send), tape_of(table)};
    const Spec spec_send(send.logup), spec_table(table.logup);
    ts_air* air_send = nullptr;
    ts_air* air_table = nullptr;
    CHECK(ts_air_compile(ctx, tapes[0].data(), tapes[0].size(), &air_send));
    CHECK(ts_air_compile(ctx, tapes[1].data(), tapes[1].size(), &air_table));
    const ts_fri_config fri = {2, 28, 8};

    // the key: committed once, its values kept for the fill and for the table's kind-2 terms
    std::vector<uint32_t> xors = xor_table();
    ts_matrix* key_matrix = nullptr;
    CHECK(ts_matrix_upload(ctx, xors.data(), 256, 3, &key_matrix));
    ts_multi_key* key = nullptr;
    uint32_t key_root[8];
    CHECK(ts_multi_key_commit(ctx, &fri, 1, &key_matrix, 1, key_root, &key));
    ts_matrix_free(ctx, key_matrix);  // consumed by the commit: only the empty handle is left
    const ts_matrix* key_values = nullptr;
    CHECK(ts_multi_key_values(key, 0, &key_values));

    // the root of the same table with one entry changed: 3 xor 5 = 7, not 6
    xors[(3 * 16 + 5) * 3 + 2] = 7;
    ts_matrix* other_matrix = nullptr;
    CHECK(ts_matrix_upload(ctx, xors.data(), 256, 3, &other_matrix));
    ts_multi_key* other_key = nullptr;
    uint32_t other_root[8];
    CHECK(ts_multi_key_commit(ctx, &fri, 1, &other_matrix, 0, other_root, &other_key));
    ts_matrix_free(ctx, other_matrix);

    const ts_air* airs[3] = {air_send, air_send, air_table};
    const uint32_t n_public[3] = {0, 0, 0};
    const uint32_t* values[3] = {nullptr, nullptr, nullptr};
    // statement 0: senders of 2^10 and 2^6 rows; statement 1: of 2^8 and 2^12 rows -- one key serves both
    const uint64_t heights[2][2] = {{1ull << 10, 1ull << 6}, {1ull << 8, 1ull << 12}};
    std::vector<uint32_t> first_proof;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    bool all_good = true;
    for (int st = 0; st < 2; st++) {
        ts_multi_key_table tables[3];
        for (int t = 0; t < 3; t++) {
            const uint64_t h = t < 2 ? heights[st][t] : 256;
            const uint32_t w = t < 2 ? 4 : 1;
            std::vector<uint32_t> rows(h * w, 0);  // the table's multiplicity column is filled on the device below
            for (uint64_t r = 0; t < 2 && r < h; r++) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                const uint32_t a = (uint32_t)(state >> 33) & 15, b = (uint32_t)(state >> 40) & 15;
                rows[4 * r] = a;
                rows[4 * r + 1] = b;
                rows[4 * r + 2] = a ^ b;
                rows[4 * r + 3] = (uint32_t)(state >> 20) & 1;
            }
            tables[t].struct_size = sizeof(ts_multi_key_table);
            tables[t].n_public = 0;
            tables[t].air = airs[t];
            tables[t].trace = nullptr;
            tables[t].public_values = nullptr;
            tables[t].logup = t < 2 ? &spec_send.spec : &spec_table.spec;
            CHECK(ts_matrix_upload(ctx, rows.data(), h, w, &tables[t].trace));
        }
        // mult = MINUS the number of selected sends of each (a, b, a xor b), counted on the device; the table's tuple
        // is read from the key's values (kind 2)
        const ts_logup_term entry[] = {{2, 0}, {2, 1}, {2, 2}};
        const ts_logup_term looked[] = {{1, 0}, {1, 1}, {1, 2}}, weight[] = {{1, 3}};
        const ts_logup_bus_looker lookers[2] = {{1, 0, looked, weight}, {1, 0, looked, weight}};
        const ts_logup_mult_bus_spec fill = {sizeof(ts_logup_mult_bus_spec), 3, entry, 2, 0, lookers, 1, 0};
        const ts_matrix* senders[2] = {tables[0].trace, tables[1].trace};
        uint64_t n_missing = 0, first_missing[3];
        CHECK(ts_logup_multiplicities_bus_pre(ctx, &fill, key_values, tables[2].trace, senders, &n_missing, first_missing));
        if (n_missing != 0) {
            fprintf(stderr, "unexpected misses: %llu\n", (unsigned long long)n_missing);
            return 1;
        }
        ts_challenger* challenger = nullptr;
        CHECK(ts_chal_new(0, 1, &challenger));
        std::vector<uint32_t> proof(1u << 20);
        size_t n_words = 0;
        CHECK(ts_prove_multi_key(ctx, &fri, challenger, key, tables, 3, proof.data(), proof.size(), &n_words));
        proof.resize(n_words);

        ts_challenger* fresh = nullptr;
        CHECK(ts_chal_new(0, 1, &fresh));
        uint32_t exposed[12], bus_sum[4] = {1, 1, 1, 1};
        int verdict = -1;
        CHECK(ts_verify_multi_key(&fri, fresh, key_root, airs, 3, values, n_public, proof.data(), proof.size(), exposed,
                                  12, bus_sum, &verdict));
        const bool zero = !(bus_sum[0] | bus_sum[1] | bus_sum[2] | bus_sum[3]);
        printf("multi_key: statement %d, senders of %llu and %llu rows against the 2^8 xor table of the key, TSPF v%u "
               "proof of %zu words, verify -> %d, bus sum %s\n", st, (unsigned long long)heights[st][0],
               (unsigned long long)heights[st][1], proof[1], n_words, verdict, zero ? "zero" : "not zero");
        all_good = all_good && verdict == 0 && zero;
        if (st == 0) first_proof = proof;
        ts_chal_free(challenger);
        ts_chal_free(fresh);
        for (int t = 0; t < 3; t++) ts_matrix_free(ctx, tables[t].trace);
    }

    ts_challenger* fresh = nullptr;
    CHECK(ts_chal_new(0, 1, &fresh));
    uint32_t exposed[12], bus_sum[4];
    int verdict = -1;
    CHECK(ts_verify_multi_key(&fri, fresh, other_root, airs, 3, values, n_public, first_proof.data(), first_proof.size(),
                              exposed, 12, bus_sum, &verdict));
    printf("multi_key: statement 0 under a key with one entry changed: %s (verdict %d)\n",
           verdict != 0 ? "rejected" : "ACCEPTED", verdict);
    ts_chal_free(fresh);
    ts_multi_key_free(ctx, other_key);
    ts_multi_key_free(ctx, key);
    ts_air_free(ctx, air_send);
    ts_air_free(ctx, air_table);
    ts_ctx_destroy(ctx);
    return all_good && verdict != 0 ? 0 : 1;
}
