// examples/rom_fetch_resident.cpp -- columns DEFINED BY ANOTHER TABLE, fetched in HBM, against the public C ABI only
// (include/tapstark.h + the header-only AIR capture).  A machine trace of 2^6 rows fetches two instructions per row
// from a program ROM of 2^4 rows (pc, opcode, arg) whose pc values are sparse and in no order: a row number is no key.
// The ROM is a preprocessed matrix in a key committed ONCE.  The producer knows pc and sel of every slot; opcode and
// arg are the ROM's.
//   1. the key is committed once (ts_multi_key_commit) and lends its values;
//   2. the UNFILLED trace is uploaded -- the only trace upload of the statement;
//   3. ts_matrix_join_rows fills opcode and arg against the key's values, one call per fetch slot, chained with
//      TS_JOIN_KEEP so that each call keeps what the other wrote;
//   4. ts_logup_multiplicities_bus_pre fills the ROM table's multiplicities from the filled trace;
//   5. ts_prove_multi_key proves, ts_verify_multi_key accepts against the key root, the bus sum is zero;
//   6. one pc is changed to a value the ROM does not hold: the join reports that row as first_missing.
//
//   g++ -std=c++17 -I include examples/rom_fetch_resident.cpp -L tap-stark_amd/lib -ltapstark_hip -o rom_fetch_resident
//   ./rom_fetch_resident
#include <stdio.h>

#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t TAG = 13;  // the constant first value of this bus's tuples
constexpr uint32_t N = 64, ROM = 16, K = 2, W = 4 * K;

// main columns (pc, opcode, arg, sel) per slot: the row sends (TAG, pc, opcode, arg) sel times, sel boolean
struct FetchAir {
    ts::air::LogUp logup{{{{1, 3}, {{0, TAG}, {1, 0}, {1, 1}, {1, 2}}}, {{1, 7}, {{0, TAG}, {1, 4}, {1, 5}, {1, 6}}}}};
    uint32_t width() const { return W; }
    uint32_t preprocessed_width() const { return 0; }
    void eval(ts::air::Builder& builder) const {
        for (uint32_t i = 0; i < K; i++) {
            const ts::air::Expr sel = builder.local()[4 * i + 3];
            const ts::air::Expr sel_minus_one = sel - 1;
            builder.assert_zero(sel * sel_minus_one);
        }
        logup.eval(builder);
    }
};

// preprocessed columns (pc, opcode, arg) -- a matrix of the key --, one main column `mult` = MINUS the number of times
// the row was fetched.  No other constraint: the key fixes what the ROM holds.
struct RomAir {
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

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next_word() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
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
    const FetchAir fetch;
    const RomAir rom_air;
    const std::vector<uint32_t> tapes[2] = {tape_of(fetch), tape_of(rom_air)};
    const Spec spec_fetch(fetch.logup), spec_rom(rom_air.logup);
    ts_air* air_fetch = nullptr;
    ts_air* air_rom = nullptr;
    CHECK(ts_air_compile(ctx, tapes[0].data(), tapes[0].size(), &air_fetch));
    CHECK(ts_air_compile(ctx, tapes[1].data(), tapes[1].size(), &air_rom));
    const ts_fri_config fri = {2, 28, 8};

    // 1. the ROM: row j holds pc = 4096 + 16 * ((5 j + 3) mod 16) + j -- distinct, sparse, in no order
    std::vector<uint32_t> rom(ROM * 3);
    for (uint32_t j = 0; j < ROM; j++) {
        rom[3 * j] = 4096 + 16 * ((5 * j + 3) % ROM) + j;
        rom[3 * j + 1] = next_word() % 64;
        rom[3 * j + 2] = next_word() % ts::air::P;
    }
    ts_matrix* key_matrix = nullptr;
    CHECK(ts_matrix_upload(ctx, rom.data(), ROM, 3, &key_matrix));
    ts_multi_key* key = nullptr;
    uint32_t key_root[8];
    CHECK(ts_multi_key_commit(ctx, &fri, 1, &key_matrix, 1, key_root, &key));
    ts_matrix_free(ctx, key_matrix);  // consumed by the commit: only the empty handle is left
    const ts_matrix* rom_values = nullptr;
    CHECK(ts_multi_key_values(key, 0, &rom_values));

    // 2. the unfilled trace: pc and sel of every slot; opcode and arg are 0
    std::vector<uint32_t> trace(N * W, 0);
    uint32_t n_selected = 0;
    for (uint32_t r = 0; r < N; r++)
        for (uint32_t i = 0; i < K; i++) {
            trace[W * r + 4 * i] = rom[3 * (next_word() % ROM)];
            trace[W * r + 4 * i + 3] = next_word() & 1;
            n_selected += trace[W * r + 4 * i + 3];
        }
    ts_matrix* unfilled = nullptr;
    CHECK(ts_matrix_upload(ctx, trace.data(), N, W, &unfilled));

    // 3. the fetch, in HBM: slot i's pc against the ROM's column 0, on the rows its sel selects
    ts::air::Join joins[K] = {ts::air::Join(TS_JOIN_KEEP), ts::air::Join(TS_JOIN_KEEP)};
    ts_matrix* filled = unfilled;
    for (uint32_t i = 0; i < K; i++) {
        using ts::air::Join;
        joins[i].key(Join::col(4 * i), Join::col(0)).when(Join::col(4 * i + 3));
        joins[i].fetch(1, 4 * i + 1).fetch(2, 4 * i + 2);
        ts_matrix* next = nullptr;
        CHECK(ts_matrix_join_rows(ctx, joins[i].spec(), filled, rom_values, &next, nullptr, nullptr));  // a miss is an error
        ts_matrix_free(ctx, filled);
        filled = next;
    }
    std::vector<uint32_t> got(N * W);
    CHECK(ts_matrix_download(ctx, filled, got.data()));
    uint32_t n_right = 0;
    for (uint32_t r = 0; r < N; r++)
        for (uint32_t i = 0; i < K; i++) {
            const uint32_t* slot = &got[W * r + 4 * i];
            uint32_t j = 0;
            while (rom[3 * j] != slot[0]) j++;
            n_right += slot[3] ? slot[1] == rom[3 * j + 1] && slot[2] == rom[3 * j + 2] : slot[1] == 0 && slot[2] == 0;
        }
    printf("rom_fetch_resident: %u rows x %u slots, %u selected, %u slots hold what the ROM says\n", N, K, n_selected,
           n_right);

    // 4. the ROM table's multiplicities from the filled trace, against the key's values (kind 2)
    std::vector<uint32_t> zeros(ROM, 0);
    ts_matrix* rom_trace = nullptr;
    CHECK(ts_matrix_upload(ctx, zeros.data(), ROM, 1, &rom_trace));
    const ts_logup_term entry[] = {{2, 0}, {2, 1}, {2, 2}};
    const ts_logup_term looked[] = {{1, 0}, {1, 1}, {1, 2}, {1, 4}, {1, 5}, {1, 6}}, weight[] = {{1, 3}, {1, 7}};
    const ts_logup_bus_looker lookers[1] = {{K, 0, looked, weight}};
    const ts_logup_mult_bus_spec fill = {sizeof(ts_logup_mult_bus_spec), 3, entry, 1, 0, lookers, 1, 0};
    const ts_matrix* senders[1] = {filled};
    uint64_t n_missing = 0, first_missing[3];
    CHECK(ts_logup_multiplicities_bus_pre(ctx, &fill, rom_values, rom_trace, senders, &n_missing, first_missing));

    // 5. prove and verify against the key root
    ts_multi_key_table tables[2];
    tables[0] = {sizeof(ts_multi_key_table), 0, air_fetch, filled, nullptr, &spec_fetch.spec};
    tables[1] = {sizeof(ts_multi_key_table), 0, air_rom, rom_trace, nullptr, &spec_rom.spec};
    ts_challenger* challenger = nullptr;
    CHECK(ts_chal_new(0, 1, &challenger));
    std::vector<uint32_t> proof(1u << 20);
    size_t n_words = 0;
    CHECK(ts_prove_multi_key(ctx, &fri, challenger, key, tables, 2, proof.data(), proof.size(), &n_words));
    const ts_air* airs[2] = {air_fetch, air_rom};
    const uint32_t n_public[2] = {0, 0};
    const uint32_t* values[2] = {nullptr, nullptr};
    ts_challenger* fresh = nullptr;
    CHECK(ts_chal_new(0, 1, &fresh));
    uint32_t exposed[8], bus_sum[4] = {1, 1, 1, 1};
    int verdict = -1;
    CHECK(ts_verify_multi_key(&fri, fresh, key_root, airs, 2, values, n_public, proof.data(), n_words, exposed, 8,
                              bus_sum, &verdict));
    const bool zero = !(bus_sum[0] | bus_sum[1] | bus_sum[2] | bus_sum[3]);
    printf("rom_fetch_resident: %llu misses in the fill, TSPF v%u proof of %zu words, verify -> %d, bus sum %s\n",
           (unsigned long long)n_missing, proof[1], n_words, verdict, zero ? "zero" : "not zero");

    // 6. one pc the ROM does not hold: the join names the row
    uint32_t bad_row = 0;
    while (!trace[W * bad_row + 3]) bad_row++;
    bad_row += 5;
    while (!trace[W * bad_row + 3]) bad_row++;
    trace[W * bad_row] = 7;
    ts_matrix* bad = nullptr;
    CHECK(ts_matrix_upload(ctx, trace.data(), N, W, &bad));
    ts_matrix* bad_out = nullptr;
    uint64_t bad_missing = 0, bad_first = 0;
    CHECK(ts_matrix_join_rows(ctx, joins[0].spec(), bad, rom_values, &bad_out, &bad_missing, &bad_first));
    ts_matrix* refused_out = nullptr;
    const ts_status refused = ts_matrix_join_rows(ctx, joins[0].spec(), bad, rom_values, &refused_out, nullptr, nullptr);
    printf("rom_fetch_resident: pc of row %u changed to 7: %llu miss, first_missing %llu; without a count: status %d, %s\n",
           bad_row, (unsigned long long)bad_missing, (unsigned long long)bad_first, (int)refused, ts_last_error(ctx));
    const bool named = bad_missing == 1 && bad_first == bad_row && refused == TS_ERR_INVARIANT && refused_out == nullptr;

    ts_matrix_free(ctx, bad_out);
    ts_matrix_free(ctx, bad);
    ts_chal_free(challenger);
    ts_chal_free(fresh);
    ts_matrix_free(ctx, filled);  // (consumed by the proof: only the empty handles are left)
    ts_matrix_free(ctx, rom_trace);
    ts_multi_key_free(ctx, key);
    ts_air_free(ctx, air_fetch);
    ts_air_free(ctx, air_rom);
    ts_ctx_destroy(ctx);
    const bool good = n_right == N * K && n_missing == 0 && verdict == 0 && zero && named;
    printf("rom_fetch_resident: %s\n", good ? "as expected" : "NOT as expected");
    return good ? 0 : 1;
}
