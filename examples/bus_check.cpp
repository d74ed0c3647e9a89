// examples/bus_check.cpp -- "before you prove": the statement of examples/multi_bus.cpp (two sender tables put
// (TAG, value) on a LogUp bus, a range table of another height takes every value off) with one sent value outside the
// table, checked with ts_check_multi instead of being proved.  Every table's constraints hold, so a proof would verify
// and only its bus sum would be non-zero -- a random-looking extension element.  The check names the tuple that is
// out of balance, the table and row that sent it, and each table's share of it; after the value is put right it says
// "balanced".  Against the public C ABI only (include/tapstark.h + the header-only AIR capture).
//
//   g++ -std=c++17 -I include examples/bus_check.cpp -L tap-stark_amd/lib -ltapstark_hip -o bus_check
//   ./bus_check
#include <stdio.h>

#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t TAG = 7;  // the constant first value of this bus's tuples: another bus takes another tag

// main columns (value_0, sel_0, ..., value_{k-1}, sel_{k-1}): row r sends (TAG, value_i) sel_i times, sel_i boolean
struct BusSendAir {
    uint32_t k;
    ts::air::LogUp logup;
    static std::vector<ts::air::LogUpInteraction> interactions(uint32_t k) {
        std::vector<ts::air::LogUpInteraction> its;
        for (uint32_t i = 0; i < k; i++) its.push_back({{1, 2 * i + 1}, {{0, TAG}, {1, 2 * i}}});
        return its;
    }
    explicit BusSendAir(uint32_t k_) : k(k_), logup(interactions(k_)) {}
    uint32_t width() const { return 2 * k; }
    void eval(ts::air::Builder& builder) const {
        const auto& local = builder.local();
        for (uint32_t i = 0; i < k; i++) {
            const ts::air::Expr sel = local[2 * i + 1];
            const ts::air::Expr sel_minus_one = sel - 1;
            builder.assert_zero(sel * sel_minus_one);
        }
        logup.eval(builder);
    }
};

// main columns (table, mult): the table column is the row index, `mult` holds MINUS the number of times the senders
// sent the row's entry
struct BusRangeAir {
    ts::air::LogUp logup{{{{1, 1}, {{0, TAG}, {1, 0}}}}};
    uint32_t width() const { return 2; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(local[0]);
        auto when_transition = builder.when_transition();
        const ts::air::Expr step = local[0] + 1;
        when_transition.assert_eq(next[0], step);
        logup.eval(builder);
    }
};

template <class Air>
std::vector<uint32_t> tape_of(const Air& air) {
    ts::air::Builder builder(air.width(), 0, 0, air.logup.aux_width(), ts::air::LogUp::n_challenges,
                             ts::air::LogUp::n_exposed);
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
    const BusSendAir send2(2), send1(1);
    const BusRangeAir range;
    const std::vector<uint32_t> tapes[3] = {tape_of(send2), tape_of(send1), tape_of(range)};
    const Spec spec_send2(send2.logup), spec_send1(send1.logup), spec_range(range.logup);
    const ts_logup_spec* specs[3] = {&spec_send2.spec, &spec_send1.spec, &spec_range.spec};
    ts_air* airs[3] = {nullptr, nullptr, nullptr};
    for (int t = 0; t < 3; t++) CHECK(ts_air_compile(ctx, tapes[t].data(), tapes[t].size(), &airs[t]));

    // senders of 2^10 rows (two sends per row) and 2^6 rows (one), a range table of 2^8 entries
    const uint64_t heights[3] = {1ull << 10, 1ull << 6, 1ull << 8};
    const uint32_t widths[3] = {send2.width(), send1.width(), range.width()};
    // any gamma and beta serve a check: nothing is proved with them
    const uint32_t challenges[8] = {12345, 678, 9, 10, 11, 12, 13, 14};
    bool as_expected = true;

    for (int round = 0; round < 2; round++) {  // 0: one sent value is no table entry; 1: it is put right
        std::vector<uint32_t> rows[3];
        uint64_t state = 0x9E3779B97F4A7C15ull;
        for (int t = 0; t < 2; t++) {
            rows[t].resize(heights[t] * widths[t]);
            for (uint64_t r = 0; r < heights[t]; r++)
                for (uint32_t i = 0; i < widths[t] / 2; i++) {
                    state = state * 6364136223846793005ull + 1442695040888963407ull;
                    uint32_t value = (uint32_t)((state >> 33) % heights[2]);
                    const uint32_t sel = (uint32_t)((state >> 20) & 1);
                    if (round == 0 && t == 1 && r == 5) value = (uint32_t)heights[2];  // sent, and in no table row
                    rows[t][r * widths[t] + 2 * i] = value;
                    rows[t][r * widths[t] + 2 * i + 1] = t == 1 && r == 5 ? 1 : sel;
                }
        }
        rows[2].resize(heights[2] * 2);
        for (uint64_t r = 0; r < heights[2]; r++) {
            rows[2][2 * r] = (uint32_t)r;
            rows[2][2 * r + 1] = 0;  // filled on the device below
        }
        ts_multi_bus_table tables[3];
        for (int t = 0; t < 3; t++) {
            tables[t].struct_size = sizeof(ts_multi_bus_table);
            tables[t].n_public = 0;
            tables[t].air = airs[t];
            tables[t].trace = nullptr;
            tables[t].public_values = nullptr;
            tables[t].logup = specs[t];
            CHECK(ts_matrix_upload(ctx, rows[t].data(), heights[t], widths[t], &tables[t].trace));
        }
        // mult = MINUS the number of selected sends of each entry, counted on the device over both sender traces
        const ts_logup_term entry[] = {{1, 0}};
        const ts_logup_term looked2[] = {{1, 0}, {1, 2}}, weights2[] = {{1, 1}, {1, 3}};
        const ts_logup_term looked1[] = {{1, 0}}, weights1[] = {{1, 1}};
        const ts_logup_bus_looker lookers[2] = {{2, 0, looked2, weights2}, {1, 0, looked1, weights1}};
        const ts_logup_mult_bus_spec fill = {sizeof(ts_logup_mult_bus_spec), 1, entry, 2, 1, lookers, 1, 0};
        const ts_matrix* senders[2] = {tables[0].trace, tables[1].trace};
        uint64_t n_missing = 0, first_missing[3];
        CHECK(ts_logup_multiplicities_bus(ctx, &fill, tables[2].trace, senders, &n_missing, first_missing));

        // the traces stay with their handles: the same tables could go to ts_prove_multi_bus afterwards
        int32_t bad_table = 0;
        int64_t first_violation = 0;
        ts_bus_report report;
        report.struct_size = sizeof(ts_bus_report);
        ts_bus_share shares[3];
        CHECK(ts_check_multi(ctx, nullptr, tables, 3, challenges, &bad_table, &first_violation, &report, shares));
        printf("bus_check: constraints %s; %llu contributions to %llu tuples, %llu out of balance\n",
               bad_table < 0 ? "hold in every table" : "VIOLATED", (unsigned long long)report.n_contributions,
               (unsigned long long)report.n_tuples, (unsigned long long)report.n_unbalanced);
        if (report.n_unbalanced) {
            printf("bus_check: unbalanced: table %u, row %u, interaction %u sent (", report.first_table, report.first_row,
                   report.first_interaction);
            for (uint32_t q = 0; q < report.n_values; q++) printf(q ? ", %u" : "%u", report.tuple[q]);
            printf("), multiplicity sum %u\n", report.sum);
            for (int t = 0; t < 3; t++) {
                if (shares[t].count)
                    printf("bus_check:   table %d: %llu contributions, sum %u, first at row %u, interaction %u\n", t,
                           (unsigned long long)shares[t].count, shares[t].sum, shares[t].first_row,
                           shares[t].first_interaction);
                else
                    printf("bus_check:   table %d: no contribution\n", t);
            }
        } else {
            printf("bus_check: balanced\n");
        }
        const bool planted = report.n_unbalanced == 1 && report.first_table == 1 && report.first_row == 5 &&
                             report.first_interaction == 0 && report.n_values == 2 && report.tuple[0] == TAG &&
                             report.tuple[1] == heights[2] && report.sum == 1 && shares[1].count == 1 &&
                             shares[0].count == 0 && shares[2].count == 0;
        as_expected = as_expected && bad_table == -1 && first_violation == -1 &&
                      (round == 0 ? planted && n_missing == 1 : report.n_unbalanced == 0 && n_missing == 0);
        for (int t = 0; t < 3; t++) ts_matrix_free(ctx, tables[t].trace);
    }
    for (int t = 0; t < 3; t++) ts_air_free(ctx, airs[t]);
    ts_ctx_destroy(ctx);
    return as_expected ? 0 : 1;
}
