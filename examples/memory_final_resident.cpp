// examples/memory_final_resident.cpp -- the final state of memory as a table of its own, every trace made in HBM: one
// row per touched address with its final value, the clock of its last access and the number of its accesses -- what a
// continuation hands to the next segment.  Between the one upload of the accesses and the verified proof no trace comes
// back to the host.
//   1. ts_matrix_derive, source program, and ts_matrix_sort_rows by (addr, clk): the sorted memory table;
//   2. ts_matrix_derive, gap program; ts_matrix_derive, last program: last = live (1 - next.cont), a column of its own
//      row and the row after it -- 1 on the last access of every address;
//   3. ts_matrix_collect_rows with a TGRP tape (include/tapstark.h "grouped rows"): ONE call groups the sorted table by
//      addr and gives (addr, last clk, last value, count, live = 1, recv = p - 1) per address: the final table;
//   4. the range table and its multiplicities, as in examples/memory_table_resident.cpp;
//   5. ts_prove_multi_bus over the four tables;  6. ts_verify_multi_bus: accepted, the bus sums to zero;
//   7. one final value changed in HBM (a derive over the final table): ts_check_multi names the table, the row and the
//      tuple nobody receives.
//
//   g++ -std=c++17 -I include examples/memory_final_resident.cpp -L tap-stark_amd/lib -ltapstark_hip -o memory_final_resident
//   ./memory_final_resident
#include <stdio.h>

#include <map>
#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t P = 0x78000001;
constexpr uint32_t MEM_TAG = 11, RANGE_TAG = 7, FIN_TAG = 23;
constexpr uint64_t N = 64;  // accesses, and the height of every table but the final one
constexpr uint32_t N_ADDR = 8;
constexpr uint64_t CHANGED_ROW = 3;  // of the final table

using ts::air::DExpr;
using ts::air::Expr;
using ts::air::Group;

struct MemoryAccessAir {
    ts::air::LogUp logup{{{{1, 4}, {{0, MEM_TAG}, {1, 0}, {1, 1}, {1, 2}, {1, 3}}}}};
    uint32_t width() const { return 5; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        const Expr sel = local[4], is_write = local[3];
        builder.assert_zero(sel * (sel - 1));
        builder.assert_zero(is_write * (is_write - 1));
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(local[1]);
        auto when_transition = builder.when_transition();
        when_transition.assert_eq(next[1], local[1] + 1);
        builder.assert_zero(local[0] * sel * (sel - 1));
        logup.eval(builder);
    }
};

// the memory table of examples/memory_table_resident.cpp with `last` (column 8) and its send
struct MemoryTableFinalAir {
    ts::air::LogUp logup{{{{1, 5}, {{0, MEM_TAG}, {1, 0}, {1, 1}, {1, 2}, {1, 3}}},
                          {{1, 4}, {{0, RANGE_TAG}, {1, 6}}},
                          {{1, 8}, {{0, FIN_TAG}, {1, 0}, {1, 1}, {1, 2}}}}};
    uint32_t width() const { return 9; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        const Expr live = local[4], start = local[7], is_write = local[3], last = local[8];
        const Expr next_cont = next[4] - next[7];
        builder.assert_zero(live * (live - 1));
        builder.assert_zero(start * (start - 1));
        builder.assert_zero(is_write * (is_write - 1));
        builder.assert_zero(start * (live - 1));
        builder.assert_zero(local[5] + live);
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(live - start);
        builder.assert_zero(start * (is_write - 1));
        auto t = builder.when_transition();
        t.assert_zero((live - 1) * next[4]);
        t.assert_zero(next_cont * (next[0] - local[0]));
        t.assert_zero(next_cont * (next[3] - 1) * (next[2] - local[2]));
        t.assert_zero(next[7] * (next[0] - local[0] - 1 - next[6]) + next_cont * (next[1] - local[1] - 1 - next[6]));
        builder.assert_zero(last * (last - 1));
        t.assert_zero(last + live * (next_cont - 1));  // last = live (1 - next.cont)
        auto when_last_row = builder.when_last_row();
        when_last_row.assert_zero(last - live);
        logup.eval(builder);
    }
};

struct MemoryFinalAir {  // (addr, clk, value, count, live, recv)
    ts::air::LogUp logup{{{{1, 5}, {{0, FIN_TAG}, {1, 0}, {1, 1}, {1, 2}}}}};
    uint32_t width() const { return 6; }
    void eval(ts::air::Builder& builder) const {
        const auto& local = builder.local();
        const Expr live = local[4];
        builder.assert_zero(live * (live - 1));
        builder.assert_zero(local[5] + live);
        builder.assert_zero(local[0] * live * (live - 1));
        logup.eval(builder);
    }
};

struct RangeAir {
    ts::air::LogUp logup{{{{1, 1}, {{0, RANGE_TAG}, {1, 0}}}}};
    uint32_t width() const { return 2; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(local[0]);
        when_first_row.assert_zero(local[0] * next[0]);
        auto when_transition = builder.when_transition();
        when_transition.assert_eq(next[0], local[0] + 1);
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

// ---- the row programs and the group spec
std::vector<uint32_t> source_program() {  // width 5 -> 7: columns 0 .. 4 copied, recv = -live, gap = 0
    ts::air::Derive b(5);
    b.output(-b.col(4), 5);
    b.output(b.constant(0), 6);
    return b.tape();
}

std::vector<uint32_t> gap_program() {  // width 8, column 6 overwritten
    ts::air::Derive b(8);
    const DExpr start = b.col(7);
    const DExpr by_addr = start * (b.col(0) - b.prev(0));
    const DExpr by_clk = (1 - start) * (b.col(1) - b.prev(1));
    const DExpr step = by_addr + by_clk - 1;
    b.output(b.col(4) * (1 - b.is_first_row()) * step, 6);
    return b.tape();
}

std::vector<uint32_t> last_program() {  // width 8 -> 9: last = live (1 - (1 - is_last_row) (next.live - next.start))
    ts::air::Derive b(8);
    const DExpr goes_on = (1 - b.is_last_row()) * (b.next(4) - b.next(7));
    b.output(b.col(4) * (1 - goes_on), 8);
    return b.tape();
}

std::vector<uint32_t> final_spec() {  // the sorted table grouped by addr, the live rows only; the pad row is all zero
    Group g(9, 6, {Group::col(0)}, Group::col(4));
    g.terms({Group::first(0), Group::last(1), Group::last(2), Group::count(), Group::constant(1), Group::constant(P - 1)});
    return g.tape();
}

std::vector<uint32_t> change_program(uint64_t row) {  // width 6: value + 1 on one row
    ts::air::Derive b(6);
    b.output(b.col(2) + (b.row() - row).is_zero(), 2);
    return b.tape();
}

std::vector<uint32_t> index_program() {  // width 2: column 0 = the row index, column 1 copied
    ts::air::Derive b(2);
    b.output(b.row(), 0);
    return b.tape();
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
    const MemoryAccessAir access_air;
    const MemoryTableFinalAir table_air;
    const MemoryFinalAir final_air;
    const RangeAir range_air;
    const std::vector<uint32_t> tapes[4] = {tape_of(access_air), tape_of(table_air), tape_of(final_air), tape_of(range_air)};
    const Spec spec_access(access_air.logup), spec_table(table_air.logup), spec_final(final_air.logup),
        spec_range(range_air.logup);
    const ts_logup_spec* specs[4] = {&spec_access.spec, &spec_table.spec, &spec_final.spec, &spec_range.spec};
    ts_air* airs[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int t = 0; t < 4; t++) CHECK(ts_air_compile(ctx, tapes[t].data(), tapes[t].size(), &airs[t]));

    // the accesses in execution order: reads return the last write, the first access of an address is a write
    std::vector<uint32_t> trace(N * 5);
    std::map<uint32_t, uint32_t> memory, last_clock;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (uint64_t r = 0; r < N; r++) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t addr = (uint32_t)((state >> 33) % N_ADDR);
        const bool write = ((state >> 20) & 1) || !memory.count(addr);
        if (write) memory[addr] = (uint32_t)((state >> 8) % P);
        last_clock[addr] = (uint32_t)r;
        const uint32_t row[5] = {addr, (uint32_t)r, memory[addr], write, 1};
        for (int c = 0; c < 5; c++) trace[r * 5 + c] = row[c];
    }

    const std::vector<uint32_t> source = source_program(), gap = gap_program(), last = last_program(),
                                group = final_spec(), index = index_program(), change = change_program(CHANGED_ROW);
    uint32_t n_sources = 0, out_width = 0;
    CHECK(ts_collect_check(group.data(), group.size(), &n_sources, &out_width));
    bool as_expected = n_sources == 1 && out_width == 6;
    const ts_fri_config fri = {2, 28, 8};
    for (int round = 0; round < 2; round++) {  // 0: proved and verified (a proof consumes its traces); 1: one final
                                               // value changed in HBM, checked
        // the only trace the host ever holds goes up; everything below happens in HBM
        ts_matrix *d_access = nullptr, *d_source = nullptr, *d_sorted = nullptr, *d_gapped = nullptr, *d_table = nullptr,
                  *d_final = nullptr;
        CHECK(ts_matrix_upload(ctx, trace.data(), N, 5, &d_access));
        CHECK(ts_matrix_derive(ctx, source.data(), source.size(), d_access, &d_source));
        ts_sort_spec sort;
        sort.struct_size = sizeof(ts_sort_spec);
        sort.n_keys = 2;
        sort.key_columns[0] = 0;
        sort.key_columns[1] = 1;
        sort.key_columns[2] = sort.key_columns[3] = 0;
        sort.group_keys = 1;
        sort.flags = TS_SORT_GROUP_START;
        sort.n_live = N;
        CHECK(ts_matrix_sort_rows(ctx, &sort, d_source, &d_sorted));
        CHECK(ts_matrix_derive(ctx, gap.data(), gap.size(), d_sorted, &d_gapped));
        CHECK(ts_matrix_derive(ctx, last.data(), last.size(), d_gapped, &d_table));
        ts_matrix_free(ctx, d_source);
        ts_matrix_free(ctx, d_sorted);
        ts_matrix_free(ctx, d_gapped);

        // the final table: ONE group call over the sorted table
        const ts_matrix* sources[1] = {d_table};
        uint64_t n_groups = 0, final_height = 0;
        uint32_t final_width = 0;
        CHECK(ts_matrix_collect_rows(ctx, group.data(), group.size(), sources, 0, &d_final, &n_groups));
        CHECK(ts_matrix_dims(d_final, &final_height, &final_width));
        if (round == 0)
            printf("memory_final_resident: %llu accesses over %u addresses: %llu groups, final table of %llu rows x %u "
                   "grouped in HBM\n", (unsigned long long)N, N_ADDR, (unsigned long long)n_groups,
                   (unsigned long long)final_height, final_width);
        as_expected = as_expected && n_groups == memory.size() && final_width == 6 && final_height >= n_groups &&
                      CHANGED_ROW < n_groups;
        if (round == 1) {  // value + 1 on one row of the final table
            ts_matrix* d_changed = nullptr;
            CHECK(ts_matrix_derive(ctx, change.data(), change.size(), d_final, &d_changed));
            ts_matrix_free(ctx, d_final);
            d_final = d_changed;
        }

        // the range table: (row index, multiplicity) from a matrix of zeros
        const std::vector<uint32_t> zeros(N * 2, 0);
        ts_matrix *d_zero = nullptr, *d_range = nullptr;
        CHECK(ts_matrix_upload(ctx, zeros.data(), N, 2, &d_zero));
        CHECK(ts_matrix_derive(ctx, index.data(), index.size(), d_zero, &d_range));
        ts_matrix_free(ctx, d_zero);
        const ts_logup_term entry[] = {{1, 0}}, gap_col[] = {{1, 6}}, live[] = {{1, 4}};
        const ts_logup_bus_looker looker = {1, 0, gap_col, live};
        const ts_logup_mult_bus_spec fill = {sizeof(ts_logup_mult_bus_spec), 1, entry, 1, 1, &looker, 1, 0};
        const ts_matrix* lookers[1] = {d_table};
        uint64_t n_missing = 0, first_missing[3];
        CHECK(ts_logup_multiplicities_bus(ctx, &fill, d_range, lookers, &n_missing, first_missing));
        as_expected = as_expected && n_missing == 0;

        ts_matrix* traces[4] = {d_access, d_table, d_final, d_range};
        ts_multi_bus_table tables[4];
        for (int t = 0; t < 4; t++) {
            tables[t].struct_size = sizeof(ts_multi_bus_table);
            tables[t].n_public = 0;
            tables[t].air = airs[t];
            tables[t].trace = traces[t];
            tables[t].public_values = nullptr;
            tables[t].logup = specs[t];
        }
        if (round == 0) {
            ts_challenger *challenger = nullptr, *fresh = nullptr;
            CHECK(ts_chal_new(0, 1, &challenger));
            CHECK(ts_chal_new(0, 1, &fresh));
            std::vector<uint32_t> proof(1u << 20);
            size_t n_words = 0;
            CHECK(ts_prove_multi_bus(ctx, &fri, challenger, tables, 4, proof.data(), proof.size(), &n_words));
            const ts_air* const_airs[4] = {airs[0], airs[1], airs[2], airs[3]};
            const uint32_t n_public[4] = {0, 0, 0, 0};
            const uint32_t* values[4] = {nullptr, nullptr, nullptr, nullptr};
            uint32_t exposed[16], bus_sum[4] = {1, 1, 1, 1};
            int verdict = -1;
            CHECK(ts_verify_multi_bus(&fri, fresh, const_airs, 4, values, n_public, proof.data(), n_words, exposed, 16,
                                      bus_sum, &verdict));
            const bool zero = !(bus_sum[0] | bus_sum[1] | bus_sum[2] | bus_sum[3]);
            printf("memory_final_resident: proof of %zu words, verify -> %d, bus sum %s\n", n_words, verdict,
                   zero ? "zero" : "not zero");
            as_expected = as_expected && verdict == 0 && zero;
            ts_chal_free(challenger);
            ts_chal_free(fresh);
        } else {
            const uint32_t challenges[8] = {12345, 678, 9, 10, 11, 12, 13, 14};  // any serve a check
            int32_t bad_table = 0;
            int64_t first_violation = 0;
            ts_bus_report report;
            report.struct_size = sizeof(ts_bus_report);
            ts_bus_share shares[4];
            CHECK(ts_check_multi(ctx, nullptr, tables, 4, challenges, &bad_table, &first_violation, &report, shares));
            printf("memory_final_resident: final value changed in row %llu of the final table: constraints %s; %llu "
                   "tuples out of balance\n", (unsigned long long)CHANGED_ROW,
                   bad_table < 0 ? "hold in every table" : "VIOLATED", (unsigned long long)report.n_unbalanced);
            printf("memory_final_resident: unbalanced: table %u, row %u sent (", report.first_table, report.first_row);
            for (uint32_t q = 0; q < report.n_values; q++) printf(q ? ", %u" : "%u", report.tuple[q]);
            printf("), multiplicity sum %u\n", report.sum);
            // the sorted table still sends the true tuple, which nobody receives.  On a sorted table the groups come in
            // address order: row CHANGED_ROW of the final table is the fourth address
            auto it = memory.begin();
            for (uint64_t k = 0; k < CHANGED_ROW; k++) ++it;
            as_expected = as_expected && bad_table < 0 && report.n_unbalanced == 2 && report.first_table == 1 &&
                          report.first_interaction == 2 && report.n_values == 4 && report.tuple[0] == FIN_TAG &&
                          report.tuple[1] == it->first && report.tuple[2] == last_clock[it->first] &&
                          report.tuple[3] == it->second && report.sum == 1;
        }
        for (int t = 0; t < 4; t++) ts_matrix_free(ctx, traces[t]);
    }
    for (int t = 0; t < 4; t++) ts_air_free(ctx, airs[t]);
    ts_ctx_destroy(ctx);
    printf("memory_final_resident: %s\n", as_expected ? "as expected" : "NOT as expected");
    return as_expected ? 0 : 1;
}
