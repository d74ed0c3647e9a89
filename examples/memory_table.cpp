// examples/memory_table.cpp -- a memory table on the bus, against the public C ABI only (include/tapstark.h + the
// header-only AIR capture).  64 accesses of a small memory stand in execution order in one table (MemoryAccessAir);
// a second table (MemoryTableAir) holds the same accesses sorted by (address, clock), where "a read returns the last
// value written" is a constraint between neighbouring rows.  That second table is made in HBM: ts_matrix_sort_rows
// orders the rows and appends the group-start column.  A LogUp bus ties the two tables, and a range table takes the
// `gap` of every sorted row, which is what makes "sorted" a proved statement.  The three tables are proved with
// ts_prove_multi_bus and verified, and the bus sums to zero.  Then one read value is changed in the sorted table and
// ts_check_multi names the access that no longer has a partner.
//
//   g++ -std=c++17 -I include examples/memory_table.cpp -L tap-stark_amd/lib -ltapstark_hip -o memory_table
//   ./memory_table
#include <stdio.h>

#include <map>
#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t P = 0x78000001;
constexpr uint32_t MEM_TAG = 11, RANGE_TAG = 7;
constexpr uint64_t N = 64;       // accesses, and the height of all three tables
constexpr uint32_t N_ADDR = 8;

using ts::air::Expr;

// main columns (addr, clk, value, is_write, sel): the row sends (MEM_TAG, addr, clk, value, is_write) sel times
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
        logup.eval(builder);
    }
};

// main columns (addr, clk, value, is_write, live, recv, gap, start), sorted by (addr, clk); `start` is the group-start
// column of ts_matrix_sort_rows.  The row receives the access (recv = -live) and sends (RANGE_TAG, gap) live times.
struct MemoryTableAir {
    ts::air::LogUp logup{{{{1, 5}, {{0, MEM_TAG}, {1, 0}, {1, 1}, {1, 2}, {1, 3}}}, {{1, 4}, {{0, RANGE_TAG}, {1, 6}}}}};
    uint32_t width() const { return 8; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        const Expr live = local[4], start = local[7], is_write = local[3];
        const Expr next_cont = next[4] - next[7];
        builder.assert_zero(live * (live - 1));
        builder.assert_zero(start * (start - 1));
        builder.assert_zero(is_write * (is_write - 1));
        builder.assert_zero(start * (live - 1));
        builder.assert_zero(local[5] + live);
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(live - start);
        builder.assert_zero(start * (is_write - 1));  // the first access of an address is a write
        auto t = builder.when_transition();
        t.assert_zero((live - 1) * next[4]);                                     // dead rows stay dead
        t.assert_zero(next_cont * (next[0] - local[0]));                         // one address per group
        t.assert_zero(next_cont * (next[3] - 1) * (next[2] - local[2]));         // a read returns the last value
        t.assert_zero(next[7] * (next[0] - local[0] - 1 - next[6]) + next_cont * (next[1] - local[1] - 1 - next[6]));
        logup.eval(builder);
    }
};

// main columns (table, mult): the table column is the row index
struct RangeAir {
    ts::air::LogUp logup{{{{1, 1}, {{0, RANGE_TAG}, {1, 0}}}}};
    uint32_t width() const { return 2; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(local[0]);
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
    const MemoryAccessAir access_air;
    const MemoryTableAir table_air;
    const RangeAir range_air;
    const std::vector<uint32_t> tapes[3] = {tape_of(access_air), tape_of(table_air), tape_of(range_air)};
    const Spec spec_access(access_air.logup), spec_table(table_air.logup), spec_range(range_air.logup);
    const ts_logup_spec* specs[3] = {&spec_access.spec, &spec_table.spec, &spec_range.spec};
    ts_air* airs[3] = {nullptr, nullptr, nullptr};
    for (int t = 0; t < 3; t++) CHECK(ts_air_compile(ctx, tapes[t].data(), tapes[t].size(), &airs[t]));
    const uint32_t widths[3] = {5, 8, 2};

    // the accesses in execution order: reads return the last write, the first access of an address is a write
    std::vector<uint32_t> accesses(N * 5), source(N * 7);
    std::map<uint32_t, uint32_t> memory;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (uint64_t r = 0; r < N; r++) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t addr = (uint32_t)((state >> 33) % N_ADDR);
        const bool write = ((state >> 20) & 1) || !memory.count(addr);
        if (write) memory[addr] = (uint32_t)((state >> 8) % P);
        const uint32_t row[5] = {addr, (uint32_t)r, memory[addr], write, 1};
        for (int c = 0; c < 5; c++) accesses[r * 5 + c] = row[c];
        for (int c = 0; c < 4; c++) source[r * 7 + c] = row[c];
        source[r * 7 + 4] = 1;      // live
        source[r * 7 + 5] = P - 1;  // recv = -live
        source[r * 7 + 6] = 0;      // gap: derived below
    }

    // sorted by (addr, clk) in HBM, with the group-start column appended as column 7
    ts_matrix *d_source = nullptr, *d_sorted = nullptr;
    CHECK(ts_matrix_upload(ctx, source.data(), N, 7, &d_source));
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
    // `gap` is a derived arithmetic column: the caller's own (here on the host; in production a kernel of the caller
    // over ts_matrix_device_ptr)
    std::vector<uint32_t> sorted(N * 8);
    CHECK(ts_matrix_download(ctx, d_sorted, sorted.data()));
    ts_matrix_free(ctx, d_source);
    ts_matrix_free(ctx, d_sorted);
    uint32_t groups = 0, changed_row = 0;
    for (uint64_t r = 0; r < N; r++) {
        const uint32_t* row = &sorted[r * 8];
        groups += row[7];
        if (r) sorted[r * 8 + 6] = (row[7] ? row[0] - row[-8] : row[1] - row[-7]) - 1;
        if (!changed_row && !row[3]) changed_row = (uint32_t)r;  // the first read of the sorted table
    }
    printf("memory_table: %llu accesses over %u addresses sorted in HBM, %u groups\n", (unsigned long long)N, N_ADDR,
           groups);

    const ts_fri_config fri = {2, 28, 8};
    bool as_expected = true;
    for (int round = 0; round < 2; round++) {  // 0: proved and verified; 1: one read value changed, checked
        std::vector<uint32_t> table = sorted, range(N * 2);
        if (round == 1) table[changed_row * 8 + 2] ^= 1;
        for (uint64_t r = 0; r < N; r++) range[2 * r] = (uint32_t)r;  // mult: filled on the device below
        const uint32_t* rows[3] = {accesses.data(), table.data(), range.data()};
        ts_multi_bus_table tables[3];
        for (int t = 0; t < 3; t++) {
            tables[t].struct_size = sizeof(ts_multi_bus_table);
            tables[t].n_public = 0;
            tables[t].air = airs[t];
            tables[t].trace = nullptr;
            tables[t].public_values = nullptr;
            tables[t].logup = specs[t];
            CHECK(ts_matrix_upload(ctx, rows[t], N, widths[t], &tables[t].trace));
        }
        // mult = MINUS the number of live rows whose gap is the entry
        const ts_logup_term entry[] = {{1, 0}}, gap[] = {{1, 6}}, live[] = {{1, 4}};
        const ts_logup_bus_looker looker = {1, 0, gap, live};
        const ts_logup_mult_bus_spec fill = {sizeof(ts_logup_mult_bus_spec), 1, entry, 1, 1, &looker, 1, 0};
        const ts_matrix* lookers[1] = {tables[1].trace};
        uint64_t n_missing = 0, first_missing[3];
        CHECK(ts_logup_multiplicities_bus(ctx, &fill, tables[2].trace, lookers, &n_missing, first_missing));
        as_expected = as_expected && n_missing == 0;

        if (round == 0) {
            ts_challenger *challenger = nullptr, *fresh = nullptr;
            CHECK(ts_chal_new(0, 1, &challenger));
            CHECK(ts_chal_new(0, 1, &fresh));
            std::vector<uint32_t> proof(1u << 20);
            size_t n_words = 0;
            CHECK(ts_prove_multi_bus(ctx, &fri, challenger, tables, 3, proof.data(), proof.size(), &n_words));
            const ts_air* const_airs[3] = {airs[0], airs[1], airs[2]};
            const uint32_t n_public[3] = {0, 0, 0};
            const uint32_t* values[3] = {nullptr, nullptr, nullptr};
            uint32_t exposed[12], bus_sum[4] = {1, 1, 1, 1};
            int verdict = -1;
            CHECK(ts_verify_multi_bus(&fri, fresh, const_airs, 3, values, n_public, proof.data(), n_words, exposed, 12,
                                      bus_sum, &verdict));
            const bool zero = !(bus_sum[0] | bus_sum[1] | bus_sum[2] | bus_sum[3]);
            printf("memory_table: proof of %zu words, verify -> %d, bus sum %s\n", n_words, verdict,
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
            ts_bus_share shares[3];
            CHECK(ts_check_multi(ctx, nullptr, tables, 3, challenges, &bad_table, &first_violation, &report, shares));
            const uint32_t* was = &sorted[changed_row * 8];
            printf("memory_table: read value changed in sorted row %u: constraint violated in table %d at row %lld; "
                   "%llu tuples out of balance\n", changed_row, bad_table, (long long)(first_violation >> 16),
                   (unsigned long long)report.n_unbalanced);
            printf("memory_table: unbalanced: table %u, row %u sent (", report.first_table, report.first_row);
            for (uint32_t q = 0; q < report.n_values; q++) printf(q ? ", %u" : "%u", report.tuple[q]);
            printf("), multiplicity sum %u\n", report.sum);
            // the access table still sends the true read; nobody receives it any more
            as_expected = as_expected && bad_table == 1 && first_violation >> 16 == (int64_t)changed_row - 1 &&
                          report.n_unbalanced == 2 && report.first_table == 0 && report.first_row == was[1] &&
                          report.n_values == 5 && report.tuple[0] == MEM_TAG && report.tuple[1] == was[0] &&
                          report.tuple[2] == was[1] && report.tuple[3] == was[2] && report.tuple[4] == 0 &&
                          report.sum == 1 && shares[0].count == 1 && shares[1].count == 0 && shares[2].count == 0;
        }
        for (int t = 0; t < 3; t++) ts_matrix_free(ctx, tables[t].trace);
    }
    for (int t = 0; t < 3; t++) ts_air_free(ctx, airs[t]);
    ts_ctx_destroy(ctx);
    printf("memory_table: %s\n", as_expected ? "as expected" : "NOT as expected");
    return as_expected ? 0 : 1;
}
