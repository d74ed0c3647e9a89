// examples/memory_fill_resident.cpp -- examples/memory_table_resident.cpp for a table that does not know yet what its
// reads return: the table-side source holds 0 in `value` on every read, and the values are found in HBM, by a scan.
//   1. ts_matrix_derive, source program: the accesses (addr, clk, value, is_write, sel) become the unsorted table
//      (.., value = is_write * value, live = sel, recv = -live, gap = 0);
//   2. ts_matrix_sort_rows by (addr, clk), the group-start column appended;
//   3. ts_matrix_derive, helper program: two columns appended, a = live (1 - is_write), b = is_write * value;
//   4. ts_matrix_scan: value[i] = a[i] value[i-1] + b[i], started over from 0 where `start` is 1 -- a read returns the
//      last value written to its address; out_width 8 drops the two helper columns again;
//   5. ts_matrix_derive, gap program, as in memory_table_resident.cpp;
//   6. the range table and its multiplicities;  7. ts_prove_multi_bus;  8. ts_verify_multi_bus: accepted, the bus sums to
//      zero -- against the access table, whose reads hold the values the program saw.
// The one download, before the proof consumes the traces, is for the printout.
//
//   g++ -std=c++17 -I include examples/memory_fill_resident.cpp -L tap-stark_amd/lib -ltapstark_hip -o memory_fill_resident
//   ./memory_fill_resident
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

using ts::air::DExpr;
using ts::air::Expr;

// the three AIRs of examples/memory_table.cpp
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
        builder.assert_zero(start * (is_write - 1));
        auto t = builder.when_transition();
        t.assert_zero((live - 1) * next[4]);
        t.assert_zero(next_cont * (next[0] - local[0]));
        t.assert_zero(next_cont * (next[3] - 1) * (next[2] - local[2]));
        t.assert_zero(next[7] * (next[0] - local[0] - 1 - next[6]) + next_cont * (next[1] - local[1] - 1 - next[6]));
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

// ---- the four row programs and the scan
std::vector<uint32_t> source_program() {  // width 5 -> 7: value zeroed on reads, recv = -live, gap = 0
    ts::air::Derive b(5);
    b.output(-b.col(4), 5);
    b.output(b.constant(0), 6);
    b.output(b.col(3) * b.col(2), 2);
    return b.tape();
}

std::vector<uint32_t> helper_program() {  // width 8 -> 10: a = live (1 - is_write), b = is_write * value
    ts::air::Derive b(8);
    const DExpr is_write = b.col(3);
    b.output(b.col(4) * (1 - is_write), 8);
    b.output(is_write * b.col(2), 9);
    return b.tape();
}

ts::air::Scan fill_scan() {  // width 10 -> 8: value = a * previous value + b, from 0 where start is 1
    ts::air::Scan s(8);
    s.add(2, ts::air::Scan::col(8), ts::air::Scan::col(9), 0, 7);
    return s;
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
    const MemoryTableAir table_air;
    const RangeAir range_air;
    const std::vector<uint32_t> tapes[3] = {tape_of(access_air), tape_of(table_air), tape_of(range_air)};
    const Spec spec_access(access_air.logup), spec_table(table_air.logup), spec_range(range_air.logup);
    const ts_logup_spec* specs[3] = {&spec_access.spec, &spec_table.spec, &spec_range.spec};
    ts_air* airs[3] = {nullptr, nullptr, nullptr};
    for (int t = 0; t < 3; t++) CHECK(ts_air_compile(ctx, tapes[t].data(), tapes[t].size(), &airs[t]));

    // the accesses in execution order: reads return the last write, the first access of an address is a write
    std::vector<uint32_t> accesses(N * 5);
    std::map<uint32_t, uint32_t> memory;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (uint64_t r = 0; r < N; r++) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t addr = (uint32_t)((state >> 33) % N_ADDR);
        const bool write = ((state >> 20) & 1) || !memory.count(addr);
        if (write) memory[addr] = (uint32_t)((state >> 8) % P);
        const uint32_t row[5] = {addr, (uint32_t)r, memory[addr], write, 1};
        for (int c = 0; c < 5; c++) accesses[r * 5 + c] = row[c];
    }

    // the only trace the host ever holds goes up; everything below happens in HBM
    ts_matrix *d_access = nullptr, *d_source = nullptr, *d_sorted = nullptr, *d_helped = nullptr, *d_filled = nullptr,
              *d_table = nullptr;
    CHECK(ts_matrix_upload(ctx, accesses.data(), N, 5, &d_access));
    const std::vector<uint32_t> source = source_program(), helper = helper_program(), gap = gap_program(),
                                index = index_program();
    const ts::air::Scan fill = fill_scan();
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
    CHECK(ts_matrix_derive(ctx, helper.data(), helper.size(), d_sorted, &d_helped));
    uint32_t last_value = 0;
    CHECK(ts_matrix_scan(ctx, &fill.spec(), d_helped, &d_filled, &last_value));
    CHECK(ts_matrix_derive(ctx, gap.data(), gap.size(), d_filled, &d_table));
    ts_matrix_free(ctx, d_source);
    ts_matrix_free(ctx, d_sorted);
    ts_matrix_free(ctx, d_helped);
    ts_matrix_free(ctx, d_filled);

    // the range table: (row index, multiplicity) from a matrix of zeros
    const std::vector<uint32_t> zeros(N * 2, 0);
    ts_matrix *d_zero = nullptr, *d_range = nullptr;
    CHECK(ts_matrix_upload(ctx, zeros.data(), N, 2, &d_zero));
    CHECK(ts_matrix_derive(ctx, index.data(), index.size(), d_zero, &d_range));
    ts_matrix_free(ctx, d_zero);
    // mult = MINUS the number of live rows whose gap is the entry
    const ts_logup_term entry[] = {{1, 0}}, gap_col[] = {{1, 6}}, live[] = {{1, 4}};
    const ts_logup_bus_looker looker = {1, 0, gap_col, live};
    const ts_logup_mult_bus_spec mult = {sizeof(ts_logup_mult_bus_spec), 1, entry, 1, 1, &looker, 1, 0};
    const ts_matrix* lookers[1] = {d_table};
    uint64_t n_missing = 0, first_missing[3];
    CHECK(ts_logup_multiplicities_bus(ctx, &mult, d_range, lookers, &n_missing, first_missing));
    bool as_expected = n_missing == 0;
    printf("memory_fill_resident: %llu accesses over %u addresses: table and range table made in HBM, %llu gaps "
           "outside the range table\n", (unsigned long long)N, N_ADDR, (unsigned long long)n_missing);

    // the first group of the table: what its reads return was found by the scan (the proof consumes the traces, so the
    // one download, for this printout, comes before it)
    std::vector<uint32_t> table(N * 8);
    CHECK(ts_matrix_download(ctx, d_table, table.data()));
    printf("memory_fill_resident: address %u:", table[0]);
    for (uint64_t r = 0; r < N && (r == 0 || !table[r * 8 + 7]); r++) {
        printf(" clk %u %s %u;", table[r * 8 + 1], table[r * 8 + 3] ? "writes" : "reads", table[r * 8 + 2]);
        as_expected = as_expected && table[r * 8 + 2] == accesses[(uint64_t)table[r * 8 + 1] * 5 + 2];
    }
    printf("\nmemory_fill_resident: the last row's value %u\n", last_value);
    as_expected = as_expected && last_value == table[(N - 1) * 8 + 2];

    ts_matrix* traces[3] = {d_access, d_table, d_range};
    ts_multi_bus_table tables[3];
    for (int t = 0; t < 3; t++) {
        tables[t].struct_size = sizeof(ts_multi_bus_table);
        tables[t].n_public = 0;
        tables[t].air = airs[t];
        tables[t].trace = traces[t];
        tables[t].public_values = nullptr;
        tables[t].logup = specs[t];
    }
    const ts_fri_config fri = {2, 28, 8};
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
    CHECK(ts_verify_multi_bus(&fri, fresh, const_airs, 3, values, n_public, proof.data(), n_words, exposed, 12, bus_sum,
                              &verdict));
    const bool zero = !(bus_sum[0] | bus_sum[1] | bus_sum[2] | bus_sum[3]);
    printf("memory_fill_resident: proof of %zu words, verify -> %d, bus sum %s\n", n_words, verdict,
           zero ? "zero" : "not zero");
    as_expected = as_expected && verdict == 0 && zero;
    ts_chal_free(challenger);
    ts_chal_free(fresh);
    for (int t = 0; t < 3; t++) ts_matrix_free(ctx, tables[t].trace);
    for (int t = 0; t < 3; t++) ts_air_free(ctx, airs[t]);
    ts_ctx_destroy(ctx);
    printf("memory_fill_resident: %s\n", as_expected ? "as expected" : "NOT as expected");
    return as_expected ? 0 : 1;
}
