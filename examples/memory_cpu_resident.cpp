// examples/memory_cpu_resident.cpp -- examples/memory_fill_resident.cpp for a producer that has no access table: a
// machine trace with one row per step and two conditional access slots per row.  The access table is made in HBM:
//   1. ts_matrix_collect_rows: slot a (a read) and slot b (a read or a write) of every CPU row, where selected, become
//      rows (addr, ts, value, is_write, 1) in execution order, padded with zero rows to a power of two; n_live comes
//      back from the call;
//   2. ts_matrix_derive, source program; 3. ts_matrix_sort_rows by (addr, ts) with that n_live; 4. ts_matrix_derive,
//      helper program; 5. ts_matrix_scan: the value every read returns; 6. ts_matrix_derive, gap program;
//   7. the range table and its multiplicities;  8. ts_prove_multi_bus over (CPU table, memory table, range table);
//   9. ts_verify_multi_bus: accepted, the bus sums to zero.
// The only trace that goes up is the CPU trace.  Then one read value of the CPU trace is changed, the same route is
// taken again, and ts_check_multi names the tuple nobody receives.
//
//   g++ -std=c++17 -I include examples/memory_cpu_resident.cpp -L tap-stark_amd/lib -ltapstark_hip -o memory_cpu_resident
//   ./memory_cpu_resident
#include <stdio.h>

#include <map>
#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t P = 0x78000001;
constexpr uint32_t MEM_TAG = 11, RANGE_TAG = 7;
constexpr uint64_t N_CPU = 32;   // CPU rows: at most 64 accesses, timestamps below 64
constexpr uint64_t N_RANGE = 64;
constexpr uint32_t N_ADDR = 8;
enum { CLK, TS_A, ADDR_A, VAL_A, SEL_A, TS_B, ADDR_B, VAL_B, WR_B, SEL_B, CPU_WIDTH };

using ts::air::Collect;
using ts::air::DExpr;
using ts::air::Expr;

struct MemoryCpuAir {
    ts::air::LogUp logup{{{{1, SEL_A}, {{0, MEM_TAG}, {1, ADDR_A}, {1, TS_A}, {1, VAL_A}, {0, 0}}},
                          {{1, SEL_B}, {{0, MEM_TAG}, {1, ADDR_B}, {1, TS_B}, {1, VAL_B}, {1, WR_B}}}}};
    uint32_t width() const { return CPU_WIDTH; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        for (int c : {SEL_A, SEL_B, WR_B}) {
            const Expr b = local[c];
            builder.assert_zero(b * (b - 1));
        }
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(local[CLK]);
        auto when_transition = builder.when_transition();
        when_transition.assert_eq(next[CLK], local[CLK] + 1);
        builder.assert_eq(local[TS_A], local[CLK] * 2);
        builder.assert_eq(local[TS_B], local[CLK] * 2 + 1);
        logup.eval(builder);
    }
};

// the memory table and the range table of examples/memory_fill_resident.cpp
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

// ---- the collect spec, the four row programs and the scan
std::vector<uint32_t> collect_spec() {  // width 10 -> (addr, ts, value, is_write, sel = 1), one row per selected slot
    Collect c({CPU_WIDTH}, 5);
    c.emit(0, Collect::col(SEL_A),
           {Collect::col(ADDR_A), Collect::col(TS_A), Collect::col(VAL_A), Collect::constant(0), Collect::constant(1)});
    c.emit(0, Collect::col(SEL_B),
           {Collect::col(ADDR_B), Collect::col(TS_B), Collect::col(VAL_B), Collect::col(WR_B), Collect::constant(1)});
    return c.tape();
}

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
    const MemoryCpuAir cpu_air;
    const MemoryTableAir table_air;
    const RangeAir range_air;
    const std::vector<uint32_t> tapes[3] = {tape_of(cpu_air), tape_of(table_air), tape_of(range_air)};
    const Spec spec_cpu(cpu_air.logup), spec_table(table_air.logup), spec_range(range_air.logup);
    const ts_logup_spec* specs[3] = {&spec_cpu.spec, &spec_table.spec, &spec_range.spec};
    ts_air* airs[3] = {nullptr, nullptr, nullptr};
    for (int t = 0; t < 3; t++) CHECK(ts_air_compile(ctx, tapes[t].data(), tapes[t].size(), &airs[t]));

    // the machine: slot a reads an address that has been written, on some rows; slot b reads or writes, on most rows;
    // the first access of an address is a write
    std::vector<uint32_t> cpu(N_CPU * CPU_WIDTH);
    std::map<uint32_t, uint32_t> memory;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto draw = [&state] {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(state >> 33);
    };
    uint64_t n_selected = 0, changed_row = N_CPU;
    for (uint64_t r = 0; r < N_CPU; r++) {
        uint32_t* row = &cpu[r * CPU_WIDTH];
        row[CLK] = (uint32_t)r;
        row[TS_A] = (uint32_t)(2 * r);
        row[TS_B] = (uint32_t)(2 * r + 1);
        row[ADDR_A] = draw() % N_ADDR;
        row[SEL_A] = (draw() & 1) && memory.count(row[ADDR_A]);
        row[VAL_A] = row[SEL_A] ? memory[row[ADDR_A]] : draw() % P;
        row[ADDR_B] = draw() % N_ADDR;
        row[SEL_B] = (draw() & 3) != 0;
        row[WR_B] = (draw() & 1) || !memory.count(row[ADDR_B]);
        row[VAL_B] = row[WR_B] ? draw() % P : memory[row[ADDR_B]];
        if (row[WR_B] && row[SEL_B]) memory[row[ADDR_B]] = row[VAL_B];
        n_selected += row[SEL_A] + row[SEL_B];
        if (row[SEL_A] && changed_row == N_CPU && r >= N_CPU / 2) changed_row = r;  // a read of slot a, for round 1
    }
    if (changed_row == N_CPU) {
        fprintf(stderr, "the machine made no read in slot a\n");
        return 1;
    }

    const std::vector<uint32_t> collect = collect_spec(), source = source_program(), helper = helper_program(),
                                gap = gap_program(), index = index_program();
    const ts::air::Scan fill = fill_scan();
    const ts_fri_config fri = {2, 28, 8};
    bool as_expected = true;
    for (int round = 0; round < 2; round++) {  // 0: proved and verified; 1: one read value changed, checked
        std::vector<uint32_t> trace = cpu;
        if (round == 1) trace[changed_row * CPU_WIDTH + VAL_A] = (trace[changed_row * CPU_WIDTH + VAL_A] + 1) % P;
        // the only trace the host ever holds goes up; everything below happens in HBM
        ts_matrix *d_cpu = nullptr, *d_access = nullptr, *d_source = nullptr, *d_sorted = nullptr, *d_helped = nullptr,
                  *d_filled = nullptr, *d_table = nullptr;
        CHECK(ts_matrix_upload(ctx, trace.data(), N_CPU, CPU_WIDTH, &d_cpu));
        const ts_matrix* sources[1] = {d_cpu};
        uint64_t n_live = 0, height = 0;
        uint32_t width = 0;
        CHECK(ts_matrix_collect_rows(ctx, collect.data(), collect.size(), sources, 0, &d_access, &n_live));
        CHECK(ts_matrix_dims(d_access, &height, &width));
        if (round == 0)
            printf("memory_cpu_resident: %llu CPU rows, %llu of %llu slots selected: access table of %llu rows x %u "
                   "collected in HBM\n", (unsigned long long)N_CPU, (unsigned long long)n_live,
                   (unsigned long long)(2 * N_CPU), (unsigned long long)height, width);
        uint64_t least = 1;  // out_height 0: the least power of two that holds the selected slots
        while (least < n_live) least <<= 1;
        as_expected = as_expected && n_live == n_selected && height == least && height <= N_RANGE && width == 5;
        CHECK(ts_matrix_derive(ctx, source.data(), source.size(), d_access, &d_source));
        ts_sort_spec sort;
        sort.struct_size = sizeof(ts_sort_spec);
        sort.n_keys = 2;
        sort.key_columns[0] = 0;
        sort.key_columns[1] = 1;
        sort.key_columns[2] = sort.key_columns[3] = 0;
        sort.group_keys = 1;
        sort.flags = TS_SORT_GROUP_START;
        sort.n_live = n_live;
        CHECK(ts_matrix_sort_rows(ctx, &sort, d_source, &d_sorted));
        CHECK(ts_matrix_derive(ctx, helper.data(), helper.size(), d_sorted, &d_helped));
        CHECK(ts_matrix_scan(ctx, &fill.spec(), d_helped, &d_filled, nullptr));
        CHECK(ts_matrix_derive(ctx, gap.data(), gap.size(), d_filled, &d_table));
        ts_matrix_free(ctx, d_access);
        ts_matrix_free(ctx, d_source);
        ts_matrix_free(ctx, d_sorted);
        ts_matrix_free(ctx, d_helped);
        ts_matrix_free(ctx, d_filled);

        // the range table: (row index, multiplicity) from a matrix of zeros
        const std::vector<uint32_t> zeros(N_RANGE * 2, 0);
        ts_matrix *d_zero = nullptr, *d_range = nullptr;
        CHECK(ts_matrix_upload(ctx, zeros.data(), N_RANGE, 2, &d_zero));
        CHECK(ts_matrix_derive(ctx, index.data(), index.size(), d_zero, &d_range));
        ts_matrix_free(ctx, d_zero);
        // mult = MINUS the number of live rows whose gap is the entry
        const ts_logup_term entry[] = {{1, 0}}, gap_col[] = {{1, 6}}, live[] = {{1, 4}};
        const ts_logup_bus_looker looker = {1, 0, gap_col, live};
        const ts_logup_mult_bus_spec mult = {sizeof(ts_logup_mult_bus_spec), 1, entry, 1, 1, &looker, 1, 0};
        const ts_matrix* lookers[1] = {d_table};
        uint64_t n_missing = 0, first_missing[3];
        CHECK(ts_logup_multiplicities_bus(ctx, &mult, d_range, lookers, &n_missing, first_missing));
        as_expected = as_expected && n_missing == 0;

        ts_matrix* traces[3] = {d_cpu, d_table, d_range};
        ts_multi_bus_table tables[3];
        for (int t = 0; t < 3; t++) {
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
            CHECK(ts_prove_multi_bus(ctx, &fri, challenger, tables, 3, proof.data(), proof.size(), &n_words));
            const ts_air* const_airs[3] = {airs[0], airs[1], airs[2]};
            const uint32_t n_public[3] = {0, 0, 0};
            const uint32_t* values[3] = {nullptr, nullptr, nullptr};
            uint32_t exposed[12], bus_sum[4] = {1, 1, 1, 1};
            int verdict = -1;
            CHECK(ts_verify_multi_bus(&fri, fresh, const_airs, 3, values, n_public, proof.data(), n_words, exposed, 12,
                                      bus_sum, &verdict));
            const bool zero = !(bus_sum[0] | bus_sum[1] | bus_sum[2] | bus_sum[3]);
            printf("memory_cpu_resident: proof of %zu words, verify -> %d, bus sum %s\n", n_words, verdict,
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
            const uint32_t* was = &cpu[changed_row * CPU_WIDTH];
            printf("memory_cpu_resident: read value changed in CPU row %llu: constraints %s; %llu tuples out of balance\n",
                   (unsigned long long)changed_row, bad_table < 0 ? "hold in every table" : "VIOLATED",
                   (unsigned long long)report.n_unbalanced);
            printf("memory_cpu_resident: unbalanced: table %u, row %u sent (", report.first_table, report.first_row);
            for (uint32_t q = 0; q < report.n_values; q++) printf(q ? ", %u" : "%u", report.tuple[q]);
            printf("), multiplicity sum %u\n", report.sum);
            // the CPU sends the changed read; the memory table, filled from the writes, receives the true one
            as_expected = as_expected && bad_table < 0 && report.n_unbalanced == 2 && report.first_table == 0 &&
                          report.first_row == changed_row && report.first_interaction == 0 && report.n_values == 5 &&
                          report.tuple[0] == MEM_TAG && report.tuple[1] == was[ADDR_A] && report.tuple[2] == was[TS_A] &&
                          report.tuple[3] == (was[VAL_A] + 1) % P && report.tuple[4] == 0 && report.sum == 1;
        }
        for (int t = 0; t < 3; t++) ts_matrix_free(ctx, tables[t].trace);
    }
    for (int t = 0; t < 3; t++) ts_air_free(ctx, airs[t]);
    ts_ctx_destroy(ctx);
    printf("memory_cpu_resident: %s\n", as_expected ? "as expected" : "NOT as expected");
    return as_expected ? 0 : 1;
}
