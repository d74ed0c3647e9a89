// examples/span_chip_resident.cpp -- a chip with a data-dependent number of rows per call, made in HBM: a machine trace
// with one row per step, some of which call a block instruction over `len` words from `base` (a memset, a load
// multiple); the chip spends one row per element.
//   1. ts_matrix_expand_rows: every selected call row becomes `len` rows (id, base, len, j, first, last, live = 1,
//      addr = base + j) in (call, element) order, padded with zero rows to a power of two; n_live comes back;
//   2. ts_matrix_derive appends recv = 0 - first: the chip receives a call once, on its first element;
//   3. the range table and its multiplicities from the chip's addr column: ts_logup_multiplicities_bus;
//   4. ts_prove_multi_bus over (call table, chip table, range table);  5. ts_verify_multi_bus: accepted, bus sum zero.
// The only trace that goes up is the call trace.  Then one span is made to reach past the range table, the same route
// is taken again, and ts_check_multi names the address nobody receives.  The chip AIR is a demonstrator of the route,
// not a vetted chip.
//
//   g++ -std=c++17 -I include examples/span_chip_resident.cpp -L tap-stark_amd/lib -ltapstark_hip -o span_chip_resident
//   ./span_chip_resident
#include <stdio.h>

#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t SPAN_TAG = 17, RANGE_TAG = 7;
constexpr uint64_t N_CALLS = 32;
constexpr uint32_t MAX_LEN = 7;
constexpr uint64_t N_RANGE = 64;  // addresses 0 .. 63
enum { ID, BASE, LEN, SEL, CALL_WIDTH };
enum { C_ID, C_BASE, C_LEN, C_J, C_FIRST, C_LAST, C_LIVE, C_ADDR, C_RECV, CHIP_WIDTH };

using ts::air::Expand;
using ts::air::Expr;

struct SpanCallAir {
    ts::air::LogUp logup{{{{1, SEL}, {{0, SPAN_TAG}, {1, ID}, {1, BASE}, {1, LEN}}}}};
    uint32_t width() const { return CALL_WIDTH; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        const Expr sel = local[SEL];
        builder.assert_zero(sel * (sel - 1));
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(local[ID]);
        auto when_transition = builder.when_transition();
        when_transition.assert_eq(next[ID], local[ID] + 1);
        builder.assert_zero(local[BASE] * sel * (sel - 1));  // implied; constraint degree 3, as the chip
        logup.eval(builder);
    }
};

struct SpanChipAir {
    ts::air::LogUp logup{{{{1, C_RECV}, {{0, SPAN_TAG}, {1, C_ID}, {1, C_BASE}, {1, C_LEN}}},
                          {{1, C_LIVE}, {{0, RANGE_TAG}, {1, C_ADDR}}}}};
    uint32_t width() const { return CHIP_WIDTH; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        const Expr first = local[C_FIRST], last = local[C_LAST], live = local[C_LIVE], j = local[C_J];
        const Expr next_cont = next[C_LIVE] - next[C_FIRST];
        builder.assert_zero(first * (first - 1));
        builder.assert_zero(last * (last - 1));
        builder.assert_zero(live * (live - 1));
        builder.assert_zero(first * (live - 1));
        builder.assert_zero(last * (live - 1));
        builder.assert_zero(local[C_RECV] + first);
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(live - first);
        builder.assert_zero(first * j);
        builder.assert_zero(last * (local[C_LEN] - 1 - j));
        builder.assert_eq(local[C_ADDR], local[C_BASE] + j);
        auto t = builder.when_transition();
        t.assert_zero((live - 1) * next[C_LIVE]);
        for (int c : {C_ID, C_BASE, C_LEN}) t.assert_zero(next_cont * (next[c] - local[c]));
        t.assert_zero(next_cont * (next[C_J] - j - 1));
        t.assert_zero(last * next_cont);
        t.assert_zero(live * (last - 1) * (next_cont - 1));
        auto when_last_row = builder.when_last_row();
        when_last_row.assert_zero(live * (last - 1));
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

std::vector<uint32_t> expand_spec() {  // width 4 -> 8, `len` rows per selected call; the pad row is all zero: a dead row
    Expand e(CALL_WIDTH, 8, MAX_LEN);
    e.count(Expand::col(LEN)).when(Expand::col(SEL));
    e.terms({Expand::col(ID), Expand::col(BASE), Expand::col(LEN), Expand::inner(), Expand::first(), Expand::last(),
             Expand::constant(1), Expand::stepped(BASE, 1)});
    return e.tape();
}

std::vector<uint32_t> recv_program() {  // width 8 -> 9: recv = 0 - first
    ts::air::Derive b(8);
    b.output(-b.col(C_FIRST), C_RECV);
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
    const SpanCallAir call_air;
    const SpanChipAir chip_air;
    const RangeAir range_air;
    const std::vector<uint32_t> tapes[3] = {tape_of(call_air), tape_of(chip_air), tape_of(range_air)};
    const Spec spec_call(call_air.logup), spec_chip(chip_air.logup), spec_range(range_air.logup);
    const ts_logup_spec* specs[3] = {&spec_call.spec, &spec_chip.spec, &spec_range.spec};
    ts_air* airs[3] = {nullptr, nullptr, nullptr};
    for (int t = 0; t < 3; t++) CHECK(ts_air_compile(ctx, tapes[t].data(), tapes[t].size(), &airs[t]));

    // the machine: about half of the steps call the block instruction, over 1 .. 7 words inside the range table; the
    // other rows hold a base and a length all the same, which nobody sends
    std::vector<uint32_t> calls(N_CALLS * CALL_WIDTH);
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto draw = [&state] {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(state >> 33);
    };
    uint64_t n_elements = 0, n_selected = 0, moved_row = N_CALLS;
    for (uint64_t r = 0; r < N_CALLS; r++) {
        uint32_t* row = &calls[r * CALL_WIDTH];
        row[ID] = (uint32_t)r;
        row[LEN] = 1 + draw() % MAX_LEN;
        row[BASE] = draw() % (uint32_t)(N_RANGE + 1 - row[LEN]);
        row[SEL] = draw() & 1;
        if (row[SEL]) {
            n_elements += row[LEN];
            n_selected++;
            if (moved_row == N_CALLS && r >= N_CALLS / 2 && row[LEN] >= 2) moved_row = r;  // a span, for round 1
        }
    }
    if (moved_row == N_CALLS) {
        fprintf(stderr, "the machine made no call of two words or more\n");
        return 1;
    }

    const std::vector<uint32_t> expand = expand_spec(), recv = recv_program(), index = index_program();
    const ts_fri_config fri = {2, 28, 8};
    bool as_expected = true;
    for (int round = 0; round < 2; round++) {  // 0: proved and verified; 1: one span past the range table, checked
        std::vector<uint32_t> trace = calls;
        // its last element is address N_RANGE, the first one outside the table
        if (round == 1) trace[moved_row * CALL_WIDTH + BASE] = (uint32_t)(N_RANGE + 1 - trace[moved_row * CALL_WIDTH + LEN]);
        // the only trace the host ever holds goes up; everything below happens in HBM
        ts_matrix *d_calls = nullptr, *d_rows = nullptr, *d_chip = nullptr;
        CHECK(ts_matrix_upload(ctx, trace.data(), N_CALLS, CALL_WIDTH, &d_calls));
        uint64_t n_live = 0, height = 0;
        uint32_t width = 0;
        CHECK(ts_matrix_expand_rows(ctx, expand.data(), expand.size(), d_calls, 0, &d_rows, &n_live));
        CHECK(ts_matrix_dims(d_rows, &height, &width));
        if (round == 0)
            printf("span_chip_resident: %llu call rows, %llu of them selected: chip table of %llu elements in %llu "
                   "rows x %u expanded in HBM\n", (unsigned long long)N_CALLS, (unsigned long long)n_selected,
                   (unsigned long long)n_live, (unsigned long long)height, width);
        uint64_t least = 1;  // out_height 0: the least power of two that holds the elements
        while (least < n_live) least <<= 1;
        as_expected = as_expected && n_live == n_elements && height == least && width == 8;
        CHECK(ts_matrix_derive(ctx, recv.data(), recv.size(), d_rows, &d_chip));
        ts_matrix_free(ctx, d_rows);

        // the range table: (row index, multiplicity) from a matrix of zeros
        const std::vector<uint32_t> zeros(N_RANGE * 2, 0);
        ts_matrix *d_zero = nullptr, *d_range = nullptr;
        CHECK(ts_matrix_upload(ctx, zeros.data(), N_RANGE, 2, &d_zero));
        CHECK(ts_matrix_derive(ctx, index.data(), index.size(), d_zero, &d_range));
        ts_matrix_free(ctx, d_zero);
        // mult = MINUS the number of live rows whose addr is the entry
        const ts_logup_term entry[] = {{1, 0}}, addr_col[] = {{1, C_ADDR}}, live[] = {{1, C_LIVE}};
        const ts_logup_bus_looker looker = {1, 0, addr_col, live};
        const ts_logup_mult_bus_spec mult = {sizeof(ts_logup_mult_bus_spec), 1, entry, 1, 1, &looker, 1, 0};
        const ts_matrix* lookers[1] = {d_chip};
        uint64_t n_missing = 0, first_missing[3];
        CHECK(ts_logup_multiplicities_bus(ctx, &mult, d_range, lookers, &n_missing, first_missing));
        as_expected = as_expected && n_missing == (round == 0 ? 0u : 1u);

        ts_matrix* traces[3] = {d_calls, d_chip, d_range};
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
            printf("span_chip_resident: proof of %zu words, verify -> %d, bus sum %s\n", n_words, verdict,
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
            printf("span_chip_resident: span of call row %llu moved past the range table: constraints %s; %llu tuple out "
                   "of balance\n", (unsigned long long)moved_row, bad_table < 0 ? "hold in every table" : "VIOLATED",
                   (unsigned long long)report.n_unbalanced);
            printf("span_chip_resident: unbalanced: table %u, row %u sent (", report.first_table, report.first_row);
            for (uint32_t q = 0; q < report.n_values; q++) printf(q ? ", %u" : "%u", report.tuple[q]);
            printf("), multiplicity sum %u\n", report.sum);
            // the chip sends the address of the span's last element, which the range table does not hold
            as_expected = as_expected && bad_table < 0 && report.n_unbalanced == 1 && report.first_table == 1 &&
                          report.first_interaction == 1 && report.n_values == 2 && report.tuple[0] == RANGE_TAG &&
                          report.tuple[1] == N_RANGE && report.sum == 1;
        }
        for (int t = 0; t < 3; t++) ts_matrix_free(ctx, tables[t].trace);
    }
    for (int t = 0; t < 3; t++) ts_air_free(ctx, airs[t]);
    ts_ctx_destroy(ctx);
    printf("span_chip_resident: %s\n", as_expected ? "as expected" : "NOT as expected");
    return as_expected ? 0 : 1;
}
