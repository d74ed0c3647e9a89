// examples/sponge_chip_resident.cpp -- a chip whose state column is a NONLINEAR recurrence, filled in HBM: a machine
// trace with one row per step, some of which call a sponge over the `len` words w0, w0 + 1, ...; the chip spends one row
// per absorbed word, acc = (the IV on a call's first row, else the state of the row before) + word, state = acc^7.
//   1. ts_matrix_expand_rows: every selected call row becomes `len` rows (first, last, id, word, 0, 0) in (call, word)
//      order, padded to a power of two with rows that start a call of their own;
//   2. the iterate form of ts_matrix_derive -- a TITR program with one carry, a group per call -- fills acc and state:
//      one lane per call walks its rows;
//   3. ts_matrix_join_rows fetches each call's digest, the state of its last row, back into the call trace by id;
//   4. ts_prove_multi_bus over (call table, chip table);  5. ts_verify_multi_bus: accepted, bus sum zero.
// The only trace that goes up is the call trace, and no trace comes down.  Then one absorbed word is changed after the
// digests were fetched, the chip is filled again, and ts_check_multi names the digest nobody receives.  The chip AIR is
// a demonstrator of the route, not a vetted chip.
//
//   g++ -std=c++17 -I include examples/sponge_chip_resident.cpp -L tap-stark_amd/lib -ltapstark_hip -o sponge_chip_resident
//   ./sponge_chip_resident
#include <stdio.h>

#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t SPONGE_TAG = 19, IV = 0x5EED, P = 0x78000001u;
constexpr uint64_t N_CALLS = 32;
constexpr uint32_t MAX_LEN = 12;
enum { ID, W0, LEN, SEL, DIGEST, RECV, CALL_WIDTH };
enum { C_FIRST, C_LAST, C_ID, C_WORD, C_ACC, C_STATE, CHIP_WIDTH };

using ts::air::DExpr;
using ts::air::Expand;
using ts::air::Expr;

struct SpongeCallAir {
    ts::air::LogUp logup{{{{1, RECV}, {{0, SPONGE_TAG}, {1, ID}, {1, DIGEST}}}}};
    uint32_t width() const { return CALL_WIDTH; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        const Expr sel = local[SEL];
        builder.assert_zero(sel * (sel - 1));
        builder.assert_zero(local[RECV] + sel);
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(local[ID]);
        auto when_transition = builder.when_transition();
        when_transition.assert_eq(next[ID], local[ID] + 1);
        builder.assert_zero(local[W0] * sel * (sel - 1));  // implied; constraint degree 3, as every bus AIR
        logup.eval(builder);
    }
};

struct SpongeChipAir {
    ts::air::LogUp logup{{{{1, C_LAST}, {{0, SPONGE_TAG}, {1, C_ID}, {1, C_STATE}}}}};
    uint32_t width() const { return CHIP_WIDTH; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        const Expr first = local[C_FIRST], last = local[C_LAST], acc = local[C_ACC];
        builder.assert_zero(first * (first - 1));
        builder.assert_zero(last * (last - 1));
        const Expr a2 = acc * acc;
        const Expr a4 = a2 * a2;
        builder.assert_eq(local[C_STATE], a4 * a2 * acc);  // degree 7
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_eq(acc, local[C_WORD] + IV);
        auto t = builder.when_transition();
        const Expr stops = next[C_FIRST] - 1;  // 0 where the next row starts a call, -1 where it continues one
        t.assert_eq(next[C_ACC], next[C_FIRST] * IV - stops * local[C_STATE] + next[C_WORD]);
        t.assert_zero(stops * (next[C_ID] - local[C_ID]));
        t.assert_zero(last * stops);
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

std::vector<uint32_t> expand_spec() {  // width 6 -> 6, `len` rows per selected call; a pad row starts a call of its own
    Expand e(CALL_WIDTH, CHIP_WIDTH, MAX_LEN, {1});
    e.count(Expand::col(LEN)).when(Expand::col(SEL));
    e.terms({Expand::first(), Expand::last(), Expand::col(ID), Expand::stepped(W0, 1), Expand::constant(0),
             Expand::constant(0)});
    return e.tape();
}

std::vector<uint32_t> sponge_program() {  // one carry: the state after the previous row of the call
    ts::air::Iterate b(CHIP_WIDTH, C_FIRST, MAX_LEN);
    DExpr state = b.carry(IV);
    DExpr word = b.col(C_WORD);
    DExpr acc = state + word;
    DExpr a2 = acc * acc;
    DExpr a4 = a2 * a2;
    DExpr a6 = a4 * a2;
    DExpr next = a6 * acc;
    b.set_carry(state, next);
    b.output(acc, C_ACC);
    b.output(next, C_STATE);
    return b.tape();
}

uint32_t pow7(uint64_t x) {
    const uint64_t x2 = x * x % P, x4 = x2 * x2 % P;
    return (uint32_t)(x4 * x2 % P * x % P);
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
    const SpongeCallAir call_air;
    const SpongeChipAir chip_air;
    const std::vector<uint32_t> tapes[2] = {tape_of(call_air), tape_of(chip_air)};
    const Spec spec_call(call_air.logup), spec_chip(chip_air.logup);
    const ts_logup_spec* specs[2] = {&spec_call.spec, &spec_chip.spec};
    ts_air* airs[2] = {nullptr, nullptr};
    for (int t = 0; t < 2; t++) CHECK(ts_air_compile(ctx, tapes[t].data(), tapes[t].size(), &airs[t]));

    // the machine: about half of the steps call the sponge, over 1 .. 12 words; the digest column is blank
    std::vector<uint32_t> trace(N_CALLS * CALL_WIDTH, 0);
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto draw = [&rng] {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(rng >> 33);
    };
    uint64_t n_words_absorbed = 0, n_selected = 0, changed_call = N_CALLS;
    uint32_t changed_digest = 0;
    for (uint64_t r = 0; r < N_CALLS; r++) {
        uint32_t* row = &trace[r * CALL_WIDTH];
        row[ID] = (uint32_t)r;
        row[W0] = draw() % P;
        row[LEN] = 1 + draw() % MAX_LEN;
        row[SEL] = draw() & 1;
        row[RECV] = row[SEL] ? P - 1 : 0;
        if (!row[SEL]) continue;
        n_words_absorbed += row[LEN];
        n_selected++;
        if (changed_call == N_CALLS && r >= N_CALLS / 2) {  // the call whose last word round 1 changes, and its digest
            changed_call = r;
            uint32_t state = IV;
            for (uint32_t j = 0; j < row[LEN]; j++) state = pow7(((uint64_t)state + row[W0] + j) % P);
            changed_digest = state;
        }
    }
    if (changed_call == N_CALLS) {
        fprintf(stderr, "the machine made no call in its second half\n");
        return 1;
    }

    const std::vector<uint32_t> expand = expand_spec(), program = sponge_program();
    const ts_fri_config fri = {3, 28, 8};  // state = acc^7: eight quotient chunks
    bool as_expected = true;
    // the only trace the host ever holds goes up; everything below happens in HBM
    ts_matrix *d_blank = nullptr, *d_rows = nullptr, *d_chip = nullptr, *d_calls = nullptr;
    CHECK(ts_matrix_upload(ctx, trace.data(), N_CALLS, CALL_WIDTH, &d_blank));
    uint64_t n_live = 0, height = 0;
    uint32_t width = 0;
    CHECK(ts_matrix_expand_rows(ctx, expand.data(), expand.size(), d_blank, 0, &d_rows, &n_live));
    CHECK(ts_matrix_dims(d_rows, &height, &width));
    printf("sponge_chip_resident: %llu call rows, %llu of them selected: chip table of %llu words in %llu rows x %u "
           "expanded in HBM\n", (unsigned long long)N_CALLS, (unsigned long long)n_selected, (unsigned long long)n_live,
           (unsigned long long)height, width);
    as_expected = as_expected && n_live == n_words_absorbed && width == CHIP_WIDTH;
    CHECK(ts_matrix_derive(ctx, program.data(), program.size(), d_rows, &d_chip));  // the iterate form: a TITR tape

    // digest <- the state of the chip row with the call's id and last = 1
    const ts_logup_term src_keys[] = {{1, ID}, {0, 1}}, table_keys[] = {{1, C_ID}, {1, C_LAST}};
    const uint32_t table_columns[] = {C_STATE}, dst_columns[] = {DIGEST}, defaults[] = {0};
    const ts_join_spec join = {sizeof(ts_join_spec), 2, src_keys, table_keys, {1, SEL}, 1, table_columns, dst_columns,
                               defaults, TS_JOIN_KEEP, 0};
    CHECK(ts_matrix_join_rows(ctx, &join, d_blank, d_chip, &d_calls, nullptr, nullptr));  // a miss would be an error
    ts_matrix_free(ctx, d_blank);

    for (int round = 0; round < 2; round++) {  // 0: proved and verified; 1: one absorbed word changed, checked
        ts_matrix* chip = d_chip;
        if (round == 1) {
            // the last word of one call is taken one further, in HBM: a TDER program over the expanded rows, then the
            // sponge again; the call trace keeps the digest it fetched before
            ts::air::Derive b(CHIP_WIDTH);
            DExpr id = b.col(C_ID);
            DExpr hit = (id - changed_call).is_zero() * b.col(C_LAST);
            b.output(b.col(C_WORD) + hit, C_WORD);
            const std::vector<uint32_t> bump = b.tape();
            ts_matrix* d_bumped = nullptr;
            CHECK(ts_matrix_derive(ctx, bump.data(), bump.size(), d_rows, &d_bumped));
            CHECK(ts_matrix_derive(ctx, program.data(), program.size(), d_bumped, &chip));
            ts_matrix_free(ctx, d_bumped);
        }
        ts_matrix* traces[2] = {d_calls, chip};
        ts_multi_bus_table tables[2];
        for (int t = 0; t < 2; t++) {
            tables[t].struct_size = sizeof(ts_multi_bus_table);
            tables[t].n_public = 0;
            tables[t].air = airs[t];
            tables[t].trace = traces[t];
            tables[t].public_values = nullptr;
            tables[t].logup = specs[t];
        }
        if (round == 1) {
            const uint32_t challenges[8] = {12345, 678, 9, 10, 11, 12, 13, 14};  // any serve a check
            int32_t bad_table = 0;
            int64_t first_violation = 0;
            ts_bus_report report;
            report.struct_size = sizeof(ts_bus_report);
            ts_bus_share shares[2];
            CHECK(ts_check_multi(ctx, nullptr, tables, 2, challenges, &bad_table, &first_violation, &report, shares));
            printf("sponge_chip_resident: last word of call %llu changed: constraints %s; %llu tuples out of balance\n",
                   (unsigned long long)changed_call, bad_table < 0 ? "hold in every table" : "VIOLATED",
                   (unsigned long long)report.n_unbalanced);
            printf("sponge_chip_resident: unbalanced: table %u, row %u: (", report.first_table, report.first_row);
            for (uint32_t q = 0; q < report.n_values; q++) printf(q ? ", %u" : "%u", report.tuple[q]);
            printf("), multiplicity sum %u\n", report.sum);
            // the machine still receives the digest of the words as they were, which the chip no longer sends
            as_expected = as_expected && bad_table < 0 && report.n_unbalanced == 2 && report.first_table == 0 &&
                          report.first_row == changed_call && report.n_values == 3 && report.tuple[0] == SPONGE_TAG &&
                          report.tuple[1] == changed_call && report.tuple[2] == changed_digest;
            ts_matrix_free(ctx, chip);
        } else {
            // round 1 reads d_rows and d_calls again, and a proof consumes its traces: it gets copies made in HBM
            ts::air::Derive same_calls(CALL_WIDTH), same_chip(CHIP_WIDTH);
            same_calls.output(same_calls.col(ID), ID);
            same_chip.output(same_chip.col(C_ID), C_ID);
            const std::vector<uint32_t> copy_calls = same_calls.tape(), copy_chip = same_chip.tape();
            CHECK(ts_matrix_derive(ctx, copy_calls.data(), copy_calls.size(), d_calls, &tables[0].trace));
            CHECK(ts_matrix_derive(ctx, copy_chip.data(), copy_chip.size(), d_chip, &tables[1].trace));
            ts_challenger *challenger = nullptr, *fresh = nullptr;
            CHECK(ts_chal_new(0, 1, &challenger));
            CHECK(ts_chal_new(0, 1, &fresh));
            std::vector<uint32_t> proof(1u << 20);
            size_t n_words = 0;
            CHECK(ts_prove_multi_bus(ctx, &fri, challenger, tables, 2, proof.data(), proof.size(), &n_words));
            const ts_air* const_airs[2] = {airs[0], airs[1]};
            const uint32_t n_public[2] = {0, 0};
            const uint32_t* values[2] = {nullptr, nullptr};
            uint32_t exposed[8], bus_sum[4] = {1, 1, 1, 1};
            int verdict = -1;
            CHECK(ts_verify_multi_bus(&fri, fresh, const_airs, 2, values, n_public, proof.data(), n_words, exposed, 8,
                                      bus_sum, &verdict));
            const bool zero = !(bus_sum[0] | bus_sum[1] | bus_sum[2] | bus_sum[3]);
            printf("sponge_chip_resident: proof of %zu words, verify -> %d, bus sum %s\n", n_words, verdict,
                   zero ? "zero" : "not zero");
            as_expected = as_expected && verdict == 0 && zero;
            ts_chal_free(challenger);
            ts_chal_free(fresh);
            for (int t = 0; t < 2; t++) ts_matrix_free(ctx, tables[t].trace);
        }
    }
    ts_matrix_free(ctx, d_rows);
    ts_matrix_free(ctx, d_chip);
    ts_matrix_free(ctx, d_calls);
    for (int t = 0; t < 2; t++) ts_air_free(ctx, airs[t]);
    ts_ctx_destroy(ctx);
    printf("sponge_chip_resident: %s\n", as_expected ? "as expected" : "NOT as expected");
    return as_expected ? 0 : 1;
}
