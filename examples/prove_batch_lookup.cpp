// examples/prove_batch_lookup.cpp -- lookup AIRs in batch lanes, against the public C ABI only: ONE call of
// ts_prove_batch_lookup proves statements of three different AIRs on three lanes (one context and one host thread
// each, inside the library):
//   lane 0  TableLookupAir: the table in a preprocessed column, committed once as the lane's key.  The aux source is
//           DECLARATIVE -- a ts_logup_spec the library runs on the lane's stream -- and the multiplicity column is
//           handed over zeroed and filled in the lane (ts_logup_multiplicities' work), so the host computes neither.
//   lane 1  RangeLookupAir: challenge-phase columns through a C CALLBACK that calls ts_logup_aux_build; it runs on
//           the lane's thread with the lane's context.
//   lane 2  FibonacciAir: neither a key nor aux columns.
// Every proof is TSPF v5 and is verified with ts_verify_pre_aux and a fresh challenger; every lookup sum is
// checked to be zero, which is the caller's job.
//
//   g++ -std=c++17 -pthread -I include examples/prove_batch_lookup.cpp -L tap-stark_amd/lib -ltapstark_hip -o prove_batch_lookup
//   ./prove_batch_lookup [log_n] [items per lane]     (defaults 10, 2; exit status 0 only if every check holds)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "tapstark.h"
#include "tapstark_air.hpp"

namespace {

constexpr uint32_t P = 0x78000001u;

struct TableLookupAir {  // as examples/table_lookup_air.cpp
    ts::air::LogUp logup{{{{0, 1}, {{1, 0}}}, {{1, 1}, {{2, 0}}}}};
    uint32_t width() const { return 2; }
    uint32_t preprocessed_width() const { return 1; }
    void eval(ts::air::Builder& builder) const { logup.eval(builder); }
};

struct RangeLookupAir {  // as examples/lookup_air.cpp
    ts::air::LogUp logup{{{{0, 1}, {{1, 0}}}, {{1, 2}, {{1, 1}}}}};
    uint32_t width() const { return 3; }
    void eval(ts::air::Builder& builder) const {
        const auto &local = builder.local(), &next = builder.next();
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_zero(local[1]);
        auto when_transition = builder.when_transition();
        const ts::air::Expr step = local[1] + 1;
        when_transition.assert_eq(next[1], step);
        logup.eval(builder);
    }
};

struct FibonacciAir {  // as examples/prove_batch.cpp
    uint32_t width() const { return 2; }
    void eval(ts::air::Builder& builder) const {
        const auto& pis = builder.public_values();
        const auto a = pis[0], b = pis[1], x = pis[2];
        const auto &local = builder.local(), &next = builder.next();
        auto when_first_row = builder.when_first_row();
        when_first_row.assert_eq(local[0], a);
        when_first_row.assert_eq(local[1], b);
        auto when_transition = builder.when_transition();
        when_transition.assert_eq(local[1], next[0]);
        when_transition.assert_eq(local[0] + local[1], next[1]);
        builder.when_last_row().assert_eq(local[1], x);
    }
};

// lane 1's aux source: called on the lane's thread, after the trace is committed and the challenges are drawn
ts_status build_logup_columns(void* user, ts_ctx* ctx, const ts_matrix* trace, const uint32_t* challenges,
                              uint32_t n_challenges, ts_matrix** aux_out, uint32_t* exposed_out) {
    if (n_challenges != 2) return TS_ERR_INVALID;
    return ts_logup_aux_build(ctx, static_cast<const ts_logup_spec*>(user), trace, challenges, aux_out, exposed_out);
}

#define CHECK(ctx, call)                                                                 \
    do {                                                                                 \
        ts_status _s = (call);                                                           \
        if (_s != TS_OK) {                                                               \
            fprintf(stderr, "%s -> status %d: %s\n", #call, (int)_s, ts_last_error(ctx)); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

}  // namespace

int main(int argc, char** argv) {
    const unsigned log_n = argc > 1 ? (unsigned)atoi(argv[1]) : 10;
    const uint32_t per_lane = argc > 2 ? (uint32_t)atoi(argv[2]) : 2;
    if (log_n < 1 || log_n > 20 || per_lane < 1 || per_lane > 64) {
        fprintf(stderr, "usage: prove_batch_lookup [log_n in 1..20] [items per lane in 1..64]\n");
        return 1;
    }
    const uint64_t n = 1ull << log_n;
    const ts_fri_config fri = {2, 28, 8};

    ts_ctx* ctxs[3] = {nullptr, nullptr, nullptr};
    for (ts_ctx*& c : ctxs)
        if (ts_ctx_create(0, &c) != TS_OK) {
            fprintf(stderr, "no MI355X context: %s\n", ts_last_error(nullptr));
            return 2;  // no fallback path exists
        }

    // the three AIRs, one per lane
    TableLookupAir table_air;
    ts::air::Builder tb(table_air.width(), 0, table_air.preprocessed_width(), table_air.logup.aux_width(),
                        ts::air::LogUp::n_challenges, ts::air::LogUp::n_exposed);
    table_air.eval(tb);
    RangeLookupAir range_air;
    ts::air::Builder rb(range_air.width(), 0, 0, range_air.logup.aux_width(), ts::air::LogUp::n_challenges,
                        ts::air::LogUp::n_exposed);
    range_air.eval(rb);
    FibonacciAir fib_air;
    ts::air::Builder fb(fib_air.width(), 3);
    fib_air.eval(fb);
    const std::vector<uint32_t> tapes[3] = {tb.tape(), rb.tape(), fb.tape()};
    const ts_air* airs[3];
    for (int l = 0; l < 3; l++) {
        ts_air* a = nullptr;
        CHECK(ctxs[l], ts_air_compile(ctxs[l], tapes[l].data(), tapes[l].size(), &a));
        airs[l] = a;
    }

    // lane 0's key: the table 0 .. n-1 committed once; the commit consumes its matrix, so the row-major values the
    // spec's kind-2 terms read are a second upload.  Both serve every item of the lane and are never consumed.
    std::vector<uint32_t> table(n);
    for (uint64_t r = 0; r < n; r++) table[r] = (uint32_t)r;
    ts_matrix *key_matrix = nullptr, *table_rows = nullptr;
    CHECK(ctxs[0], ts_matrix_upload(ctxs[0], table.data(), n, 1, &key_matrix));
    CHECK(ctxs[0], ts_matrix_upload(ctxs[0], table.data(), n, 1, &table_rows));
    const uint32_t shifts[1] = {1};
    uint32_t key_root[8];
    ts_pcs_data* key = nullptr;
    CHECK(ctxs[0], ts_pcs_commit(ctxs[0], &fri, 1, &key_matrix, shifts, key_root, &key));
    ts_batch_lane lanes[3] = {};
    for (ts_batch_lane& l : lanes) l.struct_size = sizeof(ts_batch_lane);
    lanes[0].key = key;
    lanes[0].key_values = table_rows;

    // lane 0: the LogUp spec and the fill of the multiplicity column (column 1: MINUS the number of lookups of the
    // row's table entry), both run by the library
    const ts_logup_term value0[] = {{1, 0}}, table0[] = {{2, 0}}, one[] = {{0, 1}};
    const ts_logup_interaction table_its[] = {{{0, 1}, 1, value0}, {{1, 1}, 1, table0}};
    const ts_logup_spec table_spec = {sizeof(ts_logup_spec), 2, table_its};
    ts_logup_mult_spec fill = {};
    fill.struct_size = sizeof(ts_logup_mult_spec);
    fill.n_values = 1;
    fill.table = table0;
    fill.n_lookups = 1;
    fill.lookups = value0;
    fill.weights = one;
    fill.out_column = 1;
    fill.negate = 1;
    // lane 1: the spec its callback hands to ts_logup_aux_build
    const ts_logup_term table1[] = {{1, 1}};
    const ts_logup_interaction range_its[] = {{{0, 1}, 1, value0}, {{1, 2}, 1, table1}};
    ts_logup_spec range_spec = {sizeof(ts_logup_spec), 2, range_its};

    // the statements, interleaved over the lanes
    const uint32_t N = 3 * per_lane;
    const size_t cap = 1u << 21;
    std::vector<std::vector<uint32_t>> traces(N), pis(N), proofs(N, std::vector<uint32_t>(cap));
    std::vector<uint32_t> exposed(4 * N, 1);
    std::vector<ts_batch_lookup_item> items(N);
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (uint32_t i = 0; i < N; i++) {
        const uint32_t lane = i % 3;
        const uint32_t w = lane == 1 ? 3 : 2;
        traces[i].assign(n * w, 0);
        if (lane == 2) {
            uint32_t l = i % P, r = (3 * i + 1) % P;
            pis[i] = {l, r, 0};
            for (uint64_t k = 0; k < n; k++) {
                traces[i][2 * k] = l;
                traces[i][2 * k + 1] = r;
                const uint32_t nx = (uint32_t)(((uint64_t)l + r) % P);
                l = r;
                r = nx;
            }
            pis[i][2] = traces[i][2 * (n - 1) + 1];
        } else {
            std::vector<uint32_t> counts(n, 0);
            for (uint64_t r = 0; r < n; r++) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                const uint32_t value = (uint32_t)((state >> 33) % n);
                traces[i][w * r] = value;
                counts[value]++;
            }
            // lane 0 leaves the multiplicity column zero: the lane fills it.  Lane 1 carries table and multiplicity.
            if (lane == 1)
                for (uint64_t r = 0; r < n; r++) {
                    traces[i][3 * r + 1] = (uint32_t)r;
                    traces[i][3 * r + 2] = (P - counts[r]) % P;
                }
        }
        ts_batch_lookup_item& it = items[i];
        it = ts_batch_lookup_item{};
        it.struct_size = sizeof(ts_batch_lookup_item);
        it.lane = lane;
        it.host_trace = traces[i].data();
        it.height = n;
        it.width = w;
        it.n_public = (uint32_t)pis[i].size();
        it.public_values = pis[i].empty() ? nullptr : pis[i].data();
        it.proof_out = proofs[i].data();
        it.cap_words = cap;
        it.exposed_out = &exposed[4 * i];
        it.cap_exposed = 4;
        if (lane == 0) {
            it.logup = &table_spec;
            it.mult = &fill;
            it.n_mult = 1;
        } else if (lane == 1) {
            it.aux_fn = build_logup_columns;
            it.aux_user = &range_spec;
        }
    }

    const ts_status st = ts_prove_batch_lookup(ctxs, airs, lanes, 3, &fri, items.data(), N, 0.0, 0);
    bool ok = st == TS_OK;
    if (!ok) fprintf(stderr, "ts_prove_batch_lookup -> status %d\n", (int)st);
    bool zero = true;
    for (uint32_t i = 0; i < N && ok; i++) {
        const ts_batch_lookup_item& it = items[i];
        const uint32_t lane = it.lane;
        if (it.status != TS_OK) {
            fprintf(stderr, "item %u (lane %u) -> status %d: %s\n", i, lane, (int)it.status, ts_last_error(ctxs[lane]));
            ok = false;
            break;
        }
        ts_challenger* fresh = nullptr;
        if (ts_chal_new(0, 1, &fresh) != TS_OK) return 1;
        int verdict = -1;
        uint32_t sum[4] = {1, 1, 1, 1};
        const ts_status vs = ts_verify_pre_aux(&fri, airs[lane], fresh, lane == 0 ? key_root : nullptr, proofs[i].data(),
                                               it.n_words, it.public_values, it.n_public, lane == 2 ? nullptr : sum,
                                               lane == 2 ? 0 : 4, &verdict);
        ts_chal_free(fresh);
        ok = ok && vs == TS_OK && verdict == 0 && proofs[i][1] == 5;
        if (lane != 2) {
            const bool same = it.n_exposed == 4 && sum[0] == exposed[4 * i] && sum[1] == exposed[4 * i + 1] &&
                              sum[2] == exposed[4 * i + 2] && sum[3] == exposed[4 * i + 3];
            zero = zero && same && !(sum[0] | sum[1] | sum[2] | sum[3]);
        }
        printf("prove_batch_lookup: item %u on lane %u: %zu words (TSPF v%u), verify -> %d, %.3f ms\n", i, lane,
               it.n_words, proofs[i][1], verdict, it.wall_ms);
    }
    if (ok && zero)
        printf("prove_batch_lookup: %u statements of 2^%u rows on 3 lanes: every proof verified, every lookup sum is "
               "zero\n", N, log_n);

    ts_matrix_free(ctxs[0], table_rows);
    ts_matrix_free(ctxs[0], key_matrix);
    ts_pcs_data_free(ctxs[0], key);
    for (int l = 0; l < 3; l++) {
        ts_air_free(ctxs[l], const_cast<ts_air*>(airs[l]));
        ts_ctx_destroy(ctxs[l]);
    }
    return ok && zero ? 0 : 1;
}
