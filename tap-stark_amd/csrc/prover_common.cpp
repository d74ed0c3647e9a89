// The stages that prove (prover.cpp), prove_sharded (sharded.cpp) and prove_tap (tap_prover.cpp) have in
// common, each written once: the LDE stage of a commitment, the description of a committed batch's
// columns, the statement check, a few host numerics and the writer of the proof words.
#include <stdlib.h>
#include <string.h>

#include <optional>

#include "prover_internal.hpp"

namespace ts {

// small uploads go through the context's page-locked arena: truly asynchronous, and the caller's
// buffer (a stack temporary, a vector about to die) is free as soon as this returns
// (uploads above 1 MiB -- lock-script tables, script blobs -- go straight from the caller's buffer,
// which the caller keeps alive until its next blocking call)
void h2d(Context& ctx, void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    const void* from = bytes <= (1u << 20) ? ctx.stage(src, bytes) : src;
    TS_HIP(hipMemcpyAsync(dst, from, bytes, hipMemcpyHostToDevice, ctx.stream));
}
void d2h_sync(Context& ctx, void* dst, const void* src, size_t bytes) {
    if (bytes) TS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
}

unsigned log2_strict(uint64_t n) {
    unsigned k = 0;
    while ((1ull << k) < n) k++;
    TS_REQUIRE((1ull << k) == n, TS_ERR_INVALID, "height must be a power of two");
    return k;
}

// canonical-domain EF helpers for the handful of host-side scalars
Ef efc_mul(Ef a, Ef b) { return ef_mul(a, ef_to_mont(b)); }
Ef efc_mul_base(Ef a, uint32_t b) { return ef_mul_base(a, to_mont(b)); }
Ef efc_pow(Ef a, uint64_t e) { return ef_from_mont(ef_pow(ef_to_mont(a), e)); }

// ------------------------------------------------------------------ a committed batch's columns
std::vector<const uint32_t*> column_pointers(const std::vector<ColMat>& ldes, uint64_t height) {
    std::vector<const uint32_t*> cols;
    for (auto& cm : ldes)
        if (!height || cm.height == height)
            for (uint32_t c = 0; c < cm.width; c++) cols.push_back(cm.d + (uint64_t)c * cm.col_stride);
    return cols;
}

bool columns_as_one_matrix(const std::vector<ColMat>& ldes, uint64_t height, uint32_t max_width, ColMat& one) {
    const ColMat* first = nullptr;
    uint32_t wsum = 0;
    for (auto& cm : ldes)
        if (cm.height == height) {
            if (!first) first = &cm;
            if (cm.col_stride != first->col_stride || cm.d != first->d + (uint64_t)wsum * first->col_stride)
                return false;
            wsum += cm.width;
        }
    if (!wsum || (max_width && wsum > max_width)) return false;
    one = *first;
    one.width = wsum;
    return true;
}

LeafMats PcsData::leaf_mats() const {
    LeafMats lm;
    memset(&lm, 0, sizeof lm);
    lm.n_mats = (uint32_t)ldes.size();
    for (size_t i = 0; i < ldes.size(); i++) {
        lm.d[i] = ldes[i].d;
        lm.col_stride[i] = ldes[i].col_stride;
        lm.width[i] = ldes[i].width;
        lm.row_shift[i] = (uint8_t)(log_height - log2_strict(ldes[i].height));
        lm.total_width += ldes[i].width;
    }
    lm.cols = col_table_uploaded ? col_table.p : nullptr;
    return lm;
}

LeafMats PcsData::leaf_mats_with_table(Context& ctx) {
    if (!col_table_uploaded) {
        const std::vector<const uint32_t*> cols = column_pointers(ldes);
        col_table = DevBuf<const uint32_t*>(&ctx, cols.size());
        h2d(ctx, col_table.p, cols.data(), cols.size() * sizeof(const uint32_t*));
        col_table_uploaded = true;
    }
    return leaf_mats();
}

// ------------------------------------------------------------------ the LDE stage of a commitment
void lde_stage(Context& ctx, const FriConfig& fri, std::vector<DeviceMatrix>& evals,
               const std::vector<uint32_t>& domain_shifts, uint32_t beta0, uint32_t n_beta, bool allow_pair,
               PcsData& data, bool keep_row_major) {
    TS_REQUIRE(!evals.empty() && evals.size() <= (size_t)MAX_BATCH_MATS, TS_ERR_INVALID,
               "commit: between 1 and MAX_BATCH_MATS (64) matrices per batch");
    TS_REQUIRE(evals.size() == domain_shifts.size(), TS_ERR_INVALID, "commit: one domain per matrix");
    uint64_t max_n = 0;
    bool same_height = true;
    size_t total_w = 0;
    for (size_t i = 0; i < evals.size(); i++) {
        const DeviceMatrix& m = evals[i];
        TS_REQUIRE(m.width >= 1 && m.buf.p, TS_ERR_INVALID, "commit: empty matrix");
        TS_REQUIRE(domain_shifts[i] != 0 && domain_shifts[i] < P, TS_ERR_INVALID, "bad domain shift");
        log2_strict(m.height);
        max_n = std::max(max_n, m.height);
        same_height = same_height && m.height == evals[0].height;
        total_w += m.width;
    }
    TS_REQUIRE(same_height || !n_beta, TS_ERR_INVALID, "sharded commit: matrices of one height expected");
    const unsigned log_N = log2_strict(max_n) + fri.log_blowup;
    TS_REQUIRE(log_N <= 27, TS_ERR_INVALID, "commit: LDE larger than the two-adic subgroup");
    ctx.ensure_lde_twiddles(std::max(1u, log_N));
    // rows held of the LDE of a matrix of height n: all, or the n_beta owned cosets
    auto lde_rows = [&](uint64_t n) { return n_beta ? (uint64_t)n_beta * n : n << fri.log_blowup; };
    data.log_height = log2_strict(lde_rows(max_n));
    auto push_lde = [&](uint32_t* d, uint64_t rows, uint32_t width) {
        ColMat cm;
        cm.d = d;
        cm.height = rows;
        cm.width = width;
        cm.col_stride = rows;
        data.ldes.push_back(cm);
    };

    StageTimer t(&ctx, "coset_lde");
    // A batch of equal-height matrices (the quotient chunks) gets ONE allocation, matrix after
    // matrix: to the leaf hash and to the opening's dot products it is then a single matrix of
    // the summed width (strided addressing, one launch) instead of a pointer table / a launch each.
    const bool batched = same_height && evals.size() > 1;
    DevBuf<uint32_t> batch;
    if (batched) batch = DevBuf<uint32_t>(&ctx, total_w * lde_rows(evals[0].height));
    size_t batch_col = 0;
    // exactly two column-major matrices of one shape (the two quotient chunks of a degree-3 AIR):
    // ONE set of LDE launches for both (coset_lde: evals2) -- 8 columns instead of 4 twice
    static const bool pair_knob = [] { const char* e = getenv("TS_LDE_PAIR"); return !e || atoi(e) != 0; }();
    if (allow_pair && pair_knob && batched && evals.size() == 2 && evals[0].width == evals[1].width &&
        evals[0].layout == DeviceMatrix::COL_MAJOR_BITREV && evals[1].layout == DeviceMatrix::COL_MAJOR_BITREV) {
        const uint64_t n = evals[0].height, rows = lde_rows(n);
        const uint32_t w = evals[0].width;
        // two_adic_pcs.rs:235: shift = Val::generator() / domain.shift
        coset_lde(ctx, evals[0].buf.p, n, 2 * w, log2_strict(n), fri.log_blowup,
                  mul(GENERATOR, inv_canon(domain_shifts[0])), batch.p, rows, beta0, n_beta, false, evals[1].buf.p,
                  mul(GENERATOR, inv_canon(domain_shifts[1])), w);
        for (size_t i = 0; i < 2; i++) {
            push_lde(batch.p + i * (size_t)w * rows, rows, w);
            evals[i].buf.reset();  // consumed
        }
        data.lde_storage.push_back(std::move(batch));
        return;
    }
    for (size_t i = 0; i < evals.size(); i++) {
        DeviceMatrix& m = evals[i];
        const uint64_t n = m.height, rows = lde_rows(n);
        const unsigned log_n = log2_strict(n);
        DevBuf<uint32_t> colmajor;
        uint32_t* ev = m.buf.p;
        bool r16 = false;  // the transpose already ran the first round of the inverse transform
        if (m.layout == DeviceMatrix::ROW_MAJOR) {
            // (a sharded rank transposes and inverts every column, then runs the forward transforms of its
            // own cosets: sharding the inverse by column cost more in all-gathers than it saved, HISTORY.md)
            std::optional<StageTimer> tt;
            if (n_beta) tt.emplace(&ctx, "lde: transpose (every column on every rank)");
            colmajor = DevBuf<uint32_t>(&ctx, (size_t)m.width * n);
            r16 = launch_transpose_bitrev_r16(ctx, m.buf.p, colmajor.p, log_n, m.width, n);
            if (!r16) launch_transpose_bitrev(ctx, m.buf.p, colmajor.p, log_n, m.width, n);
            ev = colmajor.p;
        }
        DevBuf<uint32_t> own;
        uint32_t* lde;
        if (batched) {
            lde = batch.p + batch_col * rows;
            batch_col += m.width;
        } else {
            own = DevBuf<uint32_t>(&ctx, (size_t)m.width * rows);
            lde = own.p;
        }
        // two_adic_pcs.rs:235: shift = Val::generator() / domain.shift
        coset_lde(ctx, ev, n, m.width, log_n, fri.log_blowup, mul(GENERATOR, inv_canon(domain_shifts[i])), lde,
                  rows, beta0, n_beta, r16);
        push_lde(lde, rows, m.width);
        if (!batched) data.lde_storage.push_back(std::move(own));
        if (!(keep_row_major && m.layout == DeviceMatrix::ROW_MAJOR)) m.buf.reset();  // consumed
    }
    if (batched) data.lde_storage.push_back(std::move(batch));
}

bool reduce_low_wanted(uint32_t opened_columns) {
    if (const char* e = getenv("TS_REDUCE_LOW"); e && *e) return atoi(e) != 0;
    return opened_columns >= REDUCE_LOW_MIN_WIDTH;
}

// ------------------------------------------------------------------ the statement
Statement check_statement(const FriConfig& fri, const AirProgram& air, uint32_t trace_width, uint64_t degree,
                          size_t n_public_values) {
    TS_REQUIRE(trace_width == air.width, TS_ERR_INVALID, "prove: trace width != AIR width");
    TS_REQUIRE(n_public_values == air.n_public, TS_ERR_INVALID, "prove: wrong number of public values");
    Statement s;
    s.log_degree = log2_strict(degree);  // prover.rs:43-44
    s.lqd = air.log_quotient_degree;     // :46
    s.qd = 1u << s.lqd;
    s.log_N = s.log_degree + fri.log_blowup;
    s.w = air.width;
    // two_adic_pcs.rs:256: assert!(lde.height() >= domain.size())
    TS_REQUIRE(s.lqd <= fri.log_blowup, TS_ERR_INVARIANT,
               "quotient domain larger than the committed LDE (log_quotient_degree > log_blowup)");
    return s;
}

// ------------------------------------------------------------------ host numerics
std::vector<uint32_t> air_consts_mont(const AirProgram& air, const uint32_t* pis, size_t n) {
    TS_REQUIRE(n == air.n_public_slots(), TS_ERR_INVALID, "wrong number of public values");
    std::vector<uint32_t> consts(std::max<size_t>(air.const_canonical.size(), 1), 0);
    for (size_t k = 0; k < air.const_canonical.size(); k++) {
        const uint32_t v = air.const_public_idx[k] != ~0u ? pis[air.const_public_idx[k]] : air.const_canonical[k];
        TS_REQUIRE(v < P, TS_ERR_INVALID, "non-canonical public value");
        consts[k] = to_mont(v);
    }
    return consts;
}

Ef bary_scale(Ef point, uint32_t coset_gen, uint64_t n) {
    Ef un = efc_pow(efc_mul_base(point, inv_canon(coset_gen)), n);
    un.c[0] = sub(un.c[0], 1);
    return efc_mul_base(un, inv_canon((uint32_t)(n % P)));
}

std::vector<uint32_t> chunk_domain_shifts(uint32_t base_shift, unsigned log_degree, unsigned lqd) {
    std::vector<uint32_t> shifts(1u << lqd);
    const uint32_t gq = two_adic_generator(log_degree + lqd);
    for (uint32_t c = 0; c < shifts.size(); c++) shifts[c] = mul(base_shift, pow_canon(gq, c));
    return shifts;
}

// ------------------------------------------------------------------ proof words
// Proof (uni-stark/src/prover.rs:105-118): header, the two commitments, the opened values, then the
// FriProof (fri/src/proof.rs): round roots, per query the input proof and the commit-phase openings,
// the final polynomial and the proof-of-work witness.
size_t ProofWriter::words_per_query(const std::vector<Batch>& batches, const std::vector<unsigned>& round_depths,
                                    size_t n_pass_through) {
    size_t n = 1 + 5 * n_pass_through;
    for (auto& b : batches) {
        n += 1 + b.mats->size() + 1 + 8 * (size_t)b.depth;
        for (auto& m : *b.mats) n += m.width;
    }
    for (unsigned d : round_depths) n += 8 + 1 + 8 * (size_t)d;
    return n;
}

void ProofWriter::header(uint32_t version, unsigned log_degree, uint32_t width, uint32_t qd, uint32_t extra) {
    out_.push_back(TSPF_MAGIC);
    out_.push_back(version);
    out_.push_back(log_degree);
    out_.push_back(width);
    out_.push_back(qd);
    if (version >= 2) out_.push_back(extra);
}

void ProofWriter::header_multi(const std::vector<TableShape>& tables, uint32_t version) {
    out_.push_back(TSPF_MAGIC);
    out_.push_back(version);
    out_.push_back((uint32_t)tables.size());
    for (auto& t : tables) {
        out_.push_back(t.log_degree);
        out_.push_back(t.width);
        out_.push_back(t.qd);
        if (version >= 7) {
            out_.push_back(t.aux_width);
            out_.push_back(t.n_exposed);
        }
        if (version >= 8) out_.push_back(t.preprocessed_width);
    }
}

void ProofWriter::opened_values(const std::vector<Ef>& values) {
    for (auto& e : values) words(e.c, 4);
}

void ProofWriter::path(std::initializer_list<Path> parts) {
    for (auto& part : parts) {
        if (!swap_) words(part.digests, 8 * part.depth);
        else for (size_t k = 0; k < 8 * part.depth; k++) out_.push_back(__builtin_bswap32(part.digests[k]));
    }
}

// fri.rs:109-118: [(log_height, value)] by descending height
void ProofWriter::pass_through_value(unsigned log_height, const uint32_t value[4]) {
    out_.push_back(log_height);
    words(value, 4);
}

// input_proof: one BatchOpening per commit round (two_adic_pcs.rs:399-414): the opened row of every
// matrix in commit order, then the path
void ProofWriter::batch_opening(const std::vector<ColMat>& mats, const uint32_t* row, unsigned depth,
                                std::initializer_list<Path> parts) {
    out_.push_back((uint32_t)mats.size());
    for (auto& m : mats) {
        out_.push_back(m.width);
        words(row, m.width);
        row += m.width;
    }
    out_.push_back(depth);
    path(parts);
}

// commit_phase_openings (fri/src/prover.rs:69-90): the pair of values, then the path
void ProofWriter::round_opening(const uint32_t values[8], unsigned depth, std::initializer_list<Path> parts) {
    words(values, 8);
    out_.push_back(depth);
    path(parts);
}

void ProofWriter::finish(Ef final_poly, uint32_t pow_witness) {
    words(final_poly.c, 4);
    out_.push_back(pow_witness);
}

// ------------------------------------------------------------------ the query-phase gather
unsigned QueryGather::add_indices(const std::vector<uint32_t>& indices) {
    lists_.emplace_back();
    lists_.back().indices = indices;
    return (unsigned)lists_.size() - 1;
}

// the one place that lays out the output buffer: job after job, [query][words of one answer] each
QueryGather::Slot QueryGather::take(const List& l, size_t words_per_query) {
    const Slot s{words_, words_per_query};
    words_ += l.indices.size() * words_per_query;
    return s;
}

QueryGather::Slot QueryGather::add_rows(unsigned list, const LeafMats& mats, unsigned shift) {
    List& l = lists_.at(list);
    const Slot s = take(l, mats.total_width);
    RowGatherJob jb{};
    jb.mats = mats;
    jb.shift = shift;
    jb.out = s.at;
    l.rows.push_back(jb);
    l.max_row_width = std::max(l.max_row_width, mats.total_width);
    return s;
}

// kernels.hpp: vec == nullptr is "path only", log_leaves == 0 "values only"
QueryGather::Opening QueryGather::add_desc(unsigned list, const Ef* vec, const uint32_t* tree, unsigned log_leaves,
                                           unsigned shift) {
    List& l = lists_.at(list);
    FriGatherDesc d{};
    d.vec = reinterpret_cast<const uint32_t*>(vec);
    d.tree = tree;
    d.log_leaves = log_leaves;
    d.shift = shift;
    Opening o;
    if (vec) d.out_vals = (o.vals = take(l, 8)).at;
    if (tree) d.out_path = (o.path = take(l, 8 * (size_t)log_leaves)).at;
    l.descs.push_back(d);
    l.max_log_leaves = std::max(l.max_log_leaves, d.log_leaves);
    return o;
}
QueryGather::Slot QueryGather::add_path(unsigned list, const uint32_t* tree, unsigned log_leaves, unsigned shift) {
    return add_desc(list, nullptr, tree, log_leaves, shift).path;
}
QueryGather::Opening QueryGather::add_round(unsigned list, const Ef* vec, const uint32_t* tree, unsigned log_leaves,
                                            unsigned shift) {
    return add_desc(list, vec, tree, log_leaves, shift);
}
QueryGather::Slot QueryGather::add_values(unsigned list, const Ef* vec, unsigned shift) {
    return add_desc(list, vec, nullptr, 0, shift).vals;
}

void QueryGather::run() {
    static_assert(sizeof(RowGatherJob) % 8 == 0 && sizeof(FriGatherDesc) % 8 == 0, "tables stay 8-byte aligned");
    size_t b_rows = 0, b_descs = 0, b_idx = 0;
    for (auto& l : lists_) {
        b_rows += l.rows.size() * sizeof(RowGatherJob);
        b_descs += l.descs.size() * sizeof(FriGatherDesc);
        b_idx += l.indices.size() * 4;
    }
    if (!b_idx) return;
    // every list's row jobs, then every list's descriptors, then the indices
    std::vector<unsigned char> up(b_rows + b_descs + b_idx);
    auto put = [](unsigned char*& at, const void* src, size_t bytes) {
        if (bytes) memcpy(at, src, bytes);
        at += bytes;
    };
    unsigned char *rows = up.data(), *descs = rows + b_rows, *idx = descs + b_descs;
    for (auto& l : lists_) {
        put(rows, l.rows.data(), l.rows.size() * sizeof(RowGatherJob));
        put(descs, l.descs.data(), l.descs.size() * sizeof(FriGatherDesc));
        put(idx, l.indices.data(), l.indices.size() * 4);
    }
    DevBuf<unsigned char> d_up(&ctx_, up.size());
    h2d(ctx_, d_up.p, up.data(), up.size());
    DevBuf<uint32_t> d_out(&ctx_, std::max<size_t>(words_, 1));
    rows = d_up.p, descs = rows + b_rows, idx = descs + b_descs;
    for (auto& l : lists_) {
        launch_gather_queries(ctx_, reinterpret_cast<const RowGatherJob*>(rows), (uint32_t)l.rows.size(),
                              l.max_row_width, reinterpret_cast<const FriGatherDesc*>(descs), (uint32_t)l.descs.size(),
                              l.max_log_leaves, reinterpret_cast<const uint32_t*>(idx), (uint32_t)l.indices.size(),
                              d_out.p);
        rows += l.rows.size() * sizeof(RowGatherJob);
        descs += l.descs.size() * sizeof(FriGatherDesc);
        idx += l.indices.size() * 4;
    }
    out_.resize(words_);
    d2h_sync(ctx_, out_.data(), d_out.p, words_ * 4);
}

// ------------------------------------------------------------------ ts_bench_stage
// One stage of the path in a sustained loop on resident, arbitrary data (measurement aid; the values
// are whatever the previous repetition left -- valid lazy-range field elements, never checked):
//   stage 0: coset_lde of a 2^log_n x width matrix (all three NTT passes, every coset)
//   stage 1: BFMmcs::commit's hashing of a 2^(log_n + log_blowup) x width matrix (leaves + tree)
// Returns the mean time of a repetition from HIP events on the context's stream.
double bench_stage(Context& c, int stage, unsigned log_n, uint32_t width, unsigned log_blowup, uint32_t reps) {
    TS_REQUIRE(stage >= 0 && stage <= 4 && width >= 1 && width <= 256 && reps >= 1 && log_n >= 1 &&
                   log_n + log_blowup <= 27,
               TS_ERR_INVALID, "bench_stage: stage 0 .. 4, width 1..256, log_n + log_blowup <= 27");
    // stages 2, 3, 4: ONE pass of the LDE alone (inverse contiguous / strided middle / forward
    // contiguous; two-pass plans only, ntt_plan.hpp), on whatever the buffers hold
    struct MaskGuard {
        Context& c;
        ~MaskGuard() { c.lde_pass_mask = 7; }
    } guard_mask{c};
    if (stage >= 2) {
        TS_REQUIRE(ntt_plan(log_n).two_pass, TS_ERR_INVALID, "bench_stage: single LDE passes exist for log_n > 12 only");
        c.lde_pass_mask = 1u << (stage - 2);
    }
    const bool is_lde = stage != 1;
    const uint64_t n = 1ull << log_n, N = n << log_blowup;
    c.ensure_twiddles(log_n + log_blowup);
    DevBuf<uint32_t> lde(&c, (size_t)width * N), in(&c, is_lde ? (size_t)width * n : 1);
    TS_HIP(hipMemsetAsync(lde.p, 0x11, (size_t)width * N * 4, c.stream));  // 0x11111111 < p
    if (is_lde) TS_HIP(hipMemsetAsync(in.p, 0x11, (size_t)width * n * 4, c.stream));
    DevBuf<uint32_t> tree(&c, stage == 1 ? merkle_total_digests(log_n + log_blowup) * 8 : 1);
    std::vector<const uint32_t*> cols(width);
    for (uint32_t k = 0; k < width; k++) cols[k] = lde.p + (uint64_t)k * N;
    DevBuf<const uint32_t*> d_cols(&c, width);
    TS_HIP(hipMemcpyAsync(d_cols.p, cols.data(), width * sizeof(const uint32_t*), hipMemcpyHostToDevice, c.stream));
    c.sync();
    LeafMats lm;
    memset(&lm, 0, sizeof lm);
    lm.n_mats = 1;
    lm.d[0] = lde.p;
    lm.col_stride[0] = N;
    lm.width[0] = width;
    lm.total_width = width;
    lm.cols = d_cols.p;
    auto once = [&] {
        if (is_lde) coset_lde(c, in.p, n, width, log_n, log_blowup, GENERATOR, lde.p, N);
        else launch_commit_tree(c, lm, log_n + log_blowup, tree.p);
    };
    once();  // tables, first-touch
    hipEvent_t e0, e1;
    TS_HIP(hipEventCreate(&e0));
    TS_HIP(hipEventCreate(&e1));
    TS_HIP(hipEventRecord(e0, c.stream));
    for (uint32_t r = 0; r < reps; r++) once();
    TS_HIP(hipEventRecord(e1, c.stream));
    c.sync();
    float ms = 0;
    TS_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return (double)ms / reps;
}

}  // namespace ts
