// The spec of ts_matrix_collect_rows: the checks that need no matrix, the plan they leave, and the plain sequential
// loop over host rows.  No device code and no context: ts_collect_check and ts_collect_rows_host are all of this, and
// ts_matrix_collect_rows makes the same checks first.
#include "collect.hpp"

#include <string>

#include "context.hpp"

namespace ts {

CollectPlan collect_check(const uint32_t* spec, size_t n_words) {
    TS_REQUIRE(spec != nullptr, TS_ERR_INVALID, "collect: null spec");
    TS_REQUIRE(n_words >= 5, TS_ERR_INVALID, "collect: the spec is shorter than its header");
    TS_REQUIRE(spec[0] == COLLECT_MAGIC, TS_ERR_INVALID, "collect: bad magic (not a TCOL spec)");
    TS_REQUIRE(spec[1] == 1, TS_ERR_INVALID, "collect: unknown spec version " + std::to_string(spec[1]));
    const uint32_t n_sources = spec[2], n_emitters = spec[3], out_width = spec[4];
    TS_REQUIRE(n_sources >= 1 && n_sources <= COLLECT_MAX_SOURCES, TS_ERR_INVALID,
               "collect: n_sources " + std::to_string(n_sources) + " outside [1, " + std::to_string(COLLECT_MAX_SOURCES) + "]");
    TS_REQUIRE(n_emitters >= 1 && n_emitters <= COLLECT_MAX_EMITTERS, TS_ERR_INVALID,
               "collect: n_emitters " + std::to_string(n_emitters) + " outside [1, " + std::to_string(COLLECT_MAX_EMITTERS) + "]");
    TS_REQUIRE(out_width >= 1 && out_width <= COLLECT_MAX_WIDTH, TS_ERR_INVALID,
               "collect: out_width " + std::to_string(out_width) + " outside [1, " + std::to_string(COLLECT_MAX_WIDTH) + "]");
    const size_t record = 3 + 2 * (size_t)out_width;
    const size_t want = 5 + (size_t)n_sources + out_width + n_emitters * record;
    TS_REQUIRE(n_words == want, TS_ERR_INVALID,
               "collect: " + std::to_string(n_words) + " words, the header asks for " + std::to_string(want));

    CollectPlan plan;
    plan.n_sources = n_sources;
    plan.out_width = out_width;
    const uint32_t* w = spec + 5;
    for (uint32_t s = 0; s < n_sources; s++, w++) {
        TS_REQUIRE(*w >= 1 && *w <= COLLECT_MAX_SRC_WIDTH, TS_ERR_INVALID,
                   "collect: source " + std::to_string(s) + ": src_width outside [1, 2^16]");
        plan.src_width.push_back(*w);
    }
    for (uint32_t c = 0; c < out_width; c++, w++) {
        TS_REQUIRE(*w < P, TS_ERR_INVALID, "collect: pad word " + std::to_string(c) + " is not below p");
        plan.pad.push_back(*w);
    }
    const uint32_t* records = w;
    for (uint32_t e = 0; e < n_emitters; e++) {
        const uint32_t* r = records + e * record;
        const std::string at = "collect: emitter " + std::to_string(e) + ": ";
        const uint32_t source = r[0], sel_kind = r[1], sel_value = r[2];
        TS_REQUIRE(source < n_sources, TS_ERR_INVALID, at + "source " + std::to_string(source) + " outside the spec's sources");
        const uint32_t width = plan.src_width[source];
        TS_REQUIRE(sel_kind <= 1, TS_ERR_INVALID, at + "selector kind must be 0 (always) or 1 (column)");
        TS_REQUIRE(sel_kind == 1 || sel_value == 1, TS_ERR_INVALID, at + "a constant selector must be 1");
        TS_REQUIRE(sel_kind == 0 || sel_value < width, TS_ERR_INVALID, at + "the selector column is outside the source");
        for (uint32_t c = 0; c < out_width; c++) {
            const uint32_t kind = r[3 + 2 * c], value = r[4 + 2 * c];
            const std::string term = at + "term " + std::to_string(c) + ": ";
            TS_REQUIRE(kind <= C_ROW, TS_ERR_INVALID, term + "kind must be 0 (constant), 1 (column) or 2 (row index)");
            TS_REQUIRE(kind != C_CONST || value < P, TS_ERR_INVALID, term + "the constant is not below p");
            TS_REQUIRE(kind != C_COL || value < width, TS_ERR_INVALID, term + "the column is outside the source");
            TS_REQUIRE(kind != C_ROW || value == 0, TS_ERR_INVALID, term + "the value word of a row index must be 0");
        }
    }
    // grouped by source, spec order kept inside a source
    for (uint32_t s = 0; s < n_sources; s++) {
        plan.first_emitter[s] = (uint32_t)plan.sel.size();
        for (uint32_t e = 0; e < n_emitters; e++) {
            const uint32_t* r = records + e * record;
            if (r[0] != s) continue;
            plan.sel.push_back(r[1] ? r[2] : COLLECT_ALWAYS);
            for (uint32_t c = 0; c < out_width; c++) plan.terms.push_back({r[3 + 2 * c], r[4 + 2 * c]});
        }
    }
    for (uint32_t s = n_sources; s <= COLLECT_MAX_SOURCES; s++) plan.first_emitter[s] = (uint32_t)plan.sel.size();
    return plan;
}

void collect_check_out_height(uint64_t out_height) {
    TS_REQUIRE(out_height <= COLLECT_MAX_HEIGHT && (out_height & (out_height - 1)) == 0, TS_ERR_INVALID,
               "collect: out_height " + std::to_string(out_height) + " is neither 0 nor a power of two in [1, 2^27]");
}

uint64_t collect_height(uint64_t n_live, uint64_t out_height) {
    TS_REQUIRE(out_height == 0 || n_live <= out_height, TS_ERR_INVALID,
               "collect: " + std::to_string(n_live) + " rows selected, out_height " + std::to_string(out_height));
    TS_REQUIRE(n_live <= COLLECT_MAX_HEIGHT, TS_ERR_INVALID,
               "collect: " + std::to_string(n_live) + " rows selected, more than 2^27");
    if (out_height) return out_height;
    uint64_t h = 1;
    while (h < n_live) h <<= 1;
    return h;
}

uint64_t collect_count_host(const CollectPlan& plan, const uint32_t* const* src, const uint64_t* heights) {
    uint64_t n = 0;
    for (uint32_t s = 0; s < plan.n_sources; s++) {
        const uint64_t width = plan.src_width[s];
        for (uint32_t e = plan.first_emitter[s]; e < plan.first_emitter[s + 1]; e++) {
            const uint32_t sel = plan.sel[e];
            if (sel == COLLECT_ALWAYS) {
                n += heights[s];
                continue;
            }
            for (uint64_t row = 0; row < heights[s]; row++) n += collect_fires(src[s][row * width + sel]);
        }
    }
    return n;
}

void collect_rows_host(const CollectPlan& plan, const uint32_t* const* src, const uint64_t* heights, uint64_t height,
                       uint32_t* out) {
    const uint32_t W = plan.out_width;
    uint64_t at = 0;
    for (uint32_t s = 0; s < plan.n_sources; s++)
        for (uint64_t row = 0; row < heights[s]; row++) {
            const uint32_t* r = src[s] + row * plan.src_width[s];
            for (uint32_t e = plan.first_emitter[s]; e < plan.first_emitter[s + 1]; e++) {
                const uint32_t sel = plan.sel[e];
                if (sel != COLLECT_ALWAYS && !collect_fires(r[sel])) continue;
                const CollectTermWord* t = plan.terms.data() + (size_t)e * W;
                uint32_t* o = out + at++ * W;
                for (uint32_t c = 0; c < W; c++)
                    o[c] = t[c].kind == C_CONST ? t[c].value : t[c].kind == C_COL ? r[t[c].value] : (uint32_t)row;
            }
        }
    for (; at < height; at++)
        for (uint32_t c = 0; c < W; c++) out[at * W + c] = plan.pad[c];
}

}  // namespace ts
