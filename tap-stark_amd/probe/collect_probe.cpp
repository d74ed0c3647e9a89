// The checks and the host loop of ts_matrix_collect_rows (csrc/collect.cpp) as a stand-alone program, so that
// tests/test_collect_cpu.py can run them under AddressSanitizer and UBSan: compiled together with collect.cpp, no
// library and no device.  Input: a file of little-endian 32-bit words,
//   n_cases, then per case: n_words, the spec, out_height, n_sources, per source {height, n_data_words, data}
// Every buffer is sized exactly, so a read or write past the end of a source or of the result is a report.  Output: one
// line per case, "refused: TEXT" or "height n_live fnv1a-of-the-result-words".
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "collect.hpp"
#include "context.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint32_t> in;
    uint32_t w;
    while (fread(&w, 4, 1, f) == 1) in.push_back(w);
    fclose(f);
    size_t at = 0;
    auto take = [&]() -> uint32_t {
        if (at >= in.size()) {
            fprintf(stderr, "the case file ends early\n");
            exit(2);
        }
        return in[at++];
    };
    const uint32_t n_cases = take();
    for (uint32_t k = 0; k < n_cases; k++) {
        const uint32_t n_words = take();
        std::vector<uint32_t> spec(n_words);  // its own allocation: a read past the spec is a report
        for (uint32_t& x : spec) x = take();
        const uint64_t out_height = take();
        const uint32_t n_sources = take();
        std::vector<std::vector<uint32_t>> data(n_sources);
        std::vector<uint64_t> heights(n_sources);
        for (uint32_t s = 0; s < n_sources; s++) {
            heights[s] = take();
            data[s].resize(take());
            for (uint32_t& x : data[s]) x = take();
        }
        try {
            const ts::CollectPlan plan = ts::collect_check(spec.data(), spec.size());
            TS_REQUIRE(plan.n_sources == n_sources, ts::TS_ERR_INVALID, "probe: the case has another number of sources");
            std::vector<const uint32_t*> ptrs;
            for (uint32_t s = 0; s < n_sources; s++) {
                TS_REQUIRE(data[s].size() == heights[s] * plan.src_width[s], ts::TS_ERR_INVALID, "probe: bad source size");
                ptrs.push_back(data[s].data());
            }
            ts::collect_check_out_height(out_height);
            const uint64_t live = ts::collect_count_host(plan, ptrs.data(), heights.data());
            const uint64_t height = ts::collect_height(live, out_height);
            std::vector<uint32_t> out((size_t)height * plan.out_width);
            ts::collect_rows_host(plan, ptrs.data(), heights.data(), height, out.data());
            uint64_t h = 0xcbf29ce484222325ull;
            for (uint32_t x : out)
                for (int b = 0; b < 4; b++) h = (h ^ ((x >> (8 * b)) & 255)) * 0x100000001b3ull;
            printf("%llu %llu %016llx\n", (unsigned long long)height, (unsigned long long)live, (unsigned long long)h);
        } catch (const ts::Error& e) {
            printf("refused: %s\n", e.what());
        }
    }
    return 0;
}
