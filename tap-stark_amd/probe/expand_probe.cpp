// The checks and the host loop of ts_matrix_expand_rows (csrc/expand.cpp) as a stand-alone program, so that
// tests/test_expand_cpu.py can run them under AddressSanitizer and UBSan: compiled together with expand.cpp, no
// library and no device.  Input: a file of little-endian 32-bit words,
//   n_cases, then per case: n_words, the spec, out_height, height, n_data_words, data
// Every buffer is sized exactly, so a read or write past the end of the source or of the result is a report.  Output:
// one line per case, "refused: TEXT" or "height n_live fnv1a-of-the-result-words".
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "context.hpp"
#include "expand.hpp"

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
        const uint64_t height = take();
        std::vector<uint32_t> data(take());
        for (uint32_t& x : data) x = take();
        try {
            const ts::ExpandPlan plan = ts::expand_check(spec.data(), spec.size());
            TS_REQUIRE(data.size() == height * plan.src_width, ts::TS_ERR_INVALID, "probe: bad source size");
            ts::expand_check_out_height(out_height);
            const ts::ExpandTotals totals = ts::expand_count_host(plan, data.data(), height);
            const uint64_t used = ts::expand_height(plan, totals, out_height);
            std::vector<uint32_t> out((size_t)used * plan.out_width);
            ts::expand_rows_host(plan, data.data(), height, used, out.data());
            uint64_t h = 0xcbf29ce484222325ull;
            for (uint32_t x : out)
                for (int b = 0; b < 4; b++) h = (h ^ ((x >> (8 * b)) & 255)) * 0x100000001b3ull;
            printf("%llu %llu %016llx\n", (unsigned long long)used, (unsigned long long)totals.total,
                   (unsigned long long)h);
        } catch (const ts::Error& e) {
            printf("refused: %s\n", e.what());
        }
    }
    return 0;
}
