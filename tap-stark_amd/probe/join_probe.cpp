// The checks and the host loop of ts_matrix_join_rows (csrc/join.cpp) as a stand-alone program, so that
// tests/test_join_cpu.py can run them under AddressSanitizer and UBSan: compiled together with join.cpp, no library and
// no device.  Input: a file of little-endian 32-bit words,
//   n_cases, then per case: size_ok, n_keys, n_keys x {kind, value} on the source, the same on the table, when {kind,
//   value}, n_fetch, n_fetch table columns, n_fetch dst columns, n_fetch defaults, flags, table_rows,
//   src_height, src_width, the source's words, same (1: the table IS the source), else table_height, table_width, words
// Every buffer is sized exactly, so a read or write past the end of a key list, a matrix or the result is a report.
// Output: one line per case, "refused: TEXT" or "out_width n_missing first_missing fnv1a-of-the-result-words".
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "context.hpp"
#include "join.hpp"

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
    auto take_terms = [&](uint32_t n) {
        std::vector<ts::JoinTerm> t(n);  // its own allocation: a read past the list is a report
        for (ts::JoinTerm& x : t) {
            x.kind = take();
            x.value = take();
        }
        return t;
    };
    auto take_words = [&](size_t n) {
        std::vector<uint32_t> t(n);
        for (uint32_t& x : t) x = take();
        return t;
    };
    const uint32_t n_cases = take();
    for (uint32_t k = 0; k < n_cases; k++) {
        ts::JoinSpecIn spec = {};
        spec.size_ok = take() != 0;
        spec.n_keys = take();
        if (spec.n_keys > 64) return 2;
        const std::vector<ts::JoinTerm> src_keys = take_terms(spec.n_keys), table_keys = take_terms(spec.n_keys);
        spec.src_keys = src_keys.data();
        spec.table_keys = table_keys.data();
        spec.when.kind = take();
        spec.when.value = take();
        spec.n_fetch = take();
        if (spec.n_fetch > 64) return 2;
        const std::vector<uint32_t> tc = take_words(spec.n_fetch), dc = take_words(spec.n_fetch), df = take_words(spec.n_fetch);
        spec.table_columns = tc.data();
        spec.dst_columns = dc.data();
        spec.defaults = df.data();
        spec.flags = take();
        spec.table_rows = take();
        const uint64_t src_height = take();
        const uint32_t src_width = take();
        const std::vector<uint32_t> src = take_words((size_t)src_height * src_width);
        const bool same = take() != 0;
        uint64_t table_height = src_height;
        uint32_t table_width = src_width;
        std::vector<uint32_t> own;
        if (!same) {
            table_height = take();
            table_width = take();
            own = take_words((size_t)table_height * table_width);
        }
        const uint32_t* table = same ? src.data() : own.data();
        try {
            const ts::JoinPlan plan = ts::join_check(spec, src_width, table_width);
            const uint64_t n_table = ts::join_table_rows(plan, src_height, table_height);
            std::vector<uint32_t> match;
            uint64_t first = ~0ull;
            const uint64_t n_missing = ts::join_match_host(plan, src.data(), src_height, table, n_table, match, &first);
            std::vector<uint32_t> out((size_t)src_height * plan.out_width);
            ts::join_rows_host(plan, src.data(), src_height, table, match, out.data());
            uint64_t h = 0xcbf29ce484222325ull;
            for (uint32_t x : out)
                for (int b = 0; b < 4; b++) h = (h ^ ((x >> (8 * b)) & 255)) * 0x100000001b3ull;
            printf("%u %llu %lld %016llx\n", plan.out_width, (unsigned long long)n_missing, (long long)first,
                   (unsigned long long)h);
        } catch (const ts::Error& e) {
            printf("refused: %s\n", e.what());
        }
    }
    return 0;
}
