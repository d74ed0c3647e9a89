// The checks, the lowering and the host loop of a TITR program (csrc/derive.cpp, csrc/iterate.cpp) as a stand-alone
// program, so that tests/test_iterate_cpu.py can run them under AddressSanitizer and UBSan: compiled together with
// those two files, no library and no device.  Input: a file of little-endian 32-bit words,
//   n_cases, then per case: n_words, the tape, src_width, height, n_data_words, data
// Every buffer is sized exactly, so a read or write past the end of the tape, the source, the slot file or the result
// is a report.  Output: one line per case, "refused: TEXT" or "out_width n_instructions n_live fnv1a-of-the-result-words".
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "context.hpp"
#include "derive.hpp"

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
        std::vector<uint32_t> tape(n_words);  // its own allocation: a read past the tape is a report
        for (uint32_t& x : tape) x = take();
        const uint32_t src_width = take();
        const uint64_t height = take();
        std::vector<uint32_t> data(take());
        for (uint32_t& x : data) x = take();
        try {
            const ts::DeriveProgram prog = ts::derive_lower(tape.data(), tape.size(), src_width);
            TS_REQUIRE(data.size() == height * prog.src_width, ts::TS_ERR_INVALID, "probe: bad source size");
            std::vector<uint32_t> out((size_t)height * prog.out_width);
            ts::derive_rows_host(prog, data.data(), height, out.data());
            uint64_t h = 0xcbf29ce484222325ull;
            for (uint32_t x : out)
                for (int b = 0; b < 4; b++) h = (h ^ ((x >> (8 * b)) & 255)) * 0x100000001b3ull;
            printf("%u %u %u %016llx\n", prog.out_width, prog.n_nodes_kept, prog.n_live, (unsigned long long)h);
        } catch (const ts::Error& e) {
            printf("refused: %s\n", e.what());
        }
    }
    return 0;
}
