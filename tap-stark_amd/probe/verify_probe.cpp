// The host-only verifier of the single-table formats as a stand-alone program, for a sanitizer build
// (tests/test_single_cpu.py builds it with -fsanitize=address,undefined and runs it; no GPU, no Python in the process).
//
//     verify_probe CASES.bin
//
// CASES.bin is a flat little-endian dump of u32 words, one record after another:
//     version, expected verdict, log_blowup, num_queries, proof_of_work_bits, n_tape, n_public, has_root, n_words,
//     tape[n_tape], public values[n_public], root[8 if has_root], proof[n_words]
// Prints one line per record and exits 1 if a verdict differs from the expected one, 2 on a malformed file.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "host.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint32_t> w;
    uint32_t word;
    while (fread(&word, 4, 1, f) == 1) w.push_back(word);
    fclose(f);
    size_t pos = 0, record = 0;
    int bad = 0;
    while (pos < w.size()) {
        if (w.size() - pos < 9) return 2;
        const uint32_t* h = &w[pos];
        const size_t n_tape = h[5], n_public = h[6], n_root = h[7] ? 8 : 0, n_words = h[8];
        pos += 9;
        if (w.size() - pos < n_tape + n_public + n_root + n_words) return 2;
        // every array in a buffer of its exact size: a read past its end is the sanitizer's to see
        const std::vector<uint32_t> tape(w.begin() + pos, w.begin() + pos + n_tape);
        pos += n_tape;
        const std::vector<uint32_t> pis(w.begin() + pos, w.begin() + pos + n_public);
        pos += n_public;
        const std::vector<uint32_t> root(w.begin() + pos, w.begin() + pos + n_root);
        pos += n_root;
        const std::vector<uint32_t> proof(w.begin() + pos, w.begin() + pos + n_words);
        pos += n_words;
        ts::FriConfig fri;
        fri.log_blowup = h[2];
        fri.num_queries = h[3];
        fri.proof_of_work_bits = h[4];
        const ts::AirProgram air = ts::compile_air(tape.data(), tape.size());
        ts::BfChallenger chal(0, true);
        std::vector<uint32_t> exposed;
        const int verdict = ts::verify(h[0], fri, air, chal, proof.data(), proof.size(), pis, n_root ? root.data() : nullptr,
                                       h[0] >= 4 ? &exposed : nullptr);
        printf("record %zu: TSPF v%u, %zu words: verdict %d (expected %u), %zu exposed words\n", record++, h[0], n_words,
               verdict, h[1], exposed.size());
        bad |= verdict != (int)h[1];
    }
    return bad;
}
