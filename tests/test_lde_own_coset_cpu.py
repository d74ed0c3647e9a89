"""lde_own_coset (csrc/ntt_plan.hpp): which block of a whole coset LDE is its input.  Host only: a plain g++
program prints it for shifts that put H_n on each block in turn and for shifts that put it on none, and the output
is compared with the same question answered in Python integers."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tap-stark_amd", "csrc")
P = 0x78000001
G27 = 0x1A427A41

MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "ntt_plan.hpp"
int main(int argc, char** argv) {
    for (int i = 1; i + 2 < argc; i += 3)
        printf("%d\n", ts::lde_own_coset((unsigned)atoi(argv[i]), (unsigned)atoi(argv[i + 1]),
                                         (uint32_t)strtoul(argv[i + 2], nullptr, 10)));
    return 0;
}
"""


def bitrev(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2) if bits else 0


def own_coset(log_n, b, shift):
    """the definition: the beta with shift * w_N^bitrev_b(beta) = 1"""
    if log_n + b > 27 or not 0 < shift < P:
        return -1
    w = pow(G27, 1 << (27 - (log_n + b)), P)
    hits = [beta for beta in range(1 << b) if shift * pow(w, bitrev(beta, b), P) % P == 1]
    assert len(hits) <= 1
    return hits[0] if hits else -1


def cases():
    out = []
    for log_n in (0, 3, 12, 20, 23):
        for b in (0, 1, 2, 3):
            w = pow(G27, 1 << (27 - (log_n + b)), P)
            for e in range(1 << b):
                out.append((log_n, b, pow(w, P - 1 - e, P)))  # w_N^-e: block bitrev_b(e)
            wn = pow(G27, 1 << (27 - log_n), P)
            w2 = pow(G27, 1 << (27 - (log_n + b + 1)), P)
            # the trace commit's shift, 0 and p, an element of H_n other than 1, the next finer root
            out += [(log_n, b, 31), (log_n, b, 0), (log_n, b, P), (log_n, b, wn), (log_n, b, w2)]
    # the flagship's two quotient chunks (domain shifts 31 and 31 w_2n) and its reduced opening
    w2n = pow(G27, 1 << (27 - 21), P)
    out += [(20, 2, 1), (20, 2, 31 * pow(31 * w2n, P - 2, P) % P), (26, 1, 1), (26, 2, 1)]
    return out


def test_own_coset_by_the_definition(tmp_path):
    src, exe = tmp_path / "own_main.cpp", tmp_path / "own_main"
    src.write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe), str(src)],
                   check=True)
    cs = cases()
    args = [str(v) for c in cs for v in c]
    got = [int(x) for x in subprocess.run([str(exe), *args], check=True, capture_output=True, text=True).stdout.split()]
    want = [own_coset(*c) for c in cs]
    assert got == want, [(c, g, w) for c, g, w in zip(cs, got, want) if g != w]
    # the flagship: chunk 0 and the reduced opening on block 0, chunk 1 on block 1
    assert [own_coset(*c) for c in cs[-4:-2]] == [0, 1]
    # every block of every blowup is some shift's own, and some shifts have none
    assert {(b, w) for (_, b, _), w in zip(cs, want)} >= {(b, beta) for b in range(4) for beta in range(-1, 1 << b)}
