"""The NTT pass plan (csrc/ntt_plan.hpp) is host-only and free of HIP: a plain g++ program prints it for every
height and the limit checks, and the output is compared with the table written out here -- what coset_lde and
dft_columns each derived on their own before the plan had one owner."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tap-stark_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include "ntt_plan.hpp"
using namespace ts;
static void refusal(const char* what, unsigned log_n, uint32_t ncols, uint64_t sa, uint64_t sb, bool lde) {
    const char* why = ntt_plan_refusal(ntt_plan(log_n), ncols, sa, sb, lde);
    printf("%s: %s\n", what, why ? why : "ok");
}
int main() {
    for (unsigned log_n = 0; log_n <= 26; log_n++) {
        const NttPlan p = ntt_plan(log_n);
        const char* mid = p.mid == NttMid::GENERIC ? "generic" : p.mid == NttMid::FIXED256 ? "fixed" : "tile16384";
        printf("%u %s LM=%u sA=%u log_T=%u log_len=%u row_shift=%u %s fused=%d chunks=%u tiles=%u chunk_log=%u\n",
               p.log_n, p.two_pass ? "two" : "one", p.LM, p.sA, p.log_T, p.log_len, p.row_shift, mid,
               (int)p.fused_first_round, p.chunks, p.tiles, lde_chunk_log(log_n));
        if (ntt_plan_refusal(p, 1, 4, 4, false) || ntt_plan_refusal(p, NTT_MAX_COLS, 8, 0, true)) return 1;
    }
    refusal("27 dft", 27, 1, 4, 0, false);
    refusal("27 lde", 27, 1, 4, 4, true);
    refusal("stride 6 one pass dft", 12, 3, 6, 0, false);
    refusal("stride 6 one pass lde", 12, 3, 6, 6, true);
    refusal("stride 6 two pass dft", 13, 3, 6, 0, false);
    refusal("in stride 6 two pass lde", 13, 3, 6, 8, true);
    refusal("out stride 6 two pass lde", 13, 3, 8, 6, true);
    refusal("65535 columns", 13, 65535, 8, 8, true);
    refusal("65536 columns dft", 13, 65536, 8, 0, false);
    refusal("65536 columns lde", 5, 65536, 8, 8, true);
    return 0;
}
"""


def row(log_n, passes, lm, sa, log_t, mid):
    two = passes == "two"
    return (f"{log_n} {passes} LM={lm} sA={sa} log_T={log_t} log_len={sa if two else log_n} "
            f"row_shift={lm if two else 0} {mid} fused={int(two)} chunks={1 << sa} "
            f"tiles={1 << (lm - log_t) if two else 1} chunk_log={lm}")


# log_n -> (passes, LM, sA, log_T, middle variant): the table of the plan, written out
TABLE = {lg: ("one", 12, 0, 0, "generic") for lg in range(13)}
TABLE.update({
    13: ("two", 12, 1, 6, "generic"), 14: ("two", 12, 2, 6, "generic"), 15: ("two", 12, 3, 6, "generic"),
    16: ("two", 12, 4, 6, "generic"), 17: ("two", 12, 5, 6, "generic"), 18: ("two", 12, 6, 6, "generic"),
    19: ("two", 12, 7, 6, "generic"),
    20: ("two", 12, 8, 5, "fixed"), 21: ("two", 13, 8, 5, "fixed"), 22: ("two", 14, 8, 5, "fixed"),
    23: ("two", 12, 11, 2, "generic"), 24: ("two", 12, 12, 1, "generic"), 25: ("two", 12, 13, 0, "generic"),
    26: ("two", 12, 14, 0, "tile16384"),
})

REFUSALS = [
    "27 dft: dft: height above 2^26",
    "27 lde: coset_lde: log_n > 26",
    "stride 6 one pass dft: ok",
    "stride 6 one pass lde: ok",
    "stride 6 two pass dft: dft: column stride must be a multiple of 4 elements",
    "in stride 6 two pass lde: coset_lde: column strides must be multiples of 4 elements",
    "out stride 6 two pass lde: coset_lde: column strides must be multiples of 4 elements",
    "65535 columns: ok",
    "65536 columns dft: dft: more than 65535 columns",
    "65536 columns lde: coset_lde: bad column count",
]


@pytest.fixture(scope="module")
def plan_output(tmp_path_factory):
    td = tmp_path_factory.mktemp("ntt_plan")
    src, exe = td / "plan_main.cpp", td / "plan_main"
    src.write_text(MAIN)
    # plain g++, no HIP include path: the header must stand on its own
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe), str(src)],
                   check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()


def test_plan_table(plan_output):
    assert sorted(TABLE) == list(range(27))
    assert plan_output[:27] == [row(lg, *TABLE[lg]) for lg in range(27)]


def test_plan_limits(plan_output):
    assert plan_output[27:] == REFUSALS
