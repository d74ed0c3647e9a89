"""The alpha ledger of the PCS opening (csrc/open_plan.hpp) is host-only and free of HIP: a plain g++ program
drives it through the visit sequences of the three provers and checks every offset, constant, folded weight and
rescaled opened value against schoolbook arithmetic (repeated multiplication, % p) written out in the program.
The same program runs once more as a stand-alone binary under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tap-stark_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include <map>
#include "open_plan.hpp"
using namespace ts;

// schoolbook EF4 = F[x]/(x^4 - 11) on canonical words: the reference the ledger is checked against
static Ef nmul(Ef a, Ef b) {
    uint64_t r[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r[i + j] = (r[i + j] + (uint64_t)a.c[i] * b.c[j]) % P;
    Ef o;
    for (int i = 0; i < 4; i++) o.c[i] = (uint32_t)((r[i] + (i < 3 ? 11 * r[i + 4] : 0)) % P);
    return o;
}
static Ef nadd(Ef a, Ef b) {
    Ef o;
    for (int i = 0; i < 4; i++) o.c[i] = (uint32_t)(((uint64_t)a.c[i] + b.c[i]) % P);
    return o;
}
static Ef npow(Ef a, uint64_t e) {  // repeated multiplication
    Ef r = Ef{{1, 0, 0, 0}};
    for (uint64_t i = 0; i < e; i++) r = nmul(r, a);
    return r;
}
static uint32_t lcg = 12345;
static Ef next_ef() {  // fixed canonical values
    Ef o;
    for (int i = 0; i < 4; i++) {
        lcg = lcg * 1664525u + 1013904223u;
        o.c[i] = lcg % P;
    }
    return o;
}

static int failures = 0;
static void expect(bool ok, const char* what, const char* seq, size_t visit) {
    if (!ok) {
        printf("MISMATCH %s: %s at visit %zu\n", seq, what, visit);
        failures++;
    }
}

struct V { unsigned log_h; uint32_t width; int slot; };

static void run(const char* name, const V* seq, size_t n, uint32_t max_w) {
    const Ef alpha = Ef{{0x12345678u % P, 0x0badcafeu % P, 77, P - 1}};
    AlphaLedger ledger(alpha, max_w);
    expect(ledger.powers().size() == 4 * (size_t)max_w, "powers size", name, 0);
    for (uint32_t i = 0; i < max_w; i++)
        expect(ef_eq(ef_from_mont(ledger.power(i)), npow(alpha, i)), "alpha power", name, i);
    std::map<unsigned, uint64_t> widths_before;
    std::map<unsigned, Ef> k[2];
    for (size_t v = 0; v < n; v++) {
        const V s = seq[v];
        std::vector<Ef> ys(s.width);
        for (Ef& y : ys) y = next_ef();
        const AlphaLedger::Visit got = ledger.visit(s.log_h, ys.data(), s.width, s.slot);
        const Ef off = npow(alpha, widths_before[s.log_h]);
        expect(ef_eq(ef_from_mont(got.off), off), "offset", name, v);
        Ef rys = ef_zero();
        for (uint32_t i = 0; i < s.width; i++) rys = nadd(rys, nmul(npow(alpha, i), ys[i]));
        expect(ef_eq(got.rys, rys), "reduced ys", name, v);
        if (!k[s.slot].count(s.log_h)) k[s.slot][s.log_h] = ef_zero();
        k[s.slot][s.log_h] = nadd(k[s.slot][s.log_h], nmul(off, rys));
        for (int slot = 0; slot < 2; slot++)
            for (auto& [log_h, want] : k[slot]) expect(ef_eq(ledger.k(log_h, slot), want), "k0 / k1", name, v);
        std::vector<uint32_t> folded(3, 0xdeadbeefu);  // appended to, not overwritten
        ledger.fold_weights(got.off, s.width, folded);
        expect(folded.size() == 3 + 4 * (size_t)s.width && folded[2] == 0xdeadbeefu, "folded size", name, v);
        for (uint32_t i = 0; i < s.width && folded.size() == 3 + 4 * (size_t)s.width; i++) {
            Ef w;
            memcpy(w.c, &folded[3 + 4 * (size_t)i], 16);
            expect(ef_eq(ef_from_mont(w), nmul(npow(alpha, i), off)), "folded weight", name, v);
        }
        widths_before[s.log_h] += s.width;
    }
    for (unsigned h = 0; h < AlphaLedger::MAX_LOG_HEIGHT; h++)
        if (!widths_before.count(h))
            expect(ef_eq(ledger.k(h, 0), ef_zero()) && ef_eq(ledger.k(h, 1), ef_zero()), "untouched height", name, h);
}

static void rescale(uint32_t width, uint32_t np) {
    std::vector<Ef> raw((size_t)width * np), out((size_t)width * np + 1);
    for (Ef& r : raw) r = next_ef();
    const Ef scale[2] = {next_ef(), next_ef()};
    const Ef guard = Ef{{1, 2, 3, 4}};
    out[(size_t)width * np] = guard;
    opened_from_raw(raw.data(), width, np, scale, out.data());
    for (uint32_t p = 0; p < np; p++)
        for (uint32_t c = 0; c < width; c++)
            expect(ef_eq(out[(size_t)p * width + c], nmul(raw[(size_t)c * np + p], scale[p])), "rescale", "rescale",
                   p * width + c);
    expect(ef_eq(out[(size_t)width * np], guard), "rescale wrote past the end", "rescale", np);
}

int main() {
    // prove(): trace at two points, then qd chunks at the first; w = 5, qd = 2
    const V plain[] = {{10, 5, 0}, {10, 5, 1}, {10, 4, 0}, {10, 4, 0}};
    run("plain", plain, 4, 5);
    // key, aux, trace at two points each, then the chunks; pw = 3, aw = 2, w = 5, qd = 1
    const V four[] = {{9, 3, 0}, {9, 3, 1}, {9, 2, 0}, {9, 2, 1}, {9, 5, 0}, {9, 5, 1}, {9, 4, 0}};
    run("four rounds", four, 7, 5);
    // prove_multi: two traces of widths 2 and 7 at different heights, then their chunks (1 and 2 of them)
    const V multi[] = {{8, 2, 0}, {8, 2, 1}, {12, 7, 0}, {12, 7, 1}, {8, 4, 0}, {12, 4, 0}, {12, 4, 0}};
    run("two heights", multi, 7, 7);
    rescale(3, 1);
    rescale(3, 2);
    rescale(8, 1);  // the chunks' shape: 4 qd columns at one point
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan_dir(tmp_path_factory):
    td = tmp_path_factory.mktemp("open_plan")
    (td / "open_plan_main.cpp").write_text(MAIN)
    return td


def _build_and_run(td, exe, extra):
    # plain g++, no HIP include path: the header must stand on its own
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, "-o", str(td / exe),
                    str(td / "open_plan_main.cpp")], check=True)
    return subprocess.run([str(td / exe)], capture_output=True, text=True)


def test_ledger_against_schoolbook_arithmetic(plan_dir):
    r = _build_and_run(plan_dir, "open_plan_main", ["-O1"])
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr


def test_ledger_clean_under_sanitizers(plan_dir):
    """A stand-alone host binary with its own main: nothing is preloaded."""
    r = _build_and_run(plan_dir, "open_plan_main_san",
                       ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
