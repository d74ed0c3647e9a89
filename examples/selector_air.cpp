// The capture of an AIR with preprocessed columns in C++ (include/tapstark_air.hpp): SelectorAir of
// tap-stark_amd/airs.py, word for word the tape the Python builder gives.  Prints the version-2 tape, one word
// per line; needs neither the library nor a GPU:
//     g++ -std=c++17 -I include examples/selector_air.cpp -o selector_air && ./selector_air
// Hand the words to ts_air_compile and the committed (sel, rc, spare) matrix to ts_prove_pre as the key.
#include <stdio.h>

#include "tapstark_air.hpp"

using ts::air::Builder;
using ts::air::Expr;

// preprocessed (sel, rc, spare), main (a, b, c), public values [a_0, c_last].  Every operand is named before it
// is used: C++ leaves the evaluation order of an operator's operands open, the node order of the tape is fixed.
static void eval(Builder& b) {
    const auto &pl = b.preprocessed(0), &pn = b.preprocessed(1);
    const auto &local = b.local(), &next = b.next(), &pis = b.public_values();
    const Expr sel = pl[0], rc = pl[1];
    const Expr a = local[0], bb = local[1], c = local[2];
    const Expr mul_row = sel * (a * bb - c);
    const Expr not_sel = b.constant(1) - sel;
    const Expr add_row = not_sel * (a + bb + rc - c);
    b.assert_zero(mul_row + add_row);  // the row multiplies or adds, as the key says
    auto when_transition = b.when_transition();
    when_transition.assert_eq(next[0], c);
    when_transition.assert_eq(next[1], bb + pn[1]);  // reads the preprocessed NEXT row
    b.when_first_row().assert_eq(a, pis[0]);
    b.when_last_row().assert_eq(c, pis[1]);
}

int main() {
    Builder b(3, 2, 3);
    eval(b);
    for (uint32_t w : b.tape()) printf("%u\n", w);
    return 0;
}
