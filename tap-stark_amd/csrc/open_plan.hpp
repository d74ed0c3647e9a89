// The host arithmetic of the PCS opening (reference fri/src/two_adic_pcs.rs:331-383), with one owner: the powers
// of the batching challenge alpha, the num_reduced counter per height, the offsets alpha^num_reduced, the
// reduced opened values <alpha powers, ys> and the constants and folded weights the one-pass reduce kernels
// take.  open_reduce_slab, TwoAdicFriPcs::open (prover.cpp) and open_classes (prove_multi.cpp) launch different
// kernels and all keep their books here.  Host only and free of HIP, so that a plain C++ compiler can build it
// (tests/test_open_plan_cpu.py drives it against naive arithmetic).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "bb.hpp"

namespace ts {

// alpha^0 .. alpha^(count-1) in Montgomery form, 4 words each: what the kernels take as `alpha_pows`
inline std::vector<uint32_t> alpha_powers_mont(Ef alpha, size_t count) {
    std::vector<uint32_t> pw(4 * count);
    const Ef am = ef_to_mont(alpha);
    Ef cur = ef_one_mont();
    for (size_t i = 0; i < count; i++) {
        memcpy(&pw[4 * i], cur.c, 16);
        cur = ef_mul(cur, am);
    }
    return pw;
}

class AlphaLedger {
public:
    static constexpr unsigned MAX_LOG_HEIGHT = 32;  // :331 reduced_openings: [_; 32]

    // max_width: the widest matrix that will be visited (or folded)
    AlphaLedger(Ef alpha, uint32_t max_width)
        : alpha_mont_(ef_to_mont(alpha)), powers_(alpha_powers_mont(alpha, max_width)) {
        for (unsigned h = 0; h < MAX_LOG_HEIGHT; h++) {
            num_reduced_[h] = 0;
            k_[h][0] = k_[h][1] = ef_zero();
        }
    }

    const std::vector<uint32_t>& powers() const { return powers_; }
    Ef power(uint32_t i) const {  // alpha^i, Montgomery
        Ef p;
        memcpy(p.c, &powers_[4 * (size_t)i], 16);
        return p;
    }

    struct Visit {
        Ef off;  // alpha^num_reduced before this visit (:371), Montgomery
        Ef rys;  // dot_product(alpha.powers(), ys) (:372), canonical
    };
    // One (matrix, point) of two_adic_pcs.rs:371-383 at height 2^log_h: `ys` are the matrix's `width` opened
    // values at the point (canonical).  Adds off * rys to the height's constant k(log_h, slot) -- slot 0 or 1:
    // which of the (at most two) points of the height the visit belongs to -- and advances num_reduced (:383).
    Visit visit(unsigned log_h, const Ef* ys, uint32_t width, int slot) {
        Visit v;
        v.off = ef_pow(alpha_mont_, num_reduced_[log_h]);
        v.rys = ef_zero();
        for (uint32_t i = 0; i < width; i++) v.rys = ef_add(v.rys, ef_mul(ys[i], power(i)));  // canonical x Montgomery
        k_[log_h][slot] = ef_add(k_[log_h][slot], ef_mul(v.rys, v.off));
        num_reduced_[log_h] += width;
        return v;
    }
    // sum over the visits of (log_h, slot) of off * rys, canonical: k0 / k1 of the one-pass reduce kernels
    Ef k(unsigned log_h, int slot) const { return k_[log_h][slot]; }

    // appends alpha^k * off for k < width (Montgomery, 4 words each): with these as column weights ONE dot product
    // over a matrix's row gives off * S, and over the rows of several matrices the sum of theirs
    void fold_weights(Ef off, uint32_t width, std::vector<uint32_t>& out) const {
        for (uint32_t k = 0; k < width; k++) {
            const Ef wk = ef_mul(power(k), off);
            out.insert(out.end(), wk.c, wk.c + 4);
        }
    }

private:
    Ef alpha_mont_;
    std::vector<uint32_t> powers_;
    uint64_t num_reduced_[MAX_LOG_HEIGHT];  // :332
    Ef k_[MAX_LOG_HEIGHT][2];
};

// The barycentric dot kernels leave raw sums as [col][point]; p(z_p) = scale[p] * sum (scale: bary_scale, canonical).
// out[p * width + c] = raw[c * n_points + p] * scale[p]: the opened values in (point, column) order.
inline void opened_from_raw(const Ef* raw, uint32_t width, uint32_t n_points, const Ef* scale, Ef* out) {
    for (uint32_t p = 0; p < n_points; p++) {
        const Ef sm = ef_to_mont(scale[p]);
        for (uint32_t c = 0; c < width; c++) out[(size_t)p * width + c] = ef_mul(raw[(size_t)c * n_points + p], sm);
    }
}

}  // namespace ts
