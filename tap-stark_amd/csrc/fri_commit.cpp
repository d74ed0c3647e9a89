// bf_commit_phase (fri/src/prover.rs:93-141) and the proof-of-work step (:43), shared by prove / fri_prove
// (prover.cpp) and prove_sharded (sharded.cpp).  The transcript moves to the device for the whole phase: per
// round the kernel that makes the root observes it and samples beta, the fold reads beta from device memory,
// and once the vector is short (and no further input is waiting to be added) the remaining rounds run inside
// one workgroup (launch_fri_tail).  One D2H at the end brings back roots, the final values and the challenger
// state.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "prover_internal.hpp"

namespace ts {

void fri_commit_begin(Context& ctx, const FriConfig& fri, unsigned log_max_height,
                      const BfChallenger& challenger, FriCommit& st) {
    TS_REQUIRE(log_max_height >= fri.log_blowup, TS_ERR_INVALID, "FRI: vector shorter than the blowup");
    st.R_total = log_max_height - fri.log_blowup;
    DevChallenger hc;
    challenger.export_dev(hc);
    static_assert(sizeof(DevChallenger) <= 64 * 4, "the challenger's slot in the block");
    const size_t n_roots = std::max<size_t>(8 * (size_t)st.R_total, 8);
    st.d_block = DevBuf<uint32_t>(&ctx, 64 + n_roots + 4 * (size_t)fri.blowup());
    st.d_chal.p = st.d_block.p;
    st.d_roots.p = st.d_block.p + 64;
    st.d_final.p = reinterpret_cast<Ef*>(st.d_block.p + 64 + n_roots);  // 16-byte aligned: 64 + 8 R words
    uint32_t slot[64] = {0};
    static_assert(sizeof(DevChallenger) <= FRI_POW_WORD * 4, "the hint word lies behind the challenger");
    memcpy(slot, &hc, sizeof hc);
    slot[FRI_POW_WORD] = FRI_POW_NONE;
    h2d(ctx, st.d_chal.p, slot, sizeof slot);
    st.d_betas = DevBuf<Ef>(&ctx, std::max<size_t>(st.R_total, 1));
}

void FriCommit::round(Context& ctx, bool defer_next, const TopStep& top, uint64_t h_global, uint64_t row0) {
    FriRound r;
    const uint64_t h = len / 2;
    r.log_leaves = log2_strict(h);
    const size_t ri = rounds.size();
    DevBuf<uint32_t> tree(&ctx, merkle_total_digests(r.log_leaves) * 8);
    if (deferred) cur = DevBuf<Ef>(&ctx, len);
    // :113 commit_matrix, :114-116 observe + sample (in the kernel that makes the root, or in `top`)
    FriRoundLaunch l{deferred, deferred ? d_betas.p + ri - 1 : nullptr, cur.p, h, tree.p};
    if (!top) {
        l.ch = dch();
        l.root_out = d_roots.p + 8 * ri;
        l.beta_out = d_betas.p + ri;
    }
    l.h_global = h_global;
    l.row0 = row0;
    launch_fri_commit_round(ctx, l);
    if (top) top(tree.p + 8 * (merkle_total_digests(r.log_leaves) - 1), ri);
    r.vec = cur.p;
    r.tree = tree.p;
    if (defer_next) {
        deferred = cur.p;  // :119 happens inside the next launch
        keep_vecs.push_back(std::move(cur));
    } else {
        DevBuf<Ef> out(&ctx, h);
        launch_fri_fold_dev(ctx, cur.p, h, d_betas.p + ri, out.p, nullptr, h_global, row0);  // :119 fold_matrix
        keep_vecs.push_back(std::move(cur));
        cur = std::move(out);
        deferred = nullptr;
    }
    keep_trees.push_back(std::move(tree));
    rounds.push_back(r);
    len = h;
}

void fri_commit_rounds(Context& ctx, const FriConfig& fri, DevBuf<Ef> folded, uint64_t len,
                       std::vector<DevBuf<Ef>>& inputs, const std::vector<unsigned>& log_lens,
                       size_t next_in, FriCommit& st) {
    st.cur = std::move(folded);
    st.len = len;
    st.deferred = nullptr;
    // rounds done with one launch each; the rest goes to the tail kernel
    auto big = [&](uint64_t l) {
        return l > fri.blowup() && (l > (1ull << FRI_TAIL_LOG) || next_in < inputs.size());
    };
    while (big(st.len)) {  // :111
        const uint64_t h = st.len / 2;
        const bool add_pending = next_in < inputs.size() && (1ull << log_lens[next_in]) == h;
        // the next vector is needed in memory now only if an input is added to it or it holds the final values;
        // otherwise the next launch folds it: the next round's, or the tail kernel's (one launch less)
        st.round(ctx, /*defer_next=*/!add_pending && h > fri.blowup());
        if (add_pending) {  // :124-126 izip!(&mut folded, v).for_each(|(c, x)| *c += x)
            launch_vec_add(ctx, st.cur.p, inputs[next_in].p, h);
            st.keep_vecs.push_back(std::move(inputs[next_in]));
            next_in++;
        }
    }
    TS_REQUIRE(next_in == inputs.size(), TS_ERR_INVARIANT, "FRI: an input was never folded in");
    if (st.len > fri.blowup()) {  // tail rounds in one workgroup
        const uint32_t L0 = (uint32_t)st.len;
        DevBuf<Ef> tail_vecs(&ctx, 2 * (size_t)L0);
        DevBuf<uint32_t> tail_trees(&ctx, 8 * 2 * (size_t)L0);
        const size_t ri = st.rounds.size();
        static const bool host_grind = [] { const char* e = getenv("TS_HOST_GRIND"); return e && atoi(e) != 0; }();
        launch_fri_tail(ctx, st.deferred ? st.deferred : st.cur.p, L0, fri.blowup(), st.dch(), tail_vecs.p,
                        tail_trees.p, st.d_roots.p + 8 * ri, st.d_betas.p + ri, st.d_final.p, fri.proof_of_work_bits,
                        host_grind ? nullptr : st.d_chal.p + FRI_POW_WORD,
                        st.deferred ? st.d_betas.p + ri - 1 : nullptr);
        uint32_t L = L0;
        size_t voff = 0, toff = 0;
        while (L > fri.blowup()) {
            FriRound r;
            r.log_leaves = log2_strict(L / 2);
            r.vec = tail_vecs.p + voff;
            r.tree = tail_trees.p + 8 * toff;
            st.rounds.push_back(r);
            voff += L;
            toff += L - 1;
            L >>= 1;
        }
        st.len = L;
        st.keep_vecs.push_back(std::move(tail_vecs));
        st.keep_trees.push_back(std::move(tail_trees));
    } else {
        TS_HIP(hipMemcpyAsync(st.d_final.p, st.cur.p, st.len * sizeof(Ef), hipMemcpyDeviceToDevice, ctx.stream));
    }
    st.keep_vecs.push_back(std::move(st.cur));
    st.final_len = st.len;
}

Ef fri_commit_finish(Context& ctx, const FriConfig& fri, BfChallenger& challenger, FriCommit& st) {
    // :129-134 `blowup` evaluations of a constant polynomial
    TS_REQUIRE(st.final_len == fri.blowup(), TS_ERR_INVARIANT, "FRI: folded length != blowup");
    TS_REQUIRE(st.rounds.size() == st.R_total, TS_ERR_INVARIANT, "FRI: round count");
    const uint32_t R_total = st.R_total;
    std::vector<Ef> fin(st.final_len);
    std::vector<uint32_t> roots(std::max<size_t>(8 * (size_t)R_total, 8));
    DevChallenger hc;
    std::vector<uint32_t> block(st.d_block.n);
    ctx.d2h_point(block.data(), st.d_block.p, block.size() * 4);
    memcpy(&hc, block.data(), sizeof hc);
    st.pow_hint = block[FRI_POW_WORD];
    memcpy(roots.data(), block.data() + 64, roots.size() * 4);
    memcpy(fin.data(), block.data() + 64 + roots.size(), fin.size() * sizeof(Ef));
    challenger.import_dev(hc);
    for (uint32_t r = 0; r < R_total; r++) memcpy(st.rounds[r].root, &roots[8 * (size_t)r], 32);
    const Ef final_poly = fin[0];
    for (auto& x : fin)
        if (!ef_eq(x, final_poly))
            throw FinalPolyNotConstant("FRI: final polynomial is not constant (assert_eq!(x, final_poly))");
    return final_poly;
}

uint32_t fri_pow_witness(Context& ctx, BfChallenger& challenger, unsigned bits, const FriCommit& st) {
    if (st.pow_hint < (1u << 12)) {
        BfChallenger clone = challenger;
        if (clone.check_witness(bits, st.pow_hint)) {
            challenger = clone;
            ctx.pow_hints_accepted++;
            return st.pow_hint;
        }
        ctx.pow_hints_rejected++;  // never expected: the device search and the host sponge disagree
    }
    ctx.pow_host_grinds++;
    return challenger.grind(bits);
}

}  // namespace ts
