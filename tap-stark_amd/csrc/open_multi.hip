// The opening kernels of a multi-table proof (prove_multi.cpp; reference fri/src/two_adic_pcs.rs:260-389 `open`
// over two rounds of mixed heights).  The chunks of a table have the table's height, so every committed matrix
// of one LDE height -- a height class -- is opened at the same two points at most: all of them at zeta, the
// traces at zeta omega_n too.  That is the shape k_reduce_fused (open.hip) runs for one table; here the
// matrices of a class come from a job table in device memory instead of a by-value struct, which cost that
// kernel VGPRs with 64 pointers (see its comment) and would not hold 64 + 64 matrices at all.
#include "kernels.hpp"
#include "open_dev.hpp"

namespace ts {

// ------------------------------------------------------------------ reduce, one pass per height class
// ro[X] = inv(x - z0) * ( sum_m off_{m,0} S_m(X) - k0 ) + inv(x - z1) * ( sum_{m trace} off_{m,1} S_m(X) - k1 )
// S_m = the alpha-power row dot of matrix m (row_dot_acc, lazy accumulation).  A trace's S_m is shared by its
// two openings, as in k_reduce_fused; the chunks' terms off_{m,0} S_m are ONE running dot product over the
// columns of every chunk with the weights alpha^k off_{m,0} folded on the host.  One pair of inverses and one
// 16-byte store per row; ro is not read.  Every lane reads jobs[j] at the same j: scalar loads.
__global__ void __launch_bounds__(256)
k_reduce_class(const ClassJob* __restrict__ jobs, uint32_t n_jobs, unsigned log_h, const uint32_t* __restrict__ W,
               uint32_t gen_mont, const uint32_t* __restrict__ alpha_pows, ClassReduceArgs a, Ef* __restrict__ ro) {
    const uint64_t X = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= (1ull << log_h)) return;
    Ef g0 = ef_zero(), g1 = ef_zero();
    uint64_t acc[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < n_jobs; j++) {
        const uint32_t* d = jobs[j].d;
        const uint64_t stride = jobs[j].col_stride;
        const uint32_t width = jobs[j].width;
        if (jobs[j].has_next) {
            const Ef S = row_dot_alpha(d, stride, width, X, alpha_pows);
            g0 = ef_add(g0, ef_mul(S, jobs[j].off[0]));  // canonical x Montgomery -> canonical
            g1 = ef_add(g1, ef_mul(S, jobs[j].off[1]));
        } else {
            row_dot_acc(acc, d, stride, width, X, jobs[j].weights);
        }
    }
    const Ef D{{lazy_finish(acc[0]), lazy_finish(acc[1]), lazy_finish(acc[2]), lazy_finish(acc[3])}};
    g0 = ef_sub(ef_add(g0, D), a.k0);
    g1 = ef_sub(g1, a.k1);
    // x_X = 31 * omega_h^bitrev(X), Montgomery
    const uint32_t x = mont_mul(gen_mont, root_bitrev(W, log_h, X));
    Ef inv_d[2];
    inv_denoms<2>(x, a.z_mont, inv_d);
    const Ef r = ef_add(ef_mul(g0, inv_d[0]), ef_mul(g1, inv_d[1]));
    *reinterpret_cast<uint4*>(ro + X) = make_uint4(r.c[0], r.c[1], r.c[2], r.c[3]);
}

void launch_reduce_class(Context& ctx, const ClassJob* d_jobs, uint32_t n_jobs, unsigned log_h,
                         const uint32_t* d_alpha_pows_mont, const ClassReduceArgs& args, Ef* ro) {
    TS_REQUIRE(n_jobs >= 1 && d_jobs && ro, TS_ERR_INVALID, "reduce_class: no matrices");
    TS_REQUIRE(log_h <= 27, TS_ERR_INVALID, "reduce_class: height above the two-adic subgroup");
    ctx.ensure_twiddles(log_h == 0 ? 1 : log_h);
    const uint64_t h = 1ull << log_h;
    TS_LAUNCH(ctx, k_reduce_class, dim3((unsigned)((h + 255) / 256)), dim3(256), 0, d_jobs, n_jobs, log_h,
              (const uint32_t*)ctx.d_twiddle_fwd, to_mont(GENERATOR), d_alpha_pows_mont, args, ro);
    TS_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ barycentric finish, any number of jobs
// k_bary_finish<N> (open.hip) with the jobs in device memory: workgroup b adds up four output words of job
// groups[b].x, the groups[b].y-th four of them.
__global__ void __launch_bounds__(256)
k_bary_finish_jobs(const BaryFinishJob* __restrict__ jobs, const uint2* __restrict__ groups) {
    const uint2 g = groups[blockIdx.x];
    const BaryFinishJob j = jobs[g.x];
    bary_finish_group(j.partial, j.out, j.n_blocks, j.n_words, g.y);
}

void launch_bary_finish_jobs(Context& ctx, const BaryFinishJob* d_jobs, const uint2* d_groups, uint32_t n_groups) {
    if (n_groups == 0) return;
    TS_REQUIRE(d_jobs && d_groups, TS_ERR_INVALID, "bary_finish_jobs: null table");
    TS_LAUNCH(ctx, k_bary_finish_jobs, dim3(n_groups), dim3(256), 0, d_jobs, d_groups);
    TS_HIP(hipGetLastError());
}

}  // namespace ts
