// LogUp columns of a challenge-phase (aux) trace, built in HBM from the still-resident main trace.
//
// Two challenges gamma, beta.  Interaction i on row r has the denominator d_i = gamma + sum_j beta^j v_ij(r) and
// the fraction m_i(r) / d_i.  Interactions are paired: group g holds 2g and 2g+1 (the last group one if K is
// odd).  The row-major aux matrix (n x 4 (G + 1), canonical) holds h_g(r), the group's sum, in columns
// 4g .. 4g+3 and phi(r) = sum_{r' < r} sum_g h_g(r') in the last four; S = phi(n-1) + sum_g h_g(n-1) is exposed.
//
// Three plain launches, no grid barrier, no flag another workgroup waits for (logup_aux_build_multi: the same three
// over the workgroups of SEVERAL tables, the specs in a job table in device memory -- the *_jobs kernels below):
//   k_logup_rows    one thread per row (LOGUP_RPT rows in turn): the fractions, with ONE base-field inversion
//                   per batch of LOGUP_BATCH denominators (ef_inv_parts + a running product, as open.hip); the
//                   row's sum goes into the phi slot, the workgroup's sum into totals[workgroup]
//   k_logup_totals  one workgroup: totals -> their exclusive prefix sums, in passes of LOGUP_SCAN_THREADS
//   k_logup_scan    the workgroup-local exclusive scan of the row sums plus the workgroup's offset -> phi; the
//                   thread of row n-1 writes S
// Extension addition is exact, so the association does not matter: the words are those of a serial sum.
// A zero denominator (its norm is zero) is reported through *flag = min(row * K + i); its batch runs on with the
// norm replaced by one, so nothing else is disturbed and the host discards the output.
#include <stdlib.h>
#include <string.h>

#include <string>

#include "logup_dev.hpp"

namespace ts {

constexpr int LOGUP_THREADS = 256;
constexpr int LOGUP_RPT = 4;              // rows per thread at most: a workgroup owns up to 1024 rows
constexpr int LOGUP_BATCH = 4;            // denominators per base-field inversion: two groups
constexpr int LOGUP_SCAN_THREADS = 128;   // totals per pass of k_logup_totals

struct LogupDev {
    uint32_t K, G, width, aux_width, table_width;
    Ef gamma_mont;                        // gamma R
    Ef beta_pow[LOGUP_MAX_VALUES];        // beta^j R^2: times a canonical value = (beta^j v) R
    LogupInteractionDev it[LOGUP_MAX_INTERACTIONS];
};

__device__ __forceinline__ Ef ef_shfl_up(Ef v, unsigned delta) {
    return Ef{{(uint32_t)__shfl_up((int)v.c[0], delta, 64), (uint32_t)__shfl_up((int)v.c[1], delta, 64),
               (uint32_t)__shfl_up((int)v.c[2], delta, 64), (uint32_t)__shfl_up((int)v.c[3], delta, 64)}};
}

// Inclusive scan over the workgroup's threads (NW waves of 64): wave-64 shuffles inside a wave, LDS across
// waves.  Returns the inclusive sum at this thread; `total` is the workgroup's sum.  Every thread calls it.
template <int NW>
__device__ __forceinline__ Ef block_scan_inclusive(Ef v, Ef (&wave_sums)[NW], Ef& total) {
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const Ef up = ef_shfl_up(v, d);
        if (lane >= d) v = ef_add(v, up);
    }
    __syncthreads();  // (a second call reuses wave_sums)
    if (lane == 63) wave_sums[wv] = v;
    __syncthreads();
    Ef before = ef_zero();
    total = ef_zero();
#pragma unroll
    for (int k = 0; k < NW; k++) {
        const Ef s = wave_sums[k];
        if (k < (int)wv) before = ef_add(before, s);
        total = ef_add(total, s);
    }
    return ef_add(v, before);
}

// sum_g h_g(r), with the h_g written to the row's first 4 G words
__device__ __forceinline__ Ef logup_row(const LogupDev& s, const uint32_t* __restrict__ row,
                                        const uint32_t* __restrict__ table_row, uint64_t r,
                                        uint32_t* __restrict__ aux_row, unsigned long long* __restrict__ flag,
                                        unsigned long long flag_base = 0) {
    Ef sum = ef_zero();
    for (uint32_t i0 = 0; i0 < s.K; i0 += LOGUP_BATCH) {
        Ef num[LOGUP_BATCH];
        uint32_t nrm[LOGUP_BATCH], pre[LOGUP_BATCH], mult[LOGUP_BATCH];
        uint32_t run = R_MOD_P;
#pragma unroll
        for (int j = 0; j < LOGUP_BATCH; j++) {
            const uint32_t i = i0 + j;
            num[j] = ef_zero();
            nrm[j] = R_MOD_P;
            mult[j] = 0;
            if (i < s.K) {
                Ef d = s.gamma_mont;
                const uint32_t nv = s.it[i].n_values;
#pragma unroll
                for (int q = 0; q < LOGUP_MAX_VALUES; q++)
                    if (q < (int)nv)
                        d = ef_add(d, ef_mul_base(s.beta_pow[q], mult_term(s.it[i].kind[q], s.it[i].val[q], row, table_row)));
                ef_inv_parts(d, num[j], nrm[j]);
                if (nrm[j] == 0) {  // d == 0: reported, and the batch goes on as if the norm were one
                    atomicMin(flag, flag_base + (unsigned long long)r * s.K + i);
                    nrm[j] = R_MOD_P;
                }
                mult[j] = mult_term(s.it[i].m_kind, s.it[i].m_val, row, table_row);
            }
            pre[j] = run;
            run = mont_mul(run, nrm[j]);
        }
        uint32_t inv = mont_inv(run);
        Ef frac[LOGUP_BATCH];
#pragma unroll
        for (int j = LOGUP_BATCH - 1; j >= 0; j--) {
            const uint32_t ninv = mont_mul(inv, pre[j]);
            inv = mont_mul(inv, nrm[j]);
            // (1/d) R times the canonical multiplicity: canonical m / d
            frac[j] = ef_mul_base(ef_mul_base(num[j], ninv), mult[j]);
        }
#pragma unroll
        for (int g = 0; g < LOGUP_BATCH / 2; g++) {
            if (i0 + 2 * g < s.K) {
                const Ef h = ef_add(frac[2 * g], frac[2 * g + 1]);
                *reinterpret_cast<Ef*>(aux_row + 4 * (i0 / 2 + g)) = h;
                sum = ef_add(sum, h);
            }
        }
    }
    return sum;
}

// workgroup `block` of one table: rows [block * block_rows, ...), its sum into totals[block]
template <bool TABLE>
__device__ __forceinline__ void logup_rows_block(const LogupDev& s, const uint32_t* __restrict__ trace,
                                                 const uint32_t* __restrict__ table, uint64_t n, uint32_t block_rows,
                                                 uint32_t rpt, uint32_t block, uint32_t* __restrict__ aux,
                                                 Ef* __restrict__ totals, unsigned long long* __restrict__ flag,
                                                 unsigned long long flag_base) {
    __shared__ Ef wave_sums[LOGUP_THREADS / 64];
    const uint64_t base = (uint64_t)block * block_rows;
    Ef mine = ef_zero();
    for (uint32_t k = 0; k < rpt; k++) {
        const uint32_t local = threadIdx.x * rpt + k;
        const uint64_t r = base + local;
        if (local < block_rows && r < n) {
            uint32_t* aux_row = aux + r * s.aux_width;
            const uint32_t* row = trace + r * s.width;
            const Ef sum = logup_row(s, row, TABLE ? table + r * s.table_width : row, r, aux_row, flag, flag_base);
            *reinterpret_cast<Ef*>(aux_row + 4 * s.G) = sum;  // the phi slot, until k_logup_scan
            mine = ef_add(mine, sum);
        }
    }
    Ef total;
    block_scan_inclusive<LOGUP_THREADS / 64>(mine, wave_sums, total);
    if (threadIdx.x == 0) totals[block] = total;
}

// TABLE = false is the kernel as it was before table terms (the table row is the trace's row again and folds
// away); TABLE = true reads a second row-major matrix
template <bool TABLE>
__global__ void __launch_bounds__(LOGUP_THREADS)
k_logup_rows(const LogupDev s, const uint32_t* __restrict__ trace, const uint32_t* __restrict__ table, uint64_t n,
             uint32_t block_rows, uint32_t rpt,
             uint32_t* __restrict__ aux, Ef* __restrict__ totals, unsigned long long* __restrict__ flag) {
    logup_rows_block<TABLE>(s, trace, table, n, block_rows, rpt, blockIdx.x, aux, totals, flag, 0);
}

// totals[b] <- sum_{b' < b} totals[b'], b < n_blocks
__device__ __forceinline__ void logup_totals_scan(Ef* __restrict__ totals, uint32_t n_blocks) {
    __shared__ Ef wave_sums[LOGUP_SCAN_THREADS / 64];
    Ef carry = ef_zero();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += LOGUP_SCAN_THREADS) {  // (uniform bounds: every thread loops alike)
        const uint32_t b = b0 + threadIdx.x;
        const Ef v = b < n_blocks ? totals[b] : ef_zero();
        Ef pass;
        const Ef incl = block_scan_inclusive<LOGUP_SCAN_THREADS / 64>(v, wave_sums, pass);
        if (b < n_blocks) totals[b] = ef_add(carry, ef_sub(incl, v));
        carry = ef_add(carry, pass);
    }
}

__global__ void __launch_bounds__(LOGUP_SCAN_THREADS)
k_logup_totals(Ef* __restrict__ totals, uint32_t n_blocks) {
    logup_totals_scan(totals, n_blocks);
}

// workgroup `block` of one table: the row sums in the phi slots -> phi, from offsets[block] on
__device__ __forceinline__ void logup_scan_block(uint32_t aux_width, uint32_t G, uint64_t n, uint32_t block_rows,
                                                 uint32_t rpt, uint32_t block, uint32_t* __restrict__ aux,
                                                 const Ef* __restrict__ offsets, Ef* __restrict__ S) {
    __shared__ Ef wave_sums[LOGUP_THREADS / 64];
    const uint64_t base = (uint64_t)block * block_rows;
    Ef sums[LOGUP_RPT];
    Ef mine = ef_zero();
#pragma unroll
    for (int k = 0; k < LOGUP_RPT; k++) {
        const uint32_t local = threadIdx.x * rpt + k;
        const uint64_t r = base + local;
        sums[k] = ef_zero();
        if (k < (int)rpt && local < block_rows && r < n)
            sums[k] = *reinterpret_cast<const Ef*>(aux + r * aux_width + 4 * G);
        mine = ef_add(mine, sums[k]);
    }
    Ef total;
    const Ef incl = block_scan_inclusive<LOGUP_THREADS / 64>(mine, wave_sums, total);
    Ef run = ef_add(offsets[block], ef_sub(incl, mine));
#pragma unroll
    for (int k = 0; k < LOGUP_RPT; k++) {
        const uint32_t local = threadIdx.x * rpt + k;
        const uint64_t r = base + local;
        if (k < (int)rpt && local < block_rows && r < n) {
            *reinterpret_cast<Ef*>(aux + r * aux_width + 4 * G) = run;
            run = ef_add(run, sums[k]);
            if (r == n - 1) *S = run;
        }
    }
}

__global__ void __launch_bounds__(LOGUP_THREADS)
k_logup_scan(uint32_t aux_width, uint32_t G, uint64_t n, uint32_t block_rows, uint32_t rpt,
             uint32_t* __restrict__ aux, const Ef* __restrict__ offsets, Ef* __restrict__ S) {
    logup_scan_block(aux_width, G, n, block_rows, rpt, blockIdx.x, aux, offsets, S);
}

// ---- every table of a multi-table proof in the same three launches (logup_aux_build_multi).  The specs live in a
// job table in device memory instead of the launch argument (logup_dev.hpp: job_of_block, the typed pointers).
struct LogupJob {
    LogupDev s;
    GlobalConstWords trace;
    GlobalWords aux;
    uint64_t n;
    uint32_t first_block, n_blocks;  // its workgroups in the rows and scan launches = its stretch of `totals`
    uint32_t index;                  // the table's number: the high word of a zero-denominator report, its S slot
    uint32_t pad;
    GlobalConstWords table;     // the row-major values of its preprocessed columns (kind-2 terms), or null
    uint64_t pad2;
};

// TABLES = false is the kernel of logup_aux_build_multi, unchanged.  TABLES = true is launched only when some job
// has a table (logup_aux_build_multi_pre): a job with one runs logup_rows_block<true>, a job without keeps the
// <false> body; the choice depends on the job alone, so it is the same in every lane of the workgroup.  A second
// instantiation rather than one kernel with the branch: with the branch the kernel takes the 66 VGPRs and occupancy
// 7 of the table body (k_logup_rows<true> has the same), and every bus proof without a key would run at them
// instead of 64 and 8 (profiles/multi_key_kernel_resources.txt).  Neither form uses scratch.
template <bool TABLES>
__global__ void __launch_bounds__(LOGUP_THREADS)
k_logup_rows_jobs(const LogupJob* __restrict__ jobs, const uint32_t* __restrict__ first, uint32_t n_jobs,
                  uint32_t block_rows, uint32_t rpt, Ef* __restrict__ totals, unsigned long long* __restrict__ flag) {
    const LogupJob& j = jobs[job_of_block(first, n_jobs)];
    if (TABLES && j.table)
        logup_rows_block<true>(j.s, (const uint32_t*)j.trace, (const uint32_t*)j.table, j.n, block_rows, rpt,
                               blockIdx.x - j.first_block, (uint32_t*)j.aux, totals + j.first_block, flag,
                               (unsigned long long)j.index << 32);
    else
        logup_rows_block<false>(j.s, (const uint32_t*)j.trace, nullptr, j.n, block_rows, rpt, blockIdx.x - j.first_block, (uint32_t*)j.aux,
                                totals + j.first_block, flag, (unsigned long long)j.index << 32);
}

// one workgroup per table: the scan never crosses into another table's totals
__global__ void __launch_bounds__(LOGUP_SCAN_THREADS)
k_logup_totals_jobs(const LogupJob* __restrict__ jobs, Ef* __restrict__ totals) {
    const LogupJob& j = jobs[blockIdx.x];
    logup_totals_scan(totals + j.first_block, j.n_blocks);
}

__global__ void __launch_bounds__(LOGUP_THREADS)
k_logup_scan_jobs(const LogupJob* __restrict__ jobs, const uint32_t* __restrict__ first, uint32_t n_jobs,
                  uint32_t block_rows, uint32_t rpt, const Ef* __restrict__ totals, Ef* __restrict__ S) {
    const LogupJob& j = jobs[job_of_block(first, n_jobs)];
    logup_scan_block(j.s.aux_width, j.s.G, j.n, block_rows, rpt, blockIdx.x - j.first_block, (uint32_t*)j.aux,
                     totals + j.first_block, S + j.index);
}

uint32_t logup_aux_width(const LogupSpec& spec, uint32_t max_kind) {
    const size_t K = spec.interactions.size();
    TS_REQUIRE(K >= 1 && K <= LOGUP_MAX_INTERACTIONS, TS_ERR_INVALID,
               "logup: between 1 and 16 interactions");
    for (const LogupInteraction& it : spec.interactions) {
        TS_REQUIRE(it.values.size() >= 1 && it.values.size() <= LOGUP_MAX_VALUES, TS_ERR_INVALID,
                   "logup: between 1 and 8 values per interaction");
        const char* kinds = max_kind >= 2 ? "logup: term kind must be 0 (constant), 1 (column) or 2 (preprocessed column)"
                                          : "logup: term kind must be 0 (constant) or 1 (column)";
        TS_REQUIRE(it.multiplicity.kind <= max_kind, TS_ERR_INVALID, kinds);
        for (const LogupTerm& t : it.values) TS_REQUIRE(t.kind <= max_kind, TS_ERR_INVALID, kinds);
    }
    return 4 * ((uint32_t)(K + 1) / 2 + 1);
}

static uint32_t logup_block_rows() {
    uint32_t rows = LOGUP_THREADS * LOGUP_RPT;
    if (const char* e = getenv("TS_LOGUP_BLOCK_ROWS"); e && *e) {
        const long v = atol(e);
        TS_REQUIRE(v >= 1 && v <= LOGUP_THREADS * LOGUP_RPT, TS_ERR_INVALID,
                   "TS_LOGUP_BLOCK_ROWS must be in [1, 1024]");
        rows = (uint32_t)v;
    }
    return rows;
}

// The device form of `spec` over `trace` (and `table`) for challenges = gamma ++ beta; every refusal of the builder
// about the spec, the matrices and the challenges is made here, before anything is allocated.
static LogupDev logup_dev(Context& ctx, const LogupSpec& spec, const DeviceMatrix& trace, const uint32_t challenges[8],
                          const DeviceMatrix* table, bool takes_table) {
    LogupDev s;
    memset(&s, 0, sizeof s);
    const uint32_t max_kind = takes_table ? 2 : 1;
    s.aux_width = logup_aux_width(spec, max_kind);
    s.K = (uint32_t)spec.interactions.size();
    s.G = (s.K + 1) / 2;
    require_resident(ctx, trace, "logup", "the trace");
    s.width = trace.width;
    if (table) {
        require_resident(ctx, *table, "logup", "the preprocessed table");
        TS_REQUIRE(table->height == trace.height, TS_ERR_INVALID, "logup: the preprocessed table must have the trace's height");
        s.table_width = table->width;
    }
    for (const LogupInteraction& it : spec.interactions) {
        require_term("logup", it.multiplicity, max_kind, trace.width, table);
        for (const LogupTerm& tm : it.values) require_term("logup", tm, max_kind, trace.width, table);
    }
    load_interactions(spec, s.it);
    for (int k = 0; k < 8; k++) TS_REQUIRE(challenges[k] < P, TS_ERR_INVALID, "logup: non-canonical challenge");
    const Ef gamma = ef_to_mont(Ef{{challenges[0], challenges[1], challenges[2], challenges[3]}});
    const Ef beta = ef_to_mont(Ef{{challenges[4], challenges[5], challenges[6], challenges[7]}});
    s.gamma_mont = gamma;
    Ef bp = ef_one_mont();
    for (uint32_t q = 0; q < LOGUP_MAX_VALUES; q++) {
        s.beta_pow[q] = ef_to_mont(bp);
        bp = ef_mul(bp, beta);
    }
    return s;
}

void logup_check_spec(Context& ctx, const LogupSpec& spec, const DeviceMatrix& trace, const DeviceMatrix* table) {
    const uint32_t no_challenges[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)logup_dev(ctx, spec, trace, no_challenges, table, /*takes_table=*/true);
}

DeviceMatrix logup_aux_build(Context& ctx, const LogupSpec& spec, const DeviceMatrix& trace,
                             const uint32_t challenges[8], uint32_t exposed[4], const DeviceMatrix* table,
                             bool takes_table) {
    StageTimer t(&ctx, "logup aux build");
    const LogupDev s = logup_dev(ctx, spec, trace, challenges, table, takes_table);

    const uint64_t n = trace.height;
    const uint32_t block_rows = logup_block_rows();
    const uint32_t rpt = (block_rows + LOGUP_THREADS - 1) / LOGUP_THREADS;
    const uint64_t n_blocks = (n + block_rows - 1) / block_rows;
    TS_REQUIRE(n_blocks <= (1u << 27), TS_ERR_INVALID, "logup: too many workgroups");
    DeviceMatrix aux;
    aux.buf = DevBuf<uint32_t>(&ctx, n * s.aux_width);
    aux.height = n;
    aux.width = s.aux_width;
    aux.layout = DeviceMatrix::ROW_MAJOR;
    DevBuf<Ef> totals(&ctx, n_blocks);
    // {flag (two words), pad, pad, S}: one copy back
    DevBuf<Ef> back(&ctx, 2);
    TS_HIP(hipMemsetAsync(back.p, 0xff, 2 * sizeof(Ef), ctx.stream));
    unsigned long long* flag = reinterpret_cast<unsigned long long*>(back.p);
    // (no spec with a kind-2 term gets here without a table: `term` above)
    if (table)
        TS_LAUNCH_NAMED(ctx, "k_logup_rows_pre", k_logup_rows<true>, dim3((unsigned)n_blocks), dim3(LOGUP_THREADS), 0, s, trace.buf.p,
                  (const uint32_t*)table->buf.p, n, block_rows, rpt, aux.buf.p, totals.p, flag);
    else
        TS_LAUNCH_NAMED(ctx, "k_logup_rows", k_logup_rows<false>, dim3((unsigned)n_blocks), dim3(LOGUP_THREADS), 0, s, trace.buf.p,
                  (const uint32_t*)nullptr, n, block_rows, rpt, aux.buf.p, totals.p, flag);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_logup_totals, dim3(1), dim3(LOGUP_SCAN_THREADS), 0, totals.p, (uint32_t)n_blocks);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_logup_scan, dim3((unsigned)n_blocks), dim3(LOGUP_THREADS), 0, s.aux_width, s.G, n, block_rows, rpt,
              aux.buf.p, totals.p, back.p + 1);
    TS_HIP(hipGetLastError());
    uint32_t host[8];
    d2h_sync(ctx, host, back.p, sizeof host);
    const unsigned long long f = (unsigned long long)host[0] | ((unsigned long long)host[1] << 32);
    if (f != ~0ull)
        throw Error(TS_ERR_INVARIANT, "logup: zero denominator at row " + std::to_string(f / s.K) + ", interaction " +
                                          std::to_string(f % s.K));
    memcpy(exposed, host + 4, 16);
    return aux;
}

// n logup_aux_build calls with one set of challenges in three launches, one upload and one copy back.
std::vector<DeviceMatrix> logup_aux_build_multi(Context& ctx, const std::vector<const LogupSpec*>& specs,
                                                const std::vector<const DeviceMatrix*>& traces,
                                                const uint32_t challenges[8], uint32_t* exposed,
                                                const uint32_t* table_ids,
                                                const std::vector<const DeviceMatrix*>* tables) {
    StageTimer t(&ctx, "logup aux build");
    const size_t T = specs.size();
    TS_REQUIRE(T >= 1 && T <= LOGUP_MAX_TABLES && traces.size() == T && (!tables || tables->size() == T), TS_ERR_INVALID,
               "logup: between 1 and 64 tables, one trace per spec");
    bool any_table = false;
    const uint32_t block_rows = logup_block_rows();
    const uint32_t rpt = (block_rows + LOGUP_THREADS - 1) / LOGUP_THREADS;
    // every refusal first: nothing is allocated before the last table passed
    std::vector<LogupJob> jobs(T);
    std::vector<uint32_t> first(T + 1, 0);
    uint64_t n_blocks = 0;
    for (size_t k = 0; k < T; k++) {
        TS_REQUIRE(specs[k] && traces[k], TS_ERR_INVALID, "logup: null spec or trace");
        LogupJob& j = jobs[k];
        memset((void*)&j, 0, sizeof j);
        const DeviceMatrix* table = tables ? (*tables)[k] : nullptr;
        j.s = logup_dev(ctx, *specs[k], *traces[k], challenges, table, /*takes_table=*/tables != nullptr);
        j.table = table ? (GlobalConstWords)table->buf.p : nullptr;
        any_table = any_table || table;
        j.n = traces[k]->height;
        j.trace = (GlobalConstWords)traces[k]->buf.p;
        j.index = (uint32_t)k;
        j.first_block = first[k] = (uint32_t)n_blocks;
        j.n_blocks = (uint32_t)((j.n + block_rows - 1) / block_rows);
        n_blocks += j.n_blocks;
        TS_REQUIRE(n_blocks <= (1u << 30), TS_ERR_INVALID, "logup: too many workgroups");
    }
    first[T] = (uint32_t)n_blocks;
    std::vector<DeviceMatrix> aux(T);
    for (size_t k = 0; k < T; k++) {
        aux[k].buf = DevBuf<uint32_t>(&ctx, jobs[k].n * jobs[k].s.aux_width);
        aux[k].height = jobs[k].n;
        aux[k].width = jobs[k].s.aux_width;
        aux[k].layout = DeviceMatrix::ROW_MAJOR;
        jobs[k].aux = (GlobalWords)aux[k].buf.p;
    }
    const JobTable<LogupJob> d_tab = upload_jobs(ctx, jobs, first);
    const LogupJob* d_jobs = d_tab.jobs;
    const uint32_t* d_first = d_tab.first;
    DevBuf<Ef> totals(&ctx, n_blocks);
    // {flag (two words), pad, pad, S_0 .. S_{T-1}}: one copy back
    DevBuf<Ef> back(&ctx, 1 + T);
    TS_HIP(hipMemsetAsync(back.p, 0xff, (1 + T) * sizeof(Ef), ctx.stream));
    unsigned long long* flag = reinterpret_cast<unsigned long long*>(back.p);
    if (any_table)
        TS_LAUNCH_NAMED(ctx, "k_logup_rows_jobs_pre", k_logup_rows_jobs<true>, dim3((unsigned)n_blocks), dim3(LOGUP_THREADS), 0,
                        d_jobs, d_first, (uint32_t)T, block_rows, rpt, totals.p, flag);
    else
        TS_LAUNCH_NAMED(ctx, "k_logup_rows_jobs", k_logup_rows_jobs<false>, dim3((unsigned)n_blocks), dim3(LOGUP_THREADS), 0,
                        d_jobs, d_first, (uint32_t)T, block_rows, rpt, totals.p, flag);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_logup_totals_jobs, dim3((unsigned)T), dim3(LOGUP_SCAN_THREADS), 0, d_jobs, totals.p);
    TS_HIP(hipGetLastError());
    TS_LAUNCH(ctx, k_logup_scan_jobs, dim3((unsigned)n_blocks), dim3(LOGUP_THREADS), 0, d_jobs, d_first, (uint32_t)T,
              block_rows, rpt, (const Ef*)totals.p, back.p + 1);
    TS_HIP(hipGetLastError());
    std::vector<uint32_t> host(4 * (1 + T));
    d2h_sync(ctx, host.data(), back.p, host.size() * 4);
    if (host[0] != ~0u || host[1] != ~0u) {  // the least (table, row * K + interaction)
        const uint32_t k = host[1], K = jobs[k < T ? k : 0].s.K;
        throw Error(TS_ERR_INVARIANT, "logup: zero denominator at table " + std::to_string(table_ids && k < T ? table_ids[k] : k) + ", row " +
                                          std::to_string(host[0] / K) + ", interaction " + std::to_string(host[0] % K));
    }
    memcpy(exposed, host.data() + 4, 16 * T);
    return aux;
}

}  // namespace ts
