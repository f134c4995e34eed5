// smart_particle.hip -- one assimilation step of a bootstrap particle filter (Gordon et al. 1993; systematic resampling:
// Kitagawa 1996; the jitter of the parameters: Liu & West 2001 without the shrinkage) AROUND the ensemble launch that ran
// the particles over a window of report steps.  The definition -- the order of the operations, the integers, the draw
// layout -- is in include/smart_amd.h (smart_particle_step_hip) and DESIGN.md section 4.24; this file says it once more in
// HIP.
//
// Four small kernels, stream-ordered, nothing read back, no kernel waits on another workgroup:
//   smart_particle_weigh      one lane per particle: the window's log-likelihood from the matrix where the launch left it,
//                             logw' into logw_out, the maximum of the finite logw' and of the finite logw per block
//   smart_particle_quantise   every block reduces the block maxima to m' and m, then q_i = rint(2^22 exp(logw'_i - m')), the
//                             block's inclusive prefix sums of q (32 bits hold them) and its sums of q, q^2 and of the
//                             prior's integers
//   smart_particle_header     one workgroup: the exclusive scan of the block sums, Q, S2, the effective sample size, the
//                             decision, the offset of the comb, the evidence and the flags -- the small header the last kernel
//                             reads through wave-uniform loads
//   smart_particle_resample   one lane per child: the parent by a two-level binary search (block offsets in LDS, then the
//                             block's 256 prefix sums), the gather of its row and states, the draws and the writes
// FROM THE QUANTISATION ON EVERYTHING IS INTEGERS: no summation order can matter, and the same call gives the same bits on
// every launch.  The one atomic is an integer counter (the distinct parents: a count per block, one add).
// RANDOMNESS.  Philox4x32-10, counter (child, step, slot, 0), key (seed lo, seed hi); the comb's offset has the counter
// (2^32 - 1, step, 0, 0), a child number that no particle has.
// ARITHMETIC.  The unit is compiled with -ffp-contract=off: every operation of the weights and of the move is rounded once, as
// the numpy statement of the tests rounds it.  The operations that are not correctly rounded by definition: exp (its last bit
// moves 2^22 e by far less than 1) and the two logarithms of the evidence.
#include "smart_capi_internal.h"
#include "smart_de_move.h"
#include "smart_order_stats.h"
#include <cstdint>

namespace smart {

constexpr int kPfThreads = 256;                 // particles of a block: the unit of the two-level search
constexpr int kPfWaves = kPfThreads / kWave;
constexpr int kPfMaxBlocks = SMART_PARTICLE_MAX_PARTICLES / kPfThreads;      // 2048
constexpr int kPfPerThread = kPfMaxBlocks / kPfThreads;                      // block values a thread of one workgroup holds
constexpr double kPfUnit = 4194304.0;           // 2^22: the integer a particle of the largest weight gets
static_assert(kPfMaxBlocks == 2048 && kPfPerThread == 8, "11 + 8 probes, one workgroup scans the block sums");

// the workspace (particle_workspace_bytes): five arrays of one value per block, then the local prefix sums
struct PfWorkspace {
    double *max_post, *max_prior;               // [2048] the largest finite logw' / logw of a block (-inf: none)
    unsigned long long *sum_q, *sum_q2, *sum_prior, *offset;        // [2048]; offset: the exclusive scan of sum_q
    unsigned *local;                            // [N rounded up to blocks] the inclusive prefix sums of q inside a block
};

static PfWorkspace pf_workspace(void *workspace)
{
    char *p = (char *)workspace;
    PfWorkspace w;
    w.max_post = (double *)p, w.max_prior = w.max_post + kPfMaxBlocks;
    w.sum_q = (unsigned long long *)(w.max_prior + kPfMaxBlocks);
    w.sum_q2 = w.sum_q + kPfMaxBlocks, w.sum_prior = w.sum_q2 + kPfMaxBlocks, w.offset = w.sum_prior + kPfMaxBlocks;
    w.local = (unsigned *)(w.offset + kPfMaxBlocks);
    return w;
}

long particle_workspace_bytes(long N)
{
    const long blocks = (N + kPfThreads - 1) / kPfThreads;
    return 6l * kPfMaxBlocks * 8 + blocks * kPfThreads * 4;
}

__device__ inline bool pf_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }      // (a NaN: false)

// the largest of a block's values, the same bits in every thread (a maximum has no order); sh: kPfThreads doubles
__device__ inline double pf_block_max(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = kPfThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double a = sh[threadIdx.x], b = sh[threadIdx.x + s];
            sh[threadIdx.x] = a > b ? a : b;
        }
        __syncthreads();
    }
    const double m = sh[0];
    __syncthreads();
    return m;
}

// the sum of a block's integers, the same in every thread; sh: kPfThreads words
__device__ inline unsigned long long pf_block_sum(unsigned long long v, unsigned long long *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = kPfThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const unsigned long long t = sh[0];
    __syncthreads();
    return t;
}

// ---- weigh ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPfThreads) void smart_particle_weigh(long N, long Rw, const double *__restrict__ sim, long ld,
                                                                   const double *__restrict__ obs, double sigma0,
                                                                   double sigma1, const double *__restrict__ logw_in,
                                                                   double *__restrict__ logw_out, PfWorkspace w)
{
    __shared__ double sh[kPfThreads];
    const long i = (long)blockIdx.x * kPfThreads + threadIdx.x;
    const bool live = i < N;
    const double *col = sim + (live ? i : N - 1);
    double s = 0.0;
    bool bad = false;
    for (long t = 0; t < Rw; ++t) {
        const double o = obs[t];                // wave-uniform, and so are sigma_t and the branch
        if (o != o)
            continue;
        const double sigma = sigma0 + sigma1 * __builtin_fabs(o);
        const double x = col[t * ld];           // a wavefront reads 512 contiguous bytes of the row
        bad |= !pf_finite(x);
        const double r = (x - o) / sigma;
        s = s + r * r;
    }
    const double prior = live ? logw_in[i] : -__builtin_inf();
    const double l = -0.5 * s;
    const double post = bad ? -__builtin_inf() : prior + l;
    if (live)
        logw_out[i] = post;
    const double m1 = pf_block_max(live && pf_finite(post) ? post : -__builtin_inf(), sh);
    const double m0 = pf_block_max(pf_finite(prior) ? prior : -__builtin_inf(), sh);
    if (threadIdx.x == 0) {
        w.max_post[blockIdx.x] = m1;
        w.max_prior[blockIdx.x] = m0;
    }
}

// ---- quantise ---------------------------------------------------------------------------------------------------------
// the integer of a log-weight under the maximum m of the finite ones: rint(2^22 exp(logw - m)), 0 where it is not finite
__device__ inline unsigned long long pf_quantum(double logw, double m)
{
    if (!pf_finite(logw))
        return 0ull;
    const double d = logw - m;
    const double e = exp(d);
    return (unsigned long long)rint(kPfUnit * e);
}

__global__ __launch_bounds__(kPfThreads) void smart_particle_quantise(long N, int blocks, const double *__restrict__ logw_post,
                                                                      const double *__restrict__ logw_prior,
                                                                      const long long *__restrict__ q_in,
                                                                      long long *__restrict__ q, PfWorkspace w)
{
    __shared__ double sh[kPfThreads];
    __shared__ unsigned long long shu[kPfThreads];
    __shared__ double wave_l[kPfWaves];
    const long i = (long)blockIdx.x * kPfThreads + threadIdx.x;
    const bool live = i < N;
    unsigned long long mine = 0ull, prior = 0ull;
    if (q_in) {
        mine = live ? (unsigned long long)q_in[i] : 0ull;
    } else {
        double m1 = -__builtin_inf(), m0 = -__builtin_inf();
        for (int b = threadIdx.x; b < blocks; b += kPfThreads) {
            const double a1 = w.max_post[b], a0 = w.max_prior[b];
            m1 = a1 > m1 ? a1 : m1;
            m0 = a0 > m0 ? a0 : m0;
        }
        m1 = pf_block_max(m1, sh);
        m0 = pf_block_max(m0, sh);
        // no finite logw' at all (DEGENERATE): the particles are kept with equal weights
        if (live)
            mine = pf_finite(m1) ? pf_quantum(logw_post[i], m1) : (unsigned long long)kPfUnit;
        if (live && pf_finite(m0))
            prior = pf_quantum(logw_prior[i], m0);
    }
    // the block's inclusive prefix sums: block_scan on doubles, which hold these integers exactly (at most 256 2^22 = 2^30)
    double a[1] = {(double)mine};
    block_scan<1, kPfWaves>(a, wave_l);
    w.local[i] = (unsigned)a[0];
    if (live)
        q[i] = (long long)mine;
    const unsigned long long sq = pf_block_sum(mine, shu), sq2 = pf_block_sum(mine * mine, shu);
    const unsigned long long sp = pf_block_sum(prior, shu);
    if (threadIdx.x == 0) {
        w.sum_q[blockIdx.x] = sq;
        w.sum_q2[blockIdx.x] = sq2;
        w.sum_prior[blockIdx.x] = sp;
    }
}

// ---- header -----------------------------------------------------------------------------------------------------------
struct PfHeader {
    long N;
    int blocks;
    long Rw;
    const double *obs;          // NULL: a call with q_in (no window was weighed)
    int given;                  // q_in was given: no maxima, no evidence
    double tau;
    long long offset;           // < 0: drawn
    unsigned step, k0, k1;
    PfWorkspace w;
    double *stats;
    long long *counts;
};

__global__ __launch_bounds__(kPfThreads) void smart_particle_header(PfHeader h)
{
    __shared__ double sh[kPfThreads];
    __shared__ unsigned long long shu[kPfThreads];
    __shared__ double wave_l[kPfWaves];
    const int first = threadIdx.x * kPfPerThread;
    // the exclusive scan of the block sums: block_scan on doubles, exact (Q <= 2^41)
    double a[kPfPerThread];
    unsigned long long own[kPfPerThread], s2 = 0ull, prior = 0ull;
    double m1 = -__builtin_inf(), m0 = -__builtin_inf();
#pragma unroll
    for (int e = 0; e < kPfPerThread; ++e) {
        const int b = first + e;
        const bool in = b < h.blocks;
        own[e] = in ? h.w.sum_q[b] : 0ull;
        a[e] = (double)own[e];
        s2 += in ? h.w.sum_q2[b] : 0ull;
        prior += in ? h.w.sum_prior[b] : 0ull;
        if (in && !h.given) {
            const double a1 = h.w.max_post[b], a0 = h.w.max_prior[b];
            m1 = a1 > m1 ? a1 : m1;
            m0 = a0 > m0 ? a0 : m0;
        }
    }
    block_scan<kPfPerThread, kPfWaves>(a, wave_l);
#pragma unroll
    for (int e = 0; e < kPfPerThread; ++e)
        if (first + e < h.blocks)
            h.w.offset[first + e] = (unsigned long long)a[e] - own[e];
    const unsigned long long Q = pf_block_sum(own[0] + own[1] + own[2] + own[3] + own[4] + own[5] + own[6] + own[7], shu);
    const unsigned long long S2 = pf_block_sum(s2, shu), Q0 = pf_block_sum(prior, shu);
    m1 = pf_block_max(m1, sh);
    m0 = pf_block_max(m0, sh);
    int seen = 0;
    if (h.obs)
        for (long t = threadIdx.x; t < h.Rw; t += kPfThreads)
            seen |= h.obs[t] == h.obs[t];
    seen = __syncthreads_or(seen);
    if (threadIdx.x != 0)
        return;
    long long flags = 0;
    if (h.obs && !seen)
        flags |= SMART_PARTICLE_FLAG_NO_OBS;
    if (h.given ? Q == 0ull : !pf_finite(m1))
        flags |= SMART_PARTICLE_FLAG_DEGENERATE;
    const double Qd = (double)Q;
    double ess = Qd * Qd;
    ess = ess / (double)S2;
    const double threshold = h.tau * (double)h.N;
    const bool resample = flags == 0 && ess < threshold;
    unsigned long long rho = 0ull;
    if (resample) {
        if (h.offset >= 0) {
            rho = (unsigned long long)h.offset;
        } else {
            const Philox4 r = philox4x32_10(0xFFFFFFFFu, h.step, 0u, 0u, h.k0, h.k1);
            const double at = u53(r.w[0], r.w[1]) * Qd;
            rho = (unsigned long long)at;       // (the floor: at >= 0)
        }
        rho = rho < Q - 1 ? rho : Q - 1;
    }
    double evidence = __builtin_nan("");
    if (!h.given) {
        const double after = m1 + log((double)Q / kPfUnit), before = m0 + log((double)Q0 / kPfUnit);
        evidence = after - before;
    }
    h.stats[SMART_PARTICLE_ESS] = ess;
    h.stats[SMART_PARTICLE_EVIDENCE] = evidence;
    h.stats[SMART_PARTICLE_MAX] = h.given ? __builtin_nan("") : m1;
    h.stats[SMART_PARTICLE_MAX_PRIOR] = h.given ? __builtin_nan("") : m0;
    h.counts[SMART_PARTICLE_RESAMPLED] = resample ? 1 : 0;
    h.counts[SMART_PARTICLE_Q] = (long long)Q;
    h.counts[SMART_PARTICLE_DISTINCT] = 0;
    h.counts[SMART_PARTICLE_FLAGS] = flags;
    h.counts[SMART_PARTICLE_OFFSET] = (long long)rho;
    h.counts[SMART_PARTICLE_S2] = (long long)S2;
    h.counts[SMART_PARTICLE_Q_PRIOR] = (long long)Q0;
    h.counts[7] = 0;
}

// ---- resample + move --------------------------------------------------------------------------------------------------
struct PfMove {
    long N;
    int blocks, d;
    DeKey key;                  // gen: the step
    DeBox box;
    unsigned jitter;            // the dimensions whose scale is not 0: the others are copied
    int z_dim;                  // the dimension that is Z, or -1: Z does not vary and is read from the parent's row
    int z_column;
    double area;
    double noise[SMART_PARTICLE_STATES];
    const double *rows_in;
    double *rows_out;
    long ld;
    const double *states_in;
    double *states_out;
    const double *logw_post;    // logw' (logw_out after the weigh kernel, or logw_in in a call with q_in)
    double *logw_out;
    int *parents;
    PfWorkspace w;
    const long long *counts;    // the header
    long long *distinct;        // &counts[SMART_PARTICLE_DISTINCT]
};

// a_j = #{i : N C_i <= t}, t = j Q + rho < N Q: the blocks that end at or below t (11 probes in LDS), then the particles of
// the next block that do (8 probes over its prefix sums)
__device__ inline long pf_parent(const PfMove &p, const unsigned long long *ends, unsigned long long t)
{
    const unsigned long long n = (unsigned long long)p.N;
    int lo = 0, hi = p.blocks;                  // the count lies in [lo, hi); ends[blocks - 1] = Q and N Q > t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (n * ends[mid] <= t)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int b = lo < p.blocks - 1 ? lo : p.blocks - 1;
    const unsigned long long before = p.w.offset[b];
    const unsigned *local = p.w.local + (long)b * kPfThreads;
    const long left = p.N - (long)b * kPfThreads;
    int l0 = 0, l1 = left < kPfThreads ? (int)left : kPfThreads;
    while (l0 < l1) {
        const int mid = (l0 + l1) >> 1;
        if (n * (before + local[mid]) <= t)
            l0 = mid + 1;
        else
            l1 = mid;
    }
    const long a = (long)b * kPfThreads + l0;
    return a < p.N - 1 ? a : p.N - 1;
}

template <bool RESAMPLE, bool MOVE>
__global__ __launch_bounds__(kPfThreads) void smart_particle_resample(PfMove p)
{
    __shared__ unsigned long long ends[kPfMaxBlocks];
    const long j = (long)blockIdx.x * kPfThreads + threadIdx.x;
    const bool live = j < p.N;
    const bool resampled = p.counts[SMART_PARTICLE_RESAMPLED] != 0;           // wave-uniform loads of the header
    const bool degenerate = (p.counts[SMART_PARTICLE_FLAGS] & SMART_PARTICLE_FLAG_DEGENERATE) != 0;
    long parent = live ? j : p.N - 1;
    if constexpr (RESAMPLE) {
        int firsts;
        if (resampled) {
            const unsigned long long Q = (unsigned long long)p.counts[SMART_PARTICLE_Q];
            const unsigned long long rho = (unsigned long long)p.counts[SMART_PARTICLE_OFFSET];
            for (int b = threadIdx.x; b < p.blocks; b += kPfThreads)
                ends[b] = p.w.offset[b] + p.w.sum_q[b];
            __syncthreads();
            parent = pf_parent(p, ends, (unsigned long long)(live ? j : p.N - 1) * Q + rho);
            // a child is the first of its parent where the child before it has another one (a_j does not decrease)
            long before = -1;
            if (threadIdx.x == 0 && j > 0)
                before = pf_parent(p, ends, (unsigned long long)(j - 1) * Q + rho);
            __syncthreads();                    // (ends is read no more: its first words carry the parents now)
            long *seen = (long *)ends;
            seen[threadIdx.x + 1] = parent;
            if (threadIdx.x == 0)
                seen[0] = before;
            __syncthreads();
            firsts = __syncthreads_count(live && seen[threadIdx.x] != parent);
        } else {
            firsts = __syncthreads_count(live);
        }
        if (threadIdx.x == 0)
            atomicAdd((unsigned long long *)p.distinct, (unsigned long long)firsts);
        if (live)
            p.parents[j] = (int)parent;
    } else {
        if (live) {             // (held inside the ensemble whatever the caller left there)
            const long given = p.parents[j];
            parent = given < 0 ? 0 : (given < p.N ? given : p.N - 1);
        }
    }
    if constexpr (MOVE) {
        if (!live)
            return;
        // ---- the parameters: the jitter and the box of smart_de_move.h, a move of weight 0 from the parent's own row
        const double *from = p.rows_in + parent * p.ld;
        double base[kDeMaxDims], y[kDeMaxDims];
        for (int c = 0; c < p.d; ++c)
            base[c] = from[p.box.columns[c]];
        const bool out = de_move((unsigned)j, p.key, p.d, p.jitter, p.box, base, base, base, 0.0, y);
        de_launch_row(p.d, p.box, out, base, y, p.rows_out + j * p.ld);
        double Z = from[p.z_column];
        if (p.z_dim >= 0)
            Z = out ? base[p.z_dim] : y[p.z_dim];
        double cap = Z / 6.0;
        cap = cap / 1e3;
        cap = cap * p.area;
        // ---- the states: a relative perturbation, the six soil layers held below their capacity
        const double *x = p.states_in + parent * SMART_PARTICLE_STATES;
        double *x_out = p.states_out + j * SMART_PARTICLE_STATES;
#pragma unroll
        for (int s = 0; s < SMART_PARTICLE_STATES; s += 2) {
            const Philox4 r = philox4x32_10((unsigned)j, p.key.gen, 18u + s / 2, 0u, p.key.k0, p.key.k1);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                double f = 2.0 * u53(r.w[2 * e], r.w[2 * e + 1]);
                f = f - 1.0;
                f = p.noise[s + e] * f;
                f = 1.0 + f;
                double v = x[s + e] * f;
                if (s + e >= SMART_PARTICLE_FIRST_LAYER && s + e < SMART_PARTICLE_FIRST_LAYER + 6)
                    v = v > cap ? cap : v;
                x_out[s + e] = v;
            }
        }
        p.logw_out[j] = resampled || degenerate ? 0.0 : p.logw_post[j];
    }
}

// ---- launch (validated by smart_analysis_capi.hip) -------------------------------------------------------------------
int launch_particle(const ParticleCall &c, hipStream_t s)
{
    const long N = c.n_particles;
    const int blocks = (int)((N + kPfThreads - 1) / kPfThreads);
    const PfWorkspace w = pf_workspace(c.workspace);
    const DeKey key = de_key(c.step, c.seed);
    if (c.phases & SMART_PARTICLE_WEIGH) {
        if (!c.q_in)
            hipLaunchKernelGGL(smart_particle_weigh, dim3(blocks), dim3(kPfThreads), 0, s, N, c.n_reports, c.sim, c.ld_sim,
                               c.obs, c.sigma0, c.sigma1, c.logw_in, c.logw_out, w);
        hipLaunchKernelGGL(smart_particle_quantise, dim3(blocks), dim3(kPfThreads), 0, s, N, blocks, c.logw_out, c.logw_in,
                           (const long long *)c.q_in, (long long *)c.q, w);
        PfHeader h;
        h.N = N, h.blocks = blocks, h.Rw = c.n_reports, h.obs = c.q_in ? nullptr : c.obs, h.given = c.q_in != nullptr;
        h.tau = c.tau, h.offset = c.offset, h.step = key.gen, h.k0 = key.k0, h.k1 = key.k1;
        h.w = w, h.stats = c.stats, h.counts = (long long *)c.counts;
        hipLaunchKernelGGL(smart_particle_header, dim3(1), dim3(kPfThreads), 0, s, h);
    }
    const bool resample = (c.phases & SMART_PARTICLE_RESAMPLE) != 0, move = (c.phases & SMART_PARTICLE_MOVE) != 0;
    if (!resample && !move)
        return SMART_OK;
    PfMove p;
    p.N = N, p.blocks = blocks, p.d = c.n_dims, p.key = key;
    p.box = de_box(c.n_dims, c.lo, c.hi, c.scale, c.columns);
    p.jitter = 0, p.z_dim = -1;
    for (int j = 0; j < c.n_dims; ++j) {
        if (c.scale[j] != 0.0)
            p.jitter |= 1u << j;
        if (c.columns[j] == c.z_column)
            p.z_dim = j;
    }
    p.z_column = c.z_column, p.area = c.area_m2;
    for (int k = 0; k < SMART_PARTICLE_STATES; ++k)
        p.noise[k] = c.noise[k];
    p.rows_in = c.rows_in, p.rows_out = c.rows_out, p.ld = c.ld, p.states_in = c.states_in, p.states_out = c.states_out;
    p.logw_post = c.q_in ? c.logw_in : c.logw_out, p.logw_out = c.logw_out, p.parents = c.parents, p.w = w;
    p.counts = (const long long *)c.counts, p.distinct = (long long *)c.counts + SMART_PARTICLE_DISTINCT;
    if (resample) {
        // (a call that is cut into phases counts again: the counter starts from 0 whoever ran before)
        if (hipError_t e = hipMemsetAsync(p.distinct, 0, sizeof(long long), s))
            return hip_fail(e, "hipMemsetAsync(distinct)");
        if (move)
            hipLaunchKernelGGL((smart_particle_resample<true, true>), dim3(blocks), dim3(kPfThreads), 0, s, p);
        else
            hipLaunchKernelGGL((smart_particle_resample<true, false>), dim3(blocks), dim3(kPfThreads), 0, s, p);
    } else {
        hipLaunchKernelGGL((smart_particle_resample<false, true>), dim3(blocks), dim3(kPfThreads), 0, s, p);
    }
    return SMART_OK;
}

} // namespace smart
