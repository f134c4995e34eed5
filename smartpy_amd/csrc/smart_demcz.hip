// smart_demcz.hip -- one generation of DE-MCz (differential evolution Markov chain with sampling from the past: ter Braak &
// Vrugt 2008, Stat. Comput. 18) with the subspace crossover of DREAM (Vrugt 2016) on a uniform prior box, around the
// ensemble launch that scores the proposals.  The definition -- the draw layout, the order of the operations, the bounds --
// is in include/smart_amd.h (smart_demcz_step_hip) and DESIGN.md section 4.20; this file says it once more in HIP.
//
// Two small kernels, one lane per chain, stream-ordered, no host synchronisation, no atomics:
//   smart_demcz_accept   the Metropolis decision on the proposals of generation g - 1 from their scores, the chain's state,
//                        log-density, payload and count updated in place, and (append) every chain's state after the
//                        decision written as archive row M + chain
//   smart_demcz_propose  the proposals of generation g from two rows of the archive, into the proposal matrix, the `out`
//                        flags and the varying columns of the launch matrix (the archive rows, the jump and gamma here,
//                        the move itself in smart_de_move.h, shared with smart_nsga2_vary)
// RANDOMNESS.  Philox4x32-10 (Salmon et al. 2011), counter (chain, generation, block, 0), key (seed lo, seed hi): the bits
// of a chain depend on the seed, the chain's number and the generation, never on the launch -- a call over half of the
// chains (chain_offset) draws what the call over all of them draws.
// ARITHMETIC.  The unit is compiled with -ffp-contract=off: every operation of the proposal is rounded once, as the numpy
// statement of the tests rounds it.  The one operation that is not correctly rounded by definition is log(u).
#include "smart_capi_internal.h"
#include "smart_de_move.h"
#include <cstdint>

namespace smart {

constexpr int kDemczThreads = 256;

// the log-density of a score (include/smart_amd.h: SMART_DEMCZ_SCORE_*)
__device__ inline double log_density(double score, int kind, double n_obs, double n_eff, double sigma)
{
    if (kind == SMART_DEMCZ_SCORE_RMSE) {
        const double s2 = score * score;
        return -((n_eff * 0.5) * log(n_obs * s2));
    }
    if (kind == SMART_DEMCZ_SCORE_RMSE_SIGMA) {
        const double s2 = score * score;
        return -(n_eff * s2) / ((2.0 * sigma) * sigma);
    }
    return score;
}

struct DemczAccept {
    long N;             // chains of this call
    long offset;        // the number of its first chain
    int d, n_carry;
    DeKey key;          // gen: the generation whose proposals are decided (0: the initial population takes its scores)
    double *x, *logp, *carry;
    int *accepted;
    const double *proposal;
    const unsigned char *out;
    const double *score;
    long score_stride;
    int score_kind;
    double n_obs, n_eff, sigma;
    const double *carry_new;
    int append;
    long M;
    double *archive, *archive_logp, *archive_carry;
};

__global__ __launch_bounds__(kDemczThreads) void smart_demcz_accept(DemczAccept a)
{
    const long i = (long)blockIdx.x * kDemczThreads + threadIdx.x;
    if (i >= a.N)
        return;
    const long chain = a.offset + i;
    double *x = a.x + i * a.d;
    double *carry = a.carry + i * a.n_carry;
    const double lstar = log_density(a.score[i * a.score_stride], a.score_kind, a.n_obs, a.n_eff, a.sigma);
    double l = a.logp[i];
    bool take;
    if (a.key.gen == 0) {
        take = true;        // the initial population: its state is what was launched
    } else {
        const Philox4 r = philox4x32_10((unsigned)chain, a.key.gen, 1u, 0u, a.key.k0, a.key.k1);
        const double u = u53(r.w[0], r.w[1]);
        take = !a.out[i] && lstar == lstar && log(u) < lstar - l;      // (a NaN difference: false)
        if (take) {
            const double *y = a.proposal + i * a.d;
            for (int j = 0; j < a.d; ++j)
                x[j] = y[j];
            a.accepted[i] += 1;
        }
    }
    if (take) {
        l = lstar;
        a.logp[i] = l;
        const double *fresh = a.carry_new + i * a.n_carry;
        for (int k = 0; k < a.n_carry; ++k)
            carry[k] = fresh[k];
    }
    if (a.append) {
        const long row = a.M + chain;
        double *z = a.archive + row * a.d;
        for (int j = 0; j < a.d; ++j)
            z[j] = x[j];
        a.archive_logp[row] = l;
        double *zc = a.archive_carry + row * a.n_carry;
        for (int k = 0; k < a.n_carry; ++k)
            zc[k] = carry[k];
    }
}

struct DemczPropose {
    long N, offset;
    int d;
    DeKey key;
    const double *x;
    const double *archive;
    unsigned long long M;       // archive rows to draw from, >= 2
    unsigned long long J, C;    // thresholds of the jump and of the crossover, in [0, 2^32]
    DeBox box;
    double gamma[SMART_DEMCZ_MAX_DIMS];
    double *proposal;
    unsigned char *out;
    double *rows;
    long ld;
};

__global__ __launch_bounds__(kDemczThreads) void smart_demcz_propose(DemczPropose p)
{
    const long i = (long)blockIdx.x * kDemczThreads + threadIdx.x;
    if (i >= p.N)
        return;
    const unsigned chain = (unsigned)(p.offset + i);
    const int d = p.d;
    const Philox4 r = philox4x32_10(chain, p.key.gen, 0u, 0u, p.key.k0, p.key.k1);
    const unsigned long long za = mulhi(r.w[0], p.M);
    unsigned long long zb = mulhi(r.w[1], p.M - 1);
    zb += zb >= za;
    const bool jump = (unsigned long long)r.w[2] < p.J;
    const unsigned moved = de_crossover(chain, p.key, d, p.C, (int)mulhi(r.w[3], (unsigned long long)d));
    const double gamma = jump ? 1.0 : p.gamma[__popc(moved) - 1];
    const double *x = p.x + i * d;
    double *y_out = p.proposal + i * d;
    const bool out = de_move(chain, p.key, d, moved, p.box, x, p.archive + za * d, p.archive + zb * d, gamma, y_out);
    p.out[i] = out ? 1 : 0;
    de_launch_row(d, p.box, out, x, y_out, p.rows + i * p.ld);
}

// ---- launch (validated by smart_analysis_capi.hip) -------------------------------------------------------------------
void launch_demcz(const DemczCall &c, hipStream_t s)
{
    const unsigned grid = (unsigned)((c.n_chains + kDemczThreads - 1) / kDemczThreads);
    if (c.score) {
        DemczAccept a;
        a.N = c.n_chains, a.offset = c.chain_offset, a.d = c.n_dims, a.n_carry = c.n_carry;
        a.key = de_key(c.generation - 1, c.seed);
        a.x = c.x, a.logp = c.logp, a.carry = c.carry, a.accepted = c.accepted;
        a.proposal = c.proposal, a.out = c.out;
        a.score = c.score, a.score_stride = c.score_stride, a.score_kind = c.score_kind;
        a.n_obs = (double)c.n_obs, a.n_eff = c.n_eff, a.sigma = c.sigma;
        a.carry_new = c.carry_new, a.append = c.append, a.M = c.archive_size;
        a.archive = c.archive, a.archive_logp = c.archive_logp, a.archive_carry = c.archive_carry;
        hipLaunchKernelGGL(smart_demcz_accept, dim3(grid), dim3(kDemczThreads), 0, s, a);
    }
    if (c.propose) {
        DemczPropose p;
        p.N = c.n_chains, p.offset = c.chain_offset, p.d = c.n_dims;
        p.key = de_key(c.generation, c.seed);
        p.x = c.x, p.archive = c.archive, p.M = (unsigned long long)demcz_archive_after(c);
        p.J = (unsigned long long)c.jump_threshold, p.C = (unsigned long long)c.cr_threshold;
        p.box = de_box(c.n_dims, c.lo, c.hi, c.scale, c.columns);
        for (int j = 0; j < SMART_DEMCZ_MAX_DIMS; ++j)
            p.gamma[j] = j < c.n_dims ? c.gamma[j] : 0.0;
        p.proposal = c.proposal, p.out = c.out, p.rows = c.rows, p.ld = c.ld;
        hipLaunchKernelGGL(smart_demcz_propose, dim3(grid), dim3(kDemczThreads), 0, s, p);
    }
}

} // namespace smart
