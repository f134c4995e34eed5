// smart_error_model.hip -- the residual error model of a stored discharge matrix sim[R][ld] (sample-minor): a standard
// deviation linear in the simulated flow, standardised residuals that follow an AR(1) (Schoups & Vrugt 2010; Evin et al.
// 2014).  The definition -- the terms, the order of the sums, the draw layout -- is the header comment of
// smart_error_model_loglik_hip / smart_error_model_draw_hip (include/smart_amd.h) and DESIGN.md section 4.21; this file
// says it once more in HIP.
//
// smart_error_model_loglik   the log-likelihood per sample.  A workgroup is kErrWaves wavefronts over the SAME 64 adjacent
//   samples, one lane per sample: every load of a report step is one contiguous 512-byte row segment.  The report steps
//   are cut into segments of kErrSegment steps; a round of the workgroup takes kErrWaves of them, one per wavefront, and
//     1. stages the round's observations in LDS, one step per thread, with what depends on the observations alone: the
//        step is observed, the step continues a chain (step t - 1 is observed too);
//     2. every wavefront walks its segment, kErrUnroll row loads in flight per lane.  The flags of a step are wave-uniform
//        (readfirstlane); observed / start / continuation are selects on them, never a branch, and a value at a step that
//        is not observed -- a NaN, say -- is selected away before it reaches a sum.
//   The model needs a_{t-1} across a segment boundary and nothing else: the wavefront recomputes it from row t - 1 (one
//   more row load per segment of 64) instead of waiting for the wavefront that owns that row.  The partial sums of the
//   four wavefronts go through LDS and are added in the order of the wavefronts: no atomics, and the association of
//   every sum is a function of R alone -- two launches, and launches over other N, give the same bits.
// smart_error_model_draw     one lane per output column walks the report steps in order (a true recurrence): a first pass
//   over its sample's column finds whether the sample is valid, the second draws -- a Philox block and one Box-Muller pair
//   per two steps -- and writes.  The stores of a step are contiguous across the lanes; the K lanes of a sample read the
//   same sim value.
// ARITHMETIC.  The unit is compiled with -ffp-contract=off: every operation is rounded once, as the numpy statement of the
// tests rounds it.  Not correctly rounded by definition: log, sin, cos.
#include "smart_capi_internal.h"
#include "smart_matrix_common.h"
#include "smart_philox.h"

namespace smart {

constexpr int kErrWaves = 4;                          // wavefronts per workgroup of the likelihood: the parts of a sum
constexpr int kErrSegment = SMART_ERROR_MODEL_SEGMENT; // report steps a wavefront walks per round
constexpr int kErrThreads = kErrWaves * kWave;
constexpr int kErrChunk = kErrWaves * kErrSegment;    // report steps staged per round
constexpr int kErrUnroll = 8;                         // row loads in flight per lane
constexpr int kDrawThreads = 256;
static_assert(kErrChunk == kErrThreads, "a round stages one report step per thread");
static_assert(kErrSegment % kErrUnroll == 0, "a whole segment is whole batches");

constexpr double kLnTwoPi = 1.8378770664093453; // ln(2 pi)
constexpr double kTwoPi = 6.283185307179586;

// (sigma0, sigma1, phi) of a sample, q = (1 - phi)(1 + phi), and what makes the sample invalid whatever the flows are
struct ErrorParams {
    double s0, s1, phi, q;
    bool bad;
};

__device__ inline ErrorParams error_params(const double *err, long err_ld, long i)
{
    const double *e = err + i * err_ld;
    ErrorParams p;
    p.s0 = e[0], p.s1 = e[1], p.phi = e[2];
    p.q = (1.0 - p.phi) * (1.0 + p.phi);
    p.bad = !(is_finite_bits(p.s0) && is_finite_bits(p.s1) && is_finite_bits(p.phi) && fabs(p.phi) < 1.0);
    return p;
}

__global__ __launch_bounds__(kErrThreads) void smart_error_model_loglik(long N, long R, const double *__restrict__ sim,
                                                                        long ld, const double *__restrict__ obs,
                                                                        const double *__restrict__ err, long err_ld,
                                                                        double *__restrict__ out)
{
    __shared__ double obs_s[kErrChunk + 1]; // [0]: the step before the round's first
    __shared__ unsigned flag_s[kErrChunk];  // bit 0: observed, bit 1: a continuation
    __shared__ double part[kErrWaves][2][kWave];
    __shared__ int bad_s[kErrWaves][kWave];
    __shared__ int count_s[kErrWaves][2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    long n = (long)blockIdx.x * kWave + lane;
    const bool live = n < N;
    if (!live)
        n = N - 1;
    const ErrorParams p = error_params(err, err_ld, n);
    const double *const col = sim + n;
    double ssq = 0.0, logsig = 0.0, before = 0.0; // before: a_{t-1}
    bool bad = p.bad;
    int seen_steps = 0, starts = 0; // (the same in every lane)

    auto step = [&](unsigned f, double e, double x) {
        const bool seen = f & 1u, cont = f & 2u;
        const double sigma = p.s0 + p.s1 * x;
        const double a = (e - x) / sigma;
        const double d = a - p.phi * before;
        const double term = cont ? d * d : p.q * (a * a);
        ssq += seen ? term : 0.0;
        logsig += seen ? log(sigma) : 0.0;
        bad |= seen && !(is_finite_bits(x) && sigma > 0.0);
        before = a;
        seen_steps += (int)(f & 1u);
        starts += (f & 3u) == 1u ? 1 : 0;
    };

    for (long c0 = 0; c0 < R; c0 += kErrChunk) {
        if (c0 > 0)
            __syncthreads(); // (the round before has been read)
        {
            const long r = c0 + tid;
            const double e = r < R ? obs[r] : quiet_nan();
            const bool seen = !is_nan_bits(e);
            const bool cont = seen && r >= 1 && !is_nan_bits(obs[r - 1]);
            obs_s[1 + tid] = e;
            flag_s[tid] = (seen ? 1u : 0u) | (cont ? 2u : 0u);
            if (tid == 0)
                obs_s[0] = c0 > 0 ? obs[c0 - 1] : quiet_nan();
        }
        __syncthreads();
        const int k0 = wave * kErrSegment;
        const long t0 = c0 + k0;
        const int len = (int)(R - t0 < kErrSegment ? R - t0 : kErrSegment); // (below 1: the record ends before this segment)
        if (len < 1)
            continue;
        // a_{t0 - 1} from row t0 - 1 itself (used only where step t0 continues a chain, and row t0 - 1 is observed then)
        if (t0 > 0) {
            const double xp = col[(t0 - 1) * ld];
            before = (obs_s[k0] - xp) / (p.s0 + p.s1 * xp);
        }
        int j = 0;
        for (; j + kErrUnroll <= len; j += kErrUnroll) {
            double x[kErrUnroll];
#pragma unroll
            for (int k = 0; k < kErrUnroll; ++k)
                x[k] = col[(t0 + j + k) * ld];
#pragma unroll
            for (int k = 0; k < kErrUnroll; ++k)
                step(__builtin_amdgcn_readfirstlane(flag_s[k0 + j + k]), obs_s[1 + k0 + j + k], x[k]);
        }
        for (; j < len; ++j)
            step(__builtin_amdgcn_readfirstlane(flag_s[k0 + j]), obs_s[1 + k0 + j], col[(t0 + j) * ld]);
    }
    part[wave][0][lane] = ssq;
    part[wave][1][lane] = logsig;
    bad_s[wave][lane] = bad ? 1 : 0;
    if (lane == 0) {
        count_s[wave][0] = seen_steps;
        count_s[wave][1] = starts;
    }
    __syncthreads();
    if (wave != 0 || !live)
        return;
    double total[2];
    int invalid = 0, n_seen = 0, n_starts = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double t = part[0][k][lane];
#pragma unroll
        for (int w = 1; w < kErrWaves; ++w)
            t += part[w][k][lane];
        total[k] = t;
    }
#pragma unroll
    for (int w = 0; w < kErrWaves; ++w) {
        invalid |= bad_s[w][lane];
        n_seen += count_s[w][0];
        n_starts += count_s[w][1];
    }
    double loglik = -0.5 * total[0] - total[1];
    loglik = loglik + (0.5 * (double)n_starts) * log(p.q);
    loglik = loglik - (0.5 * (double)n_seen) * kLnTwoPi;
    if (n_seen == 0)
        loglik = 0.0; // (0 ln q is a NaN where q is 0 or less: such a sample is invalid anyway)
    out[SMART_ERROR_MODEL_LOGLIK * N + n] = invalid ? -__builtin_inf() : loglik;
    out[SMART_ERROR_MODEL_SSQ * N + n] = invalid ? quiet_nan() : total[0];
    out[SMART_ERROR_MODEL_LOGSIG * N + n] = invalid ? quiet_nan() : total[1];
}

__global__ __launch_bounds__(kDrawThreads) void smart_error_model_draw(long C, long R, long K,
                                                                       const double *__restrict__ sim, long ld,
                                                                       const double *__restrict__ err, long err_ld,
                                                                       unsigned k0, unsigned k1, unsigned long long offset,
                                                                       int truncate, double *__restrict__ out, long out_ld)
{
    const long c = (long)blockIdx.x * kDrawThreads + threadIdx.x;
    if (c >= C)
        return;
    const long i = c / K;
    const ErrorParams p = error_params(err, err_ld, i);
    const double *const col = sim + i;
    double *const o = out + c;
    // is the sample valid, over every report step
    bool bad = p.bad;
    long t = 0;
    for (; t + kErrUnroll <= R; t += kErrUnroll) {
        double x[kErrUnroll];
#pragma unroll
        for (int k = 0; k < kErrUnroll; ++k)
            x[k] = col[(t + k) * ld];
#pragma unroll
        for (int k = 0; k < kErrUnroll; ++k)
            bad |= !(is_finite_bits(x[k]) && p.s0 + p.s1 * x[k] > 0.0);
    }
    for (; t < R; ++t) {
        const double x = col[t * ld];
        bad |= !(is_finite_bits(x) && p.s0 + p.s1 * x > 0.0);
    }
    if (bad) {
        for (t = 0; t < R; ++t)
            o[t * out_ld] = quiet_nan();
        return;
    }
    const unsigned column = (unsigned)(offset + (unsigned long long)c);
    const double root = sqrt(p.q);
    double a = 0.0;
    auto put = [&](long at, double x, double eps) {
        a = at == 0 ? eps / root : p.phi * a + eps;
        const double sigma = p.s0 + p.s1 * x;
        double y = x + sigma * a;
        if (truncate)
            y = y > 0.0 ? y : 0.0;
        o[at * out_ld] = y;
    };
    for (t = 0; t < R; t += 2) {
        const bool pair = t + 1 < R;
        const double x0 = col[t * ld], x1 = pair ? col[(t + 1) * ld] : 0.0;
        const Philox4 w = philox4x32_10(column, (unsigned)(t / 2), 0u, 0u, k0, k1);
        const double u1 = 1.0 - u53(w.w[0], w.w[1]), u2 = u53(w.w[2], w.w[3]);
        const double r = sqrt(-2.0 * log(u1));
        double sn, cs;
        sincos(kTwoPi * u2, &sn, &cs);
        put(t, x0, r * cs);
        if (pair)
            put(t + 1, x1, r * sn);
    }
}

// ---- launch (validated by smart_analysis_capi.hip) -------------------------------------------------------------------
void launch_error_model_loglik(long N, long R, const double *sim, long ld, const double *obs, const double *err, long err_ld,
                               double *out, hipStream_t s)
{
    const unsigned grid = (unsigned)((N + kWave - 1) / kWave);
    hipLaunchKernelGGL(smart_error_model_loglik, dim3(grid), dim3(kErrThreads), 0, s, N, R, sim, ld, obs, err, err_ld, out);
}

void launch_error_model_draw(long N, long R, long K, const double *sim, long ld, const double *err, long err_ld,
                             unsigned long long seed, long column_offset, int truncate, double *out, long out_ld,
                             hipStream_t s)
{
    const long C = N * K;
    const unsigned grid = (unsigned)((C + kDrawThreads - 1) / kDrawThreads);
    hipLaunchKernelGGL(smart_error_model_draw, dim3(grid), dim3(kDrawThreads), 0, s, C, R, K, sim, ld, err, err_ld,
                       (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (unsigned long long)column_offset,
                       truncate, out, out_ld);
}

} // namespace smart
