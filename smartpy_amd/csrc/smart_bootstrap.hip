// smart_bootstrap.hip -- the uncertainty of the objective functions of a stored discharge matrix sim[R][ld] (sample-minor)
// under resampling of WINDOWS of report steps (block bootstrap over hydrological years, leave-one-year-out jackknife): for
// every sample the seven scores of B replicates, their mean, standard deviation and K order statistics.
//
// Definition.  window[r] in {-1, 0 .. W-1}; the valid rows of window w are { r : window[r] == w, obs[r] not NaN }.
// Replicate b is the multiset union over w of the valid rows of window w, each taken counts[b][w] times; its seven values
// NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE are finish_objectives (smart_device.h) on (f(sim), f(obs)) over that multiset,
// f one of the four transforms of smart_objfn_windows.hip.  The POINT value is the replicate with every count 1.  Rules:
//   a replicate with fewer than two rows                       -> NaN in all seven columns, for every sample
//   a (sample, window) that meets a transformed value that is not finite (or whose sums overflow)
//                                                              -> NaN for every replicate of that sample whose count for
//                                                                 that window is not 0; a count of 0 leaves it untouched
//   a non-finite f(obs) in window w                            -> the same, for every sample
// MEAN and STD (ddof = 1, NaN for B < 2) over the B replicates are NaN where any replicate of the (sample, score) is; the K
// quantiles are order statistics of the B values (numpy 'inverted_cdf': an element of the set, NaN sorts last).
// The kernels do not know what a year is: bootstrap and jackknife differ in counts[][] only.
//
// The matrix is read ONCE.  The seven scores are functions of five one-pass moments, and moments taken about constants of
// the whole launch add across windows, so a replicate is an integer-weighted sum of per-window moments:
//   g   = the mean of the finite f(obs) over the valid rows of all windows (any constant serves; finite values only, so that
//         one bad observation does not reach the windows it does not lie in),
//   c_n = f(sim[r0][n]), r0 the first valid row of the launch (the same row for every sample: its address is scalar); 0
//         where that value is not finite,
//   per (window, sample)  A = sum(s - e)  B = sum((s - e)^2)  C1 = sum(s - c_n)  C2 = sum((s - c_n)^2)
//                         C3 = sum((e - g)(s - c_n)),   per window  n, sum e, sum(e - g), sum((e - g)^2).
// finish_objectives takes an observation reference that is not the exact mean (st[4] = sum(e - g) enters its covariance);
// per replicate see = sum((e - g)^2) - (sum(e - g))^2 / n.
//
// 1. smart_bootstrap_observed, grid W: every workgroup forms g and r0 with the same fixed-order tree (the same bits in
//    each), workgroup w the four observation sums of window w.
// 2. smart_bootstrap_moments, grid (ceil(N / 64), W): the geometry of smart_objfn_windows and its list, walk and
//    reduction, all from smart_window_rows.h (8 wavefronts on the same 64 samples, rows of no window or without an
//    observation never read, every element of a listed row loaded once); the two kernels differ in the observation
//    reference (g), in where the shift comes from (c_n) and in the end: the five moments go to the workspace [W][5][N].
// 3. smart_bootstrap_scores, one lane per sample, grid (ceil(cn / 64), up to 32): the wavefronts of the grid's y split the
//    replicates round-robin (at least four each).  counts[b][.] is wave-uniform: lane w loads counts[b][w] -- one
//    coalesced read per replicate -- and the count of a window is then a lane read (v_readlane) into a scalar register; a
//    window with count 0 is skipped by
//    a scalar branch, which is the "untouched" direction of the rules (0 x inf would be NaN).  The moments of the windows
//    are read from the workspace where kernel 2 left them, [W][5][N]: 512 contiguous bytes per wavefront and term, from L2
//    (W x 5 x 8 bytes per sample, 2.5 KiB at the cap -- 160 KiB per 64 samples would not fit the LDS of a compute unit).
//    That one lane holds the counts of a replicate sets the cap: smart_bootstrap_max_windows() = 64 windows.
//    The point value is the replicate the first wavefront computes ahead of its own, by the same instructions (all counts
//    1): a row of ones in counts[][] gives the bits of point[].
//    smart_bootstrap_stats then takes MEAN and STD of a chunk: one lane per (score, sample) reads its B values in
//    replicate order (coalesced: neighbouring lanes, neighbouring samples) in the one-pass form about the point value (0
//    where that is not finite) -- one association whatever the grid, and a NaN replicate makes both NaN by arithmetic.
// 4. The order statistics.  The replicates of a chunk of cn samples lie in the workspace as a matrix [B][7 cn], and the
//    quantiles are order statistics along its rows: launch_flow_duration (smart_flow_duration.hip) unchanged, with no
//    observations, no window array and no objective functions, sort form (B <= smart_bootstrap_max_resamples() = 4,096 is
//    inside its capacity of 16,384).  smart_bootstrap_place copies its [K][7 cn] answer into stats[7][2 + K][N].
// N is walked in chunks of cn samples (a multiple of 64; 7 B cn doubles stay below 128 MiB, at least 64 samples) so that the
// workspace is bounded whatever N is; a caller's replicates[B][7][N] is written beside the chunk, never instead of it, so
// stats are the same bits with and without it.
//
// Determinism.  No floating-point atomics; the list order, the round-robin and every reduction are fixed by (N, R, the
// window array, B): two launches give the same bits, whatever ld.
#include "smart_capi_internal.h"
#include "smart_device.h"
#include "smart_window_rows.h"

namespace smart {

// (smart_bootstrap_moments has the kWin* geometry of smart_window_rows.h)
constexpr int kBsWaves = 8;                     // wavefronts per workgroup of _observed and _scores (there: over b)
constexpr int kBsThreads = kBsWaves * kWave;
constexpr int kBsMaxWindows = kWave;            // one lane per window holds a replicate's counts
constexpr int kBsMaxResamples = 4096;
constexpr int kBsHead = 8;                      // doubles in front of the workspace: g, r0 (-1: no valid row)
constexpr int kBsObs = 4;                       // per window: n, sum e, sum(e - g), sum((e - g)^2)
constexpr long kBsRepDoubles = 16l << 20;       // replicate values of a chunk of samples: 128 MiB
constexpr long kBsMaxChunk = 16384;             // samples per chunk at most
constexpr int kBsCols = SMART_OBJFN_WINDOW_COLS;

// ---- the layout of the workspace, in doubles (every part starts on a multiple of 32 doubles)
struct BootstrapLayout {
    long obs, mom, quant, rep, total;   // offsets of the window sums, the moments, the order statistics, the replicates
    long chunk;                         // samples per chunk (0 without replicates)
};

static long bs_up(long x) { return (x + 31) / 32 * 32; }

static BootstrapLayout bootstrap_layout(long N, int W, int B)
{
    BootstrapLayout l;
    l.chunk = 0;
    if (B > 0) {
        long c = kBsRepDoubles / ((long)kBsCols * B) / kWave * kWave;
        c = c < kWave ? kWave : (c > kBsMaxChunk ? kBsMaxChunk : c);
        l.chunk = c < N ? c : N;
    }
    l.obs = kBsHead;
    l.mom = bs_up(l.obs + (long)kBsObs * W);
    l.quant = bs_up(l.mom + 5l * W * N);
    l.rep = bs_up(l.quant + (long)SMART_QUANTILES_MAX_PROBS * kBsCols * l.chunk);
    l.total = bs_up(l.rep + (long)B * kBsCols * l.chunk);
    return l;
}

// ---- 1. g, r0 and the observation sums of every window -----------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(kBsThreads) void smart_bootstrap_observed(long R, const double *__restrict__ obs,
                                                                      const int *__restrict__ window, int W, double eps,
                                                                      double *__restrict__ ws)
{
    __shared__ double sh[kBsThreads];
    __shared__ int first[kBsThreads];
    const int w = blockIdx.x, tid = threadIdx.x;
    double c = 0.0, s = 0.0;
    int r0 = 0x7fffffff;
    for (long r = tid; r < R; r += kBsThreads) {
        const int id = window[r];
        if (id >= 0 && id < W) {
            const double e = obs[r];
            if (!is_nan_bits(e)) {
                r0 = r0 < (int)r ? r0 : (int)r;
                const double fe = flow_transform(T, e, eps);
                if (is_finite_bits(fe)) {
                    c += 1.0;
                    s += fe;
                }
            }
        }
    }
    c = block_sum(c, sh);
    s = block_sum(s, sh);
    first[tid] = r0;
    __syncthreads();
    for (int d = kBsThreads / 2; d > 0; d >>= 1) {
        if (tid < d)
            first[tid] = first[tid] < first[tid + d] ? first[tid] : first[tid + d];
        __syncthreads();
    }
    r0 = first[0];
    const double g = c > 0.0 && is_finite_bits(s) ? s / c : 0.0;

    double n = 0.0, se = 0.0, s1 = 0.0, s2 = 0.0;
    for (long r = tid; r < R; r += kBsThreads)
        if (window[r] == w) {
            const double e = obs[r];
            if (!is_nan_bits(e)) {
                const double fe = flow_transform(T, e, eps), d = fe - g;
                n += 1.0;
                se += fe;
                s1 += d;
                s2 += d * d;
            }
        }
    n = block_sum(n, sh);
    se = block_sum(se, sh);
    s1 = block_sum(s1, sh);
    s2 = block_sum(s2, sh);
    if (tid == 0) {
        double *const o = ws + kBsHead + (long)kBsObs * w;
        o[0] = n;
        o[1] = se;
        o[2] = s1;
        o[3] = s2;
        if (w == 0) {
            ws[0] = g;
            ws[1] = r0 == 0x7fffffff ? -1.0 : (double)r0;
        }
    }
}

// ---- 2. the five moments of every (window, sample) about g and c_n ---------------------------------------------------------
template <int T>
__global__ __launch_bounds__(kWinThreads) void smart_bootstrap_moments(long N, long R, const double *__restrict__ sim, long ld,
                                                                      const double *__restrict__ obs,
                                                                      const int *__restrict__ window, double eps,
                                                                      const double *__restrict__ head,
                                                                      double *__restrict__ mom)
{
    __shared__ int cnt[kWinSub][kWinWaves];
    __shared__ int rows[kWinChunk];
    __shared__ double fes[kWinChunk];
    __shared__ double part[kWinWaves][5][kWave];
    const int w = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wr = __builtin_amdgcn_readfirstlane(tid / kWave);
    long n = (long)blockIdx.x * kWave + lane;
    const bool live = n < N;
    if (!live)
        n = N - 1;
    const double g = head[0];
    const long r0 = (long)head[1];          // (no valid row at all: every window is empty and nothing is loaded below)
    const double *const col = sim + n;
    double shift = 0.0;
    if (r0 >= 0) {
        shift = flow_transform(T, col[r0 * ld], eps);
        if (!is_finite_bits(shift))
            shift = 0.0;
    }
    double A = 0.0, B = 0.0, C1 = 0.0, C2 = 0.0, C3 = 0.0;
    auto add = [&](double e, double s) {
        const double d = s - e, u = s - shift;
        A += d;
        B += d * d;
        C1 += u;
        C2 += u * u;
        C3 += (e - g) * u;
    };
    for (long c0 = 0; c0 < R; c0 += kWinChunk) {
        double fe[kWinSub] = {}; // f(obs) of this thread's rows, for the list
        const int m = list_rows<kWinWaves, kWinSub>(
            c0, R, wr, cnt,
            [&](long r, int k) {
                if (window[r] != w)
                    return false;
                const double e = obs[r];
                if (is_nan_bits(e))
                    return false;
                fe[k] = flow_transform(T, e, eps);
                return true;
            },
            [&](int pos, long r, int k) {
                rows[pos] = (int)r;
                fes[pos] = fe[k];
            });
        walk_listed_rows<T>(wr, m, rows, fes, col, ld, eps, add);
    }

    // the wavefronts' partial moments, added in wavefront order
    double mo[5] = {A, B, C1, C2, C3};
    if (!sum_wave_moments<kWinWaves>(mo, part, wr, lane, live))
        return;
#pragma unroll
    for (int k = 0; k < 5; ++k)
        mom[((long)w * 5 + k) * N + n] = mo[k];
}

// ---- 3. the replicates: counts x moments, the seven scores -----------------------------------------------------------------
__global__ __launch_bounds__(kBsThreads) void smart_bootstrap_scores(long N, long n0, int cn, int W,
                                                                    const double *__restrict__ obsw,
                                                                    const double *__restrict__ mom,
                                                                    const unsigned short *__restrict__ counts, int B,
                                                                    double *__restrict__ point,
                                                                    double *__restrict__ replicates,
                                                                    double *__restrict__ rep)
{
    __shared__ double ow[kBsMaxWindows * kBsObs];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wr = __builtin_amdgcn_readfirstlane(tid / kWave);
    for (int i = tid; i < kBsObs * W; i += kBsThreads)
        ow[i] = obsw[i];
    __syncthreads();
    long i = (long)blockIdx.x * kWave + lane;
    const bool live = i < cn;
    if (!live)
        i = cn - 1;
    const long n = n0 + i;
    const double *const m = mom + n;
    // the wavefronts of the grid's y take the replicates round-robin; b < 0 is the point value, which the first of them
    // computes ahead of its replicates, by the instructions of a replicate
    const int first = (int)blockIdx.y * kBsWaves + wr, all = (int)gridDim.y * kBsWaves;
    for (int b = first == 0 ? -all : first; b < B; b += all) {
        int mine = 1;
        if (b >= 0)
            mine = lane < W ? (int)counts[(long)b * W + lane] : 0;
        double rn = 0.0, se = 0.0, s1 = 0.0, s2 = 0.0;
        double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < W; ++w) {
            const int c = __builtin_amdgcn_readlane(mine, w);
            if (c == 0)
                continue;       // (scalar: the window does not reach this replicate, whatever its sums hold)
            const double cd = (double)c;
            rn = fma(cd, ow[kBsObs * w], rn);
            se = fma(cd, ow[kBsObs * w + 1], se);
            s1 = fma(cd, ow[kBsObs * w + 2], s1);
            s2 = fma(cd, ow[kBsObs * w + 3], s2);
#pragma unroll
            for (int k = 0; k < 5; ++k)
                acc[k] = fma(cd, m[((long)w * 5 + k) * N], acc[k]);
        }
        const double st[5] = {rn, 0.0, se, s2 - s1 * s1 / rn, s1};
        double o[8];
        finish_objectives(st, acc[0], acc[1], acc[2], acc[3], acc[4], 0.0, quiet_nan(), o);
        const bool ok = rn >= 2.0 && is_finite_bits(se) && is_finite_bits(s2) && is_finite_bits(acc[0]) &&
                        is_finite_bits(acc[1]) && is_finite_bits(acc[2]) && is_finite_bits(acc[3]) && is_finite_bits(acc[4]);
        if (!live)
            continue;
#pragma unroll
        for (int s = 0; s < kBsCols; ++s) {
            const double x = ok ? o[s] : quiet_nan();
            if (b < 0) {
                point[n * kBsCols + s] = x;
            } else {
                rep[((long)b * kBsCols + s) * cn + i] = x;
                if (replicates)
                    replicates[((long)b * kBsCols + s) * N + n] = x;
            }
        }
    }
}

// ---- mean and standard deviation over the replicates of a chunk: one lane per (score, sample), in replicate order, the
// one-pass form about the point value (0 where that is not finite) ---------------------------------------------------------
__global__ __launch_bounds__(256) void smart_bootstrap_stats(long N, long n0, int cn, int B, int K,
                                                             const double *__restrict__ point,
                                                             const double *__restrict__ rep, double *__restrict__ stats)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x, per = (long)kBsCols * cn;
    if (e >= per)
        return;
    const long s = e / cn, n = n0 + e % cn;
    const double p = point[n * kBsCols + s];
    const double ref = is_finite_bits(p) ? p : 0.0;
    double S1 = 0.0, S2 = 0.0;
    const double *x = rep + e;
#pragma unroll 8
    for (int b = 0; b < B; ++b) {
        const double d = x[(long)b * per] - ref;
        S1 += d;
        S2 += d * d;
    }
    const double nb = (double)B;
    const double var = (S2 - S1 * S1 / nb) / (nb - 1.0);
    double *const o = stats + s * (2 + K) * N + n;
    o[0] = ref + S1 / nb;
    o[N] = B < 2 ? quiet_nan() : sqrt(var < 0.0 ? 0.0 : var);     // (a NaN passes the compare and stays one)
}

// ---- 4. the order statistics of a chunk, [K][7 cn], to their rows of stats[7][2 + K][N] ---------------------------------
__global__ __launch_bounds__(256) void smart_bootstrap_place(long N, long n0, int cn, int K, const double *__restrict__ quant,
                                                             double *__restrict__ stats)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x, per = (long)kBsCols * cn;
    if (e >= (long)K * per)
        return;
    const long k = e / per, s = (e % per) / cn, i = e % cn;
    stats[(s * (2 + K) + 2 + k) * N + n0 + i] = quant[e];
}

// ---- launch (validated by smart_analysis_capi.hip) ---------------------------------------------------------------------
int bootstrap_max_windows() { return kBsMaxWindows; }
int bootstrap_max_resamples() { return kBsMaxResamples; }

long bootstrap_workspace_bytes(long N, int W, int B, bool /*with_replicates*/)
{
    return (bootstrap_layout(N, W, B).total * 8 + 255) / 256 * 256;
}

template <int T>
static void launch_bootstrap_moments(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                                     double eps, double *ws, double *mom, hipStream_t s)
{
    hipLaunchKernelGGL(smart_bootstrap_observed<T>, dim3((unsigned)W), dim3(kBsThreads), 0, s, R, obs, window, W, eps, ws);
    hipLaunchKernelGGL(smart_bootstrap_moments<T>, dim3((unsigned)((N + kWave - 1) / kWave), (unsigned)W), dim3(kWinThreads),
                       0, s, N, R, sim, ld, obs, window, eps, ws, mom);
}

void launch_bootstrap(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                      int transform, double eps, const unsigned short *counts, int B, const double *probs, int K,
                      double *point, double *stats, double *replicates, double *ws, hipStream_t s)
{
    const BootstrapLayout l = bootstrap_layout(N, W, B);
    double *const mom = ws + l.mom;
    with_transform(transform, [&](auto t) {
        launch_bootstrap_moments<decltype(t)::value>(N, R, sim, ld, obs, window, W, eps, ws, mom, s);
    });
    const long step = B > 0 ? l.chunk : (N < kBsMaxChunk ? N : kBsMaxChunk);
    // wavefronts over the replicates: at least four replicates each, at most 32 workgroups deep
    int deep = (B + 4 * kBsWaves - 1) / (4 * kBsWaves);
    deep = deep < 1 ? 1 : (deep > 32 ? 32 : deep);
    for (long n0 = 0; n0 < N; n0 += step) {
        const int cn = (int)(N - n0 < step ? N - n0 : step);
        hipLaunchKernelGGL(smart_bootstrap_scores, dim3((unsigned)((cn + kWave - 1) / kWave), (unsigned)deep),
                           dim3(kBsThreads), 0, s, N, n0, cn, W, ws + l.obs, mom, counts, B, point, replicates, ws + l.rep);
        if (B < 1)
            continue;
        const long per = (long)kBsCols * cn;
        hipLaunchKernelGGL(smart_bootstrap_stats, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, N, n0, cn, B, K,
                           point, ws + l.rep, stats);
        // the chunk's replicates as a matrix [B][7 cn]: order statistics along its rows
        launch_flow_duration(per, (long)B, ws + l.rep, per, nullptr, nullptr, 1, probs, K, ws + l.quant,
                             SMART_TRANSFORM_NONE, 0.0, 0.0, 1.0, nullptr, nullptr, /*sort=*/true, s);
        hipLaunchKernelGGL(smart_bootstrap_place, dim3((unsigned)((K * per + 255) / 256)), dim3(256), 0, s, N, n0, cn, K,
                           ws + l.quant, stats);
    }
}

} // namespace smart
