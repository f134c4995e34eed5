// smart_objfn_windows.hip -- objective functions of a stored discharge matrix sim[R][ld] (sample-minor) PER WINDOW of
// report steps and on TRANSFORMED flows: split-sample scores (per hydrological year, season, period) and low-flow
// scores (sqrt Q, ln(Q + eps), 1 / (Q + eps)) for every sample, from the matrix where the launch left it.
//
// Definition.  window[r] in {-1, 0 .. W-1}.  For window w and sample n: rows = { r : window[r] == w, obs[r] not NaN },
// e = f(obs[rows]), s = f(sim[rows, n]); the seven values NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE are the formulas of
// montecarlo.py:193-209 on (s, e) -- finish_objectives (smart_device.h), the one the other two paths end in.  Two rules:
//   fewer than two rows                 -> NaN in all seven columns, for every sample of the window
//   a transformed value that is not finite (sqrt or ln of a negative flow, x + eps == 0, a NaN or an infinity in the
//   matrix)                             -> NaN in all seven columns of that (window, sample); a non-finite f(obs[r]) does
//                                          it for every sample of the window
//
// Geometry.  grid = (ceil(N / 64), W), a workgroup = kWinWaves wavefronts over the SAME 64 samples (the WX = 1, WR = 8
// geometry of smart_objfn_matrix).  A workgroup
//   1. forms the window's observation statistics (count, mean, sum, sum of squared deviations) in two passes over
//      window[] and obs[] -- R * 12 bytes, L2-resident -- with a fixed-order LDS tree;
//   2. walks window[] in chunks of kWinChunk rows: the rows that belong to the window and carry an observation are listed
//      IN ROW ORDER as (row, f(obs[row])) in LDS (list_rows, smart_window_rows.h) and the wavefronts take the list entries
//      round-robin (walk_listed_rows).  Rows of no window, of another window, or without an observation are never read;
//      every element of a listed row is loaded once, by one lane of one wavefront;
//   3. adds the wavefronts' partial moments through LDS in wavefront order (sum_wave_moments) and finishes.
//
// Moments: the one-pass form of smart_objfn_matrix about the window's observation mean and a per-sample shift, the
// sample's FIRST in-window transformed value (loaded by wavefront 0, handed to the others through LDS, and accumulated by
// wavefront 0 from the register it already sits in).  A non-finite transformed value needs no test of its own: u = s - shift
// is then not finite, and a sum that has taken a non-finite term never becomes finite again (inf + finite = inf, inf - inf =
// NaN) -- the rule is ONE test of C1 = sum(u) per (window, sample) at the end, of sum f(e) per window.  (A sum of finite
// values that overflows is reported the same way.)
//
// Determinism.  No floating-point atomics; the list order, the round-robin and both reductions are fixed by (N, R, the
// window array): two launches give the same bits.
#include "smart_capi_internal.h"
#include "smart_device.h"
#include "smart_window_rows.h"

namespace smart {

// each workgroup re-reads window[] and obs[] (R * 12 bytes, three times): W times per 64 samples over the launch.  The
// bound keeps that beside the matrix traffic for windows of a useful length, and the grid's y inside its 65,535.
constexpr int kWinMaxWindows = 1024;

// sum over the workgroup's kWinThreads threads, the same tree for every call
__device__ inline double win_block_sum(double v, double *sh)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = kWinThreads / 2; s > 0; s >>= 1) {
        if (tid < s)
            sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

template <int T>
__global__ __launch_bounds__(kWinThreads) void smart_objfn_windows(long N, long R, const double *__restrict__ sim, long ld,
                                                                   const double *__restrict__ obs,
                                                                   const int *__restrict__ window, double eps,
                                                                   double *__restrict__ objfn)
{
    __shared__ double sh[kWinThreads];
    __shared__ int cnt[kWinSub][kWinWaves];
    __shared__ int rows[kWinChunk];
    __shared__ double fes[kWinChunk];
    __shared__ double first[kWave];
    __shared__ double part[kWinWaves][5][kWave];
    const int w = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wr = __builtin_amdgcn_readfirstlane(tid / kWave);
    long n = (long)blockIdx.x * kWave + lane;
    const bool live = n < N;
    if (!live)
        n = N - 1;
    double *const out = objfn + ((long)w * N + n) * SMART_OBJFN_WINDOW_COLS;

    // ---- 1. the window's observations: n, mean, sum, sum((e - mean)^2), sum(e - mean) of e = f(obs) (obs_stats of
    // smart_matrix_common.h, masked by the window)
    double st[5];
    {
        double c = 0.0, s = 0.0;
        for (long r = tid; r < R; r += kWinThreads)
            if (window[r] == w) {
                const double e = obs[r];
                if (!is_nan_bits(e)) {
                    c += 1.0;
                    s += flow_transform(T, e, eps);
                }
            }
        c = win_block_sum(c, sh);
        s = win_block_sum(s, sh);
        if (c < 2.0 || !is_finite_bits(s)) { // the two rules, for the whole window (the same verdict in every thread)
            if (wr == 0 && live)
#pragma unroll
                for (int k = 0; k < SMART_OBJFN_WINDOW_COLS; ++k)
                    out[k] = quiet_nan();
            return;
        }
        const double mean = s / c;
        double s2 = 0.0, s1 = 0.0;
        for (long r = tid; r < R; r += kWinThreads)
            if (window[r] == w) {
                const double e = obs[r];
                if (!is_nan_bits(e)) {
                    const double d = flow_transform(T, e, eps) - mean;
                    s2 += d * d;
                    s1 += d;
                }
            }
        st[0] = c;
        st[1] = mean;
        st[2] = s;
        st[3] = win_block_sum(s2, sh);
        st[4] = win_block_sum(s1, sh);
    }
    const double ebar = st[1];

    // ---- 2. the rows of the window, chunk by chunk
    const double *const col = sim + n;
    double shift = 0.0;
    bool have_shift = false; // (the same in every thread of the workgroup)
    double A = 0.0, B = 0.0, C1 = 0.0, C2 = 0.0, C3 = 0.0;
    auto add = [&](double e, double s) {
        const double d = s - e, u = s - shift;
        A += d;
        B += d * d;
        C1 += u;
        C2 += u * u;
        C3 += (e - ebar) * u;
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
        if (m == 0)
            continue;
        int j = wr;
        if (!have_shift) { // entry 0 of the first chunk that has one: the sample's shift, read by wavefront 0 alone
            double s0 = 0.0;
            if (wr == 0) {
                s0 = flow_transform(T, col[(long)__builtin_amdgcn_readfirstlane(rows[0]) * ld], eps);
                first[lane] = s0;
            }
            __syncthreads();
            shift = first[lane];
            have_shift = true;
            if (wr == 0) {
                add(fes[0], s0);
                j += kWinWaves;
            }
        }
        walk_listed_rows<T>(j, m, rows, fes, col, ld, eps, add);
    }

    // ---- 3. the wavefronts' partial moments, added in wavefront order
    double mo[5] = {A, B, C1, C2, C3};
    if (!sum_wave_moments<kWinWaves>(mo, part, wr, lane, live))
        return;
    double o[8];
    finish_objectives(st, mo[0], mo[1], mo[2], mo[3], mo[4], 0.0, quiet_nan(), o);
    const bool ok = is_finite_bits(mo[2]); // some f(sim) of this sample was not finite (header comment)
#pragma unroll
    for (int k = 0; k < SMART_OBJFN_WINDOW_COLS; ++k)
        out[k] = ok ? o[k] : quiet_nan();
}

int objfn_max_windows() { return kWinMaxWindows; }

void launch_objfn_windows(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                          int transform, double eps, double *objfn, hipStream_t s)
{
    const dim3 grid((unsigned)((N + kWave - 1) / kWave), (unsigned)W), block(kWinThreads);
    with_transform(transform, [&](auto t) {
        hipLaunchKernelGGL(smart_objfn_windows<decltype(t)::value>, grid, block, 0, s, N, R, sim, ld, obs, window, eps,
                           objfn);
    });
}

} // namespace smart
