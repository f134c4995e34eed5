// smart_ensemble_scores.hip -- verification scores of the ensemble along the SAMPLE axis, per report step: for the
// members x_n = sim[r][n] with weights w_n >= 0 (or all 1) and the observation y = obs[r], with the live members (w_n > 0)
// sorted ascending x_(1) <= ... <= x_(M), W their total weight, A_i the PREFIX sums of the sorted weights (left to right),
// B_i the SUFFIX sums over j > i (right to left), P_i = A_i / W and Q_i = B_i / W:
//     CRPS     = max(x_(1) - y, 0) + max(y - x_(M), 0) + sum_{i<M} (m_i - x_(i)) P_i^2 + (x_(i+1) - m_i) Q_i^2,
//                m_i = min(max(y, x_(i)), x_(i+1))                          (the integral of (F - 1[x >= y])^2)
//     SPREAD   = sum_{i<M} (x_(i+1) - x_(i)) P_i Q_i                        (the integral of F (1 - F) = E|X - X'| / 2)
//     PIT_LOW  = sum of w over x < y, / W        PIT_HIGH = sum of w over x <= y, / W
//     MEAN     = sum of w x / W, added in sorted order
// Every term is a product of non-negative factors: Q_i comes from the suffix sum, never as 1 - P_i, and nothing cancels.
// A member of weight zero is dropped when the step is loaded (its key becomes the padding), so its value -- a NaN, an
// infinity -- decides nothing.  W == 0, or a live member that is not finite: all five NaN.  A missing observation (not
// finite, or obs == nullptr): CRPS and both PITs NaN, SPREAD and MEAN as they are.  -0.0 and +0.0 are one value
// (smart_order_keys.h).  One workgroup per report step: the matrix is sample-minor, so the step's N values are contiguous.
//
// Two forms, the same definitions:
//   LDS     N <= kEnsCapacity.  Keys (and the 16-bit sample index where there are weights) into LDS, bitonic network
//           there; 10 bytes per element, so 8192 elements are 80 KiB.  Neither running sum is ever stored: thread t owns E
//           consecutive sorted positions, scans its weights in registers in both directions, and forms the terms of its
//           own gaps from keys[i], keys[i + 1], P_i and Q_i.
//   global  any N up to 2^24.  (key, weight) pairs -- keys alone without weights -- in the caller's workspace, padded to a
//           power of two P >= kEnsBlock.  The same network with two memory levels: a stage whose distance reaches past a
//           block of kEnsBlock elements runs on the workspace (two such stages in one pass where there are two), all
//           shorter stages of a merge run on one block at a time in LDS.  ONE workgroup owns one step's buffer: __syncthreads() is the only ordering there is (no flags, no
//           hand-over between workgroups, no atomics).  The scan runs block by block: block totals first, chained into
//           carries in both directions, then the same register scan per block on top of its carries.
//
// The network in LDS (bitonic_merge_lds) and the scan (block_scan) are those of smart_order_stats.h, which says why the
// long stages on the workspace and the sum of ens_finish are spelled out here.
//
// DETERMINISM.  No floating-point atomics, every sum has ONE association for a given (N, form): the scans chain the
// elements of a thread, then the lanes of a wavefront, then the wavefronts (left to right for A, right to left for B);
// the terms are added per thread in position order, joined by a fixed butterfly over the lanes and a fixed chain over
// the wavefronts.  PIT_LOW and PIT_HIGH are the prefix sum AT the last position below (up to) y, written by the one thread
// that owns it.  Without weights A_i = i + 1 and B_i = M - 1 - i are exact integers and no scan is made.  The two forms
// associate differently and need not agree to the bit.
// Weights must be finite and >= 0 (checked by the caller, not here).
#include "smart_capi_internal.h"
#include "smart_matrix_common.h"
#include "smart_order_stats.h"
#include <cstdint>

namespace smart {

constexpr long kEnsCapacity = 8192;             // LDS form: 8192 * (8 + 2) bytes = 80 KiB of the 160 KiB of a compute unit
constexpr int kEnsBlock = 4096;                 // global form: elements of one LDS block, (8 + 8) bytes each = 64 KiB
constexpr int kEnsGlobalThreads = 1024;
constexpr long kEnsMaxSamples = 1l << 24;
static_assert(kEnsCapacity <= 65536, "sample indices are kept as 16-bit numbers");

// the first position of sorted keys[0 .. n) that holds the padding = the number of live members
__device__ inline int ens_live(const unsigned long long *keys, int n)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] == kKeyPad)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// ---- the terms ----------------------------------------------------------------------------------------------------
struct EnsSums {
    double crps, spread, mean;
};

// what sorted position i gives: its share of the mean, the PIT where it is the last position below (up to) y, and, where
// a live position follows, the terms of the gap between the two.  x, x_next: the values at i and i + 1; w, A, B: the
// weight, the inclusive prefix and the exclusive suffix at i.
__device__ inline void ens_position(double x, double x_next, bool has_next, double w, double A, double B, double W, double y,
                                    bool have_y, EnsSums &s, double *pit)
{
    s.mean += w * x;
    if (have_y) {
        if (x < y && !(has_next && x_next < y))
            pit[0] = A;
        if (x <= y && !(has_next && x_next <= y))
            pit[1] = A;
    }
    if (has_next) {
        const double P = A / W, Q = B / W;
        s.spread += (x_next - x) * P * Q;
        if (have_y) {
            const double m = fmin(fmax(y, x), x_next);
            s.crps += (m - x) * P * P + (x_next - m) * Q * Q;
        }
    }
}

// the workgroup's sums (fixed butterfly over the lanes, fixed chain over the wavefronts) and the step's five columns
template <int WAVES>
__device__ inline void ens_finish(EnsSums s, double W, int M, unsigned long long key_first, unsigned long long key_last,
                                  double y, bool have_y, const double *pit, double (*red)[16], long R, long r,
                                  double *__restrict__ out)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    double v[3] = {s.crps, s.spread, s.mean};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1)
            v[c] += __shfl_xor(v[c], d, kWave);
        if (lane == 0)
            red[c][wave] = v[c];
    }
    __syncthreads();    // (publishes pit[] as well)
    if (threadIdx.x != 0)
        return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double t = red[c][0];
        for (int x = 1; x < WAVES; ++x)
            t += red[c][x];
        v[c] = t;
    }
    const double nan = quiet_nan();
    double o[SMART_ENSEMBLE_SCORE_COLS] = {nan, nan, nan, nan, nan};
    if (M > 0 && W > 0.0 && key_first > kKeyMinusInf && key_last < kKeyPlusInf) {
        const double x_first = key_value(key_first), x_last = key_value(key_last);
        o[SMART_ENS_SPREAD] = v[1];
        o[SMART_ENS_MEAN] = v[2] / W;
        if (have_y) {
            o[SMART_ENS_CRPS] = fmax(x_first - y, 0.0) + fmax(y - x_last, 0.0) + v[0];
            o[SMART_ENS_PIT_LOW] = pit[0] / W;
            o[SMART_ENS_PIT_HIGH] = pit[1] / W;
        }
    }
#pragma unroll
    for (int c = 0; c < SMART_ENSEMBLE_SCORE_COLS; ++c)
        out[(long)c * R + r] = o[c];
}

// ---- LDS form -----------------------------------------------------------------------------------------------------
template <int CAP, int THREADS, bool WEIGHTED>
__global__ __launch_bounds__(THREADS) void smart_ensemble_scores_lds(int N, long R, const double *__restrict__ sim, long ld,
                                                                     const double *__restrict__ weights,
                                                                     const double *__restrict__ obs, double *__restrict__ out)
{
    constexpr int E = CAP / THREADS;
    constexpr int WAVES = THREADS / kWave;
    static_assert(CAP % THREADS == 0 && THREADS % kWave == 0 && WAVES <= 16 && CAP <= kEnsCapacity, "shape");
    __shared__ unsigned long long keys[CAP];
    __shared__ unsigned short idx[WEIGHTED ? CAP : 1];
    __shared__ double wave_l[16], wave_r[16], red[3][16], pit[2];
    __shared__ int live;

    const int tid = threadIdx.x;
    const long r = blockIdx.x;
    const double *row = sim + r * ld;

    for (int n = tid; n < CAP; n += THREADS) {
        unsigned long long key = kKeyPad;
        if (n < N && (!WEIGHTED || weights[n] > 0.0))
            key = value_key(row[n]);
        keys[n] = key;
        if constexpr (WEIGHTED)
            idx[n] = (unsigned short)n;
    }
    if (tid == 0)
        pit[0] = pit[1] = 0.0;
    __syncthreads();
    for (int k = 2; k <= CAP; k <<= 1)
        bitonic_merge_lds<CAP, THREADS, WEIGHTED, unsigned short>(keys, idx, k, k >> 1, 0);
    if (tid == 0)
        live = WEIGHTED ? ens_live(keys, CAP) : N;
    __syncthreads();
    const int M = live;

    const double y = obs ? obs[r] : quiet_nan();
    const bool have_y = is_finite_bits(y);
    double a[E], b[E], w[E], W;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        if constexpr (WEIGHTED)
            w[e] = i < M ? weights[idx[i]] : 0.0;
        else
            w[e] = 1.0;
        a[e] = w[e];
    }
    if constexpr (WEIGHTED) {
        double tot_r;
        block_scan<E, WAVES, true>(a, b, wave_l, wave_r, W, tot_r);
    } else {
        W = (double)M;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            a[e] = (double)(tid * E + e + 1);
            b[e] = (double)(M - 1 - (tid * E + e));
        }
    }
    EnsSums s = {0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        if (i < M) {
            const bool has_next = i + 1 < M;
            ens_position(key_value(keys[i]), has_next ? key_value(keys[i + 1]) : 0.0, has_next, w[e], a[e], b[e], W, y,
                         have_y, s, pit);
        }
    }
    ens_finish<WAVES>(s, W, M, keys[0], keys[M > 0 ? M - 1 : 0], y, have_y, pit, red, R, r, out);
}

// ---- global form --------------------------------------------------------------------------------------------------
// the workspace of step r0 + blockIdx.x: P keys, then (with weights) P weights
template <bool WEIGHTED>
__global__ __launch_bounds__(kEnsGlobalThreads) void smart_ensemble_scores_global(int N, int P, long R, long r0,
                                                                                  const double *__restrict__ sim, long ld,
                                                                                  const double *__restrict__ weights,
                                                                                  const double *__restrict__ obs,
                                                                                  double *__restrict__ out,
                                                                                  unsigned long long *workspace)
{
    constexpr int THREADS = kEnsGlobalThreads;
    constexpr int E = kEnsBlock / THREADS;
    constexpr int WAVES = THREADS / kWave;
    static_assert(kEnsBlock % THREADS == 0 && WAVES <= 16, "shape");
    __shared__ unsigned long long lk[kEnsBlock];
    __shared__ double lw[WEIGHTED ? kEnsBlock : 1];
    __shared__ double wave_l[16], wave_r[16], red[3][16], pit[2];
    __shared__ double total;
    __shared__ int live;

    const int tid = threadIdx.x;
    const long r = r0 + blockIdx.x;
    const double *row = sim + r * ld;
    unsigned long long *kg = workspace + (long)blockIdx.x * P * (WEIGHTED ? 2 : 1);
    double *wg = (double *)(kg + P);    // (not there without weights, and never touched then)
    const int blocks = P / kEnsBlock;

    if (tid == 0)
        pit[0] = pit[1] = 0.0;
    // every block of kEnsBlock elements sorted in LDS, ascending or descending by its place in the sequence
    for (int blk = 0; blk < blocks; ++blk) {
        const int g0 = blk * kEnsBlock;
        for (int t = tid; t < kEnsBlock; t += THREADS) {
            const int n = g0 + t;
            unsigned long long key = kKeyPad;
            double wn = 0.0;
            if (n < N) {
                if constexpr (WEIGHTED)
                    wn = weights[n];
                if (!WEIGHTED || wn > 0.0)
                    key = value_key(row[n]);
                else
                    wn = 0.0;
            }
            lk[t] = key;
            if constexpr (WEIGHTED)
                lw[t] = wn;
        }
        __syncthreads();
        for (int k = 2; k <= kEnsBlock; k <<= 1)
            bitonic_merge_lds<kEnsBlock, THREADS, WEIGHTED, double>(lk, lw, k, k >> 1, g0);
        for (int t = tid; t < kEnsBlock; t += THREADS) {
            kg[g0 + t] = lk[t];
            if constexpr (WEIGHTED)
                wg[g0 + t] = lw[t];
        }
        __syncthreads();
    }
    // the merges beyond a block: long stages on the workspace, the short ones block by block in LDS
    for (int k = 2 * kEnsBlock; k <= P; k <<= 1) {
        int j = k >> 1;
        // two long stages in one pass over the workspace while both reach past a block: a thread holds the four elements
        // that the stages j and j / 2 pair among themselves -- (0, 2), (1, 3), then (0, 1), (2, 3) -- at base + {0, j / 2,
        // j, j + j / 2}, base running over the positions whose bits j and j / 2 are clear; k > j, so one direction for all
        for (; (j >> 1) >= kEnsBlock; j >>= 2) {
            const int h = j >> 1;
            for (int t = tid; t < P / 4; t += THREADS) {
                const int low = t & (h - 1);
                const int base = ((t - low) << 2) | low;
                const bool up = (base & k) == 0;
                const int at[4] = {base, base + h, base + j, base + j + h};
                unsigned long long key[4];
                double wv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    key[e] = kg[at[e]];
                    if constexpr (WEIGHTED)
                        wv[e] = wg[at[e]];
                }
                auto exchange = [&](int a, int b) {
                    if ((key[a] > key[b]) == up) {
                        const unsigned long long kt = key[a];
                        key[a] = key[b];
                        key[b] = kt;
                        if constexpr (WEIGHTED) {
                            const double wt = wv[a];
                            wv[a] = wv[b];
                            wv[b] = wt;
                        }
                    }
                };
                exchange(0, 2), exchange(1, 3), exchange(0, 1), exchange(2, 3);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    kg[at[e]] = key[e];
                    if constexpr (WEIGHTED)
                        wg[at[e]] = wv[e];
                }
            }
            __syncthreads();
        }
        for (; j >= kEnsBlock; j >>= 1) {
            for (int t = tid; t < P / 2; t += THREADS) {
                const int i = 2 * t - (t & (j - 1));
                const int l = i + j;
                const bool up = (i & k) == 0;
                const unsigned long long ka = kg[i], kb = kg[l];
                if ((ka > kb) == up) {
                    kg[i] = kb;
                    kg[l] = ka;
                    if constexpr (WEIGHTED) {
                        const double wa = wg[i];
                        wg[i] = wg[l];
                        wg[l] = wa;
                    }
                }
            }
            __syncthreads();
        }
        for (int blk = 0; blk < blocks; ++blk) {
            const int g0 = blk * kEnsBlock;
            for (int t = tid; t < kEnsBlock; t += THREADS) {
                lk[t] = kg[g0 + t];
                if constexpr (WEIGHTED)
                    lw[t] = wg[g0 + t];
            }
            __syncthreads();
            bitonic_merge_lds<kEnsBlock, THREADS, WEIGHTED, double>(lk, lw, k, kEnsBlock >> 1, g0);
            for (int t = tid; t < kEnsBlock; t += THREADS) {
                kg[g0 + t] = lk[t];
                if constexpr (WEIGHTED)
                    wg[g0 + t] = lw[t];
            }
            __syncthreads();
        }
    }
    if (tid == 0)
        live = WEIGHTED ? ens_live(kg, P) : N;
    __syncthreads();
    const int M = live;
    const int chunks = (M + kEnsBlock - 1) / kEnsBlock;     // the blocks that hold a live member

    const double y = obs ? obs[r] : quiet_nan();
    const bool have_y = is_finite_bits(y);
    double W = (double)M;
    // with weights: the totals of every block in both directions (the LDS of the network is free now: lw and lk hold
    // them), chained into what lies before and behind every block
    double *carry_l = lw, *carry_r = reinterpret_cast<double *>(lk);
    if constexpr (WEIGHTED) {
        for (int c = 0; c < chunks; ++c) {
            double a[E], b[E], tot_l, tot_r;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = c * kEnsBlock + tid * E + e;
                a[e] = i < M ? wg[i] : 0.0;
            }
            block_scan<E, WAVES, true>(a, b, wave_l, wave_r, tot_l, tot_r);
            if (tid == 0) {
                carry_l[c] = tot_l;
                carry_r[c] = tot_r;
            }
        }
        __syncthreads();
        if (tid == 0) {
            double run = 0.0;
            for (int c = 0; c < chunks; ++c) {
                const double t = carry_l[c];
                carry_l[c] = run;
                run += t;
            }
            total = run;
            run = 0.0;
            for (int c = chunks - 1; c >= 0; --c) {
                const double t = carry_r[c];
                carry_r[c] = run;
                run += t;
            }
        }
        __syncthreads();
        W = total;
    }
    EnsSums s = {0.0, 0.0, 0.0};
    for (int c = 0; c < chunks; ++c) {
        double a[E], b[E], w[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = c * kEnsBlock + tid * E + e;
            if constexpr (WEIGHTED)
                w[e] = i < M ? wg[i] : 0.0;
            else
                w[e] = 1.0;
            a[e] = w[e];
        }
        if constexpr (WEIGHTED) {
            double tot_l, tot_r;
            block_scan<E, WAVES, true>(a, b, wave_l, wave_r, tot_l, tot_r);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                a[e] = carry_l[c] + a[e];
                b[e] = carry_r[c] + b[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = c * kEnsBlock + tid * E + e;
                a[e] = (double)(i + 1);
                b[e] = (double)(M - 1 - i);
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = c * kEnsBlock + tid * E + e;
            if (i < M) {
                const bool has_next = i + 1 < M;
                ens_position(key_value(kg[i]), has_next ? key_value(kg[i + 1]) : 0.0, has_next, w[e], a[e], b[e], W, y,
                             have_y, s, pit);
            }
        }
    }
    ens_finish<WAVES>(s, W, M, kg[0], kg[M > 0 ? M - 1 : 0], y, have_y, pit, red, R, r, out);
}

// ---- launch (validated by smart_analysis_capi.hip) -------------------------------------------------------------------
long ensemble_scores_lds_capacity() { return kEnsCapacity; }

long ensemble_scores_max_samples() { return kEnsMaxSamples; }

long ensemble_scores_step_bytes(long N, bool weighted) { return padded_pow2(N, kEnsBlock) * (weighted ? 16 : 8); }

void launch_ensemble_scores(long N, long R, const double *sim, long ld, const double *weights, const double *obs,
                            double *out, bool lds, void *workspace, long workspace_bytes, hipStream_t s)
{
    if (lds) {
        sort_instance<(int)kEnsCapacity>(N, [&](auto cap, auto threads) {
            const dim3 grid((unsigned)R);
            if (weights)
                hipLaunchKernelGGL((smart_ensemble_scores_lds<cap(), threads(), true>), grid, dim3(threads()), 0, s, (int)N,
                                   R, sim, ld, weights, obs, out);
            else
                hipLaunchKernelGGL((smart_ensemble_scores_lds<cap(), threads(), false>), grid, dim3(threads()), 0, s,
                                   (int)N, R, sim, ld, weights, obs, out);
        });
        return;
    }
    // report steps in batches of as many as the workspace holds, one launch per batch
    const long P = padded_pow2(N, kEnsBlock);
    const long batch = workspace_steps(workspace_bytes, ensemble_scores_step_bytes(N, weights != nullptr));
    for_each_batch(R, batch, [&](long r0, long steps) {
        if (weights)
            hipLaunchKernelGGL((smart_ensemble_scores_global<true>), dim3((unsigned)steps), dim3(kEnsGlobalThreads), 0, s,
                               (int)N, (int)P, R, r0, sim, ld, weights, obs, out, (unsigned long long *)workspace);
        else
            hipLaunchKernelGGL((smart_ensemble_scores_global<false>), dim3((unsigned)steps), dim3(kEnsGlobalThreads), 0, s,
                               (int)N, (int)P, R, r0, sim, ld, weights, obs, out, (unsigned long long *)workspace);
    });
}

} // namespace smart
