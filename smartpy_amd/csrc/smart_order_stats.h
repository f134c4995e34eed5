// smart_order_stats.h -- the WORKGROUP PRIMITIVES that the kernels which SORT along the sample axis share, each defined
// ONCE: the bitonic network in LDS over 64-bit keys (smart_order_keys.h) with a payload, and the scan of the weights in
// sorted order.  Their order of operations is what the determinism of those kernels rests on.  Users:
// smart_quantiles_sort (network, forward scan), smart_ensemble_scores_lds / _global (network, scan in both
// directions) and smart_pawn_lds / _global (network with the sample index as payload; the long stages of a merge on a
// workspace, bitonic_long_stages).  One workgroup of THREADS threads calls these together.
//
// NOT HERE, on purpose:
//   fdc_sort (smart_flow_duration.hip) sorts along TIME, one column per lane group: it interleaves the columns in LDS and
//       keeps its sub-wavefront stages in registers through lane exchanges.  That layout was chosen from measurements
//       and shares nothing with a network that has one row per workgroup; it stays where it is.
//   The long stages of smart_ensemble_scores_global spell the four-element exchange out once more, on the workspace:
//       with that text shared the ensemble kernels compute the same bits from another instruction schedule; as they
//       stand they are the code they were, instruction for instruction.
//   The workgroup sums (select_block_sums, block_count, select_kth_key, the S sum of smart_dynia_shares, ens_finish) and
//       the key range of smart_quantiles_select and smart_dynia_shares stay with their kernels for the same reason:
//       folded into one function here, smart_dynia_hip measured 0.2 - 1 % slower than before at N = 1e4 and 1e5.
#pragma once
#include "smart_matrix_common.h"
#include "smart_order_keys.h"

namespace smart {

// ---- the network --------------------------------------------------------------------------------------------------
// the stages j = j_first, j_first / 2, ... 1 of the merge k on CAP elements in LDS that stand at g0 .. g0 + CAP of the
// whole sequence (the direction of a pair is a bit of its position in the WHOLE sequence).  The payload follows its key.
// TWO STAGES A PASS: a thread holds the four elements that the stages j and j / 2 pair among themselves -- (0, 2), (1, 3),
// then (0, 1), (2, 3) -- at base + {0, j / 2, j, j + j / 2}, base running over the positions whose bits j and j / 2 are
// clear (k > j: one direction for all four).  Every element is read once and written once for two stages, and half the
// barriers are gone; a last stage j = 1 that has no partner runs alone.
template <int CAP, int THREADS, bool PAYLOAD, typename T>
__device__ inline void bitonic_merge_lds(unsigned long long *keys, T *pay, int k, int j_first, int g0)
{
    int j = j_first;
    for (; j >= 2; j >>= 2) {
        const int h = j >> 1;
        for (int t = threadIdx.x; t < CAP / 4; t += THREADS) {
            const int low = t & (h - 1);
            const int base = ((t - low) << 2) | low;
            const bool up = ((g0 + base) & k) == 0;
            const int at[4] = {base, base + h, base + j, base + j + h};
            unsigned long long key[4];
            T pv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                key[e] = keys[at[e]];
                if constexpr (PAYLOAD)
                    pv[e] = pay[at[e]];
            }
            auto exchange = [&](int a, int b) {
                if ((key[a] > key[b]) == up) {
                    const unsigned long long kt = key[a];
                    key[a] = key[b];
                    key[b] = kt;
                    if constexpr (PAYLOAD) {
                        const T pt = pv[a];
                        pv[a] = pv[b];
                        pv[b] = pt;
                    }
                }
            };
            exchange(0, 2), exchange(1, 3), exchange(0, 1), exchange(2, 3);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                keys[at[e]] = key[e];
                if constexpr (PAYLOAD)
                    pay[at[e]] = pv[e];
            }
        }
        __syncthreads();
    }
    if (j == 1) {
        for (int t = threadIdx.x; t < CAP / 2; t += THREADS) {
            const int i = 2 * t;
            const bool up = ((g0 + i) & k) == 0;
            const unsigned long long a = keys[i], b = keys[i + 1];
            if ((a > b) == up) {
                keys[i] = b;
                keys[i + 1] = a;
                if constexpr (PAYLOAD) {
                    const T pa = pay[i];
                    pay[i] = pay[i + 1];
                    pay[i + 1] = pa;
                }
            }
        }
        __syncthreads();
    }
}

// the LONG stages j = k / 2, k / 4, ... BLOCK of the merge k on P elements in memory (kg: keys, pg: the payload that
// follows its key), for a network whose shorter stages run block by block in LDS (bitonic_merge_lds from BLOCK / 2 on).
// Two stages in one pass while both reach past a block, the four-element exchange of bitonic_merge_lds; a last one alone.
// ONE workgroup owns the buffer: __syncthreads() is the only ordering.  User: smart_pawn_global (32-bit sample indices);
// the ensemble kernels keep their own text of these stages (above).
template <int BLOCK, int THREADS, typename T>
__device__ inline void bitonic_long_stages(unsigned long long *kg, T *pg, int P, int k)
{
    int j = k >> 1;
    for (; (j >> 1) >= BLOCK; j >>= 2) {
        const int h = j >> 1;
        for (int t = threadIdx.x; t < P / 4; t += THREADS) {
            const int low = t & (h - 1);
            const int base = ((t - low) << 2) | low;
            const bool up = (base & k) == 0;
            const int at[4] = {base, base + h, base + j, base + j + h};
            unsigned long long key[4];
            T pv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                key[e] = kg[at[e]];
                pv[e] = pg[at[e]];
            }
            auto exchange = [&](int a, int b) {
                if ((key[a] > key[b]) == up) {
                    const unsigned long long kt = key[a];
                    key[a] = key[b];
                    key[b] = kt;
                    const T pt = pv[a];
                    pv[a] = pv[b];
                    pv[b] = pt;
                }
            };
            exchange(0, 2), exchange(1, 3), exchange(0, 1), exchange(2, 3);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                kg[at[e]] = key[e];
                pg[at[e]] = pv[e];
            }
        }
        __syncthreads();
    }
    for (; j >= BLOCK; j >>= 1) {
        for (int t = threadIdx.x; t < P / 2; t += THREADS) {
            const int i = 2 * t - (t & (j - 1));
            const int l = i + j;
            const bool up = (i & k) == 0;
            const unsigned long long ka = kg[i], kb = kg[l];
            if ((ka > kb) == up) {
                kg[i] = kb;
                kg[l] = ka;
                const T pa = pg[i];
                pg[i] = pg[l];
                pg[l] = pa;
            }
        }
        __syncthreads();
    }
}

// ---- the scan -----------------------------------------------------------------------------------------------------
// a[e] holds the weight at position threadIdx.x * E + e of a block of E * 64 * WAVES positions.  On return a[e] is the
// INCLUSIVE prefix sum of the block at that position: the elements of a thread chained left to right, then the lanes of
// a wavefront, then the wavefronts -- a[e] = A_wave + (B_lane + L_e), each prefix the running value at the end of what
// precedes it, every chain started from 0.0 (0.0 + x is x but for the sign of a zero, which no comparison sees: both
// callers get the bits their own copies gave).  Hence a is non-decreasing along the block and stays where a weight is 0.
// With BACKWARD, b[e] is the EXCLUSIVE suffix sum as well, chained right to left in the same way.  tot_l and tot_r are
// the block's total in either direction, the same bits in every thread.  wave_l, wave_r: WAVES doubles of LDS each,
// free to be written again on return: the trailing barrier is there for the caller that scans block after block
// (smart_quantiles_sort calls once and writes cum[] behind a barrier of its own: for it this is one barrier more than its
// own copy of the scan had).
template <int E, int WAVES, bool BACKWARD>
__device__ inline void block_scan(double (&a)[E], double (&b)[E], double *wave_l, double *wave_r, double &tot_l, double &tot_r)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    double back = 0.0, fwd = 0.0;
    if constexpr (BACKWARD) {
#pragma unroll
        for (int e = E - 1; e >= 0; --e) {
            b[e] = back;
            back += a[e];
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        fwd += a[e];
        a[e] = fwd;
    }
    double before = 0.0, after = 0.0;
    for (int j = 0; j < kWave - 1; ++j) {           // the lanes to the left, chained left to right
        const double tj = __shfl(fwd, j, kWave);
        if (lane > j)
            before += tj;
    }
    if constexpr (BACKWARD) {
        for (int j = kWave - 1; j > 0; --j) {       // the lanes to the right, chained right to left
            const double tj = __shfl(back, j, kWave);
            if (lane < j)
                after += tj;
        }
    }
    if (lane == kWave - 1)
        wave_l[wave] = before + fwd;
    if (BACKWARD && lane == 0)
        wave_r[wave] = after + back;
    __syncthreads();
    double ahead = 0.0, behind = 0.0;
    tot_l = 0.0;
    tot_r = 0.0;
    for (int v = 0; v < WAVES; ++v) {
        if (v == wave)
            ahead = tot_l;
        tot_l += wave_l[v];
    }
    if constexpr (BACKWARD) {
        for (int v = WAVES - 1; v >= 0; --v) {
            if (v == wave)
                behind = tot_r;
            tot_r += wave_r[v];
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        a[e] = ahead + (before + a[e]);
        if constexpr (BACKWARD)
            b[e] = behind + (after + b[e]);
    }
    __syncthreads();    // wave_l and wave_r may be written again
}

// the forward half alone
template <int E, int WAVES>
__device__ inline void block_scan(double (&a)[E], double *wave_l)
{
    double none[E], tot_l, tot_r;
    block_scan<E, WAVES, false>(a, none, wave_l, nullptr, tot_l, tot_r);
}

} // namespace smart
