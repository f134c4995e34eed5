// smart_key_select.h -- the k-th smallest of N order-preserving keys (smart_order_keys.h) by BISECTION OVER THE KEY SPACE
// with INTEGER counts: between the smallest and the largest key that takes part, a round reads the keys once and counts
// those <= a threshold.  The scheme of smart_quantiles_select and smart_fdc_select, whose sums are of weights (doubles, in
// a fixed order, one threshold per probability); a count is an integer, so here no order matters, nothing rounds, and a
// round can afford SEVEN thresholds for its one read: they cut the interval into eight parts, three bits of the key per
// read instead of one -- 22 reads of the keys for a full-width interval, not 64.  One workgroup of THREADS threads calls
// these together; every thread gets the same answer.
#pragma once
#include "smart_matrix_common.h"
#include "smart_order_keys.h"

namespace smart {

constexpr int kSelectCuts = 7;

// how many n of 0 .. N-1 satisfy pred(n), the same number in every thread (N < 2^31).  sh: THREADS / kWave counters.
template <int THREADS, typename Pred>
__device__ inline unsigned block_count(Pred pred, long N, unsigned *sh)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned c = 0;
    for (long n = threadIdx.x; n < N; n += THREADS)
        c += pred(n) ? 1u : 0u;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1)
        c += __shfl_xor(c, d, kWave);
    if (lane == 0)
        sh[wave] = c;
    __syncthreads();
    c = 0;
    for (int v = 0; v < THREADS / kWave; ++v)
        c += sh[v];
    __syncthreads();    // sh may be written again
    return c;
}

// a key that is the same in every lane, as a scalar
__device__ inline unsigned long long uniform_key(unsigned long long k)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(k >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// the smallest key v in [kmin, kmax] with #{ n : key_at(n) <= v } >= k.  The caller guarantees that the count at kmax
// reaches k (kmax is the largest key that takes part, k at most their number); keys above kmax are never counted.
// sh: kSelectCuts * (THREADS / kWave) counters.
// A round: with q = max(1, (hi - lo) / 8) the thresholds m_j = min(hi, lo + (j + 1) q - 1), j = 0 .. 6, end the first seven
// parts of q keys (what is left is the eighth).  The first m_j whose count reaches k becomes hi and the threshold before it,
// plus one, lo; if none does, lo moves past m_6 -- which lies below hi then, since the count at hi reaches k.  An interval
// of c keys leaves at most c / 8 + 7.
template <int THREADS, typename KeyAt>
__device__ inline unsigned long long select_kth_key(KeyAt key_at, long N, unsigned k, unsigned long long kmin,
                                                    unsigned long long kmax, unsigned *sh)
{
    constexpr int WAVES = THREADS / kWave;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned long long lo = uniform_key(kmin), hi = uniform_key(kmax);
    while (lo < hi) {
        unsigned long long q = (hi - lo) >> 3;
        q = q < 1 ? 1 : q;
        unsigned long long m[kSelectCuts];
        unsigned c[kSelectCuts];
#pragma unroll
        for (int j = 0; j < kSelectCuts; ++j) {
            const unsigned long long off = (unsigned long long)(j + 1) * q - 1;    // <= 7 q - 1 <= hi - lo: no wrap
            m[j] = off < hi - lo ? lo + off : hi;
            c[j] = 0;
        }
        for (long n = threadIdx.x; n < N; n += THREADS) {
            const unsigned long long key = key_at(n);
#pragma unroll
            for (int j = 0; j < kSelectCuts; ++j)
                c[j] += key <= m[j] ? 1u : 0u;
        }
#pragma unroll
        for (int j = 0; j < kSelectCuts; ++j) {
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1)
                c[j] += __shfl_xor(c[j], d, kWave);
            if (lane == 0)
                sh[j * WAVES + wave] = c[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kSelectCuts; ++j) {
            unsigned t = 0;
            for (int v = 0; v < WAVES; ++v)
                t += sh[j * WAVES + v];
            c[j] = (unsigned)__builtin_amdgcn_readfirstlane((int)t);    // the same in every lane: lo, hi and m stay scalar
        }
        __syncthreads();    // sh may be written again
        bool found = false;
#pragma unroll
        for (int j = 0; j < kSelectCuts; ++j) {
            if (!found && c[j] >= k) {
                found = true;
                hi = m[j];
                if (j > 0)
                    lo = m[j - 1] + 1;
            }
        }
        if (!found)
            lo = m[kSelectCuts - 1] + 1;
    }
    return hi;
}

} // namespace smart
