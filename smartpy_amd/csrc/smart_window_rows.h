// smart_window_rows.h -- "the valid rows of window w, in row order": what the kernels that walk a window of a stored
// discharge matrix sim[R][ld] share (smart_objfn_windows, smart_bootstrap_moments, smart_signatures, smart_fdc_observed,
// smart_fdc_sort).  Every one of them looks at window[] / obs[] in chunks of 1,024 rows, kSub rows per thread of a
// workgroup of kWaves wavefronts, and lists the rows it wants in an LDS list of its own; the two moment kernels then walk
// that list and add their wavefronts' partial moments in the same way.
#pragma once

#include "smart_matrix_common.h"
#include <type_traits>

namespace smart {

// ---- the geometry of the two moment kernels (smart_objfn_windows, smart_bootstrap_moments)
constexpr int kWinWaves = 8;                      // wavefronts per workgroup, all on the same 64 samples
constexpr int kWinThreads = kWinWaves * kWave;
constexpr int kWinChunk = 1024;                   // rows of window[] looked at per compaction
constexpr int kWinSub = kWinChunk / kWinThreads;  // ... rows per thread in it
constexpr int kWinUnroll = 4;                     // row segments in flight per lane

// The rows r of [c0, c0 + kSub * kWaves * 64) below R for which valid(r, k) holds, listed IN ROW ORDER: thread t tests
// row c0 + k * threads + t in slot k (and may keep a payload of that row in registers of its caller, indexed by k); a row
// that passes is handed to place(pos, r, k), pos its place in the list -- sub-chunk after sub-chunk, wavefront after
// wavefront, lane after lane, which is ascending r.  Ballots and prefix counts through cnt[kSub][kWaves], no atomics: the
// list is a function of (R, the window array, the observations) alone, which is what makes the callers' sums
// deterministic, and for smart_signatures it is the time order its recurrences need.  -> the number of entries,
// wave-uniform (a scalar).
// TWO BARRIERS per call: one behind the counts, one behind place() -- what place() wrote is visible to every thread on
// return.  Towards the next call the caller owes nothing for cnt[] (its next writes come after the second barrier, its next
// reads after the next first one) and ONE thing for its list: a barrier between its last read of the list and the next
// call's place() -- the next call's first barrier is one, so a caller whose threads read the list only before they enter
// the next call needs none of its own.
// wr is the caller's wavefront number, threadIdx.x / 64.  The kernels of 4 and 8 wavefronts pass it as a scalar
// (readfirstlane), formed ONCE in front of their chunk loop: the kWaves compares against it then leave the loop as scalar
// selects (a readfirstlane in here stays inside the loop with them; measured: slower).  With the 16 wavefronts of the flow
// duration kernels the plain vector value measured faster, and is what fdc_compact passes.
template <int kWaves, int kSub, class Valid, class Place>
__device__ __forceinline__ int list_rows(long c0, long R, int wr, int (*cnt)[kWaves], Valid valid, Place place)
{
    constexpr int kThreads = kWaves * kWave;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    bool in[kSub];
    unsigned long long votes[kSub];
#pragma unroll
    for (int k = 0; k < kSub; ++k) {
        const long r = c0 + k * kThreads + tid;
        in[k] = r < R && valid(r, k);
        votes[k] = __ballot(in[k]);
        if (lane == 0)
            cnt[k][wr] = __popcll(votes[k]);
    }
    __syncthreads();
    int m = 0; // list entries so far
#pragma unroll
    for (int k = 0; k < kSub; ++k) {
        int before = 0, all = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) {
            const int c = cnt[k][v];
            all += c;
            before += v < wr ? c : 0;
        }
        if (in[k])
            place(m + before + __popcll(votes[k] & ((1ull << lane) - 1ull)), c0 + k * kThreads + tid, k);
        m += all;
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(m);
}

// The walk of the moment kernels over a list of m entries (rows[], fes[] = f(obs) of the row): the wavefronts take the
// entries round-robin from j on (j = the wavefront's number, or one round further where it has taken entry 0 already),
// kWinUnroll row segments (512 contiguous bytes each) in flight per lane, then the tail; add(fe, f(sim)) per entry.  The
// row of an entry is wave-uniform (readfirstlane): the address arithmetic of a load is scalar.
template <int T, class Add>
__device__ __forceinline__ void walk_listed_rows(int j, int m, const int *rows, const double *fes, const double *col, long ld,
                                                 double eps, Add add)
{
    for (; j + (kWinUnroll - 1) * kWinWaves < m; j += kWinUnroll * kWinWaves) {
        double s[kWinUnroll];
#pragma unroll
        for (int k = 0; k < kWinUnroll; ++k)
            s[k] = col[(long)__builtin_amdgcn_readfirstlane(rows[j + k * kWinWaves]) * ld];
#pragma unroll
        for (int k = 0; k < kWinUnroll; ++k)
            add(fes[j + k * kWinWaves], flow_transform(T, s[k], eps));
    }
    for (; j < m; j += kWinWaves)
        add(fes[j], flow_transform(T, col[(long)__builtin_amdgcn_readfirstlane(rows[j]) * ld], eps));
}

// The five partial moments of kWaves wavefronts on the same 64 samples, added through part[kWaves][5][64] in wavefront
// order: mo[] of wavefront wr goes in; -> true in the `live` lanes of wavefront 0, which then have the sums in mo[], false
// in every other lane, which has nothing more to do.
template <int kWaves>
__device__ __forceinline__ bool sum_wave_moments(double (&mo)[5], double (*part)[5][kWave], int wr, int lane, bool live)
{
#pragma unroll
    for (int k = 0; k < 5; ++k)
        part[wr][k][lane] = mo[k];
    __syncthreads();
    if (wr != 0 || !live)
        return false;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double t = part[0][k][lane];
#pragma unroll
        for (int v = 1; v < kWaves; ++v)
            t += part[v][k][lane];
        mo[k] = t;
    }
    return true;
}

// host side: f(the transform as a compile-time constant) -- f a generic lambda that launches `kernel<decltype(t)::value>`
template <class F>
void with_transform(int transform, F f)
{
    switch (transform) {
    case SMART_TRANSFORM_SQRT:
        f(std::integral_constant<int, SMART_TRANSFORM_SQRT>());
        break;
    case SMART_TRANSFORM_LOG:
        f(std::integral_constant<int, SMART_TRANSFORM_LOG>());
        break;
    case SMART_TRANSFORM_INVERSE:
        f(std::integral_constant<int, SMART_TRANSFORM_INVERSE>());
        break;
    default:
        f(std::integral_constant<int, SMART_TRANSFORM_NONE>());
    }
}

} // namespace smart
