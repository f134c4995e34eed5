// smart_matrix_common.h -- what the kernels that read a stored discharge matrix sim[R][ld] share (smart_objfn_matrix,
// smart_objfn_windows, smart_fdc_*, smart_signatures, smart_quantiles_*, smart_sobol_*, smart_bootstrap_*), and the few
// constants and bit tests every kernel of the library takes from ONE definition (smart_device.h includes this file).  No
// arithmetic of the model lives here.  What the kernels that walk the rows of a WINDOW share on top of it -- the in-order
// row list, the walk over it, the reduction of the partial moments -- is smart_window_rows.h.
#pragma once

#include "../../include/smart_amd.h"
#include <hip/hip_runtime.h>

namespace smart {

constexpr int kWave = 64;

// NaN test on the bit pattern (missing observation / absent constraint): survives -fno-honor-nans, and for the
// wave-uniform values it is applied to it is scalar integer work.
__device__ __forceinline__ bool is_nan_bits(double x)
{
    return (__builtin_bit_cast(unsigned long long, x) & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

// neither a NaN nor an infinity (exponent bits not all ones)
__device__ __forceinline__ bool is_finite_bits(double x)
{
    return (__builtin_bit_cast(unsigned long long, x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// a quiet NaN that does not trip -fno-honor-nans diagnostics (the fast kernels never do arithmetic on one)
__host__ __device__ __forceinline__ double quiet_nan() { return __builtin_bit_cast(double, 0x7ff8000000000000ull); }

// What smart_obs_prepare writes for the deviation e - mean of a MISSING observation: a NaN whose payload no arithmetic
// produces (a computed NaN is the canonical 0x7ff8000000000000, or carries the payload of an input NaN -- and an
// observation that is a NaN is missing whatever its payload).  A report every step tells a missing observation from the
// upper half of the deviation it has in a scalar register anyway: one s_cmp_eq_u32 (the exact NaN test of the
// observation itself in 32-bit pieces was eleven scalar instructions a step in hipcc's hands).
constexpr unsigned long long kMissingObs = 0x7ff8dead00000000ull;
__device__ __forceinline__ bool is_missing_mark(double w)
{
    return (unsigned)(__builtin_bit_cast(unsigned long long, w) >> 32) == (unsigned)(kMissingObs >> 32);
}

// the flow transforms SMART_TRANSFORM_* of the low-flow scores: x, sqrt x, ln(x + eps), 1 / (x + eps).  A kernel that is
// compiled per transform calls it with its constant.
__device__ __forceinline__ double flow_transform(int t, double x, double eps)
{
    switch (t) {
    case SMART_TRANSFORM_SQRT:
        return sqrt(x);
    case SMART_TRANSFORM_LOG:
        return log(x + eps);
    case SMART_TRANSFORM_INVERSE:
        return 1.0 / (x + eps);
    default:
        return x;
    }
}

// the probabilities of a launch, passed by value (unused entries 0)
struct MatrixProbs {
    double q[SMART_QUANTILES_MAX_PROBS];
};

// ---- block reduction helper (256 threads), deterministic order -----------------------------------------
__device__ inline double block_sum(double v, double *sh)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (tid < s)
            sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// statistics of one observation series (NaN = missing, montecarlo.py:195-196): st[0..4] = n, mean, sum,
// sum((e-mean)^2), sum(e-mean); dev[r] = e[r] - mean where kDev -- and kMissingObs where e[r] is missing: a NaN of a
// payload no arithmetic produces, so that a kernel with a report every step can tell a missing observation by ONE 32-bit
// scalar compare on the deviation it loads anyway (Reporter's other users test e itself and never read dev then).
// kDev says at compile time whether dev is written: a unit whose every call passes no dev would otherwise have the
// argument folded into the function before it is inlined, and its callers scheduled differently from the other unit's.
template <bool kDev>
__device__ inline void obs_stats(const double *obs, long R, double *st, double *dev, double *sh)
{
    double cnt = 0.0, s = 0.0;
    for (long r = threadIdx.x; r < R; r += blockDim.x) {
        const double e = obs[r];
        if (!is_nan_bits(e)) {
            cnt += 1.0;
            s += e;
        }
    }
    cnt = block_sum(cnt, sh);
    s = block_sum(s, sh);
    const double mean = s / cnt;
    double s2 = 0.0, s1 = 0.0;
    for (long r = threadIdx.x; r < R; r += blockDim.x) {
        const double e = obs[r];
        const bool missing = is_nan_bits(e);
        const double d = !missing ? e - mean : 0.0;
        s2 += d * d;
        s1 += d;
        if constexpr (kDev)
            dev[r] = missing ? __builtin_bit_cast(double, kMissingObs) : d;
    }
    s2 = block_sum(s2, sh);
    s1 = block_sum(s1, sh);
    st[0] = cnt;
    st[1] = mean;
    st[2] = s;
    st[3] = s2;
    st[4] = s1;
}

// the first report step that carries an observation (0 where none does): the row whose value is the constant of a
// sample's one-pass moments (finish_objectives, smart_device.h).  Every thread of the workgroup gets the same answer.  The
// workgroup looks at blockDim.x rows at a time -- one round finds it unless that many leading reports are all missing --
// every wavefront names the first of its 64 by a ballot, and the smallest of those goes through LDS (an index held in a
// double is exact; a minimum does not depend on the order it is taken in): two barriers a round, where a tree over the
// threads would take ten.  blockDim.x is a multiple of 64, sh holds one double per wavefront.  (With R < 1 there is no
// round and no barrier: a caller that relies on one for its own shared values places it itself.)
__device__ inline long first_observed_row(const double *obs, long R, double *sh)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, waves = blockDim.x / kWave;
    for (long base = 0; base < R; base += blockDim.x) {
        const long r = base + tid;
        const unsigned long long seen = __ballot(r < R && !is_nan_bits(obs[r]));
        if (lane == 0)
            sh[wave] = seen ? (double)(base + wave * kWave + __builtin_ctzll(seen)) : (double)R;
        __syncthreads();
        double first = sh[0];
        for (int w = 1; w < waves; ++w)
            first = sh[w] < first ? sh[w] : first;
        __syncthreads(); // (sh is free again)
        if (first < (double)R)
            return (long)first;
    }
    return 0;
}

} // namespace smart
