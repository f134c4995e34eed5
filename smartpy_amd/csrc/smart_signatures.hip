// smart_signatures.hip -- hydrological signatures of a stored discharge matrix sim[R][ld] (sample-minor), per sample and
// per window of report steps: what depends on the ORDER of the report steps (baseflow index, flashiness, lag-1
// autocorrelation, rising limb density, recession, the peak and its row, pulse counts and durations above and below a
// threshold), beside the mean.  The definition is the header comment of smart_signatures_hip (include/smart_amd.h).
//
// Geometry.  One lane per sample, grid = (ceil(N / 256), W), a workgroup = kSigWaves wavefronts over 256 ADJACENT samples
// of the same window.  The clamped Lyne-Hollick filter is a true recurrence along time: a lane walks every row of its
// sample, in ascending row order.  A workgroup
//   1. walks window[] and obs[] in chunks of kSigChunk rows: the window's valid rows are listed IN ROW ORDER -- the time
//      order of the recurrences -- as (row, has-pair flag) in one word in LDS (list_rows, smart_window_rows.h);
//   2. every wavefront walks the WHOLE list, each for its own 64 samples, kSigUnroll row segments (512 contiguous bytes
//      each) in flight per lane.  Rows of no window, of another window, or without an observation are never read; every
//      element of a listed row is loaded once.
// The entry of a list is wave-uniform (readfirstlane): the address arithmetic of a load is scalar, and so is everything that
// depends on the row alone -- pair or no pair, the restart of the filter, the counts m and p.  Everything that depends on
// the value is a select: rising, falling, above or below a threshold, a new peak.  No divergent branch.
//
// Arithmetic.  One log per valid row; the previous row's logarithm is kept (a recession term is ln x_r - ln x_{r-1}, taken
// only where 0 < x_r < x_{r-1}, where both logarithms are finite).  AC1 from one-pass moments of the pairs about a
// per-sample shift, the sample's FIRST valid value, as smart_objfn_windows does.  A value that is not finite needs no test
// of its own: the sum of x never becomes finite again, and ONE test of it at the end empties the (window, sample).
//
// State: sixteen doubles and eleven 32-bit counts and flags per lane, in registers for the whole walk.  With the loads in
// flight and the logarithm's temporaries hipcc takes 113 VGPRs and no scratch under __launch_bounds__(256, 4): four
// wavefronts per SIMD (left alone it takes 154, three wavefronts).  The pair is an `if` WITHOUT an else -- what a row
// without a pair restarts is set before it: an if / else on the uniform flag makes hipcc keep the old and the new
// state side by side (51 VGPRs spilled).
//
// Determinism.  No atomics; the association of every sum is the row order: two launches give the same bits.
//
// Not built: a split of the time axis across wavefronts.  The associative form of the clamped filter composes clamp-affine
// maps, which changes the bits and needs two sweeps.
#include "smart_capi_internal.h"
#include "smart_window_rows.h"

namespace smart {

constexpr int kSigWaves = 4;                      // wavefronts per workgroup, each on 64 samples of its own
constexpr int kSigThreads = kSigWaves * kWave;
constexpr int kSigChunk = 1024;                   // rows of window[] looked at per compaction
constexpr int kSigSub = kSigChunk / kSigThreads;  // ... rows per thread in it
constexpr int kSigUnroll = 8;                     // row segments in flight per lane
constexpr int kSigWavesPerSimd = 4;               // the register allocator's bound (header comment: State)

__global__ __launch_bounds__(kSigThreads, kSigWavesPerSimd) void smart_signatures(
    long N, long R, const double *__restrict__ sim, long ld, const double *__restrict__ obs,
    const int *__restrict__ window, double alpha, const double *__restrict__ pulse, double *__restrict__ sig)
{
    __shared__ int cnt[kSigSub][kSigWaves];
    __shared__ unsigned rows[kSigChunk]; // (row << 1) | has-pair: a row is below 2^31
    const int w = blockIdx.y;
    const int wr = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    long n = (long)blockIdx.x * kSigThreads + threadIdx.x;
    const bool live = n < N;
    if (!live)
        n = N - 1;
    const double *const col = sim + n;
    const double lo = pulse ? pulse[2 * w] : quiet_nan(), hi = pulse ? pulse[2 * w + 1] : quiet_nan();
    const double gain = (1.0 + alpha) / 2.0;

    // a property of the row, not of the sample
    auto valid = [&](long r) { return (!window || window[r] == w) && (!obs || !is_nan_bits(obs[r])); };

    int m = 0, p = 0;        // valid rows and pairs so far (the same in every thread)
    bool have_shift = false; // (the same in every thread)
    double shift = 0.0, prev = 0.0, prev_u = 0.0, prev_log = 0.0, quick = 0.0;
    double sum_x = 0.0, sum_base = 0.0, sum_abs = 0.0, sum_pair = 0.0, sum_rec = 0.0;
    double Sa = 0.0, Sb = 0.0, Saa = 0.0, Sbb = 0.0, Sab = 0.0;
    double peak = -__builtin_inf();
    int peak_row = 0, n_rise = 0, n_limb = 0, n_rec = 0, hi_runs = 0, hi_rows = 0, lo_runs = 0, lo_rows = 0;
    bool was_rising = false, was_above = false, was_below = false;

    auto step = [&](unsigned entry, double x) {
        const int r = (int)(entry >> 1);
        const bool pair = entry & 1u; // row r - 1 is valid, and it was the entry before this one (the same in every lane)
        const double lx = log(x), u = x - shift;
        const bool above = x > hi, below = x < lo, top = x > peak;
        const bool rising = pair && x > prev;
        sum_x += x;
        peak_row = top ? r : peak_row;
        peak = top ? x : peak;
        // without a pair -- the window's first row, or the first after a gap -- the limbs and the runs start again ...
        n_rise += rising ? 1 : 0;
        n_limb += rising && !was_rising ? 1 : 0;
        hi_runs += above && !(pair && was_above) ? 1 : 0;
        lo_runs += below && !(pair && was_below) ? 1 : 0;
        hi_rows += above ? 1 : 0;
        lo_rows += below ? 1 : 0;
        double q = 0.0; // ... and so does the filter
        if (pair) {
            const double d = x - prev;
            const bool falling = x > 0.0 && x < prev;
            q = fmin(fmax(alpha * quick + gain * d, 0.0), x);
            sum_abs += fabs(d);
            sum_pair += x;
            Sa += prev_u;
            Sb += u;
            Saa += prev_u * prev_u;
            Sbb += u * u;
            Sab += prev_u * u;
            sum_rec += falling ? lx - prev_log : 0.0;
            n_rec += falling ? 1 : 0;
            ++p;
        }
        quick = q;
        sum_base += x - q;
        prev = x;
        prev_u = u;
        prev_log = lx;
        was_rising = rising;
        was_above = above;
        was_below = below;
        ++m;
    };

    for (long c0 = 0; c0 < R; c0 += kSigChunk) {
        bool pair[kSigSub] = {}; // row r - 1 is valid too, for the list
        const int listed = list_rows<kSigWaves, kSigSub>(
            c0, R, wr, cnt,
            [&](long r, int k) {
                if (!valid(r))
                    return false;
                pair[k] = r >= 1 && valid(r - 1);
                return true;
            },
            [&](int pos, long r, int k) { rows[pos] = ((unsigned)r << 1) | (pair[k] ? 1u : 0u); });
        int j = 0;
        if (!have_shift && listed > 0) { // entry 0 of the first chunk that has one: the sample's shift
            const unsigned e = __builtin_amdgcn_readfirstlane(rows[0]);
            shift = col[(long)(e >> 1) * ld];
            have_shift = true;
            step(e, shift);
            j = 1;
        }
        for (; j + kSigUnroll <= listed; j += kSigUnroll) {
            unsigned e[kSigUnroll];
            double x[kSigUnroll];
#pragma unroll
            for (int k = 0; k < kSigUnroll; ++k) {
                e[k] = __builtin_amdgcn_readfirstlane(rows[j + k]);
                x[k] = col[(long)(e[k] >> 1) * ld];
            }
#pragma unroll
            for (int k = 0; k < kSigUnroll; ++k) {
                step(e[k], x[k]);
                // the rows are a chain (the filter, the flags): interleaving the logarithms of eight of them buys nothing
                // and costs the registers of eight
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        for (; j < listed; ++j) {
            const unsigned e = __builtin_amdgcn_readfirstlane(rows[j]);
            step(e, col[(long)(e >> 1) * ld]);
        }
    }
    if (!live)
        return;

    double o[SMART_SIGNATURE_COLS];
    const double nan = quiet_nan();
    o[SMART_SIG_MEAN] = sum_x / (double)m;
    o[SMART_SIG_BFI] = sum_x == 0.0 ? nan : sum_base / sum_x;
    o[SMART_SIG_FLASHINESS] = p == 0 || sum_pair == 0.0 ? nan : sum_abs / sum_pair;
    {
        const double q = (double)p;
        const double va = Saa - Sa * Sa / q, vb = Sbb - Sb * Sb / q;
        o[SMART_SIG_AC1] = p < 2 || !(va > 0.0) || !(vb > 0.0) ? nan : (Sab - Sa * Sb / q) / sqrt(va * vb);
    }
    o[SMART_SIG_RLD] = n_rise == 0 ? nan : (double)n_limb / (double)n_rise;
    o[SMART_SIG_RECESSION] = n_rec == 0 ? nan : sum_rec / (double)n_rec;
    o[SMART_SIG_PEAK] = peak;
    o[SMART_SIG_PEAK_ROW] = (double)peak_row;
    const bool with_hi = !is_nan_bits(hi), with_lo = !is_nan_bits(lo);
    o[SMART_SIG_HIGH_COUNT] = with_hi ? (double)hi_runs : nan;
    o[SMART_SIG_HIGH_DURATION] = with_hi && hi_runs ? (double)hi_rows / (double)hi_runs : nan;
    o[SMART_SIG_LOW_COUNT] = with_lo ? (double)lo_runs : nan;
    o[SMART_SIG_LOW_DURATION] = with_lo && lo_runs ? (double)lo_rows / (double)lo_runs : nan;
    const bool ok = m > 0 && is_finite_bits(sum_x); // no valid row, or a value of one that is not finite (header comment)
    double *const out = sig + (long)w * SMART_SIGNATURE_COLS * N + n;
#pragma unroll
    for (int k = 0; k < SMART_SIGNATURE_COLS; ++k)
        out[(long)k * N] = ok ? o[k] : nan;
}

void launch_signatures(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                       double alpha, const double *pulse, double *sig, hipStream_t s)
{
    const dim3 grid((unsigned)((N + kSigThreads - 1) / kSigThreads), (unsigned)W), block(kSigThreads);
    hipLaunchKernelGGL(smart_signatures, grid, block, 0, s, N, R, sim, ld, obs, window, alpha, pulse, sig);
}

} // namespace smart
