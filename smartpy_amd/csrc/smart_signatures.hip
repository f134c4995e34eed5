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
// only where 0 < x_r < x_{r-1}, where both logarithms are finite).  AC1 from one-pass moments of the two pair lists, each
// about a constant of its OWN, set at the window's first pair: the x_{r-1} about that pair's x_{r-1}, the x_r about that
// pair's x_r.  Each constant is a member of the sums it centres, so the loss of digits in S2 - S1^2 / p is bounded by p
// whatever the window opens on (a flood peak, a value before a gap), and a list that is constant has every term and so its
// variance exactly 0: the NaN rule is exact.  A value that is not finite needs no test of its own: the sum of x never
// becomes finite again, and ONE test of it at the end empties the (window, sample).
//
// Counts.  A run above hi (below lo) and a rising limb are counted by what CONTINUES them: runs = rows above - pairs whose
// x_{r-1} is above too, limbs = rising pairs - rising pairs whose row r - 1 rose as well.  What row r - 1 was is read off
// values at hand (x_{r-1} against the threshold; the sign of its own difference, which a rounded subtraction keeps), so no
// flag is carried from row to row: integers either way, and about ten instructions a row less than three carried flags.
//
// State: seventeen doubles and eight 32-bit counts per lane, in registers for the whole walk.  With the loads in flight and
// the logarithm's temporaries hipcc takes 109 VGPRs and no scratch under __launch_bounds__(256, 4): four wavefronts per
// SIMD.  The pair is an `if` WITHOUT an else -- what a row without a pair
// restarts is set before it: an if / else on the uniform flag makes hipcc keep the old and the new state side by side
// (51 VGPRs spilled).  Setting AC1's two constants at the first pair costs four selects and a scalar compare in every row if
// the batches do it; so up to the window's first pair a copy of the step that has the selects walks one row at a time -- as
// a rule two rows -- and the batches run the copy that has none (a second batched copy of the full step spills 120
// bytes).  A window without a pair anywhere does not walk so to its end: eight rows none of which has a pair go through
// `alone`, the step of such a row without its logarithm.
//
// Determinism.  No atomics; the association of every sum is the row order: two launches give the same bits.
//
// Not built: a split of the time axis across wavefronts.  The associative form of the clamped filter composes clamp-affine
// maps, which changes the bits and needs two sweeps.
#include <type_traits>

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
    double shift_a = 0.0, shift_b = 0.0, prev = 0.0, prev_log = 0.0, quick = 0.0;
    double sum_x = 0.0, sum_base = 0.0, sum_abs = 0.0, sum_pair = 0.0, sum_rec = 0.0;
    double Sa = 0.0, Sb = 0.0, Saa = 0.0, Sbb = 0.0, Sab = 0.0;
    double peak = -__builtin_inf();
    double last_d = 0.0; // x_{r-1} - x_{r-2} where row r - 1 has a pair, else 0
    int peak_row = 0, n_rise = 0, n_rise_joins = 0, n_rec = 0, hi_rows = 0, hi_joins = 0, lo_rows = 0, lo_joins = 0;

    // `first`: the window's first pair may still lie ahead (std::true_type), or is behind (std::false_type)
    auto step = [&](auto first, unsigned entry, double x) {
        const int r = (int)(entry >> 1);
        const bool pair = entry & 1u; // row r - 1 is valid, and it was the entry before this one (the same in every lane)
        const double lx = log(x);
        const bool above = x > hi, below = x < lo, top = x > peak;
        sum_x += x;
        peak_row = top ? r : peak_row;
        peak = top ? x : peak;
        hi_rows += above ? 1 : 0;
        lo_rows += below ? 1 : 0;
        // without a pair -- the window's first row, or the first after a gap -- the limbs, the runs and the filter start again
        double q = 0.0, d = 0.0;
        if (pair) {
            d = x - prev;
            const bool rising = x > prev, falling = x > 0.0 && x < prev;
            // A row that continues what row r - 1 began joins it: runs = rows - joins, limbs = rising pairs - joins, in
            // integers.  What row r - 1 was is read off the values at hand (x_{r-1} against the threshold, the sign of its own
            // difference, which a rounded subtraction keeps), so no flag is carried from row to row.
            hi_joins += above && prev > hi ? 1 : 0;
            lo_joins += below && prev < lo ? 1 : 0;
            n_rise += rising ? 1 : 0;
            n_rise_joins += rising && last_d > 0.0 ? 1 : 0;
            // The window's first pair gives the two lists their constants.  Only the walk that has not met it yet pays the
            // four selects a row (p is the same in every lane).
            if constexpr (decltype(first)::value) {
                shift_a = p == 0 ? prev : shift_a;
                shift_b = p == 0 ? x : shift_b;
            }
            const double ua = prev - shift_a, ub = x - shift_b;
            q = fmin(fmax(alpha * quick + gain * d, 0.0), x);
            sum_abs += fabs(d);
            sum_pair += x;
            Sa += ua;
            Sb += ub;
            Saa += ua * ua;
            Sbb += ub * ub;
            Sab += ua * ub;
            double before_log = prev_log;
            if constexpr (decltype(first)::value)
                before_log = log(prev); // (rows walked by `alone` keep no logarithm)
            sum_rec += falling ? lx - before_log : 0.0;
            n_rec += falling ? 1 : 0;
            ++p;
        }
        quick = q;
        sum_base += x - q;
        prev = x;
        prev_log = lx;
        last_d = d;
        ++m;
    };

    // a row without a pair, before the window's first pair: what `step` does to such a row, less the logarithm (the full
    // step of a first pair takes ln x_{r-1} itself)
    auto alone = [&](int r, double x) {
        const bool top = x > peak;
        sum_x += x;
        peak_row = top ? r : peak_row;
        peak = top ? x : peak;
        hi_rows += x > hi ? 1 : 0;
        lo_rows += x < lo ? 1 : 0;
        quick = 0.0;
        sum_base += x;
        prev = x;
        last_d = 0.0;
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
        // Up to the window's first pair: batches of rows none of which has a pair take the short step; any other row the
        // full step that sets AC1's constants, one at a time -- as a rule that is the chunk's first two entries ...
        while (j < listed && p == 0) {
            if (j + kSigUnroll <= listed) {
                unsigned e[kSigUnroll], any = 0;
                double x[kSigUnroll];
#pragma unroll
                for (int k = 0; k < kSigUnroll; ++k) {
                    e[k] = __builtin_amdgcn_readfirstlane(rows[j + k]);
                    any |= e[k];
                }
                if (!(any & 1u)) {
#pragma unroll
                    for (int k = 0; k < kSigUnroll; ++k)
                        x[k] = col[(long)(e[k] >> 1) * ld];
#pragma unroll
                    for (int k = 0; k < kSigUnroll; ++k)
                        alone((int)(e[k] >> 1), x[k]);
                    j += kSigUnroll;
                    continue;
                }
            }
            const unsigned e = __builtin_amdgcn_readfirstlane(rows[j]);
            step(std::true_type{}, e, col[(long)(e >> 1) * ld]);
            ++j;
        }
        // ... and from there in batches, the two constants of AC1 fixed
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
                step(std::false_type{}, e[k], x[k]);
                // the rows are a chain (the filter, the sums): interleaving the logarithms of eight of them buys nothing
                // and costs the registers of eight
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        for (; j < listed; ++j) {
            const unsigned e = __builtin_amdgcn_readfirstlane(rows[j]);
            step(std::false_type{}, e, col[(long)(e >> 1) * ld]);
        }
    }
    if (!live)
        return;

    double o[SMART_SIGNATURE_COLS];
    const double nan = quiet_nan();
    const int n_limb = n_rise - n_rise_joins; // (step: runs = rows - joins)
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
    const int hi_runs = hi_rows - hi_joins, lo_runs = lo_rows - lo_joins;
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
