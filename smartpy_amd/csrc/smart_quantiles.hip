// smart_quantiles.hip -- weighted quantiles of a stored discharge matrix along the SAMPLE axis (the GLUE prediction
// bounds): for every report step r and probability q the smallest value v of sim[r][0..N) with
//     sum of w_n over { n : x_n <= v }  >=  q * W,     W = sum of w_n                     (numpy 'inverted_cdf')
// No interpolation; NaN sorts above +inf and a quantile that reaches it is NaN; -0.0 and +0.0 are one value; W == 0
// gives NaN.  One workgroup per report step: the matrix is sample-minor, so the step's N values are contiguous.
//
// Values are compared as ORDER-PRESERVING 64-BIT KEYS (value_key, smart_order_keys.h): unsigned order of the keys =
// numeric order of the doubles, every NaN one key above +inf, both zeros one key.
//
// Two forms, the same definition:
//   sort    N <= kSortCapacity.  Keys and sample indices into LDS, bitonic network there, inclusive scan of the weights
//           in sorted order, one binary search per probability for the first position with cum >= q*W.
//           CAPACITY.  A gfx950 compute unit has 160 KiB of LDS and hands all of it to one workgroup.  A sorted
//           element costs 18 bytes there (8 key + 2 index + 8 running weight), the scan wants 16 doubles beside them:
//           (163840 - 128) / 18 = 9095 elements would fit; the bitonic network needs a power of two, so 8192 =
//           147,584 bytes, one workgroup of 1024 threads per compute unit.  Smaller rows take the instance compiled
//           for 1024, 2048 or 4096 elements (18 / 36 / 72 KiB: several workgroups per compute unit).
//   select  any N.  No sort: all probabilities bisect the key space together, between the smallest and the largest key
//           of the row; a round reads the row once and forms S_k = sum of [key_n <= mid_k] * w_n for every k.
//
// The network and the scan of the sort form are those of smart_order_stats.h.
//
// DETERMINISM.  No floating-point atomics.  Every sum has ONE association for a given (N, form):
//   scan    block_scan: thread t owns E consecutive sorted positions, cum[i] = A_wave + (B_lane + L_i).  Hence cum[i] >=
//           cum[i-1] always and cum[i] == cum[i-1] where w_i == 0 (adding a non-negative term never lowers a rounded
//           sum): the binary search is well defined and a sample of weight zero never decides a result.  W = cum[N-1], so
//           q <= 1 is always reached.
//   select  thread t adds its elements n = t, t + T, ... in that order; a fixed butterfly joins the lanes, a fixed
//           chain the wavefronts.  The shape does not depend on mid, every term [key <= mid] * w is monotone in mid and a
//           rounded sum of non-negative terms is monotone in each: S(mid) is monotone, which the bisection relies on.
//           W is that same sum with every term in, so S(largest key) == W bit for bit.
// The threshold t = q * W is ONE multiplication, made once per step and probability; the comparison is cum >= t.
// Weights must be finite and >= 0 (checked by the caller, not here); weights == nullptr means equal weights.
#include "smart_capi_internal.h"
#include "smart_matrix_common.h"
#include "smart_order_stats.h"
#include <cstdint>

namespace smart {

constexpr long kLdsBytesPerWorkgroup = 160 * 1024;  // gfx950: the whole LDS of a compute unit
constexpr long kSortBytesPerElement = 8 + 2 + 8;    // key, sample index, running weight
constexpr long kSortScratchBytes = 16 * 8;          // the wavefronts' totals

constexpr long largest_pow2_capacity(long bytes)
{
    long cap = 1;
    while (2 * cap * kSortBytesPerElement + kSortScratchBytes <= bytes)
        cap *= 2;
    return cap;
}
constexpr long kSortCapacity = largest_pow2_capacity(kLdsBytesPerWorkgroup);
static_assert(kSortCapacity == 8192, "the sort form is instantiated for 1024 .. 8192 elements");
static_assert(kSortCapacity <= 65536, "sample indices are kept as 16-bit numbers");

// ---- sort form ------------------------------------------------------------------------------------------------------
template <int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void smart_quantiles_sort(int N, long R, const double *__restrict__ sim, long ld,
                                                                const double *__restrict__ weights, MatrixProbs probs,
                                                                int K, double *__restrict__ out)
{
    constexpr int E = CAP / THREADS;    // sorted positions per thread in the scan
    constexpr int WAVES = THREADS / kWave;
    static_assert(CAP % THREADS == 0 && THREADS % kWave == 0 && WAVES <= 16 && CAP / 2 >= THREADS, "shape");
    __shared__ unsigned long long keys[CAP];
    __shared__ double cum[CAP];
    __shared__ double wave_total[16];
    __shared__ unsigned short idx[CAP];

    const int tid = threadIdx.x;
    const long r = blockIdx.x;
    const double *row = sim + r * ld;

    for (int n = tid; n < CAP; n += THREADS) {
        keys[n] = n < N ? value_key(row[n]) : kKeyPad;
        idx[n] = (unsigned short)n;
    }
    __syncthreads();

    // bitonic network over CAP elements, ascending; the padding (above every key of the row) ends up at [N, CAP)
    for (int k = 2; k <= CAP; k <<= 1)
        bitonic_merge_lds<CAP, THREADS, true>(keys, idx, k, k >> 1, 0);

    // inclusive scan of the weights in sorted order (header: DETERMINISM)
    double w[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        w[e] = i < N ? (weights ? weights[idx[i]] : 1.0) : 0.0;
    }
    block_scan<E, WAVES>(w, wave_total);
#pragma unroll
    for (int e = 0; e < E; ++e)
        cum[tid * E + e] = w[e];
    __syncthreads();

    if (tid < K) {
        const double W = cum[N - 1];
        double v = quiet_nan();
        if (W > 0.0) {
            const double t = probs.q[tid] * W;
            int lo = 0, hi = N - 1;     // cum[N - 1] = W >= t
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cum[mid] >= t)
                    hi = mid;
                else
                    lo = mid + 1;
            }
            v = key_value(keys[lo]);
        }
        out[(long)tid * R + r] = v;
    }
}

// ---- select form ----------------------------------------------------------------------------------------------------
// threads per workgroup by the number of probabilities a launch carries: every thread keeps an interval, a threshold and
// a sum per probability in registers
constexpr int select_threads(int kb) { return kb <= 4 ? 1024 : kb <= 8 ? 512 : 256; }

// sum of v over the workgroup, the same bits in every thread: butterfly over the lanes (a + b == b + a, so both
// partners hold the same bits after every exchange), then the wavefronts' totals chained left to right
template <int KB>
__device__ inline void select_block_sums(double (&acc)[KB], double (*sh)[select_threads(KB) / kWave])
{
    constexpr int kSelectThreads = select_threads(KB);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        double v = acc[k];
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1)
            v += __shfl_xor(v, d, kWave);
        if (lane == 0)
            sh[k][wave] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        double v = sh[k][0];
        for (int x = 1; x < kSelectThreads / kWave; ++x)
            v += sh[k][x];
        acc[k] = v;
    }
    __syncthreads();
}

template <int KB>
__global__ __launch_bounds__(select_threads(KB)) void smart_quantiles_select(long N, long R, const double *__restrict__ sim,
                                                                         long ld, const double *__restrict__ weights,
                                                                         MatrixProbs probs, int K,
                                                                         double *__restrict__ out)
{
    constexpr int kSelectThreads = select_threads(KB);
    __shared__ double sh[KB][kSelectThreads / kWave];
    __shared__ unsigned long long ends[2][kSelectThreads / kWave];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    const long r = blockIdx.x;
    const double *row = sim + r * ld;

    // pass 0: W and the smallest and largest key of the row
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k)
        acc[k] = 0.0;
    unsigned long long kmin = kKeyPad, kmax = 0;
    for (long n = tid; n < N; n += kSelectThreads) {
        const unsigned long long key = value_key(row[n]);
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
        acc[0] += weights ? weights[n] : 1.0;
    }
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long a = __shfl_xor(kmin, d, kWave), b = __shfl_xor(kmax, d, kWave);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if (lane == 0) {
        ends[0][wave] = kmin;
        ends[1][wave] = kmax;
    }
    select_block_sums<KB>(acc, sh);     // (its barriers publish ends[] as well)
    for (int x = 0; x < kSelectThreads / kWave; ++x) {
        kmin = ends[0][x] < kmin ? ends[0][x] : kmin;
        kmax = ends[1][x] > kmax ? ends[1][x] : kmax;
    }
    const double W = acc[0];
    if (!(W > 0.0)) {
        if (tid < K)
            out[(long)tid * R + r] = quiet_nan();
        return;
    }

    // every thread keeps every interval: the sums come back with the same bits everywhere.  S(hi) >= t throughout
    // (S(kmax) == W >= q * W); an interval of c keys leaves at most ceil(c / 2), so the bit length of kmax - kmin
    // rounds bring every one down to a single key
    double t[KB];
    unsigned long long lo[KB], hi[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        t[k] = probs.q[k < K ? k : 0] * W;
        lo[k] = kmin;
        hi[k] = kmax;
    }
    const int rounds = kmax == kmin ? 0 : 64 - __clzll((long long)(kmax - kmin));
    for (int round = 0; round < rounds; ++round) {
        unsigned long long mid[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            mid[k] = lo[k] + ((hi[k] - lo[k]) >> 1);
            acc[k] = 0.0;
        }
        for (long n = tid; n < N; n += kSelectThreads) {
            const unsigned long long key = value_key(row[n]);
            const double w = weights ? weights[n] : 1.0;
#pragma unroll
            for (int k = 0; k < KB; ++k)
                acc[k] += key <= mid[k] ? w : 0.0;
        }
        select_block_sums<KB>(acc, sh);
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            if (acc[k] >= t[k])
                hi[k] = mid[k];
            else
                lo[k] = mid[k] + 1;
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (k < K)
                out[(long)k * R + r] = key_value(hi[k]);
    }
}

// ---- launch (validated by smart_analysis_capi.hip: 1 <= n_reports < 2^31, 1 <= n_probs <= 16, sort only within capacity) ------
long quantiles_sort_capacity() { return kSortCapacity; }

void launch_quantiles(long N, long R, const double *sim, long ld, const double *weights, const double *probs, int K,
                      double *out, bool sort, hipStream_t s)
{
    MatrixProbs p;
    for (int k = 0; k < SMART_QUANTILES_MAX_PROBS; ++k)
        p.q[k] = k < K ? probs[k] : 0.0;
    const dim3 grid((unsigned)R);
    if (sort) {
        sort_instance<(int)kSortCapacity>(N, [&](auto cap, auto threads) {
            hipLaunchKernelGGL((smart_quantiles_sort<cap(), threads()>), grid, dim3(threads()), 0, s, (int)N, R, sim, ld,
                               weights, p, K, out);
        });
    } else if (K <= 4) {
        hipLaunchKernelGGL((smart_quantiles_select<4>), grid, dim3(select_threads(4)), 0, s, N, R, sim, ld, weights, p, K, out);
    } else if (K <= 8) {
        hipLaunchKernelGGL((smart_quantiles_select<8>), grid, dim3(select_threads(8)), 0, s, N, R, sim, ld, weights, p, K, out);
    } else {
        hipLaunchKernelGGL((smart_quantiles_select<16>), grid, dim3(select_threads(16)), 0, s, N, R, sim, ld, weights, p, K,
                           out);
    }
}

} // namespace smart
