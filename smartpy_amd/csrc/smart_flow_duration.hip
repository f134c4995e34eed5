// smart_flow_duration.hip -- flow duration curves of a stored discharge matrix sim[R][ld] (sample-minor): order
// statistics ALONG TIME, per sample and per window of report steps, and the objective functions of the sorted simulation
// against the sorted observations (the fit of the curve, or of a segment of it: high flows, low flows).
//
// Definition.  For window w and sample n: rows = { r : window[r] == w (every r without a window array), obs[r] not NaN
// where obs is given }, m = |rows|, x = sim[rows, n].
//   Q(q)   = the k-th smallest of x, k = max(1, ceil(q * m)) with the product formed in double (numpy 'inverted_cdf'): an
//            element of the column, no arithmetic on the values; NaN sorts above +inf and counts; m == 0 gives NaN.
//   objfn  = finish_objectives (smart_device.h) on the pairs (s_i, e_i) = (f(x_(i)), f(obs_(i))), both sorted ascending
//            and paired by the 0-based rank i, over the ranks with lo * m <= (double)i < hi * m; f one of the four
//            transforms of smart_objfn_windows.hip.  Fewer than two such ranks -> NaN in all seven; a pair of the segment
//            whose f(x) is not finite -> NaN for that (window, sample), whose f(obs) is not finite -> for the window.
// Values are compared as the order-preserving keys of smart_order_keys.h (both zeros one key).
//
// SORT FORM (R <= 16,384).  A workgroup of 1,024 threads takes COLS adjacent samples of one window, grid =
// (ceil(N / COLS), W).  It walks window[] / obs[] in chunks of 1,024 rows, compacts its window's rows in row order into an
// LDS list (ballot + prefix counts, no atomics: smart_window_rows.h) and loads the COLS-wide pieces of those rows as
// KEYS into LDS -- 8 bytes per element, 16,384 elements = 128 KiB in every instance (CAP rows x COLS = 1,024 x 16 ..
// 16,384 x 1), 12 KiB more for the row list and the reduction: 140 of the 160 KiB a gfx950 workgroup may open.
//   LDS LAYOUT.  Interleaved: rank i of column c lies at flat position i * COLS + c.  A compare-exchange at row distance
//   j is one at flat distance j * COLS whatever the column, so ONE network sorts all columns, and the mapping thread ->
//   (column, pair) is a fixed function of the flat index:
//     j * COLS >= 64  pair P = t + 1,024 u holds positions f = 2P - (P & (jj - 1)) and f + jj: the 64 lanes of a wavefront
//                     read 64 consecutive keys = 512 contiguous bytes, each 32-lane group of a ds_read_b64 all 64 banks
//                     once: conflict-free, and so are the stores;
//     j * COLS <  64  the partner of position e is e ^ jj, a lane of the same wavefront: every thread keeps the keys of
//                     its positions e = t + 1,024 u in registers through ALL remaining stages of the merge (lane
//                     exchanges, no LDS, no barrier) -- the strided LDS pattern that would conflict 2-way never occurs.
//   The network runs over the smallest power of two of rows that holds m (the padding above it is never touched): a
//   window of 365 of 3,653 rows costs a 512-row network, not a 4,096-row one.
// The K order statistics are read straight out of LDS.  With objfn, a prologue kernel (one workgroup per window, the same
// compaction and network on the observations) leaves the window's sorted f(obs) by rank, the segment and its statistics
// (count, mean, sum, sum of squared deviations) in the caller's workspace; the main kernel reads f(obs) by rank from L2
// and forms the one-pass moments about that mean and the column's first in-segment value.  Thread t adds
// the ranks i0 + t / COLS + (1,024 / COLS) u of column t % COLS in that order; a fixed LDS tree joins the threads of a
// column.  Padding keys (ranks >= m, columns >= N) are the largest key and are never returned nor summed.
//
// SELECT FORM (any R; order statistics only).  One lane per sample (a row's 64 values are one 512-byte read), one
// wavefront per workgroup.  One pass finds the column's smallest and largest key and m; then the K probabilities bisect
// the key space together, one pass over the window's rows per round with K INTEGER counts of key <= mid per lane.  The
// smallest key v with count(key <= v) >= k is the k-th smallest key: the bits of the sort form.
//
// Determinism.  No floating-point atomics; integer counts in select; every sum of the sort form has one association for
// a given (N, R, window array, segment): two launches give the same bits.
#include "smart_capi_internal.h"
#include "smart_device.h"
#include "smart_order_keys.h"
#include "smart_window_rows.h"
#include <cstdlib>

namespace smart {

constexpr int kFdcThreads = 1024;
constexpr int kFdcWaves = kFdcThreads / kWave;
constexpr int kFdcElems = 16384;         // keys in LDS: 128 KiB
constexpr int kFdcChunk = kFdcThreads;   // rows of window[] looked at per compaction, one per thread
constexpr long kFdcCapacity = 16384;     // rows of the sort form: the COLS = 1 instance
constexpr int kFdcHead = 8;              // doubles in front of a window's sorted f(obs) in the workspace:
                                         // m, i0, i1, mean, sum, sum (e - mean)^2, sum (e - mean), usable (1 / 0)

// the rows of window w among [c0, c0 + kFdcChunk), in row order, into rows[]; -> how many (list_rows, smart_window_rows.h:
// one row per thread, no payload).  The caller puts a barrier between its last read of rows[] and the next call.
__device__ __forceinline__ int fdc_compact(long c0, long R, const double *__restrict__ obs,
                                           const int *__restrict__ window, int w, int (*cnt)[kFdcWaves], int *rows)
{
    const int wr = threadIdx.x / kWave;  // (a vector value: the sixteen compares of list_rows measured faster so)
    return list_rows<kFdcWaves, 1>(
        c0, R, wr, cnt, [&](long r, int) { return (!window || window[r] == w) && (!obs || !is_nan_bits(obs[r])); },
        [&](int pos, long r, int) { rows[pos] = (int)r; });
}

// rows of the network for m rows: a power of two >= max(m, 2) with at least one wavefront of flat positions
template <int COLS>
__device__ __forceinline__ int fdc_network_rows(int m)
{
    int cap = 2;
    while (cap < m || cap * COLS < kWave)
        cap <<= 1;
    return cap;
}

// bitonic network over `cap` rows x COLS interleaved columns, ascending in every column (header: LDS LAYOUT)
template <int COLS>
__device__ inline void fdc_sort(unsigned long long *keys, int cap)
{
    const int tid = threadIdx.x;
    const int nflat = cap * COLS;       // a multiple of 64: whole wavefronts take part or none of their lanes
    for (int k = 2; k <= cap; k <<= 1) {
        int j = k >> 1;
        for (; j * COLS >= kWave; j >>= 1) {
            const int jj = j * COLS;
            for (int p = tid; p < nflat / 2; p += kFdcThreads) {
                const int f = 2 * p - (p & (jj - 1));
                const bool up = ((f / COLS) & k) == 0;
                const unsigned long long a = keys[f], b = keys[f + jj];
                if ((a > b) == up) {
                    keys[f] = b;
                    keys[f + jj] = a;
                }
            }
            __syncthreads();
        }
        if (j > 0) {
            for (int e = tid; e < nflat; e += kFdcThreads) {
                unsigned long long v = keys[e];
                const bool up = ((e / COLS) & k) == 0;
                for (int s = j; s > 0; s >>= 1) {
                    const int jj = s * COLS;
                    const unsigned long long o = __shfl_xor(v, jj, kWave);
                    const bool smaller = ((e & jj) == 0) == up;     // this position keeps the smaller of the two
                    v = ((o < v) == smaller) ? o : v;
                }
                keys[e] = v;
            }
            __syncthreads();
        }
    }
}

// sum of v over the threads t with the same t % COLS, the same tree for every call and the result in all of them
template <int COLS>
__device__ inline double fdc_column_sum(double v, double *sh)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = kFdcThreads / 2; s >= COLS; s >>= 1) {
        if (tid < s)
            sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const double r = sh[tid % COLS];
    __syncthreads();
    return r;
}

// ---- prologue: the sorted f(obs) of every window, its segment and the segment's statistics -------------------------
__global__ __launch_bounds__(kFdcThreads) void smart_fdc_observed(long R, const double *__restrict__ obs,
                                                                 const int *__restrict__ window, int transform,
                                                                 double eps, double seg_lo, double seg_hi,
                                                                 double *__restrict__ ws)
{
    __shared__ unsigned long long keys[kFdcElems];
    __shared__ double sh[kFdcThreads];
    __shared__ int rows[kFdcChunk];
    __shared__ int cnt[1][kFdcWaves];
    const int w = blockIdx.x, tid = threadIdx.x;
    int m = 0;
    for (long c0 = 0; c0 < R; c0 += kFdcChunk) {
        const int mc = fdc_compact(c0, R, obs, window, w, cnt, rows);
        if (tid < mc)
            keys[m + tid] = value_key(obs[rows[tid]]);
        m += mc;
        __syncthreads();
    }
    const int cap = fdc_network_rows<1>(m);
    for (int e = m + tid; e < cap; e += kFdcThreads)
        keys[e] = kKeyPad;
    __syncthreads();
    fdc_sort<1>(keys, cap);

    double *const head = ws + (long)w * (kFdcHead + R);
    double *const fe = head + kFdcHead;
    const int i0 = (int)ceil(seg_lo * (double)m);           // lo * m <= i  <=>  i >= ceil(lo * m), i an integer
    const int i1 = min(m, (int)ceil(seg_hi * (double)m));   // i < hi * m   <=>  i < ceil(hi * m)
    double s = 0.0;
    for (int i = tid; i < m; i += kFdcThreads) {
        const double v = flow_transform(transform, key_value(keys[i]), eps);
        fe[i] = v;
        if (i >= i0 && i < i1)
            s += v;
    }
    s = fdc_column_sum<1>(s, sh);
    const int c = i1 - i0;
    const bool usable = c >= 2 && is_finite_bits(s);    // the two rules, for the whole window
    const double mean = usable ? s / (double)c : 0.0;
    double s2 = 0.0, s1 = 0.0;
    if (usable)
        for (int i = i0 + tid; i < i1; i += kFdcThreads) {
            const double d = flow_transform(transform, key_value(keys[i]), eps) - mean;
            s2 += d * d;
            s1 += d;
        }
    s2 = fdc_column_sum<1>(s2, sh);
    s1 = fdc_column_sum<1>(s1, sh);
    if (tid == 0) {
        head[0] = (double)m;
        head[1] = (double)i0;
        head[2] = (double)i1;
        head[3] = mean;
        head[4] = s;
        head[5] = s2;
        head[6] = s1;
        head[7] = usable ? 1.0 : 0.0;
    }
}

// ---- sort form ------------------------------------------------------------------------------------------------------
template <int CAP, int COLS>
__global__ __launch_bounds__(kFdcThreads) void smart_fdc_sort(long N, long R, const double *__restrict__ sim, long ld,
                                                             const double *__restrict__ obs,
                                                             const int *__restrict__ window, MatrixProbs probs, int K,
                                                             double *__restrict__ quant, int transform, double eps,
                                                             const double *__restrict__ ws, double *__restrict__ objfn,
                                                             int remap)
{
    static_assert(CAP * COLS == kFdcElems && kFdcThreads % COLS == 0 && COLS <= kWave, "128 KiB of keys in every instance");
    __shared__ unsigned long long keys[kFdcElems];
    __shared__ double sh[kFdcThreads];
    __shared__ int rows[kFdcChunk];
    __shared__ int cnt[1][kFdcWaves];
    const int w = blockIdx.y, tid = threadIdx.x;
    long bx = blockIdx.x;
    if (remap) {
        // workgroups are dealt round-robin over the eight XCDs: give every residue class of the block index a contiguous
        // range of sample blocks, so that the workgroups that share a 128-byte line share an L2 (a bijection for any
        // grid; placement is a matter of speed only)
        const long nb = gridDim.x, q = nb / 8, r = nb % 8, x = bx % 8;
        bx = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bx / 8;
    }
    const long n0 = bx * COLS;
    const int c = tid % COLS;           // the column of every flat position t + 1,024 u of this thread

    // ---- 1. the window's rows, chunk by chunk, as keys into LDS
    int m = 0;
    for (long c0 = 0; c0 < R; c0 += kFdcChunk) {
        const int mc = fdc_compact(c0, R, obs, window, w, cnt, rows);
        for (int e = tid; e < mc * COLS; e += kFdcThreads)
            keys[m * COLS + e] = n0 + c < N ? value_key(sim[(long)rows[e / COLS] * ld + n0 + c]) : kKeyPad;
        m += mc;
        __syncthreads();
    }
    const int cap = fdc_network_rows<COLS>(m);
    for (int e = m * COLS + tid; e < cap * COLS; e += kFdcThreads)
        keys[e] = kKeyPad;
    __syncthreads();

    // ---- 2. one network for all columns
    fdc_sort<COLS>(keys, cap);

    // ---- 3. the order statistics, straight out of LDS (thread t: probability t / COLS of column t % COLS)
    if (tid < K * COLS && n0 + c < N) {
        double v = quiet_nan();
        if (m > 0) {
            const int rank = max(1, (int)ceil(probs.q[tid / COLS] * (double)m));
            v = key_value(keys[(rank - 1) * COLS + c]);
        }
        quant[((long)w * K + tid / COLS) * N + n0 + c] = v;
    }
    if (!objfn)
        return;

    // ---- 4. the segment's moments against the sorted observations
    const double *const head = ws + (long)w * (kFdcHead + R);
    const double *const fe = head + kFdcHead;
    const int i0 = (int)head[1], i1 = (int)head[2];
    const bool usable = head[7] != 0.0;
    const double ebar = head[3];
    double mo[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (usable) {
        const double shift = flow_transform(transform, key_value(keys[i0 * COLS + c]), eps);
        for (int i = i0 + tid / COLS; i < i1; i += kFdcThreads / COLS) {
            const double e = fe[i];
            const double s = flow_transform(transform, key_value(keys[i * COLS + c]), eps);
            const double d = s - e, u = s - shift;
            mo[0] += d;
            mo[1] += d * d;
            mo[2] += u;
            mo[3] += u * u;
            mo[4] += (e - ebar) * u;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
        mo[k] = fdc_column_sum<COLS>(mo[k], sh);
    if (tid >= COLS || n0 + c >= N)
        return;
    const double st[5] = {(double)(i1 - i0), ebar, head[4], head[5], head[6]};
    double o[8];
    finish_objectives(st, mo[0], mo[1], mo[2], mo[3], mo[4], 0.0, quiet_nan(), o);
    const bool ok = usable && is_finite_bits(mo[2]);    // some f(sim) of the segment was not finite (header comment)
    double *const out = objfn + ((long)w * N + n0 + c) * SMART_OBJFN_WINDOW_COLS;
#pragma unroll
    for (int k = 0; k < SMART_OBJFN_WINDOW_COLS; ++k)
        out[k] = ok ? o[k] : quiet_nan();
}

// ---- select form ----------------------------------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(kWave) void smart_fdc_select(long N, long R, const double *__restrict__ sim, long ld,
                                                         const double *__restrict__ obs, const int *__restrict__ window,
                                                         MatrixProbs probs, int K, double *__restrict__ quant)
{
    const int w = blockIdx.y;
    long n = (long)blockIdx.x * kWave + threadIdx.x;
    const bool live = n < N;
    if (!live)
        n = N - 1;
    const double *const col = sim + n;
    // kSelUnroll rows in flight per lane; a row of another window, without an observation or past the end is not read
    // and stands as the padding key, which is above every mid and every kmax candidate
    constexpr int kSelUnroll = 4;
    auto load_keys = [&](long r0, unsigned long long (&key)[kSelUnroll]) {
        double v[kSelUnroll];
        bool in[kSelUnroll];
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) {
            const long r = r0 + u;      // (membership is the same in every lane)
            in[u] = r < R && (!window || window[r] == w) && (!obs || !is_nan_bits(obs[r]));
            v[u] = 0.0;
            if (in[u])
                v[u] = col[r * ld];
        }
        int members = 0;
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) {
            key[u] = in[u] ? value_key(v[u]) : kKeyPad;
            members += in[u] ? 1 : 0;
        }
        return members;
    };

    // pass 0: m and the smallest and largest key of the column
    unsigned long long kmin = kKeyPad, kmax = 0;
    int m = 0;
    for (long r = 0; r < R; r += kSelUnroll) {
        unsigned long long key[kSelUnroll];
        m += load_keys(r, key);
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) {
            kmin = key[u] < kmin ? key[u] : kmin;
            kmax = key[u] != kKeyPad && key[u] > kmax ? key[u] : kmax;
        }
    }
    if (m == 0) {
        if (live)
            for (int k = 0; k < K; ++k)
                quant[((long)w * K + k) * N + n] = quiet_nan();
        return;
    }
    // count(key <= hi) >= rank throughout (count(key <= kmax) = m); an interval of c keys leaves at most ceil(c / 2), so
    // the bit length of kmax - kmin rounds bring every one down to a single key -- the widest lane sets the rounds
    int rank[KB];
    unsigned long long lo[KB], hi[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        rank[k] = max(1, (int)ceil(probs.q[k] * (double)m));
        lo[k] = kmin;
        hi[k] = kmax;
    }
    int rounds = kmax == kmin ? 0 : 64 - __clzll((long long)(kmax - kmin));
    for (int d = 1; d < kWave; d <<= 1)
        rounds = max(rounds, __shfl_xor(rounds, d, kWave));
    for (int round = 0; round < rounds; ++round) {
        unsigned long long mid[KB];
        int count[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            mid[k] = lo[k] + ((hi[k] - lo[k]) >> 1);
            count[k] = 0;
        }
        for (long r = 0; r < R; r += kSelUnroll) {
            unsigned long long key[kSelUnroll];
            load_keys(r, key);
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u)
#pragma unroll
                for (int k = 0; k < KB; ++k)
                    count[k] += key[u] <= mid[k] ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            if (count[k] >= rank[k])
                hi[k] = mid[k];
            else
                lo[k] = mid[k] + 1;
        }
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (k < K)
                quant[((long)w * K + k) * N + n] = key_value(hi[k]);
    }
}

// ---- launch (validated by smart_analysis_capi.hip) ---------------------------------------------------------------------------
long flow_duration_sort_capacity() { return kFdcCapacity; }

long flow_duration_workspace_bytes(long R, int W, bool with_objfn)
{
    return with_objfn ? ((long)W * (kFdcHead + R) * 8 + 255) / 256 * 256 : 0;
}

// SMART_FDC_XCD_REMAP=1 / 0: the block-index remap of the sort form on or off (tools/bench_flow_duration.py sets both
// beside each other).  Default off: DESIGN 4.12 has the A/B
static bool fdc_remap_wanted()
{
    const char *e = std::getenv("SMART_FDC_XCD_REMAP");
    return e && e[0] == '1';
}

template <int CAP, int COLS>
static void launch_fdc_sort(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                            const MatrixProbs &p, int K, double *quant, int transform, double eps, const double *ws,
                            double *objfn, hipStream_t s)
{
    const dim3 grid((unsigned)((N + COLS - 1) / COLS), (unsigned)W);
    hipLaunchKernelGGL((smart_fdc_sort<CAP, COLS>), grid, dim3(kFdcThreads), 0, s, N, R, sim, ld, obs, window, p, K, quant,
                       transform, eps, ws, objfn, fdc_remap_wanted() ? 1 : 0);
}

void launch_flow_duration(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                          const double *probs, int K, double *quant, int transform, double eps, double seg_lo,
                          double seg_hi, double *objfn, double *ws, bool sort, hipStream_t s)
{
    MatrixProbs p;
    for (int k = 0; k < SMART_QUANTILES_MAX_PROBS; ++k)
        p.q[k] = k < K ? probs[k] : 0.0;
    if (!sort) {
        const dim3 grid((unsigned)((N + kWave - 1) / kWave), (unsigned)W), block(kWave);
        if (K <= 4)
            hipLaunchKernelGGL((smart_fdc_select<4>), grid, block, 0, s, N, R, sim, ld, obs, window, p, K, quant);
        else if (K <= 8)
            hipLaunchKernelGGL((smart_fdc_select<8>), grid, block, 0, s, N, R, sim, ld, obs, window, p, K, quant);
        else
            hipLaunchKernelGGL((smart_fdc_select<16>), grid, block, 0, s, N, R, sim, ld, obs, window, p, K, quant);
        return;
    }
    if (objfn)
        hipLaunchKernelGGL(smart_fdc_observed, dim3((unsigned)W), dim3(kFdcThreads), 0, s, R, obs, window, transform, eps,
                           seg_lo, seg_hi, ws);
    if (R <= 1024)
        launch_fdc_sort<1024, 16>(N, R, sim, ld, obs, window, W, p, K, quant, transform, eps, ws, objfn, s);
    else if (R <= 2048)
        launch_fdc_sort<2048, 8>(N, R, sim, ld, obs, window, W, p, K, quant, transform, eps, ws, objfn, s);
    else if (R <= 4096)
        launch_fdc_sort<4096, 4>(N, R, sim, ld, obs, window, W, p, K, quant, transform, eps, ws, objfn, s);
    else if (R <= 8192)
        launch_fdc_sort<8192, 2>(N, R, sim, ld, obs, window, W, p, K, quant, transform, eps, ws, objfn, s);
    else
        launch_fdc_sort<16384, 1>(N, R, sim, ld, obs, window, W, p, K, quant, transform, eps, ws, objfn, s);
}

} // namespace smart
