// smart_sobol.hip -- Sobol sensitivity indices of the rows of a matrix y[M][ld] whose columns are a Saltelli design in
// block-major order: row r holds the blocks [A ; B ; AB_0 ; ... ; AB_{k-1}], each of n contiguous doubles (a report step
// of a stored discharge matrix, or one scalar target).  First-order indices after Saltelli 2010, total indices after
// Jansen, and the standard deviation of both over B bootstrap replicates.
//
// Definition, for one row with blocks yA, yB, yAB_j:
//   mu = mean of the 2n values of A u B;  u = y - mu;  V = sum(uA^2 + uB^2) / 2n - (sum(uA + uB) / 2n)^2 (the population
//   variance of A u B in a form that does not depend on the last bits of mu);
//   S1_j = sum_i uB_i (yAB_j,i - yA_i) / (n V);      ST_j = sum_i (yA_i - yAB_j,i)^2 / (2n V).
//   Replicate b with counts c_bi (sum_i c_bi = n) keeps mu: every sum above weighted by c_bi, V_b in place of V.  The
//   result is the standard deviation (ddof = 1) of S1_bj and of ST_bj over the B replicates; B == 1 gives NaN.
// Rules: a value among the N = n (k + 2) of a row that is not finite makes every output of the row NaN -- found by ONE
// test of the sum  sum(A u B) + sum_j sum_i (yA_i - yAB_j,i)^2, which has taken every value of the row (no
// test per element); a row whose A u B is one value (smallest == largest), or whose V does not come out above 0, gives
// NaN in S1 and ST (and V = 0 for the former); yAB_j equal to yA bit for bit gives S1_j = ST_j = +0.0 exactly (every
// term is a zero added to +0.0) and +0.0 in both standard deviations.
//
// POINT KERNEL (smart_sobol_point).  One workgroup of 1,024 threads per row, thread t owns the base rows i = t + 1,024 m
// in every pass, so what it keeps of yA and uB in LDS is read back by itself alone (consecutive lanes, consecutive
// doubles: conflict-free).  Pass 1 reads yA and yB (sum, smallest, largest) -> mu; pass 2 turns yB into uB in place and
// adds the two moments; pass 3 reads every AB_j once and adds its two numerators.  The row is read from HBM once while
// 16 n bytes fit into LDS: instances for n <= 1,024 (16 KiB, many workgroups per compute unit) and n <= 8,192 (128 KiB);
// beyond that (smart_sobol_lds_capacity()) the same passes read yA and yB again, from L2.  Every sum is: per thread in
// ascending i, a butterfly over the 64 lanes, the 16 wavefronts in order.
//
// BOOTSTRAP KERNEL (smart_sobol_bootstrap), after the point kernel, whose mu and V it reads.  One workgroup of 512
// threads per row: the contraction [B x n] counts x [n x (2 + 2k)] terms with ONE LANE PER REPLICATE.  The workgroup
// builds the 2 + 2k terms (uA^2 + uB^2, uA + uB, uB d_j, d_j^2) of 128 base rows at a time in LDS; a wavefront takes 64
// replicates (counts[n][B] uint16: one coalesced 128-byte read per base row) and a fixed share of the tile's rows, the
// terms of a base row are the same address for all its lanes (broadcast reads) and each is one FMA into a register.
// With B <= 256 the eight wavefronts split the rows of a tile in 8 / ceil(B / 64) (rounded down to a power of two)
// chunks and add their registers through LDS in chunk order.  Each replicate's lane then forms V_b, S1_bj, ST_bj; the
// standard deviation is two passes about replicate 0's value (all replicates equal: exactly 0), butterfly + wavefronts
// in order.  Instances for k <= 4, 10, 16 (the registers a lane needs).
//
// Determinism.  No atomics; the shape of every sum is fixed by (n, k, B): two launches give the same bits, and the point
// kernel is the same launch with or without the bootstrap.
#include "smart_capi_internal.h"
#include "smart_matrix_common.h"

namespace smart {

constexpr int kSobThreads = 1024;                    // point kernel
constexpr int kSobWaves = kSobThreads / kWave;
constexpr int kSobSmall = 1024;                      // base rows of the small LDS instance
constexpr long kSobLdsCapacity = 8192;               // base rows whose yA and uB stay in LDS: 16 n bytes = 128 KiB
constexpr int kSobMaxParams = SMART_SOBOL_MAX_PARAMS;
constexpr int kSobSums = 2 + 2 * kSobMaxParams;      // the two moments and two numerators per parameter
constexpr int kBootThreads = 512;                    // bootstrap kernel
constexpr int kBootWaves = kBootThreads / kWave;
constexpr int kBootTile = 128;                       // base rows whose terms lie in LDS at a time
constexpr int kSobMaxResamples = kBootThreads;       // one lane per replicate
static_assert(kSobMaxParams == 16 && kBootTile % kBootWaves == 0, "instances below");

// the sum over the 64 lanes, the same bits in every lane (a + b == b + a)
__device__ __forceinline__ double sobol_wave_sum(double v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1)
        v += __shfl_xor(v, d, kWave);
    return v;
}

// ---- point estimates ------------------------------------------------------------------------------------------------
template <int CAP>
__global__ __launch_bounds__(kSobThreads) void smart_sobol_point(long n, int k, const double *__restrict__ y, long ld,
                                                                double *__restrict__ s1, double *__restrict__ st,
                                                                double *__restrict__ moments)
{
    constexpr bool kLds = CAP > 0;
    __shared__ double ya[kLds ? CAP : 1], ub[kLds ? CAP : 1];
    __shared__ double part[kSobWaves][kSobSums];
    __shared__ double fin[kSobSums];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const double *const row = y + (long)blockIdx.x * ld;
    const double dn = (double)n, two_n = 2.0 * dn;

    // ---- 1. A and B: their sum, their smallest and largest value
    double s = 0.0, lo = __builtin_inf(), hi = -__builtin_inf();
    for (long i = tid; i < n; i += kSobThreads) {
        const double a = row[i], b = row[n + i];
        if (kLds) {
            ya[i] = a;
            ub[i] = b;
        }
        s += a + b;
        lo = fmin(lo, fmin(a, b));
        hi = fmax(hi, fmax(a, b));
    }
    s = sobol_wave_sum(s);
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, d, kWave));
        hi = fmax(hi, __shfl_xor(hi, d, kWave));
    }
    if (lane == 0) {
        part[w][0] = s;
        part[w][1] = lo;
        part[w][2] = hi;
    }
    __syncthreads();
    double sab = 0.0;
    lo = __builtin_inf(), hi = -__builtin_inf();
#pragma unroll
    for (int v = 0; v < kSobWaves; ++v) {
        sab += part[v][0];
        lo = fmin(lo, part[v][1]);
        hi = fmax(hi, part[v][2]);
    }
    __syncthreads();
    const double mu = sab / two_n;

    // ---- 2. the two moments about mu; yB becomes uB where it lies
    double p = 0.0, q = 0.0;
    for (long i = tid; i < n; i += kSobThreads) {
        const double ua = (kLds ? ya[i] : row[i]) - mu, u = (kLds ? ub[i] : row[n + i]) - mu;
        if (kLds)
            ub[i] = u;
        p += ua * ua + u * u;
        q += ua + u;
    }
    p = sobol_wave_sum(p);
    q = sobol_wave_sum(q);
    if (lane == 0) {
        part[w][0] = p;
        part[w][1] = q;
    }

    // ---- 3. every AB_j, once
    for (int j = 0; j < k; ++j) {
        const double *const ab = row + (long)(2 + j) * n;
        double c1 = 0.0, ct = 0.0;
        for (long i = tid; i < n; i += kSobThreads) {
            const double a = kLds ? ya[i] : row[i], u = kLds ? ub[i] : row[n + i] - mu;
            const double d = ab[i] - a;
            c1 += u * d;
            ct += d * d;
        }
        c1 = sobol_wave_sum(c1);
        ct = sobol_wave_sum(ct);
        if (lane == 0) {
            part[w][2 + 2 * j] = c1;
            part[w][3 + 2 * j] = ct;
        }
    }
    __syncthreads();
    if (tid < 2 + 2 * k) {
        double t = 0.0;
#pragma unroll
        for (int v = 0; v < kSobWaves; ++v)
            t += part[v][tid];
        fin[tid] = t;
    }
    __syncthreads();
    if (tid >= k)
        return;
    double all = sab;           // the one sum that has taken every value of the row (header comment)
    for (int j = 0; j < k; ++j)
        all += fin[3 + 2 * j];
    const bool clean = is_finite_bits(all);
    const double m1 = fin[1] / two_n;
    const double V = lo == hi ? 0.0 : fin[0] / two_n - m1 * m1;
    const bool ok = clean && V > 0.0;
    const long o = (long)blockIdx.x * k + tid;
    s1[o] = ok ? fin[2 + 2 * tid] / (dn * V) : quiet_nan();
    st[o] = ok ? fin[3 + 2 * tid] / (two_n * V) : quiet_nan();
    if (tid == 0) {
        moments[2 * (long)blockIdx.x] = clean ? mu : quiet_nan();
        moments[2 * (long)blockIdx.x + 1] = clean ? V : quiet_nan();
    }
}

// ---- bootstrap ------------------------------------------------------------------------------------------------------
template <int KP>       // parameters the instance has registers for
__global__ __launch_bounds__(kBootThreads) void smart_sobol_bootstrap(long n, int k, const double *__restrict__ y, long ld,
                                                                     const double *__restrict__ moments,
                                                                     const unsigned short *__restrict__ counts, int B,
                                                                     double *__restrict__ s1_std, double *__restrict__ st_std)
{
    constexpr int NT = 2 + 2 * KP;
    constexpr int kTerms = kBootTile * NT, kComb = (kBootWaves / 2) * NT * kWave;
    __shared__ double sh[kComb > kTerms ? kComb : kTerms];     // the tile's terms, then the registers of a chunk
    __shared__ double first[2 * KP];
    __shared__ double partb[kBootWaves][2 * KP];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const long r = blockIdx.x;
    const double *const row = y + r * ld;
    const double mu = moments[2 * r], V = moments[2 * r + 1];
    if (!is_finite_bits(mu) || !(V > 0.0)) {      // the row's indices are NaN (the same answer in every thread)
        if (tid < k)
            s1_std[r * k + tid] = st_std[r * k + tid] = quiet_nan();
        return;
    }
    const int nbg = (B + kWave - 1) / kWave;        // wavefronts side by side over the replicates, <= 8
    int nchunk = kBootWaves / nbg;                          // ... and over the rows of a tile: 8, 4, 2, 1, 1 ...
    nchunk = 1 << (31 - __clz(nchunk));
    const int bg = w % nbg, chunk = w / nbg, per = kBootTile / nchunk;
    const bool active = chunk < nchunk;
    const int b = bg * kWave + lane;
    const bool live = active && b < B;
    const double dn = (double)n, two_n = 2.0 * dn;

    double acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
        acc[t] = 0.0;
    for (long t0 = 0; t0 < n; t0 += kBootTile) {
        const int rows = (int)(n - t0 < kBootTile ? n - t0 : kBootTile);
        __syncthreads();
        // the terms of base rows t0 .. t0 + rows - 1: thread -> (base row, parameter), adjacent lanes adjacent base rows
        for (int e = tid; e < kBootTile * KP; e += kBootThreads) {
            const int i = e % kBootTile, j = e / kBootTile;
            if (i >= rows)
                continue;
            double *const t = sh + i * NT;
            if (j < k) {
                const long g = t0 + i;
                const double a = row[g], u = row[n + g] - mu, d = row[(long)(2 + j) * n + g] - a;
                t[2 + 2 * j] = u * d;
                t[3 + 2 * j] = d * d;
                if (j == 0) {
                    const double ua = a - mu;
                    t[0] = ua * ua + u * u;
                    t[1] = ua + u;
                }
            } else {
                t[2 + 2 * j] = 0.0;
                t[3 + 2 * j] = 0.0;
            }
        }
        __syncthreads();
        if (active) {
            const int i0 = chunk * per, i1 = i0 + per < rows ? i0 + per : rows;
            // (the counts of four base rows are requested together; the rows themselves one after the other: unrolled, the
            // terms of four rows in flight cost the k <= 16 instance its registers)
            for (int i = i0; i < i1; i += 4) {
                unsigned short c4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    c4[u] = live && i + u < i1 ? counts[(t0 + i + u) * B + b] : (unsigned short)0;
#pragma unroll 1
                for (int u = 0; u < 4; ++u) {
                    if (i + u >= i1)
                        break;
                    const double c = (double)(u == 0 ? c4[0] : u == 1 ? c4[1] : u == 2 ? c4[2] : c4[3]);
                    const double *const t = sh + (i + u) * NT;
#pragma unroll
                    for (int x = 0; x < NT; ++x)
                        acc[x] = fma(c, t[x], acc[x]);
                }
            }
        }
    }
    // the chunks' registers into chunk 0's, in chunk order (nbg <= 4 here: the buffer holds kBootWaves / 2 wavefronts)
    for (int c = 1; c < nchunk; ++c) {
        __syncthreads();
        if (active && chunk == c) {
#pragma unroll
            for (int x = 0; x < NT; ++x)
                sh[(bg * NT + x) * kWave + lane] = acc[x];
        }
        __syncthreads();
        if (chunk == 0) {
#pragma unroll
            for (int x = 0; x < NT; ++x)
                acc[x] += sh[(bg * NT + x) * kWave + lane];
        }
    }

    // ---- the replicate of this lane, then the standard deviation over the replicates about replicate 0's value
    const bool mine = chunk == 0 && b < B;
    const double m1 = acc[1] / two_n, Vb = acc[0] / two_n - m1 * m1;
    double x[2 * KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        x[2 * j] = acc[2 + 2 * j] / (dn * Vb);
        x[2 * j + 1] = acc[3 + 2 * j] / (two_n * Vb);
    }
    if (tid == 0) {
#pragma unroll
        for (int t = 0; t < 2 * KP; ++t)
            first[t] = x[t];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2 * KP; ++t) {
        x[t] = mine ? x[t] - first[t] : 0.0;
        const double s = sobol_wave_sum(x[t]);
        if (lane == 0 && chunk == 0)
            partb[bg][t] = s;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2 * KP; ++t) {
        double m = 0.0;
        for (int g = 0; g < nbg; ++g)
            m += partb[g][t];
        const double e = mine ? x[t] - m / (double)B : 0.0;
        x[t] = e * e;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2 * KP; ++t) {
        const double s = sobol_wave_sum(x[t]);
        if (lane == 0 && chunk == 0)
            partb[bg][t] = s;
    }
    __syncthreads();
    if (tid < 2 * k) {
        double ss = 0.0;
        for (int g = 0; g < nbg; ++g)
            ss += partb[g][tid];
        (tid & 1 ? st_std : s1_std)[r * k + (tid >> 1)] = sqrt(ss / (double)(B - 1));     // B == 1: 0 / 0
    }
}

// ---- launch (validated by smart_analysis_capi.hip) ---------------------------------------------------------------------------
long sobol_lds_capacity() { return kSobLdsCapacity; }
int sobol_max_resamples() { return kSobMaxResamples; }
long sobol_workspace_bytes() { return 0; }      // both kernels keep what they share in the caller's moments[]

void launch_sobol(long n, int k, long M, const double *y, long ld, double *s1, double *st, double *moments,
                  const unsigned short *counts, int B, double *s1_std, double *st_std, hipStream_t s)
{
    const dim3 grid((unsigned)M);
    if (n <= kSobSmall)
        hipLaunchKernelGGL((smart_sobol_point<kSobSmall>), grid, dim3(kSobThreads), 0, s, n, k, y, ld, s1, st, moments);
    else if (n <= kSobLdsCapacity)
        hipLaunchKernelGGL((smart_sobol_point<(int)kSobLdsCapacity>), grid, dim3(kSobThreads), 0, s, n, k, y, ld, s1, st,
                           moments);
    else
        hipLaunchKernelGGL((smart_sobol_point<0>), grid, dim3(kSobThreads), 0, s, n, k, y, ld, s1, st, moments);
    if (B < 1)
        return;
    if (k <= 4)
        hipLaunchKernelGGL((smart_sobol_bootstrap<4>), grid, dim3(kBootThreads), 0, s, n, k, y, ld, moments, counts, B,
                           s1_std, st_std);
    else if (k <= 10)
        hipLaunchKernelGGL((smart_sobol_bootstrap<10>), grid, dim3(kBootThreads), 0, s, n, k, y, ld, moments, counts, B,
                           s1_std, st_std);
    else
        hipLaunchKernelGGL((smart_sobol_bootstrap<16>), grid, dim3(kBootThreads), 0, s, n, k, y, ld, moments, counts, B,
                           s1_std, st_std);
}

} // namespace smart
