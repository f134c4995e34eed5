// smart_dynia.hip -- dynamic identifiability analysis (DYNIA, Wagener et al. 2003) of a stored discharge matrix: for every
// report step r the samples are scored over the MOVING WINDOW |s - r| <= h of observed steps,
//     E[r][n] = sum over the window of |sim[s][n] - obs[s]|          (the SUM: the count is the same for every sample),
// the best `fraction` of them is retained (every tie at the cut stays in), and the retained rows' support -- 1, or
// cut - E -- is shared out over the bins of every factor: shares[r][p][b].  The definition is in include/smart_amd.h.
//
// PASS A, the window sums: one lane per sample, walking time, ADDITIONS ONLY.  A running sum that subtracts the outgoing
// term keeps the cancellation error of a flood's large terms long after the flood has left the window.  Instead time is
// tiled in blocks of w = 2h + 1 rows at the ABSOLUTE positions 0, w, 2w, ...; with t_s the term of row s (0 for a missing
// observation and beyond the record),
//     suffix_b[j] = t_{bw+w-1} + ... + t_{bw+j}   chained from the right,   prefix_b[j] = t_{bw} + ... + t_{bw+j}  from the left,
// the window that starts at row b w + j is suffix_b[j] + prefix_{b+1}[j - 1] (suffix_b[0] alone for j == 0; the windows
// cut at the start of the record are prefix_0[j - 1], block -1 being empty).  Per lane the suffix sums of one block live in
// LDS (w doubles, lds[j][lane]: no bank conflict, no barrier -- a lane only ever touches its own column); the next block is
// read ONCE, forward: its terms go into the slots the walk has just left, its prefix sums are a register, and one backward
// pass over the LDS column turns the terms into the block's suffix sums.  w - 1 additions of non-negative terms per window,
// about two additions and two LDS round trips per element whatever w is.  Block boundaries are absolute, so the association
// of a window's sum depends on (r, h) alone: not on the batch a step falls in, nor on the chunk of blocks (blockIdx.y) that
// computes it -- a chunk first rebuilds the suffix sums of the block before its own.
//
// PASS B, one workgroup per report step: the k-th smallest eligible E by bisection over the key space with integer counts
// (smart_key_select.h: seven thresholds a read), the keys in LDS up to kDyniaLdsCapacity samples and re-read from the
// batch's row beyond; then the
// retained count and S (per thread in index order, a fixed butterfly over the lanes, a fixed chain over the wavefronts);
// then the shares: wavefront p takes factor p, lane b bin b, and walks the row 64 samples at a time -- the retained lanes of
// a ballot hand their (bin, support) to the wavefront one by one, in sample order, and the lane whose bin it is adds it.
// share[p][b] is therefore the sum of its supports in ASCENDING SAMPLE ORDER, one association whatever the instance.  Beyond
// the LDS capacity that walk over the whole row is what a step costs (1,563 dependent load-ballot-branch turns per
// wavefront at N = 1e5), so there the retained rows are first compacted into LDS, in sample order, where they fit
// (kDyniaCompact of them), and the walk is over them alone: the same order, the same bits.
// No floating-point atomics, no atomics at all.
#include "smart_capi_internal.h"
#include "smart_key_select.h"
#include "smart_matrix_common.h"
#include "smart_order_keys.h"
#include <cstdint>

namespace smart {

constexpr int kDyniaMaxHalfWidth = 63;          // pass A: (2 * 63 + 1) * 64 lanes * 8 bytes = 65,024 of the 65,536 a launch gets
constexpr int kDyniaChunk = 8;                  // pass A: blocks of w rows per workgroup (one more is read to start)
constexpr long kDyniaSmallCapacity = 2048;      // pass B: 16 KiB of keys, 256 threads
constexpr long kDyniaLdsCapacity = 16384;       // pass B: 128 KiB of keys, 1024 threads; beyond: the row stays in memory
constexpr int kDyniaCompact = 10240;            // pass B, global form: retained rows compacted in LDS, 12 bytes each = 120 KiB

// ---- count[r]: the observed steps of the window, once per step ------------------------------------------------------
__global__ __launch_bounds__(256) void smart_dynia_count(long R, const double *__restrict__ obs, int h, int *__restrict__ count)
{
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R)
        return;
    const long lo = r - h < 0 ? 0 : r - h, hi = r + h > R - 1 ? R - 1 : r + h;
    int c = 0;
    for (long s = lo; s <= hi; ++s)
        c += is_finite_bits(obs[s]) ? 1 : 0;
    count[r] = c;
}

// ---- pass A ---------------------------------------------------------------------------------------------------------
// the steps r0 .. r0 + nb - 1 into E[(r - r0) * ldE + n]; blockIdx.y takes the blocks bb_first + blockIdx.y * per_chunk ...
// of the walk (a block bb gives the windows that START in block bb - 1).  A step that is not assessed gets NaN.
__global__ __launch_bounds__(kWave) void smart_dynia_sums(long N, long R, const double *__restrict__ sim, long ld,
                                                          const double *__restrict__ obs, int h,
                                                          const int *__restrict__ count, int min_valid, long r0, long nb,
                                                          long bb_first, long bb_last, long per_chunk,
                                                          double *__restrict__ E, long ldE)
{
    extern __shared__ double column[];      // [w][kWave]
    const int w = 2 * h + 1;
    const int lane = threadIdx.x;
    long n = (long)blockIdx.x * kWave + lane;
    const bool live = n < N;
    if (!live)
        n = N - 1;
    const double *col = sim + n;
    double *mine = column + lane;
    const long b_begin = bb_first + (long)blockIdx.y * per_chunk;
    const long b_end = b_begin + per_chunk < bb_last + 1 ? b_begin + per_chunk : bb_last + 1;
    for (long bb = b_begin - 1; bb < b_end; ++bb) {
        if (bb < 0) {       // the block before the record: empty
            for (int j = 0; j < w; ++j)
                mine[j * kWave] = 0.0;
            continue;
        }
        const bool emit = bb >= b_begin;
        double prefix = 0.0;
        for (int j = 0; j < w; ++j) {
            const long s = bb * w + j;
            double t = 0.0;
            if (s < R) {
                const double o = obs[s];
                if (is_finite_bits(o))
                    t = fabs(col[s * ld] - o);
            }
            const long r = s - w + h;       // the step whose window starts at row (bb - 1) w + j
            if (emit && r >= r0 && r < r0 + nb) {
                double v = mine[j * kWave] + prefix;
                if (count[r] < min_valid)
                    v = quiet_nan();
                if (live)
                    E[(r - r0) * ldE + n] = v;
            }
            prefix += t;
            mine[j * kWave] = t;
        }
        double run = 0.0;
        for (int j = w - 1; j >= 0; --j) {
            run += mine[j * kWave];
            mine[j * kWave] = run;
        }
    }
}

// ---- pass B ---------------------------------------------------------------------------------------------------------
__device__ inline double lane_value(double v, int i)    // v of lane i, i the same in every lane
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, i);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), i);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

__device__ inline void dynia_not_assessed(long r, int P, int B, double *__restrict__ shares, double *__restrict__ cut,
                                          int *__restrict__ retained)
{
    for (int i = threadIdx.x; i < P * B; i += blockDim.x)
        shares[r * P * B + i] = quiet_nan();
    if (threadIdx.x == 0) {
        cut[r] = quiet_nan();
        retained[r] = 0;
    }
}

// CAP > 0: the step's keys in LDS (N <= CAP); CAP == 0: re-read from the row
template <int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void smart_dynia_shares(long N, long r0, const double *__restrict__ E, long ldE,
                                                              const int *__restrict__ count, int min_valid, double fraction,
                                                              const unsigned char *__restrict__ cat, int P, int B,
                                                              int support, double *__restrict__ shares,
                                                              double *__restrict__ cut, int *__restrict__ retained)
{
    constexpr int WAVES = THREADS / kWave;
    static_assert(THREADS % kWave == 0 && WAVES <= 16, "shape");
    __shared__ unsigned long long keys[CAP > 0 ? CAP : 1];
    __shared__ unsigned long long ends[2][WAVES];
    __shared__ double part[WAVES];
    __shared__ unsigned counters[kSelectCuts * WAVES];
    __shared__ double packed_s[CAP == 0 ? kDyniaCompact : 1];      // the retained rows of the global form, compacted
    __shared__ int packed_n[CAP == 0 ? kDyniaCompact : 1];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    const long r = r0 + blockIdx.x;
    const double *row = E + (long)blockIdx.x * ldE;

    if (count[r] < min_valid) {
        dynia_not_assessed(r, P, B, shares, cut, retained);
        return;
    }
    if constexpr (CAP > 0) {
        for (long n = tid; n < N; n += THREADS)
            keys[n] = value_key(row[n]);
        __syncthreads();
    }
    auto key_at = [&](long n) -> unsigned long long {
        if constexpr (CAP > 0)
            return keys[n];
        else
            return value_key(row[n]);
    };

    // the eligible rows: their number, their smallest and largest key
    unsigned long long kmin = kKeyPad, kmax = 0;
    for (long n = tid; n < N; n += THREADS) {
        const unsigned long long key = key_at(n);
        if (key < kKeyPlusInf) {
            kmin = key < kmin ? key : kmin;
            kmax = key > kmax ? key : kmax;
        }
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
    const unsigned M = block_count<THREADS>([&](long n) { return key_at(n) < kKeyPlusInf; }, N, counters); // (publishes ends)
    if (M == 0) {
        dynia_not_assessed(r, P, B, shares, cut, retained);
        return;
    }
    for (int v = 0; v < WAVES; ++v) {
        kmin = ends[0][v] < kmin ? ends[0][v] : kmin;
        kmax = ends[1][v] > kmax ? ends[1][v] : kmax;
    }
    long long k = (long long)ceil(fraction * (double)M);
    k = k < 1 ? 1 : k;
    const unsigned long long cut_key = select_kth_key<THREADS>(key_at, N, (unsigned)k, kmin, kmax, counters);
    const double cut_value = key_value(cut_key);

    // the retained rows: their number, and S = the sum of cut - E over them
    const unsigned kept = block_count<THREADS>([&](long n) { return key_at(n) <= cut_key; }, N, counters);
    double S = 0.0;
    if (support == SMART_DYNIA_LINEAR) {
        for (long n = tid; n < N; n += THREADS) {
            const unsigned long long key = key_at(n);
            if (key <= cut_key)
                S += cut_value - key_value(key);
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1)
            S += __shfl_xor(S, d, kWave);
        if (lane == 0)
            part[wave] = S;
        __syncthreads();
        S = part[0];
        for (int v = 1; v < WAVES; ++v)
            S += part[v];
    }
    const bool linear = support == SMART_DYNIA_LINEAR && S > 0.0;   // S == 0: every retained row ties at the cut
    const double total = linear ? S : (double)kept;

    // the global form first COMPACTS the retained rows into LDS, in sample order, where they fit: wavefront v owns the v-th
    // contiguous part of the row, counts its retained rows, and -- the counts chained over the wavefronts -- writes their
    // (support, sample) behind those of the parts before it.  The walk below is then over kept entries, not over N.
    bool compacted = false;
    if constexpr (CAP == 0) {
        if (kept <= (unsigned)kDyniaCompact) {
            const long part_len = ((N + WAVES * kWave - 1) / (WAVES * kWave)) * kWave;
            const long beg = wave * part_len, end = beg + part_len < N ? beg + part_len : N;
            unsigned mine = 0;
            for (long n0 = beg; n0 < end; n0 += kWave) {
                const long n = n0 + lane;
                const unsigned long long key = n < end ? key_at(n) : kKeyPad;
                mine += (unsigned)__popcll(__ballot(key <= cut_key));
            }
            if (lane == 0)
                counters[wave] = mine;
            __syncthreads();
            unsigned at = 0;
            for (int v = 0; v < wave; ++v)
                at += counters[v];
            for (long n0 = beg; n0 < end; n0 += kWave) {
                const long n = n0 + lane;
                const unsigned long long key = n < end ? key_at(n) : kKeyPad;
                const bool in = key <= cut_key;
                const unsigned long long mask = __ballot(in);
                if (in) {
                    const unsigned pos = at + (unsigned)__popcll(mask & ((1ull << lane) - 1));
                    packed_s[pos] = linear ? cut_value - key_value(key) : 1.0;
                    packed_n[pos] = (int)n;
                }
                at += (unsigned)__popcll(mask);
            }
            __syncthreads();
            compacted = true;
        }
    }

    // wavefront p takes factor p, lane b bin b: the retained rows hand over (bin, support) one by one, in sample order
    for (int p = wave; p < P; p += WAVES) {
        const unsigned char *bins = cat + (long)p * N;
        double acc = 0.0;
        if (compacted) {
            for (unsigned i0 = 0; i0 < kept; i0 += kWave) {
                const unsigned i = i0 + lane;
                const int bin = i < kept ? (int)bins[packed_n[i]] : 255;
                const double s = i < kept ? packed_s[i] : 0.0;
                const int here = kept - i0 < (unsigned)kWave ? (int)(kept - i0) : kWave;
                for (int j = 0; j < here; ++j) {
                    const int bi = __builtin_amdgcn_readlane(bin, j);
                    const double sj = lane_value(s, j);
                    if (lane == bi)
                        acc += sj;
                }
            }
        } else {
            for (long n0 = 0; n0 < N; n0 += kWave) {
                const long n = n0 + lane;
                const unsigned long long key = n < N ? key_at(n) : kKeyPad;
                const bool in = key <= cut_key;
                unsigned long long mask = __ballot(in);
                if (mask == 0)
                    continue;
                const int bin = in ? (int)bins[n] : 255;
                const double s = linear ? cut_value - key_value(key) : 1.0;
                while (mask) {
                    const int i = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const int bi = __builtin_amdgcn_readlane(bin, i);
                    const double si = lane_value(s, i);
                    if (lane == bi)
                        acc += si;
                }
            }
        }
        if (lane < B)
            shares[(r * P + p) * B + lane] = acc / total;
    }
    if (tid == 0) {
        cut[r] = cut_value;
        retained[r] = (int)kept;
    }
}

// ---- launch (validated by smart_analysis_capi.hip) -----------------------------------------------------------------
int dynia_max_half_width() { return kDyniaMaxHalfWidth; }

long dynia_lds_capacity() { return kDyniaLdsCapacity; }

long dynia_step_bytes(long N) { return N * 8; }

static long floor_div(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

void launch_dynia(long N, long R, const double *sim, long ld, const double *obs, int h, int min_valid, double fraction,
                  const unsigned char *cat, int P, int B, int support, double *shares, double *cut, int *retained,
                  int *count, double *err, long ld_err, void *workspace, long workspace_bytes, hipStream_t s)
{
    const long w = 2l * h + 1;
    hipLaunchKernelGGL(smart_dynia_count, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, R, obs, h, count);
    // the E sums of a batch of steps: in err where it is wanted (every step at once), else in the workspace
    double *E = err ? err : (double *)workspace;
    const long ldE = err ? ld_err : N;
    for_each_batch(R, err ? R : workspace_steps(workspace_bytes, dynia_step_bytes(N)), [&](long r0, long nb) {
        const long bb_first = floor_div(r0 - h, w) + 1, bb_last = floor_div(r0 + nb - 1 - h, w) + 1;
        const long blocks = bb_last - bb_first + 1;
        long per_chunk = (blocks + 32767) / 32768;
        per_chunk = per_chunk < kDyniaChunk ? kDyniaChunk : per_chunk;
        const dim3 grid((unsigned)((N + kWave - 1) / kWave), (unsigned)((blocks + per_chunk - 1) / per_chunk));
        hipLaunchKernelGGL(smart_dynia_sums, grid, dim3(kWave), (size_t)(w * kWave * 8), s, N, R, sim, ld, obs, h, count,
                           min_valid, r0, nb, bb_first, bb_last, per_chunk, E, ldE);
        const dim3 steps((unsigned)nb);
        if (N <= kDyniaSmallCapacity)
            hipLaunchKernelGGL((smart_dynia_shares<(int)kDyniaSmallCapacity, 256>), steps, dim3(256), 0, s, N, r0, E, ldE,
                               count, min_valid, fraction, cat, P, B, support, shares, cut, retained);
        else if (N <= kDyniaLdsCapacity)
            hipLaunchKernelGGL((smart_dynia_shares<(int)kDyniaLdsCapacity, 1024>), steps, dim3(1024), 0, s, N, r0, E, ldE,
                               count, min_valid, fraction, cat, P, B, support, shares, cut, retained);
        else
            hipLaunchKernelGGL((smart_dynia_shares<0, 1024>), steps, dim3(1024), 0, s, N, r0, E, ldE, count, min_valid,
                               fraction, cat, P, B, support, shares, cut, retained);
    });
}

} // namespace smart
