// smart_pawn.hip -- PAWN sensitivity from the sample at hand (Pianosi & Wagener 2015, 2018): per row r of a matrix y[R][ld]
// (sample-minor: a report step of the discharge matrix, or any per-row table) and per bin b of factor p, the
// Kolmogorov-Smirnov distance between the empirical CDF of all N values and that of the n_b values whose row lies in the
// bin.  The definition is in include/smart_amd.h (smart_pawn_ks_hip).  With the row sorted ascending (order keys:
// smart_order_keys.h), position i an EVALUATION POINT where i == N - 1 or key[i] != key[i + 1] (the end of a run of ties),
// and c_b(i) the number of positions <= i whose row lies in bin b,
//     num[r][p][b] = max over the evaluation points i of |(i + 1) n_b - c_b(i) N|,      ks = num / (N n_b).
// INTEGERS UNTIL THE ONE DIVISION.  (i + 1) n_b and c_b(i) N are below 2^48 and so is their difference; they are held in
// doubles, where every product, the fused multiply-add that takes the difference and the maximum are EXACT (nothing is
// rounded below 2^53): the result is the integer the definition names, whatever the order of the work -- the launch, the
// batch, the form, the segments.  N n_b is exact too, and the quotient is the one correctly rounded division.
//
// One workgroup per row, two forms, the same walk:
//   LDS     N <= kPawnCapacity.  Keys and 16-bit sample indices in LDS (10 bytes per element, 80 KiB at 8192), sorted by
//           bitonic_merge_lds of smart_order_stats.h as it is.
//   global  any N <= 2^24.  (key, 32-bit index) pairs in the caller's workspace, padded to a power of two P >= kPawnBlock:
//           blocks sorted in LDS, the stages that reach past a block on the workspace (bitonic_long_stages), the shorter
//           ones block by block in LDS.  ONE workgroup owns one row's buffer: __syncthreads() is the only ordering.  The
//           evaluation flag of a position is then written into bit 31 of its index, so the walk reads 4 bytes a position.
// THE WALK.  The sorted positions are cut into one contiguous SEGMENT per wavefront.  The lanes of every wavefront stand
// for (factor, bin) slots: G = 64 / B factors are walked together, lane l for bin l % B of the l / B-th factor of the group
// (ten bins: six factors a pass, thirteen factors in three passes).  A wavefront takes 64 positions at a time: per factor
// of the group every lane fetches the bin of one position (cat[p][index]: a byte gathered through L2, the table is at most
// 16 N bytes), six ballots over the bits of the bin give the lanes of that factor the 64-bit MASK of the positions that lie
// in their bin (bin_mask), and the popcount of the mask is the bin's count.
// First the segment's counts (LDS form: the masks stay in registers; global form: a pass of its own), an exclusive scan of
// them over the segments gives every wavefront the counts its segment starts from -- and their total is n_b --, then the
// wavefront visits the evaluation points of its segment (a scalar loop over the set bits of the evaluation mask):
// c_b(i) = start + popcount(mask up to i).  A run of ties that crosses a segment boundary needs nothing special: the
// evaluation test reads key[i + 1].  The maxima of the segments are joined through LDS.  No atomics of any kind.
#include "smart_capi_internal.h"
#include "smart_matrix_common.h"
#include "smart_order_stats.h"
#include <cstdint>

namespace smart {

constexpr long kPawnCapacity = 8192;            // LDS form: 8192 * (8 + 2) bytes = 80 KiB of the 160 KiB of a compute unit
constexpr int kPawnBlock = 4096;                // global form: elements of one LDS block, (8 + 4) bytes each = 48 KiB
constexpr int kPawnGlobalThreads = 1024;
constexpr long kPawnMaxSamples = 1l << 24;
constexpr unsigned kPawnEval = 0x80000000u;     // global form: bit 31 of a sorted index = the position is an evaluation point
static_assert(kPawnCapacity <= 32768, "sample indices are kept as 16-bit numbers");
static_assert(SMART_PAWN_MAX_BINS <= kWave, "a lane stands for one bin of one factor");

// a lane that stands for bin b: the mask of the lanes whose position is valid and lies in bin b (bin >= n_bins: in no
// lane's mask)
__device__ inline unsigned long long bin_mask(int bin, bool valid, int n_bins, int b)
{
    unsigned long long m = __ballot(valid && bin < n_bins);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned long long has = __ballot((bin >> k) & 1);
        m &= ((b >> k) & 1) ? has : ~has;
    }
    return m;
}

// the lanes of a wavefront stand for (factor, bin) SLOTS: with B bins, G = 64 / B factors are walked together, lane l for
// bin l % B of the l / B-th factor of the group (the lanes beyond G B idle).  Ten bins: six factors a pass.
struct PawnSlot {
    int group;      // G
    int factor;     // of the group, this lane's
    int bin;        // this lane's
};

__device__ inline PawnSlot pawn_slot(int B, int lane)
{
    PawnSlot s;
    s.group = kWave / B;
    s.factor = lane / B;
    s.bin = lane - s.factor * B;
    return s;
}

// the masks of 64 positions for the `here` factors of a group: bins(g) is the bin of this lane's position on the g-th
// factor of the group; every lane keeps the mask of its own factor (a lane beyond the group: none)
template <typename F>
__device__ inline unsigned long long slot_mask(F bins, int here, bool valid, int B, const PawnSlot &slot)
{
    unsigned long long mask = 0;
    for (int g = 0; g < here; ++g) {
        const unsigned long long m = bin_mask(bins(g), valid, B, slot.bin);
        if (slot.factor == g)
            mask = m;
    }
    return mask;
}

// the evaluation points `ev` of the 64 positions i0 .. i0 + 63, for a lane with the positions of its bin in `mask` and
// `before` of them ahead of i0: best = max(best, |(i + 1) n_b - c_b(i) N|), every value an exact integer in a double
__device__ inline void pawn_chunk(unsigned long long mask, unsigned long long ev, int i0, int before, double nb, double Nd,
                                  double &best)
{
    while (ev) {    // (the same in every lane)
        const int j = __ffsll((long long)ev) - 1;
        ev &= ev - 1;
        const int c = before + __popcll(mask & ((2ull << j) - 1));
        const double d = fma((double)(i0 + j + 1), nb, -((double)c * Nd));
        best = fmax(best, fabs(d));
    }
}

// the counts of the segments -> what lies ahead of segment `wave` and n_b, for this lane's slot (publishes seg_count)
template <int WAVES>
__device__ inline void pawn_scan(int mine, int (*seg_count)[kWave], int wave, int lane, int &before, int &total)
{
    seg_count[wave][lane] = mine;
    __syncthreads();
    before = 0;
    total = 0;
    for (int v = 0; v < WAVES; ++v) {
        if (v == wave)
            before = total;
        total += seg_count[v][lane];
    }
}

// the maxima of the segments -> ks[p][b] of the row for the `live` slots of a group (two barriers a group: seg_count and
// seg_best are written again behind the second one of this group and the first one of the next at the earliest, and
// their readers are through by then)
template <int WAVES>
__device__ inline void pawn_finish(double best, int total, double (*seg_best)[kWave], int wave, int lane, double Nd, int live,
                                   double *__restrict__ out)
{
    seg_best[wave][lane] = best;
    __syncthreads();
    if (wave == 0 && lane < live) {
        double num = seg_best[0][lane];
        for (int v = 1; v < WAVES; ++v)
            num = fmax(num, seg_best[v][lane]);
        out[lane] = total > 0 ? num / (Nd * (double)total) : quiet_nan();
    }
}

__device__ inline void pawn_row_nan(int P, int B, double *__restrict__ out)
{
    for (int i = threadIdx.x; i < P * B; i += blockDim.x)
        out[i] = quiet_nan();
}

// ---- counts[p][b], once per call: one workgroup per factor ----------------------------------------------------------
__global__ __launch_bounds__(1024) void smart_pawn_counts(int N, const unsigned char *__restrict__ cat, int B,
                                                          int *__restrict__ counts)
{
    constexpr int WAVES = 1024 / kWave;
    __shared__ int seg_count[WAVES][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned char *bins = cat + (long)blockIdx.x * N;
    int mine = 0;
    for (int n0 = wave * kWave; n0 < N; n0 += WAVES * kWave) {
        const int n = n0 + lane;
        const bool valid = n < N;
        mine += __popcll(bin_mask(valid ? (int)bins[n] : 255, valid, B, lane));     // (lane b: bin b)
    }
    int before, total;
    pawn_scan<WAVES>(mine, seg_count, wave, lane, before, total);
    if (wave == 0 && lane < B)
        counts[blockIdx.x * B + lane] = total;
}

// ---- LDS form -----------------------------------------------------------------------------------------------------
template <int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void smart_pawn_lds(int N, const double *__restrict__ y, long ld,
                                                          const unsigned char *__restrict__ cat, int P, int B,
                                                          double *__restrict__ ks)
{
    constexpr int WAVES = THREADS / kWave;
    constexpr int CHUNKS = CAP / (WAVES * kWave);       // of 64 positions, per segment
    static_assert(CAP % (WAVES * kWave) == 0 && THREADS % kWave == 0 && WAVES <= 16 && CAP <= kPawnCapacity, "shape");
    __shared__ unsigned long long keys[CAP];
    __shared__ unsigned short idx[CAP];
    __shared__ int seg_count[WAVES][kWave];
    __shared__ double seg_best[WAVES][kWave];

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    const long r = blockIdx.x;
    const double *row = y + r * ld;
    double *out = ks + r * P * B;

    for (int n = tid; n < CAP; n += THREADS) {
        keys[n] = n < N ? value_key(row[n]) : kKeyPad;
        idx[n] = (unsigned short)n;
    }
    __syncthreads();
    for (int k = 2; k <= CAP; k <<= 1)
        bitonic_merge_lds<CAP, THREADS, true, unsigned short>(keys, idx, k, k >> 1, 0);
    if (keys[0] <= kKeyMinusInf || keys[N - 1] >= kKeyPlusInf) {    // a value that is not finite (every thread alike)
        pawn_row_nan(P, B, out);
        return;
    }
    // the segment of this wavefront: its evaluation points and the sample index of its positions
    const int beg = wave * CHUNKS * kWave;
    unsigned long long ev[CHUNKS];
    int sample[CHUNKS];
#pragma unroll
    for (int ch = 0; ch < CHUNKS; ++ch) {
        const int i = beg + ch * kWave + lane;
        ev[ch] = __ballot(i < N && (i == N - 1 || keys[i] != keys[i + 1]));
        sample[ch] = i < N ? (int)idx[i] : -1;
    }
    const double Nd = (double)N;
    const PawnSlot slot = pawn_slot(B, lane);
    for (int p0 = 0; p0 < P; p0 += slot.group) {
        const int here = P - p0 < slot.group ? P - p0 : slot.group;
        unsigned long long mask[CHUNKS];
        int mine = 0;
#pragma unroll
        for (int ch = 0; ch < CHUNKS; ++ch) {
            const bool valid = sample[ch] >= 0;
            const unsigned char *mine_in = cat + (long)p0 * N + (valid ? sample[ch] : 0);
            mask[ch] = slot_mask([&](int g) { return valid ? (int)mine_in[(long)g * N] : 255; }, here, valid, B, slot);
            mine += __popcll(mask[ch]);
        }
        int before, total;
        pawn_scan<WAVES>(mine, seg_count, wave, lane, before, total);
        const double nb = (double)total;
        double best = 0.0;
#pragma unroll
        for (int ch = 0; ch < CHUNKS; ++ch) {
            pawn_chunk(mask[ch], ev[ch], beg + ch * kWave, before, nb, Nd, best);
            before += __popcll(mask[ch]);
        }
        pawn_finish<WAVES>(best, total, seg_best, wave, lane, Nd, here * B, out + p0 * B);
    }
}

// ---- global form --------------------------------------------------------------------------------------------------
// the workspace of row r0 + blockIdx.x: P2 keys, then P2 32-bit sample indices
__global__ __launch_bounds__(kPawnGlobalThreads) void smart_pawn_global(int N, int P2, long r0, const double *__restrict__ y,
                                                                        long ld, const unsigned char *__restrict__ cat, int P,
                                                                        int B, double *__restrict__ ks, unsigned char *workspace)
{
    constexpr int THREADS = kPawnGlobalThreads;
    constexpr int WAVES = THREADS / kWave;
    __shared__ unsigned long long lk[kPawnBlock];
    __shared__ unsigned li[kPawnBlock];
    __shared__ int seg_count[WAVES][kWave];
    __shared__ double seg_best[WAVES][kWave];

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    const long r = r0 + blockIdx.x;
    const double *row = y + r * ld;
    double *out = ks + r * P * B;
    unsigned long long *kg = reinterpret_cast<unsigned long long *>(workspace + (long)blockIdx.x * P2 * 12);
    unsigned *ig = reinterpret_cast<unsigned *>(kg + P2);
    const int blocks = P2 / kPawnBlock;

    // every block of kPawnBlock elements sorted in LDS, ascending or descending by its place in the sequence
    for (int blk = 0; blk < blocks; ++blk) {
        const int g0 = blk * kPawnBlock;
        for (int t = tid; t < kPawnBlock; t += THREADS) {
            const int n = g0 + t;
            lk[t] = n < N ? value_key(row[n]) : kKeyPad;
            li[t] = (unsigned)n;
        }
        __syncthreads();
        for (int k = 2; k <= kPawnBlock; k <<= 1)
            bitonic_merge_lds<kPawnBlock, THREADS, true, unsigned>(lk, li, k, k >> 1, g0);
        for (int t = tid; t < kPawnBlock; t += THREADS) {
            kg[g0 + t] = lk[t];
            ig[g0 + t] = li[t];
        }
        __syncthreads();
    }
    // the merges beyond a block: long stages on the workspace, the short ones block by block in LDS
    for (int k = 2 * kPawnBlock; k <= P2; k <<= 1) {
        bitonic_long_stages<kPawnBlock, THREADS, unsigned>(kg, ig, P2, k);
        for (int blk = 0; blk < blocks; ++blk) {
            const int g0 = blk * kPawnBlock;
            for (int t = tid; t < kPawnBlock; t += THREADS) {
                lk[t] = kg[g0 + t];
                li[t] = ig[g0 + t];
            }
            __syncthreads();
            bitonic_merge_lds<kPawnBlock, THREADS, true, unsigned>(lk, li, k, kPawnBlock >> 1, g0);
            for (int t = tid; t < kPawnBlock; t += THREADS) {
                kg[g0 + t] = lk[t];
                ig[g0 + t] = li[t];
            }
            __syncthreads();
        }
    }
    if (kg[0] <= kKeyMinusInf || kg[N - 1] >= kKeyPlusInf) {      // a value that is not finite (every thread alike)
        pawn_row_nan(P, B, out);
        return;
    }
    // the evaluation flag of every position beside its index: the walk reads the indices alone
    for (int i = tid; i < N; i += THREADS)
        if (i == N - 1 || kg[i] != kg[i + 1])
            ig[i] |= kPawnEval;
    __syncthreads();

    const int seg = ((N + THREADS - 1) / THREADS) * kWave;      // positions of a segment, whole chunks of 64
    const long first = (long)wave * seg;
    const int beg = first < N ? (int)first : N, end = first + seg < N ? (int)(first + seg) : N;
    const double Nd = (double)N;
    const PawnSlot slot = pawn_slot(B, lane);
    for (int p0 = 0; p0 < P; p0 += slot.group) {
        const int here = P - p0 < slot.group ? P - p0 : slot.group;
        const unsigned char *group = cat + (long)p0 * N;
        int mine = 0;
        for (int i0 = beg; i0 < end; i0 += kWave) {
            const int i = i0 + lane;
            const bool valid = i < end;
            const unsigned at = valid ? ig[i] & ~kPawnEval : 0u;
            mine += __popcll(slot_mask([&](int g) { return valid ? (int)group[(long)g * N + at] : 255; }, here, valid, B, slot));
        }
        int before, total;
        pawn_scan<WAVES>(mine, seg_count, wave, lane, before, total);
        const double nb = (double)total;
        double best = 0.0;
        for (int i0 = beg; i0 < end; i0 += kWave) {
            const int i = i0 + lane;
            const bool valid = i < end;
            const unsigned word = valid ? ig[i] : 0u;
            const unsigned at = word & ~kPawnEval;
            const unsigned long long mask =
                slot_mask([&](int g) { return valid ? (int)group[(long)g * N + at] : 255; }, here, valid, B, slot);
            pawn_chunk(mask, __ballot((word & kPawnEval) != 0), i0, before, nb, Nd, best);
            before += __popcll(mask);
        }
        pawn_finish<WAVES>(best, total, seg_best, wave, lane, Nd, here * B, out + p0 * B);
    }
}

// ---- launch (validated by smart_analysis_capi.hip) -------------------------------------------------------------------
long pawn_lds_capacity() { return kPawnCapacity; }

long pawn_max_samples() { return kPawnMaxSamples; }

long pawn_step_bytes(long N) { return padded_pow2(N, kPawnBlock) * 12; }

void launch_pawn(long N, long R, const double *y, long ld, const unsigned char *cat, int P, int B, double *ks, int *counts,
                 bool lds, void *workspace, long workspace_bytes, hipStream_t s)
{
    hipLaunchKernelGGL(smart_pawn_counts, dim3((unsigned)P), dim3(1024), 0, s, (int)N, cat, B, counts);
    if (lds) {
        sort_instance<(int)kPawnCapacity>(N, [&](auto cap, auto threads) {
            hipLaunchKernelGGL((smart_pawn_lds<cap(), threads()>), dim3((unsigned)R), dim3(threads()), 0, s, (int)N, y, ld,
                               cat, P, B, ks);
        });
        return;
    }
    // rows in batches of as many as the workspace holds, one launch per batch
    const long P2 = padded_pow2(N, kPawnBlock);
    for_each_batch(R, workspace_steps(workspace_bytes, pawn_step_bytes(N)), [&](long r0, long steps) {
        hipLaunchKernelGGL(smart_pawn_global, dim3((unsigned)steps), dim3(kPawnGlobalThreads), 0, s, (int)N, (int)P2, r0, y,
                           ld, cat, P, B, ks, (unsigned char *)workspace);
    });
}

} // namespace smart
