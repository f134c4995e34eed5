// smart_nsga2.hip -- one generation of NSGA-II (Deb et al. 2002: non-dominated sorting, crowding distance, truncation over
// parents and offspring) with the variation of differential evolution on that selection (NSDE / GDE3), around the ensemble
// launch that scores the offspring.  The definition -- who takes part, the ranks, the value-based crowding distance, the
// total order, the draw layout, the order of the operations -- is in include/smart_amd.h (smart_nsga2_step_hip) and DESIGN.md
// section 4.22; this file says it once more in HIP.
//
// SURVIVE, over the E <= 2 N candidates (their numbers are the order: nothing is compacted):
//   smart_nsga2_keys       one lane per candidate: who takes part, the keys padded to four in the workspace (a candidate that
//                          does not take part, and the padding up to a whole mask word, hold NaN keys: every compare with
//                          them is false, so the pair loops need no flag and no ragged end)
//   smart_nsga2_dominance  the pair form of smart_pareto_count: the candidate's keys in registers, the challengers through
//                          wave-uniform loads, sliced over grid.y in whole words of 64 challengers.  Each lane builds its own
//                          words of the bit matrix D[word][candidate] (word-major: a wavefront's loads and stores of one
//                          word are contiguous) -- bit b of D[w][i]: candidate 64 w + b dominates i.  No atomics.
//   smart_nsga2_first      count[i] = the bits of column i; front 1 = the candidates that take part with count 0
//   smart_nsga2_peel       one launch per further front r: count[i] -= popcount(D[.][i] & the mask of front r - 1) for the
//                          candidates still unranked (only the mask words that are not zero are read), rank r where the
//                          count reaches 0.  A wavefront's 64 candidates are one mask word: a ballot writes it.  cum[r] =
//                          the candidates ranked up to front r (an integer counter: wavefronts add their popcounts).  A pass
//                          that finds cum[r - 1] >= N, or cum[r - 1] == cum[r - 2] (an empty front: none is left), returns
//                          at once, hands cum[r - 1] on and sets the flag the host reads once per batch of passes.
//   smart_nsga2_neighbours pair form again, the challengers in slices over grid.y: per challenger of the same rank, min, max,
//                          L and U per objective
//   smart_nsga2_crowding   the slices joined (minima and maxima: exact in any order), then the sum over the objectives
//   smart_nsga2_count_before  pair form again, sliced: the number of predecessors under (rank, -distance, e), the slices
//                          added into one integer per candidate
//   smart_nsga2_place      pos(e) = that number; the survivors scatter themselves (parameters, keys, payload, flags) into
//                          the NEXT population
// VARY:
//   smart_nsga2_vary       one lane per offspring: the tournament and the partners here, the move itself in smart_de_move.h
//                          (shared with smart_demcz_propose)
// ARITHMETIC.  The unit is compiled with -ffp-contract=off: every operation is rounded once, as the numpy statement of the
// tests rounds it; there is no operation here that is not correctly rounded (no pow, no log).
#include "smart_capi_internal.h"
#include "smart_de_move.h"
#include "smart_matrix_common.h"
#include <cstdint>

namespace smart {

constexpr int kNsThreads = 256;     // keys, dominance, first, peel, vary
constexpr int kNsPairThreads = 64;  // crowding, place: every lane walks all E challengers, so more, smaller workgroups
constexpr int kNsKeys = 4;          // a candidate's keys in the workspace: 32 bytes, whatever M is
constexpr int kNsMaxSlices = 64;    // grid.y of the dominance kernel
constexpr int kNsPartial = 4 * kNsKeys;     // doubles a slice of the crowding pass leaves per candidate: min, max, U, L per key
constexpr int kNsMaxPairSlices = 16;        // grid.y of the crowding and place passes
constexpr long kNsAlign = 256;      // of the workspace's parts
constexpr int kNsFirstBatch = 16, kNsMaxBatch = 1024;
constexpr int kRankBeyond = SMART_NSGA2_RANK_BEYOND, kRankOut = SMART_NSGA2_RANK_OUT;
static_assert(SMART_NSGA2_MAX_OBJECTIVES == kNsKeys, "the padded keys");
static_assert(SMART_NSGA2_MAX_CARRY == 16, "the arrays below");

typedef unsigned long long u64;

// ---- the workspace: ctl[2] | cum[N + 8] | mask[2][W] | keys[Eld][4] | part[Eld] | count[Eld] | rank[Eld] | dist[Eld] |
// D[max(W, 16)][Eld], for 2 N candidates: W = ceil(2 N / 64) mask words, Eld = 64 W
struct Nsga2Workspace {
    int W;
    long Eld;
    int *ctl, *cum;
    u64 *mask;
    double *keys;
    unsigned char *part;
    int *count, *rank;
    double *dist;
    u64 *D;
    long bytes;
};

static long ns_part(long bytes) { return (bytes + kNsAlign - 1) / kNsAlign * kNsAlign; }

static Nsga2Workspace nsga2_layout(long N, void *workspace)
{
    Nsga2Workspace w;
    w.W = (int)((2 * N + 63) / 64);
    w.Eld = 64l * w.W;
    char *p = (char *)workspace;
    auto take = [&](long bytes) {
        char *at = p;
        p += ns_part(bytes);
        return at;
    };
    w.ctl = (int *)take(2 * 4);
    w.cum = (int *)take((N + 8) * 4);
    w.mask = (u64 *)take(2l * w.W * 8);
    w.keys = (double *)take(w.Eld * kNsKeys * 8);
    w.part = (unsigned char *)take(w.Eld);
    w.count = (int *)take(w.Eld * 4);
    w.rank = (int *)take(w.Eld * 4);
    w.dist = (double *)take(w.Eld * 8);
    // (at least 16 words per candidate: once the fronts are peeled the matrix is done with, and the crowding kernels keep
    // their partial results there -- 16 doubles per candidate and slice)
    w.D = (u64 *)take((long)(w.W > kNsPartial ? w.W : kNsPartial) * w.Eld * 8);
    w.bytes = (long)(p - (char *)workspace);
    return w;
}

long nsga2_workspace_bytes(long N) { return nsga2_layout(N, nullptr).bytes; }

// ---- keys -----------------------------------------------------------------------------------------------------------
struct Nsga2Columns {
    int col[kNsKeys];
    int dir[kNsKeys];
    double target[kNsKeys];
};

__global__ __launch_bounds__(kNsThreads) void smart_nsga2_keys(int E, int Epad, int Np, int M,
                                                               const double *__restrict__ pop_keys,
                                                               const unsigned char *__restrict__ pop_part,
                                                               const unsigned char *__restrict__ out,
                                                               const double *__restrict__ scores, long ld, Nsga2Columns kc,
                                                               const unsigned char *__restrict__ eligible,
                                                               double *__restrict__ keys, unsigned char *__restrict__ part,
                                                               int *__restrict__ rank, double *__restrict__ dist)
{
    const int e = blockIdx.x * kNsThreads + threadIdx.x;
    if (e >= Epad)
        return;
    const double nan = __builtin_nan("");
    double k[kNsKeys] = {nan, nan, nan, nan};
    bool takes = false;
    if (e < Np) {
        takes = pop_part[e] != 0;
        for (int m = 0; m < M; ++m)
            k[m] = pop_keys[(long)e * M + m];
    } else if (e < E) {
        const int c = e - Np;
        const double *const row = scores + (long)c * ld;
        takes = out[c] == 0 && (!eligible || eligible[c] != 0);
        double x[kNsKeys] = {0.0, 0.0, 0.0, 0.0};
        for (int m = 0; m < M; ++m) {
            x[m] = row[kc.col[m]];
            takes = takes && !is_nan_bits(x[m]);
        }
        if (takes) {
            for (int m = 0; m < M; ++m) {
                const int d = kc.dir[m];
                k[m] = d == SMART_PARETO_MAX ? x[m] : (d == SMART_PARETO_MIN ? -x[m] : -fabs(x[m] - kc.target[m]));
            }
        }
    }
    for (int m = 0; m < kNsKeys; ++m)
        keys[(long)e * kNsKeys + m] = m < M ? k[m] : 0.0;
    part[e] = takes ? 1 : 0;
    rank[e] = takes ? kRankBeyond : kRankOut;
    dist[e] = 0.0;
}

// ---- dominance ------------------------------------------------------------------------------------------------------
// does the challenger at c dominate the lane's candidate?  c is the same address in every lane (a scalar load); a NaN key on
// either side makes every compare false
template <int M>
__device__ __forceinline__ unsigned ns_beats(const double *__restrict__ c, const double (&mine)[M])
{
    bool ge = c[0] >= mine[0], le = c[0] <= mine[0];
#pragma unroll
    for (int m = 1; m < M; ++m) {
        ge = ge && c[m] >= mine[m];
        le = le && c[m] <= mine[m];
    }
    return ge && !le ? 1u : 0u;
}

template <int M>
__global__ __launch_bounds__(kNsThreads) void smart_nsga2_dominance(int E, int We, int words_per_slice, long Eld,
                                                                    const double *__restrict__ keys, u64 *__restrict__ D)
{
    const int i = blockIdx.x * kNsThreads + threadIdx.x;
    const bool live = i < E;
    const double *const own = keys + (long)(live ? i : E - 1) * kNsKeys;
    double mine[M];
#pragma unroll
    for (int m = 0; m < M; ++m)
        mine[m] = own[m];
    const int w0 = blockIdx.y * words_per_slice;
    const int w1 = w0 + words_per_slice < We ? w0 + words_per_slice : We;
    for (int w = w0; w < w1; ++w) {
        const double *c = keys + (long)w * 64 * kNsKeys;
        unsigned lo = 0, hi = 0;
#pragma unroll 8
        for (int b = 0; b < 32; ++b)
            lo |= ns_beats<M>(c + b * kNsKeys, mine) << b;
        c += 32 * kNsKeys;
#pragma unroll 8
        for (int b = 0; b < 32; ++b)
            hi |= ns_beats<M>(c + b * kNsKeys, mine) << b;
        if (live)
            D[(long)w * Eld + i] = (u64)lo | ((u64)hi << 32);
    }
}

// ---- the fronts -----------------------------------------------------------------------------------------------------
// (both kernels run whole wavefronts to the ballot: lane i of the grid is bit i % 64 of mask word i / 64)
__global__ __launch_bounds__(kNsThreads) void smart_nsga2_first(int E, int We, long Eld, const u64 *__restrict__ D,
                                                                int *__restrict__ count, int *__restrict__ rank,
                                                                u64 *__restrict__ mask, int *__restrict__ cum)
{
    const int i = blockIdx.x * kNsThreads + threadIdx.x;
    const int word = i >> 6;
    bool first = false;
    if (i < E) {
        int c = 0;
        for (int w = 0; w < We; ++w)
            c += __popcll(D[(long)w * Eld + i]);
        count[i] = c;
        first = rank[i] == kRankBeyond && c == 0;
        if (first)
            rank[i] = 1;
    }
    const u64 bal = __ballot(first);
    if ((threadIdx.x & (kWave - 1)) == 0 && word < We) {
        mask[word] = bal;
        if (bal)
            atomicAdd(&cum[1], __popcll(bal));
    }
}

__global__ __launch_bounds__(kNsThreads) void smart_nsga2_peel(int E, int We, long Eld, int N, int r,
                                                               const u64 *__restrict__ D, int *__restrict__ count,
                                                               int *__restrict__ rank, const u64 *__restrict__ mask_prev,
                                                               u64 *__restrict__ mask_next, int *cum, int *ctl)
{
    const int a = cum[r - 1], b = cum[r - 2];
    const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
    if (a >= N || a == b) { // enough are ranked, or front r - 1 came out empty: none is left
        if (leader) {
            cum[r] = a;
            if (!ctl[0]) {
                ctl[1] = a == b ? r - 2 : r - 1;
                ctl[0] = 1;
            }
        }
        return;
    }
    const int i = blockIdx.x * kNsThreads + threadIdx.x;
    const int word = i >> 6;
    bool newly = false;
    if (i < E && rank[i] == kRankBeyond) {
        int c = count[i];
        for (int w = 0; w < We; ++w) {
            const u64 m = mask_prev[w];
            if (m)
                c -= __popcll(D[(long)w * Eld + i] & m);
        }
        count[i] = c;
        newly = c == 0;
        if (newly)
            rank[i] = r;
    }
    const u64 bal = __ballot(newly);
    if ((threadIdx.x & (kWave - 1)) == 0 && word < We) {
        mask_next[word] = bal;
        if (bal)
            atomicAdd(&cum[r], __popcll(bal));
    }
    if (leader)
        atomicAdd(&cum[r], a);
}

// ---- crowding -------------------------------------------------------------------------------------------------------
// The challengers of the pair passes below are cut into S slices of L over grid.y (nsga2_pair_slices, on the host); what
// a slice finds for candidate i goes to partial[(s * Eld + i) * 16 + 4 m + 0 .. 3] = min, max, U, L of key m over the
// slice's members of i's front (i itself apart).  Minima and maxima are exact: the slices combine to the same bits in any
// order.
template <int M>
__global__ __launch_bounds__(kNsPairThreads) void smart_nsga2_neighbours(int E, int L, long Eld,
                                                                        const double *__restrict__ keys,
                                                                        const int *__restrict__ rank,
                                                                        double *__restrict__ partial)
{
    const int i = blockIdx.x * kNsPairThreads + threadIdx.x;
    const bool live = i < E;
    const int ii = live ? i : E - 1;
    const int r = rank[ii];
    double mine[M], lowest[M], highest[M], up[M], down[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        mine[m] = keys[(long)ii * kNsKeys + m];
        lowest[m] = highest[m] = mine[m];
        up[m] = __builtin_inf();
        down[m] = -__builtin_inf();
    }
    const int j0 = blockIdx.y * L, j1 = j0 + L < E ? j0 + L : E;
    for (int j = j0; j < j1; ++j) {
        const bool same = rank[j] == r && j != ii;
        const double *const c = keys + (long)j * kNsKeys;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double k = c[m];
            lowest[m] = same && k < lowest[m] ? k : lowest[m];
            highest[m] = same && k > highest[m] ? k : highest[m];
            up[m] = same && k >= mine[m] && k < up[m] ? k : up[m];
            down[m] = same && k <= mine[m] && k > down[m] ? k : down[m];
        }
    }
    if (!live)
        return;
    double *const p = partial + ((long)blockIdx.y * Eld + i) * kNsPartial;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        p[4 * m + 0] = lowest[m];
        p[4 * m + 1] = highest[m];
        p[4 * m + 2] = up[m];
        p[4 * m + 3] = down[m];
    }
}

template <int M>
__global__ __launch_bounds__(kNsThreads) void smart_nsga2_crowding(int E, int S, long Eld, const double *__restrict__ keys,
                                                                  const int *__restrict__ rank,
                                                                  const double *__restrict__ partial,
                                                                  double *__restrict__ dist)
{
    const int i = blockIdx.x * kNsThreads + threadIdx.x;
    if (i >= E)
        return;
    const int r = rank[i];
    double mine[M], lowest[M], highest[M], up[M], down[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        mine[m] = keys[(long)i * kNsKeys + m];
        lowest[m] = highest[m] = mine[m];
        up[m] = __builtin_inf();
        down[m] = -__builtin_inf();
    }
    for (int s = 0; s < S; ++s) {
        const double *const p = partial + ((long)s * Eld + i) * kNsPartial;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            lowest[m] = p[4 * m + 0] < lowest[m] ? p[4 * m + 0] : lowest[m];
            highest[m] = p[4 * m + 1] > highest[m] ? p[4 * m + 1] : highest[m];
            up[m] = p[4 * m + 2] < up[m] ? p[4 * m + 2] : up[m];
            down[m] = p[4 * m + 3] > down[m] ? p[4 * m + 3] : down[m];
        }
    }
    double total = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        if (mine[m] == lowest[m] || mine[m] == highest[m]) {
            total = __builtin_inf();
        } else {
            double t = up[m] - down[m];
            const double width = highest[m] - lowest[m];
            t = t / width;
            total = total + t;
        }
    }
    dist[i] = r < kRankBeyond ? total : 0.0;
}

// ---- the place of a candidate, and the survivors' move ------------------------------------------------------------------
struct Nsga2Place {
    int E, N, Np, d, M, n_carry;
    const int *rank;
    const double *dist, *keys;
    const unsigned char *part;
    const double *pop_x, *pop_carry, *offspring, *carry_new;
    double *next_x, *next_keys, *next_carry;
    unsigned char *next_part;
    int *next_rank;
    double *next_dist;
    int *origin, *counts;
    const int *ctl, *cum, *before;
};

// before[i] += the candidates of this slice that precede i (an integer counter: the sum does not depend on the order)
__global__ __launch_bounds__(kNsPairThreads) void smart_nsga2_count_before(int E, int L, const int *__restrict__ rank,
                                                                          const double *__restrict__ dist, int *before)
{
    const int i = blockIdx.x * kNsPairThreads + threadIdx.x;
    const bool live = i < E;
    const int ii = live ? i : E - 1;
    const int r = rank[ii];
    const double far = dist[ii];
    const int j0 = blockIdx.y * L, j1 = j0 + L < E ? j0 + L : E;
    int n = 0;
    for (int j = j0; j < j1; ++j) {
        const int rj = rank[j];
        const double fj = dist[j];
        n += rj < r || (rj == r && (fj > far || (fj == far && j < ii))) ? 1 : 0;
    }
    if (live && n)
        atomicAdd(&before[i], n);
}

__global__ __launch_bounds__(kNsThreads) void smart_nsga2_place(Nsga2Place p)
{
    const int i = blockIdx.x * kNsThreads + threadIdx.x;
    if (i == 0) {
        p.counts[0] = p.ctl[1];
        p.counts[1] = p.cum[1];
    }
    if (i >= p.E)
        return;
    const int pos = p.before[i];
    if (pos >= p.N)
        return;
    const int r = p.rank[i];
    const double far = p.dist[i];
    const bool parent = i < p.Np;
    const long from = parent ? i : i - p.Np;
    const double *const x = (parent ? p.pop_x : p.offspring) + from * p.d;
    double *const y = p.next_x + (long)pos * p.d;
    for (int j = 0; j < p.d; ++j)
        y[j] = x[j];
    for (int m = 0; m < p.M; ++m)
        p.next_keys[(long)pos * p.M + m] = p.keys[(long)i * kNsKeys + m];
    if (p.n_carry > 0) {
        const double *const c = (parent ? p.pop_carry : p.carry_new) + from * p.n_carry;
        double *const cn = p.next_carry + (long)pos * p.n_carry;
        for (int k = 0; k < p.n_carry; ++k)
            cn[k] = c[k];
    }
    p.next_part[pos] = p.part[i];
    p.next_rank[pos] = r;
    p.next_dist[pos] = far;
    p.origin[pos] = i;
}

// ---- variation --------------------------------------------------------------------------------------------------------
struct Nsga2Vary {
    int N, d;
    DeKey key;
    const double *x; // the population, in tournament order
    u64 C;           // the threshold of the crossover, in [0, 2^32]
    double f;
    DeBox box;
    double *offspring;
    unsigned char *out;
    double *rows;
    long ld;
};

__global__ __launch_bounds__(kNsThreads) void smart_nsga2_vary(Nsga2Vary p)
{
    const int c = blockIdx.x * kNsThreads + threadIdx.x;
    if (c >= p.N)
        return;
    const int d = p.d;
    const u64 N = (u64)p.N;
    const Philox4 r = philox4x32_10((unsigned)c, p.key.gen, 0u, 0u, p.key.k0, p.key.k1);
    const u64 a = mulhi(r.w[0], N);
    u64 b = mulhi(r.w[1], N - 1);
    b += b >= a;
    const u64 t = a < b ? a : b;    // the binary tournament: the population lies in (rank, -distance) order
    const u64 p1 = mulhi(r.w[2], N);
    u64 p2 = mulhi(r.w[3], N - 1);
    p2 += p2 >= p1;
    const Philox4 fb = philox4x32_10((unsigned)c, p.key.gen, 1u, 0u, p.key.k0, p.key.k1);
    const unsigned crossed = de_crossover((unsigned)c, p.key, d, p.C, (int)mulhi(fb.w[0], (u64)d));
    const double *const base = p.x + t * d;
    double *const y_out = p.offspring + (long)c * d;
    const bool out = de_move((unsigned)c, p.key, d, crossed, p.box, base, p.x + p1 * d, p.x + p2 * d, p.f, y_out);
    p.out[c] = out ? 1 : 0;
    de_launch_row(d, p.box, out, base, y_out, p.rows + (long)c * p.ld);
}

// ---- launch (validated by smart_analysis_capi.hip) -------------------------------------------------------------------
// the slices of the challengers in the crowding and place passes: one per 16 mask words (1,024 challengers), at most 16 --
// 16 S <= max(W, 16) words per candidate, so S slices of partial results fit where the bit matrix was
static void nsga2_pair_slices(int E, int We, int &S, int &L)
{
    S = We / kNsPartial < 1 ? 1 : (We / kNsPartial > kNsMaxPairSlices ? kNsMaxPairSlices : We / kNsPartial);
    L = (E + S - 1) / S;
}

template <int M>
static void launch_pairs(int E, int We, long Eld, const Nsga2Workspace &w, hipStream_t s, bool crowding)
{
    if (crowding) { // (the partial results lie where the bit matrix was: the peel is over)
        int S, L;
        nsga2_pair_slices(E, We, S, L);
        double *const partial = (double *)w.D;
        const dim3 grid((unsigned)((E + kNsPairThreads - 1) / kNsPairThreads), (unsigned)S);
        hipLaunchKernelGGL((smart_nsga2_neighbours<M>), grid, dim3(kNsPairThreads), 0, s, E, L, Eld, w.keys, w.rank, partial);
        hipLaunchKernelGGL((smart_nsga2_crowding<M>), dim3((unsigned)((E + kNsThreads - 1) / kNsThreads)), dim3(kNsThreads),
                           0, s, E, S, Eld, w.keys, w.rank, partial, w.dist);
        return;
    }
    const int slices = We < kNsMaxSlices ? We : kNsMaxSlices;
    const int per = (We + slices - 1) / slices;
    const dim3 grid((unsigned)((E + kNsThreads - 1) / kNsThreads), (unsigned)((We + per - 1) / per));
    hipLaunchKernelGGL((smart_nsga2_dominance<M>), grid, dim3(kNsThreads), 0, s, E, We, per, Eld, w.keys, w.D);
}

static void launch_pairs(int M, int E, int We, long Eld, const Nsga2Workspace &w, hipStream_t s, bool crowding)
{
    if (M == 2)
        launch_pairs<2>(E, We, Eld, w, s, crowding);
    else if (M == 3)
        launch_pairs<3>(E, We, Eld, w, s, crowding);
    else
        launch_pairs<4>(E, We, Eld, w, s, crowding);
}

static int nsga2_survive(const Nsga2Call &c, hipStream_t s)
{
    const int N = (int)c.n_rows, M = c.n_objectives;
    const int Np = c.parents ? N : 0, E = Np + N;
    const Nsga2Workspace w = nsga2_layout(N, c.workspace);
    const int We = (E + 63) / 64, Epad = 64 * We;
    Nsga2Columns kc = {};
    for (int m = 0; m < M; ++m) {
        kc.col[m] = c.score_columns[m];
        kc.dir[m] = c.direction[m];
        kc.target[m] = c.direction[m] == SMART_PARETO_TARGET ? c.target[m] : 0.0;
    }
    // ctl and cum lie side by side at the head of the workspace
    HIP_TRY(hipMemsetAsync(w.ctl, 0, (size_t)((char *)w.mask - (char *)w.ctl), s));
    const unsigned blocks = (unsigned)(Epad / kNsThreads + (Epad % kNsThreads ? 1 : 0));
    hipLaunchKernelGGL(smart_nsga2_keys, dim3(blocks), dim3(kNsThreads), 0, s, E, Epad, Np, M, c.pop_keys, c.pop_part, c.out,
                       c.scores, c.ld_scores, kc, c.eligible, w.keys, w.part, w.rank, w.dist);
    launch_pairs(M, E, We, w.Eld, w, s, /*crowding=*/false);
    hipLaunchKernelGGL(smart_nsga2_first, dim3(blocks), dim3(kNsThreads), 0, s, E, We, w.Eld, w.D, w.count, w.rank,
                       w.mask + w.W, w.cum);
    // the further fronts: pass r reads the mask of front r - 1.  The last front is at most front N, so the pass that finds
    // the stop condition met is at most pass N + 2
    int r = 2, batch = kNsFirstBatch, done = 0;
    while (!done) {
        if (r > N + 2)
            return fail(SMART_E_SIZE, "smart_nsga2_step_hip: the peel has not ended after %d passes", r - 1);
        const int last = r + batch - 1 < N + 2 ? r + batch - 1 : N + 2;
        for (; r <= last; ++r)
            hipLaunchKernelGGL(smart_nsga2_peel, dim3(blocks), dim3(kNsThreads), 0, s, E, We, w.Eld, N, r, w.D, w.count,
                               w.rank, w.mask + (long)((r - 1) & 1) * w.W, w.mask + (long)(r & 1) * w.W, w.cum, w.ctl);
        HIP_TRY(hipMemcpyAsync(&done, w.ctl, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        batch = 2 * batch < kNsMaxBatch ? 2 * batch : kNsMaxBatch;
    }
    launch_pairs(M, E, We, w.Eld, w, s, /*crowding=*/true);
    // the places: the counts of the peel are done with, their array takes the numbers of predecessors
    int S, L;
    nsga2_pair_slices(E, We, S, L);
    HIP_TRY(hipMemsetAsync(w.count, 0, (size_t)E * sizeof(int), s));
    hipLaunchKernelGGL(smart_nsga2_count_before, dim3((unsigned)((E + kNsPairThreads - 1) / kNsPairThreads), (unsigned)S),
                       dim3(kNsPairThreads), 0, s, E, L, w.rank, w.dist, w.count);
    Nsga2Place p;
    p.E = E, p.N = N, p.Np = Np, p.d = c.n_dims, p.M = M, p.n_carry = c.n_carry;
    p.rank = w.rank, p.dist = w.dist, p.keys = w.keys, p.part = w.part;
    p.pop_x = c.pop_x, p.pop_carry = c.pop_carry, p.offspring = c.offspring, p.carry_new = c.carry_new;
    p.next_x = c.next_x, p.next_keys = c.next_keys, p.next_carry = c.next_carry, p.next_part = c.next_part;
    p.next_rank = c.rank, p.next_dist = c.crowding, p.origin = c.origin, p.counts = c.counts;
    p.ctl = w.ctl, p.cum = w.cum, p.before = w.count;
    hipLaunchKernelGGL(smart_nsga2_place, dim3((unsigned)((E + kNsThreads - 1) / kNsThreads)), dim3(kNsThreads), 0, s, p);
    return SMART_OK;
}

int launch_nsga2(const Nsga2Call &c, hipStream_t s)
{
    if (c.scores) {
        if (int rc = nsga2_survive(c, s))
            return rc;
    }
    if (c.vary) {
        Nsga2Vary p;
        p.N = (int)c.n_rows, p.d = c.n_dims;
        p.key = de_key(c.generation, c.seed);
        p.x = c.scores ? c.next_x : c.pop_x;
        p.C = (u64)c.cr_threshold, p.f = c.f;
        p.box = de_box(c.n_dims, c.lo, c.hi, c.scale, c.columns);
        p.offspring = c.offspring, p.out = c.out, p.rows = c.rows, p.ld = c.ld;
        hipLaunchKernelGGL(smart_nsga2_vary, dim3((unsigned)((c.n_rows + kNsThreads - 1) / kNsThreads)), dim3(kNsThreads), 0,
                           s, p);
    }
    return SMART_OK;
}

} // namespace smart
