// smart_pareto.hip -- Pareto selection: for every row of a score matrix scores[N][ld], the number of rows that dominate
// it over M <= 16 selected columns, each with a direction.  0 = the row is on the Pareto front.
//
// Definition.  key[i][m] is computed in fp64 exactly as written: x for MAX, -x for MIN, -|x - target[m]| for TARGET.
// Row i TAKES PART iff eligible is NULL or eligible[i] != 0, and none of its M selected scores is a NaN (columns that are
// not selected, and the padding of ld, are never read).  Row j dominates row i iff both take part, key[j][m] >= key[i][m]
// for every m and key[j][m] > key[i][m] for at least one m -- all >= and not all <=, IEEE compares: -0.0 equals +0.0,
// the infinities order as they do.  Rows with equal keys do not dominate each other: a front keeps its duplicates.
// dominated_by[i] = the number of rows that dominate row i, or -1 where row i does not take part.
//
// KEYS PASS (smart_pareto_keys).  One lane per row: the NaN test on the bit patterns, -1 for the rows that do not take
// part, and the E rows that do COMPACTED into keys[E][MP] of the workspace (a row's M keys together, padded with zeros
// to the instance's MP = 2, 4, 8 or 16: a challenger is one aligned piece of 16 .. 128 bytes) beside row_of[e].  The
// place of a workgroup's rows is one atomic add of its count to the one counter of the workspace (zeroed by the launch),
// the place inside the workgroup a ballot and a sum over its four wavefronts; the ORDER of the list therefore differs
// from launch to launch, and no output depends on it (a count is a sum over all challengers).
//
// PAIR KERNEL (smart_pareto_count<MP>).  One lane per candidate e, its M keys in registers for the whole launch; the
// challenger index is wave-uniform, so a challenger's keys are scalar loads from the compacted array (U = 8, 4, 2, 1
// challengers requested together per loop trip for MP = 2, 4, 8, 16) and every compare is a register against a scalar
// pair: M x `>=`, M x `<=`, the masks joined on the scalar side, one conditional integer add.  The loops are compiled
// per M (a switch inside the instance): unused slots cost no compare.  Nothing here knows N: the host launches the grid
// (ceil(N / 256), 16) without waiting for E, a workgroup whose candidates or whose slice lie beyond E returns at once, so
// the work is E^2 pairs.  The challenger range is cut into S = min(16, ceil(E / 64)) slices of L = ceil(E / S) rounded
// up to a multiple of 8 challengers (pareto_slices, from E, on the device): E = 1e4 is 157 wavefronts x 16 slices.  The
// last slices can be ragged or empty (E = 1,025: L = 72, slice 14 has 17 challengers, slice 15 none); every (candidate,
// slice < S) writes its partial count to partial[s][e].
//
// CLOSING PASS (smart_pareto_close).  dominated_by[row_of[e]] = sum over s < S of partial[s][e].  No atomic touches a
// result: two launches give the same integers whatever order the list came out in.
#include "smart_capi_internal.h"
#include "smart_matrix_common.h"

namespace smart {

constexpr int kParThreads = 256;
constexpr int kParWaves = kParThreads / kWave;
constexpr int kParMaxObjectives = SMART_PARETO_MAX_OBJECTIVES;
constexpr int kParMaxSlices = 16;  // grid.y of the pair kernel
constexpr int kParSliceFloor = 64; // a slice is worth a workgroup from this many challengers on
constexpr int kParSliceStep = 8;   // slices are whole loop trips of every instance (U divides it)
constexpr long kParAlign = 256;    // of the workspace's parts
static_assert(kParMaxObjectives == 16, "instances below");

// the selected columns of a launch, passed by value (unused entries 0)
struct ParetoColumns {
    int col[kParMaxObjectives];
    int dir[kParMaxObjectives];
    double target[kParMaxObjectives];
};

__host__ __device__ inline int pareto_padded(int M) { return M <= 2 ? 2 : (M <= 4 ? 4 : (M <= 8 ? 8 : 16)); }

// the slices of the challenger range, from E alone
__device__ __forceinline__ void pareto_slices(int E, int &S, int &L)
{
    const long want = ((long)E + kParSliceFloor - 1) / kParSliceFloor;
    S = want > kParMaxSlices ? kParMaxSlices : (want < 1 ? 1 : (int)want);
    const long per = ((long)E + S - 1) / S;
    L = (int)((per + kParSliceStep - 1) / kParSliceStep * kParSliceStep);
}

// ---- keys -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kParThreads) void smart_pareto_keys(long N, const double *__restrict__ scores, long ld,
                                                                ParetoColumns pc, int M, int MP,
                                                                const unsigned char *__restrict__ eligible,
                                                                int *__restrict__ dominated_by, int *__restrict__ count,
                                                                double *__restrict__ keys, int *__restrict__ row_of)
{
    __shared__ int wave_rows[kParWaves];
    __shared__ int block_base;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const long i = (long)blockIdx.x * kParThreads + tid;
    const double *const row = scores + (i < N ? i : N - 1) * ld;
    bool part = i < N && (!eligible || eligible[i] != 0);
    if (part) {
        for (int m = 0; m < M; ++m)
            part = part && !is_nan_bits(row[pc.col[m]]);
    }
    if (i < N && !part)
        dominated_by[i] = -1;
    const unsigned long long mask = __ballot(part);
    if (lane == 0)
        wave_rows[w] = __popcll(mask);
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int v = 0; v < kParWaves; ++v)
            total += wave_rows[v];
        block_base = total ? atomicAdd(count, total) : 0;
    }
    __syncthreads();
    if (!part)
        return;
    long e = block_base + __popcll(mask & ((1ull << lane) - 1ull));
    for (int v = 0; v < w; ++v)
        e += wave_rows[v];
    row_of[e] = (int)i;
    double *const k = keys + e * MP;
    for (int m = 0; m < M; ++m) {
        const double x = row[pc.col[m]];
        const int d = pc.dir[m];
        k[m] = d == SMART_PARETO_MAX ? x : (d == SMART_PARETO_MIN ? -x : -fabs(x - pc.target[m]));
    }
    for (int m = M; m < MP; ++m)
        k[m] = 0.0;
}

// ---- pairs ----------------------------------------------------------------------------------------------------------
// does the challenger at c dominate the lane's row?  c is the same address in every lane, so a compare is a register
// against a scalar pair and its outcome for the wavefront one 64-bit scalar: the 2 M masks are joined by scalar
// instructions, and the one that is left is handed back to the lanes as the condition of the add.  (Written with the
// wavefront's masks, not with `bool`: hipcc otherwise packs the M outcomes of a lane into bits of a vector register.)
constexpr int kCmpGe = 3, kCmpLe = 5; // ordered >= and <= (the predicate numbers of the compare builtin)
template <int M>
__device__ __forceinline__ int pareto_beats(const double *__restrict__ c, const double (&mine)[M])
{
    unsigned long long ge = __builtin_amdgcn_fcmp(c[0], mine[0], kCmpGe), le = __builtin_amdgcn_fcmp(c[0], mine[0], kCmpLe);
#pragma unroll
    for (int m = 1; m < M; ++m) {
        ge &= __builtin_amdgcn_fcmp(c[m], mine[m], kCmpGe);
        le &= __builtin_amdgcn_fcmp(c[m], mine[m], kCmpLe);
    }
    return __builtin_amdgcn_inverse_ballot_w64(ge & ~le) ? 1 : 0;
}

// the count of one lane over the n challengers from c on
template <int MP, int M>
__device__ __forceinline__ int pareto_slice(const double *__restrict__ c, int n, const double *__restrict__ own)
{
    constexpr int U = 16 / MP;   // 32 scalar registers of challengers per loop trip
    static_assert(kParSliceStep % U == 0, "a whole slice is whole loop trips");
    double mine[M];
#pragma unroll
    for (int m = 0; m < M; ++m)
        mine[m] = own[m];
    int cnt = 0, j = 0;
    for (; j + U <= n; j += U, c += U * MP) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            cnt += pareto_beats<M>(c + u * MP, mine);
    }
    if constexpr (U > 1) {
        for (; j < n; ++j, c += MP) // the ragged end of the last slice
            cnt += pareto_beats<M>(c, mine);
    }
    return cnt;
}

template <int MP>
__global__ __launch_bounds__(kParThreads) void smart_pareto_count(const int *__restrict__ count, int M,
                                                                 const double *__restrict__ keys,
                                                                 int *__restrict__ partial)
{
    const int E = *count;
    int S, L;
    pareto_slices(E, S, L);
    const int s = blockIdx.y;
    const long e0 = (long)blockIdx.x * kParThreads;
    if (s >= S || e0 >= E)
        return;
    long e = e0 + threadIdx.x;
    const bool live = e < E;
    if (!live)
        e = E - 1;
    const long j0 = (long)s * L;
    const int n = j0 >= E ? 0 : (int)(E - j0 < L ? E - j0 : L);
    const double *const c = keys + (j0 >= E ? 0 : j0) * MP, *const own = keys + e * MP;
    int cnt = 0;
    constexpr int H = MP / 2;   // the instance takes M in H + 1 .. MP (MP = 2: 1 and 2)
    switch (M - H) {
    case 1:
        cnt = pareto_slice<MP, H + 1>(c, n, own);
        break;
    case 2:
        if constexpr (H >= 2)
            cnt = pareto_slice<MP, H + 2>(c, n, own);
        break;
    case 3:
        if constexpr (H >= 4)
            cnt = pareto_slice<MP, H + 3>(c, n, own);
        break;
    case 4:
        if constexpr (H >= 4)
            cnt = pareto_slice<MP, H + 4>(c, n, own);
        break;
    case 5:
        if constexpr (H >= 8)
            cnt = pareto_slice<MP, H + 5>(c, n, own);
        break;
    case 6:
        if constexpr (H >= 8)
            cnt = pareto_slice<MP, H + 6>(c, n, own);
        break;
    case 7:
        if constexpr (H >= 8)
            cnt = pareto_slice<MP, H + 7>(c, n, own);
        break;
    case 8:
        if constexpr (H >= 8)
            cnt = pareto_slice<MP, H + 8>(c, n, own);
        break;
    default: // MP = 2, M = 1 (M - H = 0)
        if constexpr (H == 1)
            cnt = pareto_slice<MP, 1>(c, n, own);
        break;
    }
    if (live)
        partial[(long)s * E + e] = cnt;
}

// ---- closing --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kParThreads) void smart_pareto_close(const int *__restrict__ count,
                                                                 const int *__restrict__ partial,
                                                                 const int *__restrict__ row_of,
                                                                 int *__restrict__ dominated_by)
{
    const int E = *count;
    int S, L;
    pareto_slices(E, S, L);
    const long e = (long)blockIdx.x * kParThreads + threadIdx.x;
    if (e >= E)
        return;
    int total = 0;
    for (int s = 0; s < S; ++s)
        total += partial[(long)s * E + e];
    dominated_by[row_of[e]] = total;
}

// ---- launch (validated by smart_analysis_capi.hip) ------------------------------------------------------------------
static long pareto_part(long bytes) { return (bytes + kParAlign - 1) / kParAlign * kParAlign; }

// the workspace: the counter | keys[N][MP] | row_of[N] | partial[16][N], each part on a 256-byte boundary
long pareto_workspace_bytes(long N, int M)
{
    return kParAlign + pareto_part(N * pareto_padded(M) * 8) + pareto_part(N * 4) + pareto_part(kParMaxSlices * N * 4);
}

void launch_pareto(long N, const double *scores, long ld, const int *columns, const int *direction, const double *target,
                   int M, const unsigned char *eligible, int *dominated_by, void *workspace, hipStream_t s)
{
    const int MP = pareto_padded(M);
    char *const ws = (char *)workspace;
    int *const count = (int *)ws;
    double *const keys = (double *)(ws + kParAlign);
    int *const row_of = (int *)((char *)keys + pareto_part(N * MP * 8));
    int *const partial = (int *)((char *)row_of + pareto_part(N * 4));
    ParetoColumns pc = {};
    for (int m = 0; m < M; ++m) {
        pc.col[m] = columns[m];
        pc.dir[m] = direction[m];
        pc.target[m] = direction[m] == SMART_PARETO_TARGET ? target[m] : 0.0;
    }
    const unsigned blocks = (unsigned)((N + kParThreads - 1) / kParThreads);
    if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess)
        return; // (the entry reads hipGetLastError)
    hipLaunchKernelGGL(smart_pareto_keys, dim3(blocks), dim3(kParThreads), 0, s, N, scores, ld, pc, M, MP, eligible,
                       dominated_by, count, keys, row_of);
    const dim3 grid(blocks, kParMaxSlices);
    switch (MP) {
    case 2:
        hipLaunchKernelGGL((smart_pareto_count<2>), grid, dim3(kParThreads), 0, s, count, M, keys, partial);
        break;
    case 4:
        hipLaunchKernelGGL((smart_pareto_count<4>), grid, dim3(kParThreads), 0, s, count, M, keys, partial);
        break;
    case 8:
        hipLaunchKernelGGL((smart_pareto_count<8>), grid, dim3(kParThreads), 0, s, count, M, keys, partial);
        break;
    default:
        hipLaunchKernelGGL((smart_pareto_count<16>), grid, dim3(kParThreads), 0, s, count, M, keys, partial);
        break;
    }
    hipLaunchKernelGGL(smart_pareto_close, dim3(blocks), dim3(kParThreads), 0, s, count, partial, row_of, dominated_by);
}

} // namespace smart
