// smart_capi_internal.h -- what the units behind include/smart_amd.h share: the error text of the calling thread
// (smart_capi.hip), and the host-side launch and capacity functions of the kernel units.  Every unit that defines one
// of these includes this header, so the compiler holds each definition against its declaration.
#pragma once

#include "../../include/smart_amd.h"

#include <hip/hip_runtime.h>

#include <type_traits>

namespace smart {

// ---- smart_capi.hip: the text smart_last_error() returns, per thread
int fail(int code, const char *fmt, ...); // sets the text, returns code (smart_hostio.cpp, host only, declares it itself)
void clear_error();                       // what an entry does on success
int hip_fail(hipError_t e, const char *what);
int device_ready(); // SMART_OK, or SMART_E_NO_DEVICE with its text: every entry asks AFTER it has validated its arguments

#define HIP_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t _e = (expr);                                                                                        \
        if (_e != hipSuccess)                                                                                          \
            return hip_fail(_e, #expr);                                                                                \
    } while (0)

// ---- the launch rules the analysis units share (host side): stated here once, used by smart_analysis_capi.hip and by
// the launch tails of the units

// WHICH FORM RUNS.  Every method argument of the ABI is 0 = AUTO, 1 = the form with a capacity (SORT, LDS), 2 = the form
// without one (SELECT, GLOBAL); AUTO takes the first wherever the row fits.
constexpr int kMethodAuto = 0, kMethodCapacity = 1, kMethodOther = 2;
static_assert(SMART_QUANTILES_AUTO == kMethodAuto && SMART_FDC_AUTO == kMethodAuto && SMART_ENS_AUTO == kMethodAuto &&
                  SMART_PAWN_AUTO == kMethodAuto && SMART_QUANTILES_SORT == kMethodCapacity &&
                  SMART_FDC_SORT == kMethodCapacity && SMART_ENS_LDS == kMethodCapacity &&
                  SMART_PAWN_LDS == kMethodCapacity && SMART_QUANTILES_SELECT == kMethodOther &&
                  SMART_FDC_SELECT == kMethodOther && SMART_ENS_GLOBAL == kMethodOther && SMART_PAWN_GLOBAL == kMethodOther,
              "one predicate reads every method argument");
inline bool method_known(int method) { return method >= kMethodAuto && method <= kMethodOther; }
inline bool capacity_form(int method, long n, long capacity)
{
    return method == kMethodCapacity || (method == kMethodAuto && n <= capacity);
}

// WHICH INSTANCE OF A KERNEL THAT SORTS A ROW IN LDS RUNS: run(cap, threads) with the elements and the threads of the
// smallest instance that holds N, both as compile-time constants (cap(), threads()); CAPACITY is the largest instance.
template <int CAPACITY, class Run>
inline void sort_instance(long N, Run run)
{
    static_assert(CAPACITY > 4096, "the ladder ends above its last rung");
    if (N <= 1024)
        run(std::integral_constant<int, 1024>(), std::integral_constant<int, 512>());
    else if (N <= 2048)
        run(std::integral_constant<int, 2048>(), std::integral_constant<int, 1024>());
    else if (N <= 4096)
        run(std::integral_constant<int, 4096>(), std::integral_constant<int, 1024>());
    else
        run(std::integral_constant<int, CAPACITY>(), std::integral_constant<int, 1024>());
}

// HOW MANY STEPS A WORKSPACE HOLDS, where a kernel keeps step_bytes per report step (or row) and the steps go in
// batches, one launch per batch: a *_workspace_bytes entry asks for as many steps as fit in kBatchBytes, at least one,
// at most R; the launch takes as many per batch as the workspace it is given holds (the entry has seen to one).
constexpr long kBatchBytes = 256l << 20;
inline long workspace_steps(long workspace_bytes, long step_bytes) { return workspace_bytes / step_bytes; }
inline long batched_workspace_bytes(long step_bytes, long R)
{
    long steps = workspace_steps(kBatchBytes, step_bytes);
    steps = steps < 1 ? 1 : steps;
    return (steps < R ? steps : R) * step_bytes;
}
template <class Run>
inline void for_each_batch(long R, long batch, Run run) // run(first step, steps) over [0, R)
{
    for (long r0 = 0; r0 < R; r0 += batch)
        run(r0, R - r0 < batch ? R - r0 : batch);
}

// a length rounded up to a power of two of at least `block`: what a bitonic network over blocks in LDS sorts
inline long padded_pow2(long n, long block)
{
    long p = block;
    while (p < n)
        p *= 2;
    return p;
}

// ---- smart_literal.hip
struct KArgs;
void launch_literal(const KArgs &a, dim3 grid, size_t lds_bytes, hipStream_t s, bool rows);
void launch_onestep(long n, const double *in, double *out, hipStream_t s);
void launch_river(long n, const double *in, double *out, hipStream_t s);

// ---- smart_quantiles.hip
long quantiles_sort_capacity();
void launch_quantiles(long N, long R, const double *sim, long ld, const double *weights, const double *probs, int K,
                      double *out, bool sort, hipStream_t s);

// ---- smart_objfn_windows.hip
int objfn_max_windows();
void launch_objfn_windows(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                          int transform, double eps, double *objfn, hipStream_t s);

// ---- smart_flow_duration.hip
long flow_duration_sort_capacity();
long flow_duration_workspace_bytes(long R, int W, bool with_objfn);
void launch_flow_duration(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                          const double *probs, int K, double *quant, int transform, double eps, double seg_lo,
                          double seg_hi, double *objfn, double *ws, bool sort, hipStream_t s);

// ---- smart_signatures.hip
void launch_signatures(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                       double alpha, const double *pulse, double *sig, hipStream_t s);

// ---- smart_sobol.hip
long sobol_lds_capacity();
int sobol_max_resamples();
long sobol_workspace_bytes();
void launch_sobol(long n, int k, long M, const double *y, long ld, double *s1, double *st, double *moments,
                  const unsigned short *counts, int B, double *s1_std, double *st_std, hipStream_t s);

// ---- smart_bootstrap.hip
int bootstrap_max_windows();
int bootstrap_max_resamples();
long bootstrap_workspace_bytes(long N, int W, int B, bool with_replicates);
void launch_bootstrap(long N, long R, const double *sim, long ld, const double *obs, const int *window, int W,
                      int transform, double eps, const unsigned short *counts, int B, const double *probs, int K,
                      double *point, double *stats, double *replicates, double *ws, hipStream_t s);

// ---- smart_pareto.hip
long pareto_workspace_bytes(long N, int M);
void launch_pareto(long N, const double *scores, long ld, const int *columns, const int *direction, const double *target,
                   int M, const unsigned char *eligible, int *dominated_by, void *workspace, hipStream_t s);

// ---- smart_ensemble_scores.hip
long ensemble_scores_lds_capacity();
long ensemble_scores_max_samples();
long ensemble_scores_step_bytes(long N, bool weighted);
void launch_ensemble_scores(long N, long R, const double *sim, long ld, const double *weights, const double *obs,
                            double *out, bool lds, void *workspace, long workspace_bytes, hipStream_t s);

// ---- smart_dynia.hip
int dynia_max_half_width();
long dynia_lds_capacity();
long dynia_step_bytes(long N);
void launch_dynia(long N, long R, const double *sim, long ld, const double *obs, int h, int min_valid, double fraction,
                  const unsigned char *cat, int P, int B, int support, double *shares, double *cut, int *retained,
                  int *count, double *err, long ld_err, void *workspace, long workspace_bytes, hipStream_t s);

// ---- smart_pawn.hip
long pawn_lds_capacity();
long pawn_max_samples();
long pawn_step_bytes(long N);
void launch_pawn(long N, long R, const double *y, long ld, const unsigned char *cat, int P, int B, double *ks, int *counts,
                 bool lds, void *workspace, long workspace_bytes, hipStream_t s);

// ---- smart_demcz.hip: the arguments of smart_demcz_step_hip as the entry has checked them (score NULL: no accept phase)
struct DemczCall {
    long n_chains, chain_offset;
    int n_dims;
    unsigned long long seed;
    long generation, archive_size, capacity;
    double *x, *logp, *carry;
    int *accepted;
    double *proposal;
    unsigned char *out;
    const double *score;
    long score_stride;
    int score_kind;
    long n_obs;
    double n_eff, sigma;
    const double *carry_new;
    int n_carry, append;
    double *archive, *archive_logp, *archive_carry;
    int propose;
    const double *lo, *hi, *scale, *gamma; // host, n_dims each
    long jump_threshold, cr_threshold;
    double *rows;
    long ld;
    const int *columns; // host, n_dims
};
// the archive rows the propose phase of a call draws from: what the accept phase of the same call has appended included
inline long demcz_archive_after(const DemczCall &c)
{
    return c.archive_size + (c.score && c.append ? c.chain_offset + c.n_chains : 0);
}
void launch_demcz(const DemczCall &c, hipStream_t s);

// ---- smart_nsga2.hip: the arguments of smart_nsga2_step_hip as the entry has checked them (scores NULL: no survive phase)
struct Nsga2Call {
    long n_rows;
    int n_dims, n_objectives, n_carry;
    unsigned long long seed;
    long generation;
    int parents;
    const double *pop_x, *pop_keys, *pop_carry;
    const unsigned char *pop_part;
    double *next_x, *next_keys, *next_carry;
    unsigned char *next_part;
    int *rank;
    double *crowding;
    int *origin, *counts;
    double *offspring;
    unsigned char *out;
    const double *scores;
    long ld_scores;
    const int *score_columns, *direction; // host, n_objectives
    const double *target;                 // host, n_objectives (read where the direction is TARGET)
    const unsigned char *eligible;
    const double *carry_new;
    void *workspace;
    int vary;
    const double *lo, *hi, *scale; // host, n_dims each
    double f;
    long cr_threshold;
    double *rows;
    long ld;
    const int *columns; // host, n_dims
};
long nsga2_workspace_bytes(long N);
int launch_nsga2(const Nsga2Call &c, hipStream_t s); // SMART_OK, or the code of hip_fail (the flag of a peel batch is read)

// ---- smart_particle.hip: the arguments of smart_particle_step_hip as the entry has checked them
struct ParticleCall {
    long n_particles;
    int n_dims;
    unsigned long long seed;
    long step;
    int phases;
    long n_reports;
    const double *sim;
    long ld_sim;
    const double *obs;
    double sigma0, sigma1, tau;
    const int64_t *q_in;
    long long offset;
    const double *rows_in;
    double *rows_out;
    long ld;
    const int *columns; // host, n_dims
    int z_column;
    double area_m2;
    const double *lo, *hi, *scale; // host, n_dims each
    const double *noise;           // host, SMART_PARTICLE_STATES
    const double *states_in;
    double *states_out;
    const double *logw_in;
    double *logw_out;
    int64_t *q;
    int *parents;
    double *stats;
    int64_t *counts;
    void *workspace;
};
long particle_workspace_bytes(long N);
int launch_particle(const ParticleCall &c, hipStream_t s); // SMART_OK, or the code of hip_fail

// ---- smart_error_model.hip
void launch_error_model_loglik(long N, long R, const double *sim, long ld, const double *obs, const double *err, long err_ld,
                               double *out, hipStream_t s);
void launch_error_model_draw(long N, long R, long K, const double *sim, long ld, const double *err, long err_ld,
                             unsigned long long seed, long column_offset, int truncate, double *out, long out_ld,
                             hipStream_t s);

} // namespace smart
