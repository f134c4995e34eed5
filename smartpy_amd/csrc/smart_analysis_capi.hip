// smart_analysis_capi.hip -- the C ABI of the analyses of a stored discharge matrix sim[R][ld] (include/smart_amd.h):
// objective functions, weighted quantiles, objective functions per window, flow duration curves, hydrological signatures, Sobol indices, the block bootstrap of the objective functions, and of
// the Pareto selection over the scores they leave, the ensemble verification scores, the dynamic identifiability analysis and the PAWN sensitivity per report step, with their capacity and workspace entries -- validation and launch --
// and the one kernel among them that has no unit of its own, smart_objfn_matrix.  Every refusal comes before the device is asked for; the rules the entries share are the
// static helpers below, which take the entry's name for the text.
#include "smart_capi_internal.h"
#include "smart_device.h"

#include <cmath>
#include <cstdio>

namespace smart {

// Objective functions of a stored discharge matrix sim[R][ld] (sample-minor).  HBM-bound: the matrix is read
// exactly once, 8 * R bytes per sample, every wavefront load one contiguous 512-byte row segment, UNROLL of them in
// flight per lane.  Moments are taken about the observation mean (the same one-pass form as the fused path of the
// time-loop kernel).  A workgroup is WX wavefronts wide along the samples and WR deep along the report rows:
//   WX = 4, WR = 1 : one lane walks all rows of its sample (large N: enough wavefronts, 2 KB contiguous per row);
//   WX = 1, WR = 8 : 8 wavefronts share 64 samples and take the rows round-robin, partial moments are reduced
//                    through LDS in a fixed order (N ~ 1e5: 8x more wavefronts in flight).
template <int WX, int WR, int UNROLL>
__global__ __launch_bounds__(WX *WR *kWave) void smart_objfn_matrix(long N, long R, const double *__restrict__ sim,
                                                                    long ld, const double *__restrict__ obs,
                                                                    const double *__restrict__ gw_sim, double gw_obs,
                                                                    double *__restrict__ objfn)
{
    __shared__ double sh[512];
    __shared__ double st[5];
    __shared__ double part[WR > 1 ? WR : 1][5][kWave];
    obs_stats<false>(obs, R, st, nullptr, sh); // every thread stores the same five values to st
    __syncthreads();
    const long r1 = first_observed_row(obs, R, sh);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int wx = wave % WX, wr = wave / WX;
    long n = ((long)blockIdx.x * WX + wx) * kWave + lane;
    const bool live = n < N;
    if (!live)
        n = N - 1;
    const double ebar = st[1];
    const double *col = sim + n;
    // any constant per sample works (finish_objectives); the sample's value at the first OBSERVED report keeps the
    // digits: it is one of the summed values.  Row 0, where it carries no observation, is none of them -- a flood before
    // the gauge begins, a start-up value, a NaN that add() would never have seen
    const double shift = col[r1 * ld];
    double A = 0.0, B = 0.0, C1 = 0.0, C2 = 0.0, C3 = 0.0;
    auto add = [&](double e, double s) {
        if (!is_nan_bits(e)) { // montecarlo.py:195-196
            const double d = s - e, u = s - shift;
            A += d;
            B += d * d;
            C1 += u;
            C2 += u * u;
            C3 += (e - ebar) * u;
        }
    };
    long r = wr;
    for (; r + (UNROLL - 1) * WR < R; r += UNROLL * WR) { // UNROLL independent row loads in flight
        double s[UNROLL];
#pragma unroll
        for (int j = 0; j < UNROLL; ++j)
            s[j] = col[(r + j * WR) * ld];
#pragma unroll
        for (int j = 0; j < UNROLL; ++j)
            add(obs[r + j * WR], s[j]);
    }
    for (; r < R; r += WR)
        add(obs[r], col[r * ld]);
    double m[5] = {A, B, C1, C2, C3};
    if (WR > 1) { // (sum_wave_moments of smart_window_rows.h is this; called here it moved the kernel's instructions)
#pragma unroll
        for (int k = 0; k < 5; ++k)
            part[wr][k][lane] = m[k];
        __syncthreads();
        if (wr != 0)
            return;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double t = part[0][k][lane];
#pragma unroll
            for (int w = 1; w < WR; ++w)
                t += part[w][k][lane];
            m[k] = t;
        }
    }
    if (live) {
        double o[8];
        finish_objectives(st, m[0], m[1], m[2], m[3], m[4], gw_sim ? gw_sim[n] : 0.0,
                          gw_sim ? gw_obs : __builtin_nan(""), o);
        double *op = objfn + n * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            op[k] = o[k];
    }
}

// ---- the rules the entries share ------------------------------------------------------------------------------------
static int reports_fit(const char *entry, int64_t n_reports)
{
    if (n_reports > 0x7fffffffll)
        return fail(SMART_E_SIZE, "%s: n_reports %lld is more than one launch takes (2^31 - 1)", entry,
                    (long long)n_reports);
    return SMART_OK;
}

// the sizes of a matrix read per window: every count >= 1 (n_probs where the entry has one), ld, 2^31, the window cap
static int windowed_sizes(const char *entry, int64_t n_samples, int64_t n_reports, int64_t ld, int32_t n_windows,
                          const int32_t *n_probs)
{
    if (n_probs && (n_samples < 1 || n_reports < 1 || n_windows < 1 || *n_probs < 1))
        return fail(SMART_E_SIZE, "%s: need n_samples, n_reports, n_windows, n_probs >= 1 (got %lld, %lld, %d, %d)", entry,
                    (long long)n_samples, (long long)n_reports, (int)n_windows, (int)*n_probs);
    if (n_samples < 1 || n_reports < 1 || n_windows < 1)
        return fail(SMART_E_SIZE, "%s: need n_samples, n_reports, n_windows >= 1 (got %lld, %lld, %d)", entry,
                    (long long)n_samples, (long long)n_reports, (int)n_windows);
    if (ld < n_samples)
        return fail(SMART_E_SIZE, "%s: ld %lld is less than n_samples %lld", entry, (long long)ld, (long long)n_samples);
    if (int rc = reports_fit(entry, n_reports))
        return rc;
    if (n_windows > objfn_max_windows())
        return fail(SMART_E_SIZE, "%s: n_windows %d, at most %d per call", entry, (int)n_windows, objfn_max_windows());
    return SMART_OK;
}

// where the window array is optional: without one there is one window
static int window_array_given(const char *entry, const int32_t *window, int32_t n_windows)
{
    if (!window && n_windows != 1)
        return fail(SMART_E_SIZE, "%s: n_windows %d without a window array (NULL is one window)", entry, (int)n_windows);
    return SMART_OK;
}

// every probability inside (0, 1], or [0, 1] where rank 1 has a probability of its own (a NaN is outside both)
static int probs_inside(const char *entry, const double *probs, int32_t n_probs, bool zero_too)
{
    for (int32_t k = 0; k < n_probs; ++k)
        if (!((zero_too ? probs[k] >= 0.0 : probs[k] > 0.0) && probs[k] <= 1.0))
            return fail(SMART_E_SIZE, "%s: probability %d is %g, outside %s", entry, (int)k, probs[k],
                        zero_too ? "[0, 1]" : "(0, 1]");
    return SMART_OK;
}

static int eps_usable(const char *entry, double eps)
{
    if (!(eps >= 0.0) || std::isinf(eps))
        return fail(SMART_E_SIZE, "%s: eps %g must be finite and >= 0", entry, eps);
    return SMART_OK;
}

static int transform_known(const char *entry, int32_t transform)
{
    if (transform < SMART_TRANSFORM_NONE || transform > SMART_TRANSFORM_INVERSE)
        return fail(SMART_E_MODE, "%s: transform '%d' unknown.", entry, (int)transform);
    return SMART_OK;
}

// a workspace of `need` bytes: present where any are needed, and large enough
static int workspace_fits(const char *entry, bool for_objfn, const void *workspace, int64_t workspace_bytes, long need)
{
    if (need > 0 && !workspace)
        return fail(SMART_E_NULL,
                    for_objfn ? "%s: objfn needs a workspace of %ld bytes (workspace is NULL)"
                              : "%s: a workspace of %ld bytes is needed (workspace is NULL)",
                    entry, need);
    if (workspace_bytes < (workspace ? need : 0))
        return fail(SMART_E_SIZE, "%s: workspace_bytes %lld, need %ld", entry, (long long)workspace_bytes, need);
    return SMART_OK;
}

// the end of every entry, after its launch
static int launched()
{
    HIP_TRY(hipGetLastError());
    clear_error();
    return SMART_OK;
}

// the size rules of smart_sobol_indices_hip, shared with smart_sobol_workspace_bytes; 0 or the text of the refusal
static const char *sobol_sizes(int64_t n_base, int32_t n_params, int64_t n_rows, int32_t n_resamples, char *text, size_t len)
{
    if (n_base < 1 || n_base > 0x7fffffffll)
        snprintf(text, len, "n_base %lld must be in 1 .. 2^31 - 1", (long long)n_base);
    else if (n_params < 1 || n_params > SMART_SOBOL_MAX_PARAMS)
        snprintf(text, len, "n_params %d must be in 1 .. %d", (int)n_params, SMART_SOBOL_MAX_PARAMS);
    else if (n_rows < 1 || n_rows > 0x7fffffffll)
        snprintf(text, len, "n_rows %lld must be in 1 .. 2^31 - 1", (long long)n_rows);
    else if (n_resamples < 0 || n_resamples > sobol_max_resamples())
        snprintf(text, len, "n_resamples %d must be in 0 .. %d", (int)n_resamples, sobol_max_resamples());
    else
        return nullptr;
    return text;
}

// the size rules of smart_objfn_bootstrap_hip, shared with smart_bootstrap_workspace_bytes; 0 or the text of the refusal
static const char *bootstrap_sizes(int64_t n_samples, int32_t n_windows, int32_t n_resamples, char *text, size_t len)
{
    if (n_samples < 1 || n_samples > 0x7fffffffll)
        snprintf(text, len, "n_samples %lld must be in 1 .. 2^31 - 1", (long long)n_samples);
    else if (n_windows < 1 || n_windows > bootstrap_max_windows())
        snprintf(text, len, "n_windows %d must be in 1 .. %d", (int)n_windows, bootstrap_max_windows());
    else if (n_resamples < 0 || n_resamples > bootstrap_max_resamples())
        snprintf(text, len, "n_resamples %d must be in 0 .. %d", (int)n_resamples, bootstrap_max_resamples());
    else
        return nullptr;
    return text;
}

// the size rules of smart_pareto_counts_hip, shared with smart_pareto_workspace_bytes; 0 or the text of the refusal
static const char *pareto_sizes(int64_t n_rows, int32_t n_objectives, char *text, size_t len)
{
    if (n_rows < 1 || n_rows > 0x7fffffffll)
        snprintf(text, len, "n_rows %lld must be in 1 .. 2^31 - 1", (long long)n_rows);
    else if (n_objectives < 1 || n_objectives > SMART_PARETO_MAX_OBJECTIVES)
        snprintf(text, len, "n_objectives %d must be in 1 .. %d", (int)n_objectives, SMART_PARETO_MAX_OBJECTIVES);
    else
        return nullptr;
    return text;
}

// the size and method rules of smart_ensemble_scores_hip, shared with smart_ensemble_scores_workspace_bytes; SMART_OK, or
// the code of the refusal with its text
static int ensemble_sizes(int64_t n_samples, int64_t n_reports, int32_t method, char *text, size_t len)
{
    int code = SMART_E_SIZE;
    if (n_samples < 1 || n_reports < 1)
        snprintf(text, len, "need n_samples, n_reports >= 1 (got %lld, %lld)", (long long)n_samples, (long long)n_reports);
    else if (n_reports > 0x7fffffffll)
        snprintf(text, len, "n_reports %lld is more than one launch takes (2^31 - 1)", (long long)n_reports);
    else if (n_samples > ensemble_scores_max_samples())
        snprintf(text, len, "n_samples %lld, at most %lld (2^24)", (long long)n_samples,
                 (long long)ensemble_scores_max_samples());
    else if (method != SMART_ENS_AUTO && method != SMART_ENS_LDS && method != SMART_ENS_GLOBAL) {
        snprintf(text, len, "method '%d' unknown.", (int)method);
        code = SMART_E_MODE;
    } else if (method == SMART_ENS_LDS && n_samples > ensemble_scores_lds_capacity())
        snprintf(text, len, "the LDS form takes at most %lld samples, not %lld", (long long)ensemble_scores_lds_capacity(),
                 (long long)n_samples);
    else
        return SMART_OK;
    return code;
}

// the size rules of smart_dynia_hip, shared with smart_dynia_workspace_bytes; 0 or the text of the refusal
static const char *dynia_sizes(int64_t n_samples, int64_t n_reports, int32_t half_width, int32_t n_factors, int32_t n_bins,
                               char *text, size_t len)
{
    if (n_samples < 1 || n_reports < 1)
        snprintf(text, len, "need n_samples, n_reports >= 1 (got %lld, %lld)", (long long)n_samples, (long long)n_reports);
    else if (n_samples > 0x7fffffffll)
        snprintf(text, len, "n_samples %lld must be in 1 .. 2^31 - 1", (long long)n_samples);
    else if (n_reports > 0x7fffffffll)
        snprintf(text, len, "n_reports %lld is more than one launch takes (2^31 - 1)", (long long)n_reports);
    else if (half_width < 0 || half_width > dynia_max_half_width())
        snprintf(text, len, "half_width %d must be in 0 .. %d", (int)half_width, dynia_max_half_width());
    else if (n_factors < 1 || n_factors > SMART_DYNIA_MAX_FACTORS)
        snprintf(text, len, "n_factors %d must be in 1 .. %d", (int)n_factors, SMART_DYNIA_MAX_FACTORS);
    else if (n_bins < 1 || n_bins > SMART_DYNIA_MAX_BINS)
        snprintf(text, len, "n_bins %d must be in 1 .. %d", (int)n_bins, SMART_DYNIA_MAX_BINS);
    else
        return nullptr;
    return text;
}

// the size and method rules of smart_pawn_ks_hip that smart_pawn_workspace_bytes shares (ld, the factors and the bins lie
// between the sizes and the method in the entry); SMART_OK, or the code of the refusal with its text
static int pawn_sizes(int64_t n_samples, int64_t n_rows, char *text, size_t len)
{
    if (n_samples < 1 || n_rows < 1)
        snprintf(text, len, "need n_samples, n_rows >= 1 (got %lld, %lld)", (long long)n_samples, (long long)n_rows);
    else if (n_samples > pawn_max_samples())
        snprintf(text, len, "n_samples %lld, at most %lld (2^24)", (long long)n_samples, (long long)pawn_max_samples());
    else if (n_rows > 0x7fffffffll)
        snprintf(text, len, "n_rows %lld is more than one launch takes (2^31 - 1)", (long long)n_rows);
    else
        return SMART_OK;
    return SMART_E_SIZE;
}

static int pawn_method(int64_t n_samples, int32_t method, char *text, size_t len)
{
    if (method != SMART_PAWN_AUTO && method != SMART_PAWN_LDS && method != SMART_PAWN_GLOBAL) {
        snprintf(text, len, "method '%d' unknown.", (int)method);
        return SMART_E_MODE;
    }
    if (method == SMART_PAWN_LDS && n_samples > pawn_lds_capacity()) {
        snprintf(text, len, "the LDS form takes at most %lld samples, not %lld", (long long)pawn_lds_capacity(),
                 (long long)n_samples);
        return SMART_E_SIZE;
    }
    return SMART_OK;
}

} // namespace smart

using namespace smart;

extern "C" {

int smart_objfn_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                    const double *gw_sim, double gw_obs, double *objfn, void *stream)
{
    if (!sim || !obs || !objfn)
        return fail(SMART_E_NULL, "smart_objfn_hip: sim, obs and objfn are required");
    if (n_samples < 1 || n_reports < 1 || ld < n_samples)
        return fail(SMART_E_SIZE, "smart_objfn_hip: need n_samples, n_reports >= 1 and ld >= n_samples");
    if (int rc = device_ready())
        return rc;
    if (n_samples >= 4 * 65536) // >= 4 wavefronts per SIMD even with one lane per sample
        hipLaunchKernelGGL((smart_objfn_matrix<4, 1, 8>), dim3((unsigned)((n_samples + 4 * kWave - 1) / (4 * kWave))),
                           dim3(4 * kWave), 0, (hipStream_t)stream, (long)n_samples, (long)n_reports, sim, (long)ld, obs,
                           gw_sim, gw_obs, objfn);
    else
        hipLaunchKernelGGL((smart_objfn_matrix<1, 8, 4>), dim3((unsigned)((n_samples + kWave - 1) / kWave)),
                           dim3(8 * kWave), 0, (hipStream_t)stream, (long)n_samples, (long)n_reports, sim, (long)ld, obs,
                           gw_sim, gw_obs, objfn);
    return launched();
}

int smart_weighted_quantiles_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld,
                                 const double *weights, const double *probs, int32_t n_probs, double *out,
                                 int32_t method, void *stream)
{
    static const char entry[] = "smart_weighted_quantiles_hip";
    int rc;
    if (!sim || !probs || !out)
        return fail(SMART_E_NULL, "%s: sim, probs and out are required", entry);
    if (n_samples < 1 || n_reports < 1 || n_probs < 1 || ld < n_samples)
        return fail(SMART_E_SIZE, "%s: need n_samples, n_reports, n_probs >= 1 and ld >= n_samples", entry);
    if ((rc = reports_fit(entry, n_reports)))
        return rc;
    if (n_probs > SMART_QUANTILES_MAX_PROBS)
        return fail(SMART_E_SIZE, "%s: %d probabilities, at most %d per call", entry, (int)n_probs,
                    SMART_QUANTILES_MAX_PROBS);
    if ((rc = probs_inside(entry, probs, n_probs, /*zero_too=*/false)))
        return rc;
    if (method != SMART_QUANTILES_AUTO && method != SMART_QUANTILES_SORT && method != SMART_QUANTILES_SELECT)
        return fail(SMART_E_MODE, "%s: method '%d' unknown.", entry, (int)method);
    if (method == SMART_QUANTILES_SORT && n_samples > quantiles_sort_capacity())
        return fail(SMART_E_SIZE, "%s: the sort form takes at most %lld samples, not %lld", entry,
                    (long long)quantiles_sort_capacity(), (long long)n_samples);
    if ((rc = device_ready()))
        return rc;
    const bool sort = method == SMART_QUANTILES_SORT ||
                      (method == SMART_QUANTILES_AUTO && n_samples <= quantiles_sort_capacity());
    launch_quantiles((long)n_samples, (long)n_reports, sim, (long)ld, weights, probs, (int)n_probs, out, sort,
                     (hipStream_t)stream);
    return launched();
}

int64_t smart_quantiles_sort_capacity(void) { return quantiles_sort_capacity(); }

int smart_objfn_windows_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                            const int32_t *window, int32_t n_windows, int32_t transform, double eps, double *objfn,
                            void *stream)
{
    static const char entry[] = "smart_objfn_windows_hip";
    int rc;
    if (!sim || !obs || !window || !objfn)
        return fail(SMART_E_NULL, "%s: sim, obs, window and objfn are required (%s is NULL)", entry,
                    !sim ? "sim" : (!obs ? "obs" : (!window ? "window" : "objfn")));
    if ((rc = windowed_sizes(entry, n_samples, n_reports, ld, n_windows, nullptr)) || (rc = eps_usable(entry, eps)) ||
        (rc = transform_known(entry, transform)) || (rc = device_ready()))
        return rc;
    launch_objfn_windows((long)n_samples, (long)n_reports, sim, (long)ld, obs, window, (int)n_windows, (int)transform, eps,
                         objfn, (hipStream_t)stream);
    return launched();
}

int32_t smart_objfn_max_windows(void) { return objfn_max_windows(); }

int smart_flow_duration_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                            const int32_t *window, int32_t n_windows, const double *probs, int32_t n_probs,
                            double *quant, int32_t transform, double eps, double seg_lo, double seg_hi, double *objfn,
                            void *workspace, int64_t workspace_bytes, int32_t method, void *stream)
{
    static const char entry[] = "smart_flow_duration_hip";
    int rc;
    if (!sim || !probs || !quant)
        return fail(SMART_E_NULL, "%s: sim, probs and quant are required (%s is NULL)", entry,
                    !sim ? "sim" : (!probs ? "probs" : "quant"));
    if (objfn && !obs)
        return fail(SMART_E_NULL, "%s: objfn needs obs (obs is NULL)", entry);
    if ((rc = windowed_sizes(entry, n_samples, n_reports, ld, n_windows, &n_probs)) ||
        (rc = window_array_given(entry, window, n_windows)))
        return rc;
    if (n_probs > SMART_QUANTILES_MAX_PROBS)
        return fail(SMART_E_SIZE, "%s: n_probs %d, at most %d probabilities per call", entry, (int)n_probs,
                    SMART_QUANTILES_MAX_PROBS);
    if ((rc = probs_inside(entry, probs, n_probs, /*zero_too=*/true)) || (rc = eps_usable(entry, eps)))
        return rc;
    if (!(seg_lo >= 0.0 && seg_lo < seg_hi && seg_hi <= 1.0))
        return fail(SMART_E_SIZE, "%s: the segment (%g, %g) is not 0 <= seg_lo < seg_hi <= 1", entry, seg_lo, seg_hi);
    if ((rc = transform_known(entry, transform)))
        return rc;
    if (method != SMART_FDC_AUTO && method != SMART_FDC_SORT && method != SMART_FDC_SELECT)
        return fail(SMART_E_MODE, "%s: method '%d' unknown.", entry, (int)method);
    if (objfn && method == SMART_FDC_SELECT)
        return fail(SMART_E_MODE, "%s: the select form gives order statistics only (objfn given)", entry);
    const long capacity = flow_duration_sort_capacity();
    if (n_reports > capacity && (objfn || method == SMART_FDC_SORT))
        return fail(SMART_E_SIZE, "%s: %s at most %ld report steps (the sort capacity), not %lld", entry,
                    objfn ? "the objective functions of the curve take" : "the sort form takes", capacity,
                    (long long)n_reports);
    if (objfn && (rc = workspace_fits(entry, /*for_objfn=*/true, workspace, workspace_bytes,
                                      flow_duration_workspace_bytes((long)n_reports, (int)n_windows, true))))
        return rc;
    if ((rc = device_ready()))
        return rc;
    const bool sort = method != SMART_FDC_SELECT && n_reports <= capacity;
    launch_flow_duration((long)n_samples, (long)n_reports, sim, (long)ld, obs, window, (int)n_windows, probs, (int)n_probs,
                         quant, (int)transform, eps, seg_lo, seg_hi, objfn, (double *)workspace, sort,
                         (hipStream_t)stream);
    return launched();
}

int64_t smart_flow_duration_workspace_bytes(int64_t n_reports, int32_t n_windows, int32_t with_objfn)
{
    if (n_reports < 1 || n_reports > 0x7fffffffll || n_windows < 1)
        return SMART_E_SIZE;
    return flow_duration_workspace_bytes((long)n_reports, (int)n_windows, with_objfn != 0);
}

int64_t smart_flow_duration_sort_capacity(void) { return flow_duration_sort_capacity(); }

int smart_signatures_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                         const int32_t *window, int32_t n_windows, double alpha, const double *pulse, double *sig,
                         void *stream)
{
    static const char entry[] = "smart_signatures_hip";
    int rc;
    if (!sim || !sig)
        return fail(SMART_E_NULL, "%s: sim and sig are required (%s is NULL)", entry, !sim ? "sim" : "sig");
    if ((rc = windowed_sizes(entry, n_samples, n_reports, ld, n_windows, nullptr)) ||
        (rc = window_array_given(entry, window, n_windows)))
        return rc;
    if (!(alpha > 0.0 && alpha < 1.0))
        return fail(SMART_E_SIZE, "%s: alpha %g must lie inside (0, 1)", entry, alpha);
    if ((rc = device_ready()))
        return rc;
    launch_signatures((long)n_samples, (long)n_reports, sim, (long)ld, obs, window, (int)n_windows, alpha, pulse, sig,
                      (hipStream_t)stream);
    return launched();
}

int32_t smart_signature_cols(void) { return SMART_SIGNATURE_COLS; }

int smart_sobol_indices_hip(int64_t n_base, int32_t n_params, int64_t n_rows, const double *y, int64_t ld, double *s1,
                            double *st, double *moments, const uint16_t *counts, int32_t n_resamples, double *s1_std,
                            double *st_std, void *workspace, int64_t workspace_bytes, void *stream)
{
    static const char entry[] = "smart_sobol_indices_hip";
    int rc;
    if (!y || !s1 || !st || !moments)
        return fail(SMART_E_NULL, "%s: y, s1, st and moments are required (%s is NULL)", entry,
                    !y ? "y" : (!s1 ? "s1" : (!st ? "st" : "moments")));
    if (n_resamples > 0 && (!counts || !s1_std || !st_std))
        return fail(SMART_E_NULL, "%s: n_resamples %d needs counts, s1_std and st_std (%s is NULL)", entry,
                    (int)n_resamples, !counts ? "counts" : (!s1_std ? "s1_std" : "st_std"));
    char text[160];
    if (sobol_sizes(n_base, n_params, n_rows, n_resamples, text, sizeof text))
        return fail(SMART_E_SIZE, "%s: %s", entry, text);
    if (ld < n_base * (n_params + 2))
        return fail(SMART_E_SIZE, "%s: ld %lld is less than n_base * (n_params + 2) = %lld", entry, (long long)ld,
                    (long long)(n_base * (n_params + 2)));
    if ((rc = workspace_fits(entry, /*for_objfn=*/false, workspace, workspace_bytes, sobol_workspace_bytes())) ||
        (rc = device_ready()))
        return rc;
    launch_sobol((long)n_base, (int)n_params, (long)n_rows, y, (long)ld, s1, st, moments, counts, (int)n_resamples,
                 s1_std, st_std, (hipStream_t)stream);
    return launched();
}

int64_t smart_sobol_workspace_bytes(int64_t n_base, int32_t n_params, int64_t n_rows, int32_t n_resamples)
{
    char text[160];
    if (sobol_sizes(n_base, n_params, n_rows, n_resamples, text, sizeof text))
        return SMART_E_SIZE;
    return sobol_workspace_bytes();
}

int32_t smart_sobol_max_resamples(void) { return sobol_max_resamples(); }

int64_t smart_sobol_lds_capacity(void) { return sobol_lds_capacity(); }

int smart_objfn_bootstrap_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                              const int32_t *window, int32_t n_windows, int32_t transform, double eps,
                              const uint16_t *counts, int32_t n_resamples, const double *probs, int32_t n_probs,
                              double *point, double *stats, double *replicates, void *workspace, int64_t workspace_bytes,
                              void *stream)
{
    static const char entry[] = "smart_objfn_bootstrap_hip";
    int rc;
    if (!sim || !obs || !window || !point)
        return fail(SMART_E_NULL, "%s: sim, obs, window and point are required (%s is NULL)", entry,
                    !sim ? "sim" : (!obs ? "obs" : (!window ? "window" : "point")));
    if (n_resamples > 0 && (!counts || !probs || !stats))
        return fail(SMART_E_NULL, "%s: n_resamples %d needs counts, probs and stats (%s is NULL)", entry, (int)n_resamples,
                    !counts ? "counts" : (!probs ? "probs" : "stats"));
    char text[160];
    if (bootstrap_sizes(n_samples, n_windows, n_resamples, text, sizeof text))
        return fail(SMART_E_SIZE, "%s: %s", entry, text);
    if (n_reports < 1)
        return fail(SMART_E_SIZE, "%s: need n_reports >= 1 (got %lld)", entry, (long long)n_reports);
    if (ld < n_samples)
        return fail(SMART_E_SIZE, "%s: ld %lld is less than n_samples %lld", entry, (long long)ld, (long long)n_samples);
    if ((rc = reports_fit(entry, n_reports)))
        return rc;
    if (n_resamples > 0) {
        if (n_probs < 1 || n_probs > SMART_QUANTILES_MAX_PROBS)
            return fail(SMART_E_SIZE, "%s: n_probs %d must be in 1 .. %d", entry, (int)n_probs, SMART_QUANTILES_MAX_PROBS);
        if ((rc = probs_inside(entry, probs, n_probs, /*zero_too=*/false)))
            return rc;
    }
    if ((rc = eps_usable(entry, eps)) || (rc = transform_known(entry, transform)) ||
        (rc = workspace_fits(entry, /*for_objfn=*/false, workspace, workspace_bytes,
                             bootstrap_workspace_bytes((long)n_samples, (int)n_windows, (int)n_resamples,
                                                       replicates != nullptr))) ||
        (rc = device_ready()))
        return rc;
    launch_bootstrap((long)n_samples, (long)n_reports, sim, (long)ld, obs, window, (int)n_windows, (int)transform, eps,
                     counts, (int)n_resamples, probs, n_resamples > 0 ? (int)n_probs : 0, point, stats, replicates,
                     (double *)workspace, (hipStream_t)stream);
    return launched();
}

int64_t smart_bootstrap_workspace_bytes(int64_t n_samples, int32_t n_windows, int32_t n_resamples, int32_t with_replicates)
{
    char text[160];
    if (bootstrap_sizes(n_samples, n_windows, n_resamples, text, sizeof text))
        return SMART_E_SIZE;
    return bootstrap_workspace_bytes((long)n_samples, (int)n_windows, (int)n_resamples, with_replicates != 0);
}

int32_t smart_bootstrap_max_windows(void) { return bootstrap_max_windows(); }

int32_t smart_bootstrap_max_resamples(void) { return bootstrap_max_resamples(); }

int smart_pareto_counts_hip(int64_t n_rows, const double *scores, int64_t ld, const int32_t *columns,
                            const int32_t *direction, const double *target, int32_t n_objectives, const uint8_t *eligible,
                            int32_t *dominated_by, void *workspace, int64_t workspace_bytes, void *stream)
{
    static const char entry[] = "smart_pareto_counts_hip";
    int rc;
    if (!scores || !columns || !direction || !dominated_by)
        return fail(SMART_E_NULL, "%s: scores, columns, direction and dominated_by are required (%s is NULL)", entry,
                    !scores ? "scores" : (!columns ? "columns" : (!direction ? "direction" : "dominated_by")));
    char text[160];
    if (pareto_sizes(n_rows, n_objectives, text, sizeof text))
        return fail(SMART_E_SIZE, "%s: %s", entry, text);
    for (int32_t m = 0; m < n_objectives; ++m) {
        if (columns[m] < 0 || columns[m] >= ld)
            return fail(SMART_E_SIZE, "%s: column %d of objective %d is outside 0 .. ld - 1 = %lld", entry, (int)columns[m],
                        (int)m, (long long)ld - 1);
        for (int32_t k = 0; k < m; ++k)
            if (columns[k] == columns[m])
                return fail(SMART_E_SIZE, "%s: column %d is named twice (objectives %d and %d)", entry, (int)columns[m],
                            (int)k, (int)m);
    }
    for (int32_t m = 0; m < n_objectives; ++m)
        if (direction[m] != SMART_PARETO_MAX && direction[m] != SMART_PARETO_MIN && direction[m] != SMART_PARETO_TARGET)
            return fail(SMART_E_MODE, "%s: direction '%d' of objective %d unknown.", entry, (int)direction[m], (int)m);
    for (int32_t m = 0; m < n_objectives; ++m) {
        if (direction[m] != SMART_PARETO_TARGET)
            continue;
        if (!target)
            return fail(SMART_E_NULL, "%s: objective %d is a TARGET (target is NULL)", entry, (int)m);
        if (!std::isfinite(target[m]))
            return fail(SMART_E_SIZE, "%s: target %g of objective %d must be finite", entry, target[m], (int)m);
    }
    if ((rc = workspace_fits(entry, /*for_objfn=*/false, workspace, workspace_bytes,
                             pareto_workspace_bytes((long)n_rows, (int)n_objectives))) ||
        (rc = device_ready()))
        return rc;
    launch_pareto((long)n_rows, scores, (long)ld, columns, direction, target, (int)n_objectives, eligible, dominated_by,
                  workspace, (hipStream_t)stream);
    return launched();
}

int64_t smart_pareto_workspace_bytes(int64_t n_rows, int32_t n_objectives)
{
    char text[160];
    if (pareto_sizes(n_rows, n_objectives, text, sizeof text))
        return 0;
    return pareto_workspace_bytes((long)n_rows, (int)n_objectives);
}

int smart_pareto_max_objectives(void) { return SMART_PARETO_MAX_OBJECTIVES; }

int smart_ensemble_scores_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *weights,
                              const double *obs, double *out, int32_t method, void *workspace, int64_t workspace_bytes,
                              void *stream)
{
    static const char entry[] = "smart_ensemble_scores_hip";
    int rc;
    if (!sim || !out)
        return fail(SMART_E_NULL, "%s: sim and out are required (%s is NULL)", entry, !sim ? "sim" : "out");
    char text[160];
    if ((rc = ensemble_sizes(n_samples, n_reports, method, text, sizeof text)))
        return fail(rc, "%s: %s", entry, text);
    if (ld < n_samples)
        return fail(SMART_E_SIZE, "%s: ld %lld is less than n_samples %lld", entry, (long long)ld, (long long)n_samples);
    const bool lds = method == SMART_ENS_LDS || (method == SMART_ENS_AUTO && n_samples <= ensemble_scores_lds_capacity());
    if (!lds && (rc = workspace_fits(entry, /*for_objfn=*/false, workspace, workspace_bytes,
                                     ensemble_scores_step_bytes((long)n_samples, weights != nullptr))))
        return rc;
    if ((rc = device_ready()))
        return rc;
    launch_ensemble_scores((long)n_samples, (long)n_reports, sim, (long)ld, weights, obs, out, lds, workspace,
                           (long)workspace_bytes, (hipStream_t)stream);
    return launched();
}

int64_t smart_ensemble_scores_workspace_bytes(int64_t n_samples, int64_t n_reports, int32_t weighted, int32_t method)
{
    char text[160];
    if (int rc = ensemble_sizes(n_samples, n_reports, method, text, sizeof text))
        return rc;
    if (method == SMART_ENS_LDS || (method == SMART_ENS_AUTO && n_samples <= ensemble_scores_lds_capacity()))
        return 0;
    return ensemble_scores_workspace_bytes((long)n_samples, (long)n_reports, weighted != 0);
}

int64_t smart_ensemble_scores_lds_capacity(void) { return ensemble_scores_lds_capacity(); }

int smart_dynia_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                    int32_t half_width, int32_t min_valid, double fraction, const uint8_t *cat, int32_t n_factors,
                    int32_t n_bins, int32_t support, double *shares, double *cut, int32_t *retained, int32_t *count,
                    double *err, int64_t ld_err, void *workspace, int64_t workspace_bytes, void *stream)
{
    static const char entry[] = "smart_dynia_hip";
    int rc;
    if (!sim || !obs || !cat || !shares || !cut || !retained || !count)
        return fail(SMART_E_NULL, "%s: sim, obs, cat, shares, cut, retained and count are required (%s is NULL)", entry,
                    !sim ? "sim"
                         : (!obs ? "obs"
                                 : (!cat ? "cat" : (!shares ? "shares" : (!cut ? "cut" : (!retained ? "retained" : "count"))))));
    char text[160];
    if (dynia_sizes(n_samples, n_reports, half_width, n_factors, n_bins, text, sizeof text))
        return fail(SMART_E_SIZE, "%s: %s", entry, text);
    if (ld < n_samples)
        return fail(SMART_E_SIZE, "%s: ld %lld is less than n_samples %lld", entry, (long long)ld, (long long)n_samples);
    if (err && ld_err < n_samples)
        return fail(SMART_E_SIZE, "%s: ld_err %lld is less than n_samples %lld", entry, (long long)ld_err,
                    (long long)n_samples);
    if (min_valid < 1 || min_valid > 2 * half_width + 1)
        return fail(SMART_E_SIZE, "%s: min_valid %d must be in 1 .. %d (the window)", entry, (int)min_valid,
                    2 * (int)half_width + 1);
    if (!(fraction > 0.0 && fraction <= 1.0))
        return fail(SMART_E_SIZE, "%s: fraction %g is outside (0, 1]", entry, fraction);
    if (support != SMART_DYNIA_EQUAL && support != SMART_DYNIA_LINEAR)
        return fail(SMART_E_MODE, "%s: support '%d' unknown.", entry, (int)support);
    if ((rc = workspace_fits(entry, /*for_objfn=*/false, workspace, workspace_bytes, dynia_step_bytes((long)n_samples))) ||
        (rc = device_ready()))
        return rc;
    launch_dynia((long)n_samples, (long)n_reports, sim, (long)ld, obs, (int)half_width, (int)min_valid, fraction, cat,
                 (int)n_factors, (int)n_bins, (int)support, shares, cut, retained, count, err, (long)ld_err, workspace,
                 (long)workspace_bytes, (hipStream_t)stream);
    return launched();
}

int64_t smart_dynia_workspace_bytes(int64_t n_samples, int64_t n_reports, int32_t half_width, int32_t n_factors,
                                    int32_t n_bins)
{
    char text[160];
    if (dynia_sizes(n_samples, n_reports, half_width, n_factors, n_bins, text, sizeof text))
        return SMART_E_SIZE;
    return dynia_workspace_bytes((long)n_samples, (long)n_reports);
}

int32_t smart_dynia_max_half_width(void) { return dynia_max_half_width(); }

int64_t smart_dynia_lds_capacity(void) { return dynia_lds_capacity(); }

int smart_pawn_ks_hip(int64_t n_samples, int64_t n_rows, const double *y, int64_t ld, const uint8_t *cat, int32_t n_factors,
                      int32_t n_bins, double *ks, int32_t *counts, int32_t method, void *workspace, int64_t workspace_bytes,
                      void *stream)
{
    static const char entry[] = "smart_pawn_ks_hip";
    int rc;
    if (!y || !cat || !ks || !counts)
        return fail(SMART_E_NULL, "%s: y, cat, ks and counts are required (%s is NULL)", entry,
                    !y ? "y" : (!cat ? "cat" : (!ks ? "ks" : "counts")));
    char text[160];
    if ((rc = pawn_sizes(n_samples, n_rows, text, sizeof text)))
        return fail(rc, "%s: %s", entry, text);
    if (ld < n_samples)
        return fail(SMART_E_SIZE, "%s: ld %lld is less than n_samples %lld", entry, (long long)ld, (long long)n_samples);
    if (n_factors < 1 || n_factors > SMART_PAWN_MAX_FACTORS)
        return fail(SMART_E_SIZE, "%s: n_factors %d must be in 1 .. %d", entry, (int)n_factors, SMART_PAWN_MAX_FACTORS);
    if (n_bins < 1 || n_bins > SMART_PAWN_MAX_BINS)
        return fail(SMART_E_SIZE, "%s: n_bins %d must be in 1 .. %d", entry, (int)n_bins, SMART_PAWN_MAX_BINS);
    if ((rc = pawn_method(n_samples, method, text, sizeof text)))
        return fail(rc, "%s: %s", entry, text);
    const bool lds = method == SMART_PAWN_LDS || (method == SMART_PAWN_AUTO && n_samples <= pawn_lds_capacity());
    if (!lds && (rc = workspace_fits(entry, /*for_objfn=*/false, workspace, workspace_bytes, pawn_step_bytes((long)n_samples))))
        return rc;
    if ((rc = device_ready()))
        return rc;
    launch_pawn((long)n_samples, (long)n_rows, y, (long)ld, cat, (int)n_factors, (int)n_bins, ks, counts, lds, workspace,
                (long)workspace_bytes, (hipStream_t)stream);
    return launched();
}

int64_t smart_pawn_workspace_bytes(int64_t n_samples, int64_t n_rows, int32_t method)
{
    char text[160];
    int rc;
    if ((rc = pawn_sizes(n_samples, n_rows, text, sizeof text)) || (rc = pawn_method(n_samples, method, text, sizeof text)))
        return rc;
    if (method == SMART_PAWN_LDS || (method == SMART_PAWN_AUTO && n_samples <= pawn_lds_capacity()))
        return 0;
    return pawn_workspace_bytes((long)n_samples, (long)n_rows);
}

int64_t smart_pawn_lds_capacity(void) { return pawn_lds_capacity(); }

} // extern "C"
