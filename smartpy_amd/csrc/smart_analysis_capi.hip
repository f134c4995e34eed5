// smart_analysis_capi.hip -- the C ABI of the analyses of a stored discharge matrix sim[R][ld] (include/smart_amd.h):
// objective functions, weighted quantiles, objective functions per window, flow duration curves, hydrological signatures, Sobol indices, the block bootstrap of the objective functions, and of
// the Pareto selection over the scores they leave, the ensemble verification scores, the dynamic identifiability analysis and the PAWN sensitivity per report step, the residual error model (likelihood and draws), with their capacity and workspace entries -- validation and launch --
// and the one kernel among them that has no unit of its own, smart_objfn_matrix.  Every refusal comes before the device is asked for; every rule is stated once, as a
// method of the Check below, which carries the entry's name for the text.
#include "smart_capi_internal.h"
#include "smart_device.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>

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

// ---- the rules of the entries ---------------------------------------------------------------------------------------
// One Check per call, the rules in the entry's own order (the order is part of the ABI: it says which refusal wins).  The
// first rule that is broken decides: it sets the code and, where the Check carries the entry's name, the thread's text
// through fail(); every rule after it is passed over, so a rule may rely on the ones before it.  A workspace query states
// the same rules to a Check without a name: the code alone, the thread's text untouched.
struct Named {
    const char *name;
    const void *ptr;
};
#define NAMED(p) Named{#p, p}
struct Count {
    const char *name;
    long long value;
};
#define COUNT(n) Count{#n, (long long)(n)}

constexpr long long kInt32Max = 0x7fffffffll;
constexpr long long kTwo32 = 1ll << 32; // counter words and thresholds of the entries that draw

class Check
{
  public:
    explicit Check(const char *entry) : entry_(entry) {}
    int rc = SMART_OK;
    bool ok() const { return rc == SMART_OK; }
    int ready() const { return rc ? rc : device_ready(); } // before the launch: the refusal, or whether there is a device

    __attribute__((format(printf, 3, 4))) void refuse(int code, const char *fmt, ...)
    {
        if (rc)
            return;
        rc = code;
        if (!entry_)
            return;
        char text[384];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof text, fmt, ap);
        va_end(ap);
        fail(code, "%s: %s", entry_, text);
    }

    // pointers an entry cannot do without: the first that is NULL is named (the two oldest entries name none)
    void required(std::initializer_list<Named> ptrs, bool name_it = true)
    {
        const char *missing = first_null(ptrs);
        if (missing && name_it)
            refuse(SMART_E_NULL, "%s are required (%s is NULL)", names(ptrs, " and ").s, missing);
        else if (missing)
            refuse(SMART_E_NULL, "%s are required", names(ptrs, " and ").s);
    }
    // ... and those it cannot do without once `count` is above zero
    void needs(const char *what, int count, std::initializer_list<Named> ptrs)
    {
        const char *missing = count > 0 ? first_null(ptrs) : nullptr;
        if (missing)
            refuse(SMART_E_NULL, "%s %d needs %s (%s is NULL)", what, count, names(ptrs, " and ").s, missing);
    }
    // ... and those a phase of a step, or an option of it, cannot do without: "the propose phase needs", "parents need"
    void wants(const char *who_needs, std::initializer_list<Named> ptrs)
    {
        if (const char *missing = first_null(ptrs))
            refuse(SMART_E_NULL, "%s %s (%s is NULL)", who_needs, names(ptrs, " and ").s, missing);
    }
    void at_least_one(std::initializer_list<Count> counts)
    {
        bool bad = false;
        for (const Count &c : counts)
            bad |= c.value < 1;
        if (!bad)
            return;
        Text got;
        for (const Count &c : counts)
            got.add(got.s[0] ? ", " : "").add(c.value);
        refuse(SMART_E_SIZE, "need %s >= 1 (got %s)", names(counts, ", ").s, got.s);
    }
    void in_range(const char *name, long long v, long long lo, long long hi, const char *suffix = "")
    {
        if (v < lo || v > hi)
            refuse(SMART_E_SIZE, "%s %lld must be in %lld .. %s%s", name, v, lo,
                   hi == kInt32Max ? "2^31 - 1" : Text().add(hi).s, suffix);
    }
    void ld_holds(const char *name, long long ld, long long n_samples)
    {
        if (ld < n_samples)
            refuse(SMART_E_SIZE, "%s %lld is less than n_samples %lld", name, ld, n_samples);
    }
    void one_launch(const char *name, long long steps) // a grid dimension
    {
        if (steps > kInt32Max)
            refuse(SMART_E_SIZE, "%s %lld is more than one launch takes (2^31 - 1)", name, steps);
    }
    void samples_at_most(long long n_samples, long long most) // where sample indices are kept in 24 bits
    {
        if (n_samples > most)
            refuse(SMART_E_SIZE, "n_samples %lld, at most %lld (2^24)", n_samples, most);
    }
    void method_known(int method)
    {
        if (!smart::method_known(method))
            refuse(SMART_E_MODE, "method '%d' unknown.", method);
    }
    void form_fits(int method, const char *form, long long n_samples, long long capacity)
    {
        if (method == kMethodCapacity && n_samples > capacity)
            refuse(SMART_E_SIZE, "the %s form takes at most %lld samples, not %lld", form, capacity, n_samples);
    }
    // the sizes of a matrix read per window: every count >= 1 (n_probs where the entry has one), ld, 2^31, the window cap
    void windowed_sizes(int64_t n_samples, int64_t n_reports, int64_t ld, int32_t n_windows, const int32_t *n_probs)
    {
        if (n_probs)
            at_least_one({COUNT(n_samples), COUNT(n_reports), COUNT(n_windows), Count{"n_probs", *n_probs}});
        else
            at_least_one({COUNT(n_samples), COUNT(n_reports), COUNT(n_windows)});
        ld_holds("ld", ld, n_samples);
        one_launch("n_reports", n_reports);
        if (n_windows > objfn_max_windows())
            refuse(SMART_E_SIZE, "n_windows %d, at most %d per call", (int)n_windows, objfn_max_windows());
    }
    // where the window array is optional: without one there is one window
    void window_array_given(const int32_t *window, int32_t n_windows)
    {
        if (!window && n_windows != 1)
            refuse(SMART_E_SIZE, "n_windows %d without a window array (NULL is one window)", (int)n_windows);
    }
    // every probability inside (0, 1], or [0, 1] where rank 1 has a probability of its own (a NaN is outside both)
    void probs_inside(const double *probs, int32_t n_probs, bool zero_too)
    {
        for (int32_t k = 0; ok() && k < n_probs; ++k)
            if (!((zero_too ? probs[k] >= 0.0 : probs[k] > 0.0) && probs[k] <= 1.0))
                refuse(SMART_E_SIZE, "probability %d is %g, outside %s", (int)k, probs[k], zero_too ? "[0, 1]" : "(0, 1]");
    }
    void eps_usable(double eps)
    {
        if (!(eps >= 0.0) || std::isinf(eps))
            refuse(SMART_E_SIZE, "eps %g must be finite and >= 0", eps);
    }
    void transform_known(int32_t transform)
    {
        if (transform < SMART_TRANSFORM_NONE || transform > SMART_TRANSFORM_INVERSE)
            refuse(SMART_E_MODE, "transform '%d' unknown.", (int)transform);
    }
    // the objectives of a call: every column inside the matrix and named once, every direction known, a finite target
    // where the direction is TARGET.  (The loops read the arrays: they are walked only while no rule is broken, one
    // objective after the other.)  `column` and `ld_name` are the entry's words for the two.
    void objectives_hold(int32_t n_objectives, const char *column, const int32_t *columns, const char *ld_name, long long ld,
                         const int32_t *direction, const double *target)
    {
        for (int32_t m = 0; ok() && m < n_objectives; ++m) {
            if (columns[m] < 0 || columns[m] >= ld)
                refuse(SMART_E_SIZE, "%s %d of objective %d is outside 0 .. %s - 1 = %lld", column, (int)columns[m], (int)m,
                       ld_name, ld - 1);
            for (int32_t k = 0; k < m; ++k)
                if (columns[k] == columns[m])
                    refuse(SMART_E_SIZE, "%s %d is named twice (objectives %d and %d)", column, (int)columns[m], (int)k,
                           (int)m);
        }
        for (int32_t m = 0; ok() && m < n_objectives; ++m)
            if (direction[m] != SMART_PARETO_MAX && direction[m] != SMART_PARETO_MIN && direction[m] != SMART_PARETO_TARGET)
                refuse(SMART_E_MODE, "direction '%d' of objective %d unknown.", (int)direction[m], (int)m);
        for (int32_t m = 0; ok() && m < n_objectives; ++m) {
            if (direction[m] != SMART_PARETO_TARGET)
                continue;
            if (!target)
                refuse(SMART_E_NULL, "objective %d is a TARGET (target is NULL)", (int)m);
            else if (!std::isfinite(target[m]))
                refuse(SMART_E_SIZE, "target %g of objective %d must be finite", target[m], (int)m);
        }
    }
    // the box of a generational sampler's call: the launch matrix wide enough, every varying column inside it and named
    // once, finite lo <= hi per dimension
    void box_holds(int32_t n_dims, long long ld, const int32_t *columns, const double *lo, const double *hi)
    {
        if (ok() && ld < n_dims)
            refuse(SMART_E_SIZE, "ld %lld is less than n_dims %d", ld, (int)n_dims);
        for (int j = 0; ok() && j < n_dims; ++j) {
            if (columns[j] < 0 || columns[j] >= ld)
                refuse(SMART_E_SIZE, "columns[%d] %d must be in 0 .. %lld", j, (int)columns[j], ld - 1);
            for (int k = 0; ok() && k < j; ++k)
                if (columns[k] == columns[j])
                    refuse(SMART_E_SIZE, "columns[%d] and columns[%d] name the same column %d", k, j, (int)columns[j]);
            if (ok() && !(std::isfinite(lo[j]) && std::isfinite(hi[j]) && lo[j] <= hi[j]))
                refuse(SMART_E_SIZE, "lo[%d] %g and hi[%d] %g: need finite lo <= hi", j, lo[j], j, hi[j]);
        }
    }
    // a workspace of `need` bytes: present where any are needed, and large enough
    void workspace_fits(bool for_objfn, const void *workspace, int64_t workspace_bytes, long need)
    {
        if (need > 0 && !workspace)
            refuse(SMART_E_NULL,
                   for_objfn ? "objfn needs a workspace of %ld bytes (workspace is NULL)"
                             : "a workspace of %ld bytes is needed (workspace is NULL)",
                   need);
        else if (workspace_bytes < (workspace ? need : 0))
            refuse(SMART_E_SIZE, "workspace_bytes %lld, need %ld", (long long)workspace_bytes, need);
    }

  private:
    struct Text { // the lists inside a refusal
        char s[128] = "";
        Text &add(const char *piece)
        {
            strncat(s, piece, sizeof s - strlen(s) - 1);
            return *this;
        }
        Text &add(long long v)
        {
            const size_t at = strlen(s);
            snprintf(s + at, sizeof s - at, "%lld", v);
            return *this;
        }
    };
    template <class Item>
    static Text names(std::initializer_list<Item> items, const char *before_last) // "a, b and c", "a, b, c"
    {
        Text t;
        size_t i = 0;
        for (const Item &x : items)
            t.add(i++ == 0 ? "" : (i == items.size() ? before_last : ", ")).add(x.name);
        return t;
    }
    static const char *first_null(std::initializer_list<Named> ptrs)
    {
        for (const Named &p : ptrs)
            if (!p.ptr)
                return p.name;
        return nullptr;
    }
    const char *entry_; // null: a workspace query
};

// the end of every entry, after its launch
static int launched()
{
    HIP_TRY(hipGetLastError());
    clear_error();
    return SMART_OK;
}

// ---- the size rules an entry shares with its workspace query ---------------------------------------------------------
static void sobol_sizes(Check &c, int64_t n_base, int32_t n_params, int64_t n_rows, int32_t n_resamples)
{
    c.in_range("n_base", n_base, 1, kInt32Max);
    c.in_range("n_params", n_params, 1, SMART_SOBOL_MAX_PARAMS);
    c.in_range("n_rows", n_rows, 1, kInt32Max);
    c.in_range("n_resamples", n_resamples, 0, sobol_max_resamples());
}

static void bootstrap_sizes(Check &c, int64_t n_samples, int32_t n_windows, int32_t n_resamples)
{
    c.in_range("n_samples", n_samples, 1, kInt32Max);
    c.in_range("n_windows", n_windows, 1, bootstrap_max_windows());
    c.in_range("n_resamples", n_resamples, 0, bootstrap_max_resamples());
}

static void pareto_sizes(Check &c, int64_t n_rows, int32_t n_objectives)
{
    c.in_range("n_rows", n_rows, 1, kInt32Max);
    c.in_range("n_objectives", n_objectives, 1, SMART_PARETO_MAX_OBJECTIVES);
}

// (the method belongs to the sizes here: the entry tests it before ld)
static void ensemble_sizes(Check &c, int64_t n_samples, int64_t n_reports, int32_t method)
{
    c.at_least_one({COUNT(n_samples), COUNT(n_reports)});
    c.one_launch("n_reports", n_reports);
    c.samples_at_most(n_samples, ensemble_scores_max_samples());
    c.method_known(method);
    c.form_fits(method, "LDS", n_samples, ensemble_scores_lds_capacity());
}

static void dynia_sizes(Check &c, int64_t n_samples, int64_t n_reports, int32_t half_width, int32_t n_factors, int32_t n_bins)
{
    c.at_least_one({COUNT(n_samples), COUNT(n_reports)});
    c.in_range("n_samples", n_samples, 1, kInt32Max);
    c.one_launch("n_reports", n_reports);
    c.in_range("half_width", half_width, 0, dynia_max_half_width());
    c.in_range("n_factors", n_factors, 1, SMART_DYNIA_MAX_FACTORS);
    c.in_range("n_bins", n_bins, 1, SMART_DYNIA_MAX_BINS);
}

// (ld, the factors and the bins lie between the sizes and the method in the entry: two helpers)
static void pawn_sizes(Check &c, int64_t n_samples, int64_t n_rows)
{
    c.at_least_one({COUNT(n_samples), COUNT(n_rows)});
    c.samples_at_most(n_samples, pawn_max_samples());
    c.one_launch("n_rows", n_rows);
}

static void pawn_method(Check &c, int64_t n_samples, int32_t method)
{
    c.method_known(method);
    c.form_fits(method, "LDS", n_samples, pawn_lds_capacity());
}

} // namespace smart

using namespace smart;

extern "C" {

int smart_objfn_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                    const double *gw_sim, double gw_obs, double *objfn, void *stream)
{
    Check c("smart_objfn_hip");
    c.required({NAMED(sim), NAMED(obs), NAMED(objfn)}, /*name_it=*/false);
    if (n_samples < 1 || n_reports < 1 || ld < n_samples)
        c.refuse(SMART_E_SIZE, "need n_samples, n_reports >= 1 and ld >= n_samples");
    if (int rc = c.ready())
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
    Check c("smart_weighted_quantiles_hip");
    c.required({NAMED(sim), NAMED(probs), NAMED(out)}, /*name_it=*/false);
    if (n_samples < 1 || n_reports < 1 || n_probs < 1 || ld < n_samples)
        c.refuse(SMART_E_SIZE, "need n_samples, n_reports, n_probs >= 1 and ld >= n_samples");
    c.one_launch("n_reports", n_reports);
    if (n_probs > SMART_QUANTILES_MAX_PROBS)
        c.refuse(SMART_E_SIZE, "%d probabilities, at most %d per call", (int)n_probs, SMART_QUANTILES_MAX_PROBS);
    c.probs_inside(probs, n_probs, /*zero_too=*/false);
    c.method_known(method);
    c.form_fits(method, "sort", n_samples, quantiles_sort_capacity());
    if (int rc = c.ready())
        return rc;
    launch_quantiles((long)n_samples, (long)n_reports, sim, (long)ld, weights, probs, (int)n_probs, out,
                     capacity_form(method, (long)n_samples, quantiles_sort_capacity()), (hipStream_t)stream);
    return launched();
}

int64_t smart_quantiles_sort_capacity(void) { return quantiles_sort_capacity(); }

int smart_objfn_windows_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                            const int32_t *window, int32_t n_windows, int32_t transform, double eps, double *objfn,
                            void *stream)
{
    Check c("smart_objfn_windows_hip");
    c.required({NAMED(sim), NAMED(obs), NAMED(window), NAMED(objfn)});
    c.windowed_sizes(n_samples, n_reports, ld, n_windows, nullptr);
    c.eps_usable(eps);
    c.transform_known(transform);
    if (int rc = c.ready())
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
    Check c("smart_flow_duration_hip");
    c.required({NAMED(sim), NAMED(probs), NAMED(quant)});
    if (objfn && !obs)
        c.refuse(SMART_E_NULL, "objfn needs obs (obs is NULL)");
    c.windowed_sizes(n_samples, n_reports, ld, n_windows, &n_probs);
    c.window_array_given(window, n_windows);
    if (n_probs > SMART_QUANTILES_MAX_PROBS)
        c.refuse(SMART_E_SIZE, "n_probs %d, at most %d probabilities per call", (int)n_probs, SMART_QUANTILES_MAX_PROBS);
    c.probs_inside(probs, n_probs, /*zero_too=*/true);
    c.eps_usable(eps);
    if (!(seg_lo >= 0.0 && seg_lo < seg_hi && seg_hi <= 1.0))
        c.refuse(SMART_E_SIZE, "the segment (%g, %g) is not 0 <= seg_lo < seg_hi <= 1", seg_lo, seg_hi);
    c.transform_known(transform);
    c.method_known(method);
    if (objfn && method == SMART_FDC_SELECT)
        c.refuse(SMART_E_MODE, "the select form gives order statistics only (objfn given)");
    const long capacity = flow_duration_sort_capacity();
    if (n_reports > capacity && (objfn || method == SMART_FDC_SORT))
        c.refuse(SMART_E_SIZE, "%s at most %ld report steps (the sort capacity), not %lld",
                 objfn ? "the objective functions of the curve take" : "the sort form takes", capacity,
                 (long long)n_reports);
    if (c.ok() && objfn)
        c.workspace_fits(/*for_objfn=*/true, workspace, workspace_bytes,
                         flow_duration_workspace_bytes((long)n_reports, (int)n_windows, true));
    if (int rc = c.ready())
        return rc;
    launch_flow_duration((long)n_samples, (long)n_reports, sim, (long)ld, obs, window, (int)n_windows, probs, (int)n_probs,
                         quant, (int)transform, eps, seg_lo, seg_hi, objfn, (double *)workspace,
                         capacity_form(method, (long)n_reports, capacity), (hipStream_t)stream);
    return launched();
}

int64_t smart_flow_duration_workspace_bytes(int64_t n_reports, int32_t n_windows, int32_t with_objfn)
{
    if (n_reports < 1 || n_reports > kInt32Max || n_windows < 1) // (its own three arguments, and no more: smart_amd.h)
        return SMART_E_SIZE;
    return flow_duration_workspace_bytes((long)n_reports, (int)n_windows, with_objfn != 0);
}

int64_t smart_flow_duration_sort_capacity(void) { return flow_duration_sort_capacity(); }

int smart_signatures_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                         const int32_t *window, int32_t n_windows, double alpha, const double *pulse, double *sig,
                         void *stream)
{
    Check c("smart_signatures_hip");
    c.required({NAMED(sim), NAMED(sig)});
    c.windowed_sizes(n_samples, n_reports, ld, n_windows, nullptr);
    c.window_array_given(window, n_windows);
    if (!(alpha > 0.0 && alpha < 1.0))
        c.refuse(SMART_E_SIZE, "alpha %g must lie inside (0, 1)", alpha);
    if (int rc = c.ready())
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
    Check c("smart_sobol_indices_hip");
    c.required({NAMED(y), NAMED(s1), NAMED(st), NAMED(moments)});
    c.needs("n_resamples", n_resamples, {NAMED(counts), NAMED(s1_std), NAMED(st_std)});
    sobol_sizes(c, n_base, n_params, n_rows, n_resamples);
    if (c.ok() && ld < n_base * (n_params + 2))
        c.refuse(SMART_E_SIZE, "ld %lld is less than n_base * (n_params + 2) = %lld", (long long)ld,
                 (long long)(n_base * (n_params + 2)));
    c.workspace_fits(/*for_objfn=*/false, workspace, workspace_bytes, sobol_workspace_bytes());
    if (int rc = c.ready())
        return rc;
    launch_sobol((long)n_base, (int)n_params, (long)n_rows, y, (long)ld, s1, st, moments, counts, (int)n_resamples,
                 s1_std, st_std, (hipStream_t)stream);
    return launched();
}

int64_t smart_sobol_workspace_bytes(int64_t n_base, int32_t n_params, int64_t n_rows, int32_t n_resamples)
{
    Check c(nullptr);
    sobol_sizes(c, n_base, n_params, n_rows, n_resamples);
    return c.ok() ? sobol_workspace_bytes() : c.rc;
}

int32_t smart_sobol_max_resamples(void) { return sobol_max_resamples(); }

int64_t smart_sobol_lds_capacity(void) { return sobol_lds_capacity(); }

int smart_objfn_bootstrap_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                              const int32_t *window, int32_t n_windows, int32_t transform, double eps,
                              const uint16_t *counts, int32_t n_resamples, const double *probs, int32_t n_probs,
                              double *point, double *stats, double *replicates, void *workspace, int64_t workspace_bytes,
                              void *stream)
{
    Check c("smart_objfn_bootstrap_hip");
    c.required({NAMED(sim), NAMED(obs), NAMED(window), NAMED(point)});
    c.needs("n_resamples", n_resamples, {NAMED(counts), NAMED(probs), NAMED(stats)});
    bootstrap_sizes(c, n_samples, n_windows, n_resamples);
    c.at_least_one({COUNT(n_reports)});
    c.ld_holds("ld", ld, n_samples);
    c.one_launch("n_reports", n_reports);
    if (n_resamples > 0) { // (without replicates neither n_probs nor the probabilities are looked at)
        c.in_range("n_probs", n_probs, 1, SMART_QUANTILES_MAX_PROBS);
        c.probs_inside(probs, n_probs, /*zero_too=*/false);
    }
    c.eps_usable(eps);
    c.transform_known(transform);
    if (c.ok())
        c.workspace_fits(/*for_objfn=*/false, workspace, workspace_bytes,
                         bootstrap_workspace_bytes((long)n_samples, (int)n_windows, (int)n_resamples, replicates != nullptr));
    if (int rc = c.ready())
        return rc;
    launch_bootstrap((long)n_samples, (long)n_reports, sim, (long)ld, obs, window, (int)n_windows, (int)transform, eps,
                     counts, (int)n_resamples, probs, n_resamples > 0 ? (int)n_probs : 0, point, stats, replicates,
                     (double *)workspace, (hipStream_t)stream);
    return launched();
}

int64_t smart_bootstrap_workspace_bytes(int64_t n_samples, int32_t n_windows, int32_t n_resamples, int32_t with_replicates)
{
    Check c(nullptr);
    bootstrap_sizes(c, n_samples, n_windows, n_resamples);
    return c.ok() ? bootstrap_workspace_bytes((long)n_samples, (int)n_windows, (int)n_resamples, with_replicates != 0) : c.rc;
}

int32_t smart_bootstrap_max_windows(void) { return bootstrap_max_windows(); }

int32_t smart_bootstrap_max_resamples(void) { return bootstrap_max_resamples(); }

int smart_pareto_counts_hip(int64_t n_rows, const double *scores, int64_t ld, const int32_t *columns,
                            const int32_t *direction, const double *target, int32_t n_objectives, const uint8_t *eligible,
                            int32_t *dominated_by, void *workspace, int64_t workspace_bytes, void *stream)
{
    Check c("smart_pareto_counts_hip");
    c.required({NAMED(scores), NAMED(columns), NAMED(direction), NAMED(dominated_by)});
    pareto_sizes(c, n_rows, n_objectives);
    c.objectives_hold(n_objectives, "column", columns, "ld", (long long)ld, direction, target);
    if (c.ok())
        c.workspace_fits(/*for_objfn=*/false, workspace, workspace_bytes,
                         pareto_workspace_bytes((long)n_rows, (int)n_objectives));
    if (int rc = c.ready())
        return rc;
    launch_pareto((long)n_rows, scores, (long)ld, columns, direction, target, (int)n_objectives, eligible, dominated_by,
                  workspace, (hipStream_t)stream);
    return launched();
}

int64_t smart_pareto_workspace_bytes(int64_t n_rows, int32_t n_objectives)
{
    Check c(nullptr);
    pareto_sizes(c, n_rows, n_objectives);
    return c.ok() ? pareto_workspace_bytes((long)n_rows, (int)n_objectives) : 0; // (0, not the code: smart_amd.h)
}

int smart_pareto_max_objectives(void) { return SMART_PARETO_MAX_OBJECTIVES; }

int smart_ensemble_scores_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *weights,
                              const double *obs, double *out, int32_t method, void *workspace, int64_t workspace_bytes,
                              void *stream)
{
    Check c("smart_ensemble_scores_hip");
    c.required({NAMED(sim), NAMED(out)});
    ensemble_sizes(c, n_samples, n_reports, method);
    c.ld_holds("ld", ld, n_samples);
    const bool lds = capacity_form(method, (long)n_samples, ensemble_scores_lds_capacity());
    if (c.ok() && !lds)
        c.workspace_fits(/*for_objfn=*/false, workspace, workspace_bytes,
                         ensemble_scores_step_bytes((long)n_samples, weights != nullptr));
    if (int rc = c.ready())
        return rc;
    launch_ensemble_scores((long)n_samples, (long)n_reports, sim, (long)ld, weights, obs, out, lds, workspace,
                           (long)workspace_bytes, (hipStream_t)stream);
    return launched();
}

int64_t smart_ensemble_scores_workspace_bytes(int64_t n_samples, int64_t n_reports, int32_t weighted, int32_t method)
{
    Check c(nullptr);
    ensemble_sizes(c, n_samples, n_reports, method);
    if (!c.ok())
        return c.rc;
    if (capacity_form(method, (long)n_samples, ensemble_scores_lds_capacity()))
        return 0;
    return batched_workspace_bytes(ensemble_scores_step_bytes((long)n_samples, weighted != 0), (long)n_reports);
}

int64_t smart_ensemble_scores_lds_capacity(void) { return ensemble_scores_lds_capacity(); }

int smart_dynia_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                    int32_t half_width, int32_t min_valid, double fraction, const uint8_t *cat, int32_t n_factors,
                    int32_t n_bins, int32_t support, double *shares, double *cut, int32_t *retained, int32_t *count,
                    double *err, int64_t ld_err, void *workspace, int64_t workspace_bytes, void *stream)
{
    Check c("smart_dynia_hip");
    c.required({NAMED(sim), NAMED(obs), NAMED(cat), NAMED(shares), NAMED(cut), NAMED(retained), NAMED(count)});
    dynia_sizes(c, n_samples, n_reports, half_width, n_factors, n_bins);
    c.ld_holds("ld", ld, n_samples);
    if (err)
        c.ld_holds("ld_err", ld_err, n_samples);
    c.in_range("min_valid", min_valid, 1, 2 * (long long)half_width + 1, " (the window)");
    if (!(fraction > 0.0 && fraction <= 1.0))
        c.refuse(SMART_E_SIZE, "fraction %g is outside (0, 1]", fraction);
    if (support != SMART_DYNIA_EQUAL && support != SMART_DYNIA_LINEAR)
        c.refuse(SMART_E_MODE, "support '%d' unknown.", (int)support);
    c.workspace_fits(/*for_objfn=*/false, workspace, workspace_bytes, dynia_step_bytes((long)n_samples));
    if (int rc = c.ready())
        return rc;
    launch_dynia((long)n_samples, (long)n_reports, sim, (long)ld, obs, (int)half_width, (int)min_valid, fraction, cat,
                 (int)n_factors, (int)n_bins, (int)support, shares, cut, retained, count, err, (long)ld_err, workspace,
                 (long)workspace_bytes, (hipStream_t)stream);
    return launched();
}

int64_t smart_dynia_workspace_bytes(int64_t n_samples, int64_t n_reports, int32_t half_width, int32_t n_factors,
                                    int32_t n_bins)
{
    Check c(nullptr);
    dynia_sizes(c, n_samples, n_reports, half_width, n_factors, n_bins);
    return c.ok() ? batched_workspace_bytes(dynia_step_bytes((long)n_samples), (long)n_reports) : c.rc;
}

int32_t smart_dynia_max_half_width(void) { return dynia_max_half_width(); }

int64_t smart_dynia_lds_capacity(void) { return dynia_lds_capacity(); }

int smart_pawn_ks_hip(int64_t n_samples, int64_t n_rows, const double *y, int64_t ld, const uint8_t *cat, int32_t n_factors,
                      int32_t n_bins, double *ks, int32_t *counts, int32_t method, void *workspace, int64_t workspace_bytes,
                      void *stream)
{
    Check c("smart_pawn_ks_hip");
    c.required({NAMED(y), NAMED(cat), NAMED(ks), NAMED(counts)});
    pawn_sizes(c, n_samples, n_rows);
    c.ld_holds("ld", ld, n_samples);
    c.in_range("n_factors", n_factors, 1, SMART_PAWN_MAX_FACTORS);
    c.in_range("n_bins", n_bins, 1, SMART_PAWN_MAX_BINS);
    pawn_method(c, n_samples, method);
    const bool lds = capacity_form(method, (long)n_samples, pawn_lds_capacity());
    if (c.ok() && !lds)
        c.workspace_fits(/*for_objfn=*/false, workspace, workspace_bytes, pawn_step_bytes((long)n_samples));
    if (int rc = c.ready())
        return rc;
    launch_pawn((long)n_samples, (long)n_rows, y, (long)ld, cat, (int)n_factors, (int)n_bins, ks, counts, lds, workspace,
                (long)workspace_bytes, (hipStream_t)stream);
    return launched();
}

int64_t smart_pawn_workspace_bytes(int64_t n_samples, int64_t n_rows, int32_t method)
{
    Check c(nullptr);
    pawn_sizes(c, n_samples, n_rows);
    pawn_method(c, n_samples, method);
    if (!c.ok())
        return c.rc;
    if (capacity_form(method, (long)n_samples, pawn_lds_capacity()))
        return 0;
    return batched_workspace_bytes(pawn_step_bytes((long)n_samples), (long)n_rows);
}

int64_t smart_pawn_lds_capacity(void) { return pawn_lds_capacity(); }

// (not an analysis of a matrix, but validated by the same Check: the step of the DE-MCz sampler, smart_demcz.hip)
int smart_demcz_step_hip(int64_t n_chains, int64_t chain_offset, int32_t n_dims, uint64_t seed, int64_t generation,
                         int64_t archive_size, int64_t capacity, double *x, double *logp, double *carry, int32_t *accepted,
                         double *proposal, uint8_t *out, const double *score, int64_t score_stride, int32_t score_kind,
                         int64_t n_obs, double n_eff, double sigma, const double *carry_new, int32_t n_carry,
                         int32_t append, double *archive, double *archive_logp, double *archive_carry, int32_t propose,
                         const double *lo, const double *hi, const double *scale, const double *gamma,
                         int64_t jump_threshold, int64_t cr_threshold, double *rows, int64_t ld, const int32_t *columns,
                         void *stream)
{
    Check c("smart_demcz_step_hip");
    c.required({NAMED(x), NAMED(logp), NAMED(proposal), NAMED(out), NAMED(archive)});
    c.at_least_one({COUNT(n_chains)});
    c.in_range("chain_offset", chain_offset, 0, kTwo32 - 1);
    if (c.ok() && n_chains > kTwo32 - chain_offset)
        c.refuse(SMART_E_SIZE, "chains %lld .. %lld: a chain's number stays below 2^32", (long long)chain_offset,
                 (long long)chain_offset + (long long)n_chains - 1);
    c.in_range("n_dims", n_dims, 1, SMART_DEMCZ_MAX_DIMS);
    c.in_range("generation", generation, 1, kTwo32 - 1);
    c.in_range("capacity", capacity, 1, kInt32Max);
    c.in_range("archive_size", archive_size, 0, capacity, " (the capacity)");
    c.in_range("n_carry", n_carry, 0, SMART_DEMCZ_MAX_CARRY);
    if (!score && !propose)
        c.refuse(SMART_E_NULL, "neither phase is asked for (score is NULL and propose is 0)");
    DemczCall call{};
    call.n_chains = (long)n_chains, call.chain_offset = (long)chain_offset, call.n_dims = n_dims, call.seed = seed;
    call.generation = (long)generation, call.archive_size = (long)archive_size, call.capacity = (long)capacity;
    call.x = x, call.logp = logp, call.carry = carry, call.accepted = accepted, call.proposal = proposal, call.out = out;
    call.score = score, call.score_stride = (long)score_stride, call.score_kind = score_kind, call.n_obs = (long)n_obs;
    call.n_eff = n_eff, call.sigma = sigma, call.carry_new = carry_new, call.n_carry = n_carry, call.append = append != 0;
    call.archive = archive, call.archive_logp = archive_logp, call.archive_carry = archive_carry, call.propose = propose != 0;
    call.lo = lo, call.hi = hi, call.scale = scale, call.gamma = gamma, call.jump_threshold = (long)jump_threshold;
    call.cr_threshold = (long)cr_threshold, call.rows = rows, call.ld = (long)ld, call.columns = columns;
    if (score) { // ---- the accept phase
        if (score_kind < SMART_DEMCZ_SCORE_LOGP || score_kind > SMART_DEMCZ_SCORE_RMSE_SIGMA)
            c.refuse(SMART_E_MODE, "score_kind '%d' unknown.", (int)score_kind);
        c.in_range("score_stride", score_stride, 1, kInt32Max);
        if (score_kind == SMART_DEMCZ_SCORE_RMSE)
            c.in_range("n_obs", n_obs, 1, kInt32Max);
        if (score_kind != SMART_DEMCZ_SCORE_LOGP && !(n_eff > 0.0 && std::isfinite(n_eff)))
            c.refuse(SMART_E_SIZE, "n_eff %g must be finite and > 0", n_eff);
        if (score_kind == SMART_DEMCZ_SCORE_RMSE_SIGMA && !(sigma > 0.0 && std::isfinite(sigma)))
            c.refuse(SMART_E_SIZE, "sigma %g must be finite and > 0", sigma);
        if (!accepted)
            c.refuse(SMART_E_NULL, "the accept phase needs accepted (accepted is NULL)");
        c.needs("n_carry", n_carry, {NAMED(carry), NAMED(carry_new)});
        if (append) {
            if (!archive_logp)
                c.refuse(SMART_E_NULL, "append needs archive_logp (archive_logp is NULL)");
            c.needs("append with n_carry", n_carry, {NAMED(archive_carry)});
            if (c.ok() && archive_size + chain_offset + n_chains > capacity)
                c.refuse(SMART_E_SIZE, "append of archive rows %lld .. %lld passes the capacity %lld",
                         (long long)(archive_size + chain_offset),
                         (long long)(archive_size + chain_offset + n_chains - 1), (long long)capacity);
        }
    } else if (append) {
        c.refuse(SMART_E_NULL, "append needs the accept phase (score is NULL)");
    }
    if (propose) { // ---- the propose phase
        c.wants("the propose phase needs", {NAMED(lo), NAMED(hi), NAMED(scale), NAMED(gamma), NAMED(rows), NAMED(columns)});
        const long long after = c.ok() ? demcz_archive_after(call) : 0;
        if (c.ok() && after < 2)
            c.refuse(SMART_E_SIZE, "the propose phase draws two rows of the archive: its size is %lld, need at least 2", after);
        if (c.ok() && after > capacity)
            c.refuse(SMART_E_SIZE, "archive size %lld is more than the capacity %lld", after, (long long)capacity);
        c.in_range("jump_threshold", jump_threshold, 0, kTwo32);
        c.in_range("cr_threshold", cr_threshold, 0, kTwo32);
        c.box_holds(n_dims, (long long)ld, columns, lo, hi);
    }
    if (int rc = c.ready())
        return rc;
    launch_demcz(call, (hipStream_t)stream);
    return launched();
}

// (the step of the NSGA-II sampler, smart_nsga2.hip: the sizes the entry shares with its workspace query)
static void nsga2_sizes(Check &c, int64_t n_rows, int32_t n_objectives)
{
    c.in_range("n_rows", n_rows, 4, SMART_NSGA2_MAX_ROWS);
    c.in_range("n_objectives", n_objectives, 2, SMART_NSGA2_MAX_OBJECTIVES);
}

int smart_nsga2_step_hip(int64_t n_rows, int32_t n_dims, int32_t n_objectives, int32_t n_carry, uint64_t seed,
                         int64_t generation, int32_t parents, const double *pop_x, const double *pop_keys,
                         const double *pop_carry, const uint8_t *pop_part, double *next_x, double *next_keys,
                         double *next_carry, uint8_t *next_part, int32_t *rank, double *crowding, int32_t *origin,
                         int32_t *counts, double *offspring, uint8_t *out, const double *scores, int64_t ld_scores,
                         const int32_t *score_columns, const int32_t *direction, const double *target,
                         const uint8_t *eligible, const double *carry_new, void *workspace, int64_t workspace_bytes,
                         int32_t vary, const double *lo, const double *hi, const double *scale, double f,
                         int64_t cr_threshold, double *rows, int64_t ld, const int32_t *columns, void *stream)
{
    Check c("smart_nsga2_step_hip");
    c.required({NAMED(offspring), NAMED(out)});
    // (nsga2_sizes states the rules of n_rows and n_objectives for the workspace query; here n_dims is asked between the two,
    // and the order of refusals is ABI, so the entry states the three in its own order)
    c.in_range("n_rows", n_rows, 4, SMART_NSGA2_MAX_ROWS);
    c.in_range("n_dims", n_dims, 1, SMART_NSGA2_MAX_DIMS);
    c.in_range("n_objectives", n_objectives, 2, SMART_NSGA2_MAX_OBJECTIVES);
    c.in_range("n_carry", n_carry, 0, SMART_NSGA2_MAX_CARRY);
    c.in_range("generation", generation, 1, kTwo32 - 1);
    if (!scores && !vary)
        c.refuse(SMART_E_NULL, "neither phase is asked for (scores is NULL and vary is 0)");
    if (scores) { // ---- the survive phase
        c.wants("the survive phase needs", {NAMED(next_x), NAMED(next_keys), NAMED(next_part), NAMED(rank), NAMED(crowding),
                                            NAMED(origin), NAMED(counts), NAMED(score_columns), NAMED(direction)});
        if (parents)
            c.wants("parents need", {NAMED(pop_x), NAMED(pop_keys), NAMED(pop_part)});
        c.needs("n_carry", n_carry, {NAMED(next_carry), NAMED(carry_new)});
        if (parents)
            c.needs("parents with n_carry", n_carry, {NAMED(pop_carry)});
        c.in_range("ld_scores", ld_scores, 1, kInt32Max);
        c.objectives_hold(n_objectives, "score column", score_columns, "ld_scores", (long long)ld_scores, direction, target);
        if (c.ok())
            c.workspace_fits(/*for_objfn=*/false, workspace, workspace_bytes, nsga2_workspace_bytes((long)n_rows));
    }
    if (vary) { // ---- the vary phase
        c.wants("the vary phase needs", {NAMED(lo), NAMED(hi), NAMED(scale), NAMED(rows), NAMED(columns)});
        if (!scores && !parents)
            c.refuse(SMART_E_NULL, "the vary phase needs a population: the survive phase, or parents (scores is NULL)");
        if (!scores && !pop_x)
            c.refuse(SMART_E_NULL, "the vary phase without the survive phase reads pop_x (pop_x is NULL)");
        if (!std::isfinite(f))
            c.refuse(SMART_E_SIZE, "f %g must be finite", f);
        c.in_range("cr_threshold", cr_threshold, 0, kTwo32);
        c.box_holds(n_dims, (long long)ld, columns, lo, hi);
    }
    if (int rc = c.ready())
        return rc;
    Nsga2Call call{};
    call.n_rows = (long)n_rows, call.n_dims = n_dims, call.n_objectives = n_objectives, call.n_carry = n_carry;
    call.seed = seed, call.generation = (long)generation, call.parents = parents != 0;
    call.pop_x = pop_x, call.pop_keys = pop_keys, call.pop_carry = pop_carry, call.pop_part = pop_part;
    call.next_x = next_x, call.next_keys = next_keys, call.next_carry = next_carry, call.next_part = next_part;
    call.rank = rank, call.crowding = crowding, call.origin = origin, call.counts = counts;
    call.offspring = offspring, call.out = out, call.scores = scores, call.ld_scores = (long)ld_scores;
    call.score_columns = score_columns, call.direction = direction, call.target = target, call.eligible = eligible;
    call.carry_new = carry_new, call.workspace = workspace, call.vary = vary != 0;
    call.lo = lo, call.hi = hi, call.scale = scale, call.f = f, call.cr_threshold = (long)cr_threshold;
    call.rows = rows, call.ld = (long)ld, call.columns = columns;
    if (int rc = launch_nsga2(call, (hipStream_t)stream))
        return rc;
    return launched();
}

int64_t smart_nsga2_workspace_bytes(int64_t n_rows, int32_t n_objectives)
{
    Check c(nullptr);
    nsga2_sizes(c, n_rows, n_objectives);
    return c.ok() ? nsga2_workspace_bytes((long)n_rows) : c.rc;
}

// (the step of the particle filter, smart_particle.hip: the size the entry shares with its workspace query)
static void particle_sizes(Check &c, int64_t n_particles)
{
    c.in_range("n_particles", n_particles, 1, SMART_PARTICLE_MAX_PARTICLES);
}

int smart_particle_step_hip(int64_t n_particles, int32_t n_dims, uint64_t seed, int64_t step, int32_t phases,
                            int64_t n_reports, const double *sim, int64_t ld_sim, const double *obs, double sigma0,
                            double sigma1, double tau, const int64_t *q_in, int64_t offset, const double *rows_in,
                            double *rows_out, int64_t ld, const int32_t *columns, int32_t z_column, double area_m2,
                            const double *lo, const double *hi, const double *scale, const double *noise,
                            const double *states_in, double *states_out, const double *logw_in, double *logw_out,
                            int64_t *q, int32_t *parents, double *stats, int64_t *counts, void *workspace,
                            int64_t workspace_bytes, void *stream)
{
    Check c("smart_particle_step_hip");
    c.required({NAMED(logw_in), NAMED(logw_out), NAMED(q), NAMED(parents), NAMED(stats), NAMED(counts), NAMED(workspace)});
    particle_sizes(c, n_particles);
    c.in_range("n_dims", n_dims, 1, SMART_PARTICLE_MAX_DIMS);
    c.in_range("step", step, 0, kTwo32 - 1);
    if (phases < 1 || phases > (SMART_PARTICLE_WEIGH | SMART_PARTICLE_RESAMPLE | SMART_PARTICLE_MOVE))
        c.refuse(SMART_E_MODE, "phases '%d' unknown.", (int)phases);
    if (phases & SMART_PARTICLE_WEIGH) { // ---- the weigh phase
        if (!(tau >= 0.0 && std::isfinite(tau)))
            c.refuse(SMART_E_SIZE, "tau %g must be finite and >= 0", tau);
        if (offset >= (1ll << 41))
            c.refuse(SMART_E_SIZE, "offset %lld must be below 2^41 (negative: drawn)", (long long)offset);
        if (!q_in) {
            c.wants("the weigh phase without q_in needs", {NAMED(sim), NAMED(obs)});
            c.in_range("n_reports", n_reports, 1, kInt32Max);
            c.ld_holds("ld_sim", ld_sim, n_particles);
            if (!(sigma0 > 0.0 && std::isfinite(sigma0)))
                c.refuse(SMART_E_SIZE, "sigma0 %g must be finite and > 0", sigma0);
            if (!(sigma1 >= 0.0 && std::isfinite(sigma1)))
                c.refuse(SMART_E_SIZE, "sigma1 %g must be finite and >= 0", sigma1);
        }
    }
    if (phases & SMART_PARTICLE_MOVE) { // ---- the move phase
        c.wants("the move phase needs", {NAMED(rows_in), NAMED(rows_out), NAMED(states_in), NAMED(states_out), NAMED(lo),
                                         NAMED(hi), NAMED(scale), NAMED(noise), NAMED(columns)});
        c.box_holds(n_dims, (long long)ld, columns, lo, hi);
        c.in_range("z_column", z_column, 0, (long long)ld - 1);
        for (int j = 0; c.ok() && j < n_dims; ++j)
            if (!(scale[j] >= 0.0 && std::isfinite(scale[j])))
                c.refuse(SMART_E_SIZE, "scale[%d] %g must be finite and >= 0", j, scale[j]);
        for (int k = 0; c.ok() && k < SMART_PARTICLE_STATES; ++k)
            if (!(noise[k] >= 0.0 && noise[k] < 1.0))
                c.refuse(SMART_E_SIZE, "noise[%d] %g must be in [0, 1)", k, noise[k]);
        if (!(area_m2 > 0.0 && std::isfinite(area_m2)))
            c.refuse(SMART_E_SIZE, "area_m2 %g must be finite and > 0", area_m2);
    }
    if (c.ok())
        c.workspace_fits(/*for_objfn=*/false, workspace, workspace_bytes, particle_workspace_bytes((long)n_particles));
    if (int rc = c.ready())
        return rc;
    ParticleCall call{};
    call.n_particles = (long)n_particles, call.n_dims = n_dims, call.seed = seed, call.step = (long)step, call.phases = phases;
    call.n_reports = (long)n_reports, call.sim = sim, call.ld_sim = (long)ld_sim, call.obs = obs;
    call.sigma0 = sigma0, call.sigma1 = sigma1, call.tau = tau, call.q_in = q_in, call.offset = (long long)offset;
    call.rows_in = rows_in, call.rows_out = rows_out, call.ld = (long)ld, call.columns = columns, call.z_column = z_column;
    call.area_m2 = area_m2, call.lo = lo, call.hi = hi, call.scale = scale, call.noise = noise;
    call.states_in = states_in, call.states_out = states_out, call.logw_in = logw_in, call.logw_out = logw_out;
    call.q = q, call.parents = parents, call.stats = stats, call.counts = counts, call.workspace = workspace;
    if (int rc = launch_particle(call, (hipStream_t)stream))
        return rc;
    return launched();
}

int64_t smart_particle_workspace_bytes(int64_t n_particles)
{
    Check c(nullptr);
    particle_sizes(c, n_particles);
    return c.ok() ? particle_workspace_bytes((long)n_particles) : c.rc;
}

// ---- the residual error model (smart_error_model.hip): the rules the two entries share, in the entries' order
static void error_model_sizes(Check &c, std::initializer_list<Count> counts, int64_t n_samples, int64_t ld, int64_t err_ld)
{
    c.at_least_one(counts);
    c.ld_holds("ld", ld, n_samples);
    if (err_ld < 3)
        c.refuse(SMART_E_SIZE, "err_ld %lld is less than the 3 parameters of a row", (long long)err_ld);
}

int smart_error_model_loglik_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                                 const double *err, int64_t err_ld, double *loglik, void *stream)
{
    Check c("smart_error_model_loglik_hip");
    c.required({NAMED(sim), NAMED(obs), NAMED(err), NAMED(loglik)});
    error_model_sizes(c, {COUNT(n_samples), COUNT(n_reports)}, n_samples, ld, err_ld);
    c.one_launch("n_samples", n_samples);
    c.one_launch("n_reports", n_reports);
    if (int rc = c.ready())
        return rc;
    launch_error_model_loglik((long)n_samples, (long)n_reports, sim, (long)ld, obs, err, (long)err_ld, loglik,
                              (hipStream_t)stream);
    return launched();
}

int smart_error_model_draw_hip(int64_t n_samples, int64_t n_reports, int64_t n_replicates, const double *sim, int64_t ld,
                               const double *err, int64_t err_ld, uint64_t seed, int64_t column_offset, int32_t truncate,
                               double *out, int64_t out_ld, void *stream)
{
    Check c("smart_error_model_draw_hip");
    c.required({NAMED(sim), NAMED(err), NAMED(out)});
    error_model_sizes(c, {COUNT(n_samples), COUNT(n_reports), COUNT(n_replicates)}, n_samples, ld, err_ld);
    // the columns of the call: more than 2^32 of them are refused whatever their count is (it is not formed then)
    const bool countable = c.ok() && n_samples <= kTwo32 / n_replicates;
    const long long columns = countable ? (long long)n_samples * (long long)n_replicates : kTwo32 + 1;
    if (c.ok() && countable && out_ld < columns)
        c.refuse(SMART_E_SIZE, "out_ld %lld is less than the n_samples * n_replicates = %lld columns", (long long)out_ld,
                 columns);
    c.in_range("column_offset", column_offset, 0, kTwo32 - 1);
    if (c.ok() && columns > kTwo32 - column_offset)
        c.refuse(SMART_E_SIZE, "columns %lld ..: a column's number stays below 2^32 (%lld samples, %lld replicates)",
                 (long long)column_offset, (long long)n_samples, (long long)n_replicates);
    c.one_launch("n_reports", n_reports);
    if (int rc = c.ready())
        return rc;
    launch_error_model_draw((long)n_samples, (long)n_reports, (long)n_replicates, sim, (long)ld, err, (long)err_ld, seed,
                            (long)column_offset, truncate != 0, out, (long)out_ld, (hipStream_t)stream);
    return launched();
}

} // extern "C"

