/*
 * smart_amd.h -- C ABI of the MI355X-native SMART ensemble engine (libsmart_amd.so).
 *
 * This is the drop-in boundary for the hot path of ThibHlln/smartpy v0.2.2: the time loop
 * structure.run -> run_all_steps -> run_one_step (smartpy/structure.py:30-503).  The reference already
 * has a plug-in hook for exactly this path -- an optional extension module named `smartcpp`, looked up
 * at import time (structure.py:22-27) and used as smartcpp.allsteps (structure.py:56-62) or
 * smartcpp.onestep (structure.py:171-174).  Every entry point below states which reference interface
 * it stands in for.  INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; no torch / numpy types cross this boundary;
 *   - "device pointer" = memory the GPU can address (hipMalloc, or a torch.Tensor's data_ptr());
 *   - every function returns 0 on success or a negative SMART_E_* code, never throws; the text of the
 *     last error of the calling thread is available from smart_last_error();
 *   - buffers are owned by the caller, are not retained after the call returns and inputs are never
 *     written; launches are asynchronous on the given stream unless stated otherwise;
 *   - no global mutable state besides the per-thread error text: calls on different streams may run
 *     concurrently.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails with
 *     SMART_E_NO_DEVICE.
 *
 * Vector layouts (all IEEE fp64)
 *   parameters  p[10]  = T, C, H, D, S, Z, SK, FK, GK, RK                       (parameters.py:25)
 *   variables   v[19]  = Q_aeva, Q_ove, Q_dra, Q_int, Q_sgw, Q_dgw, Q_out,
 *                        V_ove, V_dra, V_int, V_sgw, V_dgw, V_ly1..V_ly6, V_river (structure.py:78-82)
 *   extra       x[7]   = aar, r-o_ratio, r-o_split[5]                          (structure.py:100-112)
 *   objectives  o[8]   = NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE, GW           (montecarlo.py:71-74)
 */
#ifndef SMART_AMD_H
#define SMART_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMART_AMD_ABI_VERSION 7

/* report_type, as structure.py:65-70 maps report='summary' / 'raw' */
#define SMART_REPORT_SUMMARY 1
#define SMART_REPORT_RAW 2

/* math_mode */
#define SMART_MATH_LITERAL 0 /* the reference's operation order, IEEE division, no FMA contraction:     */
                             /* bit-identical to the CPU oracle configured with the product chain for   */
                             /* s'**i (the only place where CPython calls libm)                         */
#define SMART_MATH_FAST 1    /* reciprocals hoisted out of the time loop, soil layers kept in mm,       */
                             /* reservoirs kept as outflows, FMA: <= 1e-9 relative on discharge;        */
                             /* wavefronts holding a sample with delta_sec / (k * 3600) > 2 (where the  */
                             /* reference's explicit update amplifies rounding differences) run the     */
                             /* literal arithmetic instead, and so do rows with a NaN or an infinite    */
                             /* parameter or one that is none (D or H outside [0, 1], a k <= 0,         */
                             /* T < 0.2, Z outside [1 mm, 1 m]: smart_fast_model.h wave_class).         */
                             /* The FORCING must be finite in this mode: what the                       */
                             /* reference's branches make of a NaN in it (structure.py:359, :409-419)   */
                             /* only SMART_MATH_LITERAL reproduces -- a fast launch that meets one      */
                             /* raises SMART_STATUS_NONFINITE_FORCING                                   */

/* error codes; the reference raises Exception at the cited places */
#define SMART_OK 0
#define SMART_E_NULL (-1)        /* a required pointer is NULL                                          */
#define SMART_E_SIZE (-2)        /* a size is <= 0 or inconsistent                                      */
#define SMART_E_REPORT_TYPE (-3) /* unknown report type                          (structure.py:69-70)   */
#define SMART_E_WARMUP (-4)      /* warm-up longer than the simulation           (structure.py:90-95)   */
#define SMART_E_GAP (-5)         /* summary report: length (or warm-up) is not a multiple of the gap    */
                                 /* -- np.reshape raises                         (structure.py:190)     */
#define SMART_E_NO_DEVICE (-6)   /* no HIP device / HIP runtime error (text in smart_last_error)        */
#define SMART_E_MODE (-7)        /* unknown math mode                                                   */
#define SMART_E_IO (-8)          /* a database file could not be opened / written                       */

/* plan bits (smart_plan_ensemble, SmartEnsemble.plan): what the rows and the forcing of a call need.  The fast mode
 * is a family of kernels, one per arithmetic class of a block of 64 parameter rows and per kind of forcing; a plan
 * lets a launch skip the kernels that would find nothing to do. */
#define SMART_PLAN_CLASS_REGULAR 0x01    /* rows with every k*3600 >= delta_sec, 0 <= S <= 0.5, C >= 0, Z > 0    */
#define SMART_PLAN_CLASS_STIFF 0x02      /* some k*3600 < delta_sec: clamps (structure.py:429-450) and the river's */
                                         /* 95 % rule (:492-496) are reachable                                     */
#define SMART_PLAN_CLASS_GUARD 0x04      /* S, C or Z outside those ranges: the leak guards (:383,390,397) matter  */
#define SMART_PLAN_CLASS_ILLCOND 0x08    /* delta_sec / (RK*3600) > 2 (the river), or a parameter that is none     */
                                         /* (SMART_MATH_FAST above): run in the literal arithmetic                 */
#define SMART_PLAN_FORCING_PIECEWISE 0x10 /* a catchment whose forcing is constant within every report interval    */
#define SMART_PLAN_FORCING_VARYING 0x20   /* a catchment whose forcing varies from step to step                    */
#define SMART_PLAN_FORCING_RUNS 0x80      /* a catchment whose forcing is constant over runs of k steps, k >= 2 a  */
                                          /* divisor of the report gap smaller than it (6-hourly data in an hourly  */
                                          /* run with daily reports, timeframe.py:167-186): interval engine per run */
#define SMART_PLAN_ROWS_ORDERED 0x40       /* set by the caller (not by smart_plan_ensemble): neighbouring rows behave    */
                                           /* alike -- ordered by T, then by S*Z, as smartpy_amd/engine.py does when no   */
                                           /* discharge matrix is stored.  Wave-uniform early exits then pay off sooner.  */
#define SMART_PLAN_VALID 0x100
/* ABI 7: bits 12..30 of a plan from smart_plan_ensemble hold the NUMBER of blocks of 64 rows that take the literal      */
/* arithmetic (SMART_PLAN_CLASS_ILLCOND), saturating; 0 in a plan put together by hand = not counted (the launch then    */
/* reckons with every block of the call).  The launch picks the form of that kernel from it: see literal_form.           */
#define SMART_PLAN_ILLCOND_BLOCKS_SHIFT 12
#define SMART_PLAN_ILLCOND_BLOCKS_MAX 0x7ffff

/* literal_form (ABI 7): how the rows of SMART_PLAN_CLASS_ILLCOND are laid over the wavefronts.  The same arithmetic,   */
/* the same bits either way (structure.py:267-503 in the reference's operation order).                                  */
#define SMART_LITERAL_FORM_AUTO 0  /* from the load: rows while the wavefronts of the call -- 16 per class-3 block, one    */
                                   /* per other block -- fit into two rounds over the chip's SIMDs, lanes beyond         */
#define SMART_LITERAL_FORM_ROWS 1  /* one sample per DPP row of 16 lanes, four per wavefront: a third of the             */
                                   /* instructions per step -- the latency form (few rows: config 2, the smartcpp hook)  */
#define SMART_LITERAL_FORM_LANES 2 /* one sample per lane, 64 per wavefront -- the throughput form (large daily          */
                                   /* ensembles: a seventh of the SIMD cycles per sample-step)                           */

/* status bits of a finished launch (smart_launch_status) */
#define SMART_STATUS_SLICE_TIMEOUT 0x1 /* a time slice gave up waiting for its predecessor: the block's outputs are */
                                       /* NaN from that slice on; repeat the launch with time_slices = 1            */
#define SMART_STATUS_STALE_PLAN 0x2    /* the plan did not cover a class / kind of forcing met on the device: those  */
                                       /* rows were NOT computed; repeat the launch with plan = 0                    */
#define SMART_STATUS_NONFINITE_FORCING 0x4 /* SMART_MATH_FAST met a NaN or an infinity in the forcing: its outputs are */
                                       /* not the reference's; repeat the launch with math_mode = SMART_MATH_LITERAL  */

/*
 * One ensemble launch = the whole per-sample loop that spotpy's sampler drives
 * (montecarlo.py:153-154 -> :179-186 -> smart.py:204-207 -> structure.py:30-146), for n_samples
 * parameter sets on each of n_catchments catchments.  One wavefront lane advances one sample; the time
 * loop (warm-up then simulation) runs inside the kernel with parameters and the 12 states in registers.
 *
 * All pointers are device pointers.
 */
typedef struct SmartEnsemble {
    /* ---- sizes -------------------------------------------------------------------------------- */
    int64_t n_catchments; /* C >= 1                                                                 */
    int64_t n_samples;    /* N >= 1 parameter sets per catchment                                    */
    int64_t n_steps;      /* T = len(timeseries) - 1                          (structure.py:73)      */
    int64_t n_warm;       /* W = int(warm_up_days * 86400 / delta_sec), 0 = none (structure.py:87-88); */
                          /* the warm-up replays forcing[0 .. W)              (structure.py:118-121) */
    int64_t report_gap;   /* g = T // R                                       (structure.py:75)      */
    int32_t report_type;  /* SMART_REPORT_*                                                          */
    int32_t math_mode;    /* SMART_MATH_*                                                            */
    double delta_sec;     /* simulation time step in seconds                  (structure.py:74)      */

    /* ---- inputs ------------------------------------------------------------------------------- */
    const double *area_m2; /* [C]                                                                    */
    const double *forcing; /* [C][T][2]: rain, peva in mm per step, interleaved (smart.py:141-142)   */
    const double *params;  /* [N][10] row-major, exactly the matrix lhs.py:114 produces; or [C][N][10] */
    int64_t params_catchment_stride; /* 0: every catchment runs the same N rows; else N*10          */
    const double *extra;   /* [C][7] educated guess of the initial reservoirs, or NULL: start empty   */
                           /*                                                 (structure.py:97-140)  */
    const double *initial; /* [C][N][12] states to start from instead (chained runs), or NULL;        */
                           /* used as the warm-up's start when n_warm != 0                           */
    const double *obs;     /* [C][R] observed discharge, NaN = missing (smart.py:143), or NULL        */
    const double *gw_obs;  /* [C] groundwater constraint (inout.py:134-139), NaN = none, or NULL      */

    /* ---- outputs (each nullable except gw) ----------------------------------------------------- */
    double *discharge;     /* [C][R][discharge_ld] sample-minor, so that a wavefront stores 512       */
                           /* contiguous bytes per report step; element (c, r, n) = what              */
                           /* SMART.simulate(row n)[0][r] returns                   (smart.py:208)   */
    int64_t discharge_ld;  /* >= N                                                                   */
    double *gw;            /* [C][N] groundwater contribution to runoff (structure.py:191,194-195)   */
    double *objfn;         /* [C][N][8] objective functions (montecarlo.py:193-209); needs obs;       */
                           /* column 7 (GW) is NaN where gw_obs is absent                            */
    double *final_vars;    /* [C][N][19] last row of the storage table        (structure.py:197)     */
    void *workspace;       /* device scratch of workspace_bytes bytes: observation statistics when    */
                           /* objfn != NULL ([C][8 + R] doubles, required), and the hand-over buffer   */
                           /* of a time-sliced launch (optional: without room for it the launch is     */
                           /* not sliced), and the code words of the step loop's pair blocks (optional:  */
                           /* without them it dispatches step by step).  smart_workspace_bytes() tells   */
                           /* how much all of them need.                                               */
    int64_t workspace_bytes;

    void *stream;          /* hipStream_t; NULL = the default stream                                 */

    /* ---- launch control (ABI 3; zero = the library decides) ------------------------------------- */
    int32_t time_slices;   /* 0: the library's choice (slices the time axis of launches with more blocks  */
                           /* of 64 samples than SIMDs); 1: never slice; n > 1: n slices                   */
    int32_t plan;          /* SMART_PLAN_* bits from smart_plan_ensemble for these params / forcing /      */
                           /* sizes, or 0: launch every kernel the call could need                         */
    /* ---- ABI 7 ---------------------------------------------------------------------------------- */
    int32_t literal_form;  /* SMART_LITERAL_FORM_*: 0 = chosen from the number of class-3 blocks in the plan */
    int32_t reserved0;     /* must be 0                                                                    */
} SmartEnsemble;

/* Number of report steps R for a run (structure.py:190 / :193): T // g (summary), ceil(T / g) (raw). */
int64_t smart_n_reports(int64_t n_steps, int64_t report_gap, int32_t report_type);

/* Validate and launch.  Asynchronous on e->stream.  Stands in for the spotpy repetition loop over
 * MonteCarlo.simulation + MonteCarlo.objectivefunction (montecarlo.py:179-209). */
int smart_run_ensemble_hip(const SmartEnsemble *e);

/* Validation only (no device needed): the checks smart_run_ensemble_hip performs before launching. */
int smart_check_ensemble(const SmartEnsemble *e);

/* Bytes of device scratch the call wants in e->workspace for these sizes and outputs (pointers are not read):
 * a header (status word, counters, per-catchment forcing flags), the observation statistics if e->objfn is set,
 * plus -- on a machine with a HIP device -- the hand-over buffer of the time-sliced launch the library would
 * choose, plus, for fast summary / raw runs over whole report intervals, 8 bytes per four time steps and catchment
 * (the kinds of the steps, worked out once per launch; 68 bytes per two steps where the gap is no multiple of four).
 * The library allocates nothing itself: the caller owns every buffer, which also lets the call be captured into a HIP
 * graph.  A launch without a workspace runs unsliced and reports no status. */
int64_t smart_workspace_bytes(const SmartEnsemble *e);

/* Classify the parameter rows and the forcing of a SMART_MATH_FAST call on the device (two small kernels on
 * e->stream, then SYNCHRONOUS: the answer is copied back): *plan = SMART_PLAN_VALID | the SMART_PLAN_* bits present.
 * Valid for as long as params, forcing, delta_sec, report_gap and the sizes do not change.  Needs e->workspace. */
int smart_plan_ensemble(const SmartEnsemble *e, int32_t *plan);

/* Status word of the last launch that used e->workspace (SMART_STATUS_* bits, 0 = clean).  SYNCHRONOUS: waits for
 * e->stream.  0 without a workspace. */
int smart_launch_status(const SmartEnsemble *e, int32_t *status);

/* Which kernels smart_run_ensemble_hip would launch for *e on the current device, as text for logs and benchmark
 * lines: e.g. "smart_fast_intervals[16 slices x 1563 blocks, 2 resident per SIMD]"; the literal rows of a fast call
 * with the form chosen for them: "smart_fast_illcond_lanes[1813 of 15625 blocks, one sample per lane]" (ABI 7).
 * Launches nothing. */
int smart_describe_launch(const SmartEnsemble *e, char *text, int64_t len);

/*
 * smartcpp.allsteps -- same arguments and results as run_all_steps (structure.py:149-152,197).
 * HOST pointers; synchronous (copies in, runs one sample on the GPU, copies out).
 *   nd_rain / nd_peva hold at least length_simu values (the warm-up call passes the full series with a
 *   shorter length, structure.py:118-121); nd_parameters[10]; nd_initial[19];
 *   discharge[smart_n_reports(length_simu, report_gap, report_type)]; *groundwater_component;
 *   final_vars[19].
 * Arithmetic: SMART_MATH_LITERAL (the reference's operation order; bit-identical to the ensemble's literal mode) unless
 * the environment says SMART_ALLSTEPS_MATH=fast (the fast kernels for the one sample: <= 1e-9 relative, a tenth of the
 * time).  The library keeps its device buffers and the uploaded series between calls (ABI v5): the reference calls this
 * twice per SMART.simulate() with the same series (structure.py:118-121,143-146), a calibration loop thousands of
 * times -- a call whose series starts with what is on the device uploads only what lies beyond it.  One caller at a
 * time (serialised inside).
 */
int smart_allsteps_hip(double area_m2, double delta_sec, int64_t length_simu, const double *nd_rain,
                       const double *nd_peva, const double *nd_parameters, const double *nd_initial,
                       int32_t report_type, int64_t report_gap, double *discharge,
                       double *groundwater_component, double *final_vars);

/* Counters of the smartcpp.allsteps stand-in, for tests and logs: counters[0..n) of { calls, device allocations made,
 * bytes of forcing uploaded, calls served in fast arithmetic, planning passes made for them (ABI 6: one per series,
 * length and report, not one per call) } since the library was loaded (n <= 5). */
int smart_hook_counters(int64_t *counters, int64_t n);

/*
 * smartcpp.onestep -- run_one_step (structure.py:200-264): 2 constants, 2 forcings, 10 parameters and
 * 12 states in, the 19-vector out.  HOST pointers; synchronous; n independent steps per call
 * (n = 1 reproduces the reference's call at structure.py:182-187).
 *   in[n][26]  = area, dt, rain, peva, T..RK, V_ove..V_river ;  out[n][19]
 */
int smart_onestep_hip(int64_t n, const double *in, double *out);

/*
 * run_one_step_river (structure.py:461-503) on its own: the river reservoir with its 95 % rule.  HOST pointers;
 * synchronous; n independent steps.  in[n][4] = time_gap_sec, r_in_q_riv, r_p_rk [hours], r_s_v_riv ;
 * out[n][2] = r_out_q_riv, r_s_v_riv.  (run_one_step_catchment, :267-458, is the first six outputs and the eleven
 * catchment states of smart_onestep_hip: the river does not feed back.)
 */
int smart_river_step_hip(int64_t n, const double *in, double *out);

/*
 * Objective functions of an existing discharge matrix (montecarlo.py:193-209 applied to every sample);
 * the matrix is read once (moments about the observation mean).  Device pointers; asynchronous on stream.
 *   sim[R][ld] sample-minor (the layout smart_run_ensemble_hip writes), obs[R] (NaN = missing),
 *   gw_sim[N] and gw_obs: pass NULL / NaN to skip the GW column; objfn[N][8].
 */
int smart_objfn_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                    const double *gw_sim, double gw_obs, double *objfn, void *stream);

/*
 * Weighted quantiles of an existing discharge matrix along the SAMPLE axis, per report step: the GLUE prediction
 * bounds (likelihood-weighted 5 / 50 / 95 % of the behavioural ensemble).  For one report step with values x_n and
 * weights w_n >= 0 (n < n_samples), W = sum of w_n, and a probability 0 < q <= 1:
 *     Q(q) = the smallest value v among the x_n with   sum of w_n over { n : x_n <= v }  >=  q * W.
 * No interpolation: numpy.quantile(..., method='inverted_cdf', weights=w); with equal weights the plain inverted CDF.
 * Ties need no tie-break (the sum runs over x_n <= v); a sample with w_n == 0 never decides a result; a NaN value sorts
 * above +inf, as in numpy.sort, and a quantile that reaches it is NaN; W == 0 gives NaN for every quantile of the step;
 * -0.0 and +0.0 are the same value.  The weights MUST be finite and >= 0: a precondition, not checked on the device.
 *   sim[R][ld] sample-minor (the layout smart_run_ensemble_hip writes), weights[N] or NULL = equal weights: device
 *   pointers; probs[n_probs]: HOST pointer, read before the call returns, each in (0, 1],
 *   n_probs <= SMART_QUANTILES_MAX_PROBS; out[n_probs][R]: device.  Asynchronous on stream; allocates nothing.
 * One workgroup per report step, in one of two forms (smartpy_amd/csrc/smart_quantiles.hip) that answer alike:
 *   SMART_QUANTILES_SORT    the step's values sorted in LDS, the weights scanned in that order, a binary search per
 *                           probability; n_samples <= smart_quantiles_sort_capacity(), else SMART_E_SIZE
 *   SMART_QUANTILES_SELECT  any n_samples: no sort, the probabilities bisect the 64-bit key space together
 *   SMART_QUANTILES_AUTO    sort within its capacity, select beyond
 * Deterministic: no floating-point atomics, every sum has one association for a given (n_samples, form), so two
 * launches give the same bits.  The two forms add in different orders: they agree exactly where the partial sums of the
 * weights are exact, and to the rounding of those sums otherwise.
 * Errors (all found before the device is touched): SMART_E_NULL sim, probs or out missing; SMART_E_SIZE a size < 1,
 * ld < n_samples, n_reports >= 2^31, a probability outside (0, 1] or NaN, too many probabilities, the sort form beyond
 * its capacity; SMART_E_MODE unknown method; then SMART_E_NO_DEVICE without a HIP device.
 */
#define SMART_QUANTILES_AUTO 0
#define SMART_QUANTILES_SORT 1
#define SMART_QUANTILES_SELECT 2
#define SMART_QUANTILES_MAX_PROBS 16
int smart_weighted_quantiles_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld,
                                 const double *weights, const double *probs, int32_t n_probs, double *out,
                                 int32_t method, void *stream);

/* The largest n_samples SMART_QUANTILES_SORT takes: what the LDS of a gfx950 compute unit (160 KiB, all of it open to
 * one workgroup) holds at 18 bytes per sorted element, rounded down to a power of two -- 8192.  Needs no device. */
int64_t smart_quantiles_sort_capacity(void);

/*
 * Objective functions of an existing discharge matrix PER WINDOW of report steps and on TRANSFORMED flows: split-sample
 * scores (per hydrological year, season, calibration / evaluation period) and low-flow scores, for every sample.
 *   sim[R][ld] sample-minor (the layout smart_run_ensemble_hip writes), obs[R] (NaN = missing), window[R] int32 with
 *   -1 = the report step belongs to no window, else 0 .. n_windows-1 (any other value is a broken PRECONDITION, not
 *   checked on the device), objfn[n_windows][N][SMART_OBJFN_WINDOW_COLS]: device pointers.  Asynchronous on stream;
 *   allocates nothing.
 * For window w and sample n let rows = { r : window[r] == w and obs[r] is not NaN }, e = f(obs[rows]) and
 * s = f(sim[rows, n]) with f the transform; the seven values NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE are the formulas
 * of montecarlo.py:193-209 (smart_objfn_hip's) applied to (s, e).  GW does not depend on a window and has no column.
 * Two rules of this entry's own:
 *   - fewer than two rows in a window: NaN in all seven columns, for every sample of that window;
 *   - a transformed value that is not finite (a negative flow under sqrt or ln, x + eps == 0, a NaN or an infinity in
 *     the matrix): NaN in all seven columns of that (window, sample); a non-finite f(obs[r]) does it for every sample of
 *     the window.  (numpy answers with a mixture of NaN and +-inf there.)  A sum of finite transformed values that
 *     overflows counts as not finite.
 * Rows of no window are not read, and every element of a row that belongs to a window is loaded once.  Deterministic: no
 * floating-point atomics, every sum has one association for a given (n_samples, n_reports, window array), so two
 * launches give the same bits.  n_windows <= smart_objfn_max_windows(): every window walks window[] once more.
 * Errors (all found before the device is touched): SMART_E_NULL sim, obs, window or objfn missing; SMART_E_SIZE a size
 * < 1, ld < n_samples, n_reports >= 2^31, n_windows > smart_objfn_max_windows(), eps negative or not finite;
 * SMART_E_MODE unknown transform; then SMART_E_NO_DEVICE without a HIP device.
 */
#define SMART_TRANSFORM_NONE 0     /* f(x) = x            */
#define SMART_TRANSFORM_SQRT 1     /* f(x) = sqrt(x)      */
#define SMART_TRANSFORM_LOG 2      /* f(x) = ln(x + eps)  */
#define SMART_TRANSFORM_INVERSE 3  /* f(x) = 1 / (x + eps) */
#define SMART_OBJFN_WINDOW_COLS 7  /* NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE -- GW does not depend on a window */
int smart_objfn_windows_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                            const int32_t *window, int32_t n_windows, int32_t transform, double eps,
                            double *objfn, void *stream);

/* The largest n_windows smart_objfn_windows_hip takes in one call (1024).  Needs no device. */
int32_t smart_objfn_max_windows(void);

/*
 * Flow duration curves of an existing discharge matrix: order statistics ALONG TIME, per sample and per window of report
 * steps -- the direction smart_weighted_quantiles_hip (across the samples, per report step) does not take -- and the
 * objective functions of the sorted simulation against the sorted observations, beside smart_objfn_windows_hip.
 *   sim[R][ld] sample-minor (the layout smart_run_ensemble_hip writes), obs[R] or NULL (NaN = missing), window[R] int32
 *   or NULL with the convention of smart_objfn_windows_hip (-1 = no window, else 0 .. n_windows-1; NULL = one window
 *   holding every report step, n_windows must be 1), quant[n_windows][n_probs][N] (sample-minor: the stores coalesce),
 *   objfn[n_windows][N][SMART_OBJFN_WINDOW_COLS] or NULL, workspace: device pointers; probs[n_probs]: HOST pointer, read
 *   before the call returns, each in [0, 1], n_probs <= SMART_QUANTILES_MAX_PROBS.  Asynchronous on stream; allocates
 *   nothing: the workspace is the caller's, smart_flow_duration_workspace_bytes says how much (0 without objfn).
 * For window w and sample n let rows = { r : window[r] == w, and obs[r] is not NaN where obs is given }, m = |rows| and
 * x = sim[rows, n].
 *   Q(q) = the k-th smallest of x, k = max(1, ceil(q * m)) with the product formed in double:
 *   numpy.quantile(x, q, method='inverted_cdf').  No interpolation and no arithmetic on the values: an element of the
 *   column.  A NaN sorts above +inf and counts as a value; -0.0 and +0.0 are the same value; m == 0 gives NaN.
 *   objfn (needs obs): s = f(sort(x)) and e = f(sort(obs[rows])), both ascending and paired by the 0-based rank i, f the
 *   transform (SMART_TRANSFORM_*, eps) applied AFTER the sort; the rank i takes part iff
 *   seg_lo * m <= (double)i < seg_hi * m (0 <= seg_lo < seg_hi <= 1; (0, 1) = the whole curve); the seven values NSE,
 *   KGE, KGEc, KGEa, KGEb, PBias, RMSE are the formulas of montecarlo.py:193-209 on those pairs (one-pass moments about
 *   a shift, as smart_objfn_windows_hip).  The two rules of smart_objfn_windows_hip, on the pairs that take part:
 *   - fewer than two pairs in the segment: NaN in all seven columns, for every sample of that window;
 *   - a transformed value of the segment that is not finite: NaN in all seven columns of that (window, sample); a
 *     non-finite f(obs) of the segment does it for every sample of the window.  (A NaN in a column sorts to the top: it
 *     spoils a segment that reaches the top rank, and no other.)
 * Two forms (smartpy_amd/csrc/smart_flow_duration.hip) that give the same bits:
 *   SMART_FDC_SORT    n_reports <= smart_flow_duration_sort_capacity(): a workgroup sorts the window's rows of 16 .. 1
 *                     adjacent samples in LDS (one bitonic network for all its columns) and reads the order statistics
 *                     and the segment's moments from there; beyond the capacity SMART_E_SIZE
 *   SMART_FDC_SELECT  any n_reports, order statistics only (objfn given: SMART_E_MODE): one lane per sample, the
 *                     probabilities bisect the 64-bit key space together with integer counts
 *   SMART_FDC_AUTO    sort within the capacity, select beyond -- where objfn is refused (SMART_E_SIZE): never a silent
 *                     fallback
 * Deterministic: no floating-point atomics, two launches give the same bits.
 * Errors (all found before the device is touched): SMART_E_NULL sim, probs or quant missing, objfn without obs, objfn
 * without workspace; SMART_E_SIZE a size < 1, ld < n_samples, n_reports >= 2^31, n_windows >
 * smart_objfn_max_windows() or != 1 without a window array, n_probs > 16, a probability outside [0, 1] or not finite,
 * eps negative or not finite, a segment that is not 0 <= seg_lo < seg_hi <= 1, workspace_bytes too small, the sort form
 * or objfn beyond the capacity; SMART_E_MODE unknown transform or method, objfn with SMART_FDC_SELECT; then
 * SMART_E_NO_DEVICE without a HIP device.
 */
#define SMART_FDC_AUTO 0
#define SMART_FDC_SORT 1
#define SMART_FDC_SELECT 2
int smart_flow_duration_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                            const int32_t *window, int32_t n_windows, const double *probs, int32_t n_probs,
                            double *quant, int32_t transform, double eps, double seg_lo, double seg_hi, double *objfn,
                            void *workspace, int64_t workspace_bytes, int32_t method, void *stream);

/* The workspace smart_flow_duration_hip needs, in bytes: with objfn the sorted transformed observations of every window
 * and eight statistics in front of each, (8 + n_reports) * 8 * n_windows rounded up to 256; without objfn 0.  A
 * negative SMART_E_SIZE for sizes < 1.  Needs no device (beside smart_workspace_bytes). */
int64_t smart_flow_duration_workspace_bytes(int64_t n_reports, int32_t n_windows, int32_t with_objfn);

/* The largest n_reports SMART_FDC_SORT takes: 16,384 keys of 8 bytes are the 128 KiB a workgroup keeps in LDS (of the
 * 160 KiB of a gfx950 compute unit), one column of that many rows in the narrowest instance.  Needs no device (beside
 * smart_quantiles_sort_capacity). */
int64_t smart_flow_duration_sort_capacity(void);

/*
 * Hydrological signatures of an existing discharge matrix, per sample and per window of report steps: the scores that
 * depend on the ORDER of the report steps within a window, which no other analysis of the matrix sees.
 *   sim[R][ld] sample-minor (the layout smart_run_ensemble_hip writes), obs[R] or NULL (NaN = missing), window[R] int32
 *   or NULL with the convention of smart_objfn_windows_hip (-1 = no window, else 0 .. n_windows-1; NULL = one window
 *   holding every report step, n_windows must be 1), alpha in (0, 1) the filter parameter, pulse[n_windows][2] doubles
 *   (lo, hi) or NULL, sig[n_windows][SMART_SIGNATURE_COLS][N] (sample-minor: the stores coalesce, and a column of a
 *   window is a contiguous [N] vector): device pointers.  Asynchronous on stream; allocates nothing.
 * For window w and sample n write x_r = sim[r][n].  A row r is VALID iff window[r] == w and, where obs is given, obs[r] is
 * not NaN; m is the number of valid rows.  There is a PAIR at r iff r >= 1 and rows r-1 and r are both valid; p is the
 * number of pairs.  Validity belongs to the row, not to the sample.  Everything is walked in ascending r.
 *   MEAN           sum x_r / m over the valid rows
 *   BFI            sum (x_r - f_r) / sum x_r over the valid rows, f the ONE-PASS Lyne-Hollick quick flow: f_r = 0 at a
 *                  valid row without a pair, else f_r = min(max(alpha f_{r-1} + (1 + alpha) / 2 (x_r - x_{r-1}), 0), x_r);
 *                  NaN if sum x is 0.  One forward pass only: the three-pass form of the filter needs the intermediate
 *                  series of every sample, which is a second matrix
 *   FLASHINESS     Richards-Baker: sum over the pairs |x_r - x_{r-1}| / sum over the pairs x_r; NaN if p is 0 or the
 *                  denominator is 0
 *   AC1            Pearson correlation of (x_{r-1}, x_r) over the pairs; NaN if p < 2 or either variance is <= 0
 *   RLD            rising limb density: a RISING pair has x_r > x_{r-1}; a limb starts at a rising pair at r when there
 *                  is no rising pair at r-1; limbs / rising pairs, NaN if there is no rising pair
 *   RECESSION      the mean of ln(x_r / x_{r-1}) over the pairs with 0 < x_r < x_{r-1}; NaN if there is none
 *   PEAK           the maximum of x over the valid rows
 *   PEAK_ROW       the smallest r attaining it, as a double (the caller turns it into a stamp or a timing error)
 *   HIGH_COUNT     the number of runs above hi: a run starts at a valid row with x_r > hi that has no pair, or whose
 *                  x_{r-1} <= hi
 *   HIGH_DURATION  rows with x_r > hi divided by runs; NaN with no run
 *   LOW_COUNT, LOW_DURATION   the same with x_r < lo
 * Rules: m == 0 gives NaN in all twelve columns; a valid row that holds a value that is not finite gives NaN in all twelve
 * columns of that (window, sample) -- one test of sum x at the end, as smart_objfn_windows_hip: a sum of finite values
 * that overflows counts the same way; pulse NULL, or a NaN threshold, gives NaN in the two columns that threshold feeds; a
 * missing observation or a window boundary breaks a pair, a run and a limb, and restarts the filter; comparisons are
 * strict and made on the matrix values themselves; -0.0 and +0.0 are one value.
 * Rows that are not valid are never read, and every element of a valid row is loaded once.  Deterministic: no atomics, the
 * association of every sum is the row order, two launches give the same bits.
 * Errors (all found before the device is touched): SMART_E_NULL sim or sig missing; SMART_E_SIZE a size < 1, ld <
 * n_samples, n_reports >= 2^31, n_windows > smart_objfn_max_windows() or != 1 without a window array, alpha outside
 * (0, 1) or not finite; then SMART_E_NO_DEVICE without a HIP device.
 */
#define SMART_SIGNATURE_COLS 12
#define SMART_SIG_MEAN 0
#define SMART_SIG_BFI 1
#define SMART_SIG_FLASHINESS 2
#define SMART_SIG_AC1 3
#define SMART_SIG_RLD 4
#define SMART_SIG_RECESSION 5
#define SMART_SIG_PEAK 6
#define SMART_SIG_PEAK_ROW 7
#define SMART_SIG_HIGH_COUNT 8
#define SMART_SIG_HIGH_DURATION 9
#define SMART_SIG_LOW_COUNT 10
#define SMART_SIG_LOW_DURATION 11
int smart_signatures_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                         const int32_t *window, int32_t n_windows, double alpha, const double *pulse,
                         double *sig, void *stream);

/* SMART_SIGNATURE_COLS as the library was built (12).  Needs no device. */
int32_t smart_signature_cols(void);

/*
 * Sobol sensitivity indices of the rows of a matrix whose columns are a Saltelli design in block-major order
 * (smartpy_amd.sampling.saltelli_design): first-order indices after Saltelli 2010, total indices after Jansen, and their
 * standard deviation over bootstrap replicates.
 *   y[n_rows][ld]: row r holds [A ; B ; AB_0 ; ... ; AB_{n_params-1}], each block n_base contiguous doubles -- a report
 *   step of the matrix smart_run_ensemble_hip writes, or one scalar target per row; s1, st [n_rows][n_params]; moments
 *   [n_rows][2] (mu, V); counts [n_base][n_resamples] uint16 (replicate-minor), every replicate's counts summing to
 *   n_base; s1_std, st_std [n_rows][n_params]: device pointers.  Asynchronous on stream; allocates nothing.
 * For one row: mu = the mean of the 2 n_base values of A and B, u = y - mu, V = their population variance,
 *   S1_j = sum_i uB_i (yAB_j,i - yA_i) / (n_base V),    ST_j = sum_i (yA_i - yAB_j,i)^2 / (2 n_base V).
 * Replicate b keeps mu: V_b = sum_i c_bi (uA_i^2 + uB_i^2) / 2n - (sum_i c_bi (uA_i + uB_i) / 2n)^2, and S1_bj, ST_bj are
 * the sums above weighted by c_bi over V_b.  s1_std / st_std are the standard deviations (ddof = 1) over the n_resamples
 * replicates: n_resamples == 0 writes nothing (counts, s1_std, st_std may be NULL), n_resamples == 1 gives NaN.
 * Rules: a value of a row that is not finite makes every output of that row NaN (told from one sum over the row that
 * includes the squared differences: finite values whose squared difference overflows count as not finite); V == 0 gives
 * NaN in S1, ST and the standard deviations; a parameter the values do not depend on (yAB_j equal to yA bit for bit) gives
 * +0.0 exactly in all four.  Deterministic: no floating-point atomics, every sum has a shape fixed by the sizes; s1, st
 * and moments are the same bits with and without the bootstrap.
 * Up to smart_sobol_lds_capacity() base rows a row's A and B stay in LDS and the matrix is read from HBM once; beyond, they
 * are read again from L2 (the same sums in the same order).
 * Errors (all found before the device is touched): SMART_E_NULL y, s1, st or moments missing, counts / s1_std / st_std
 * missing with n_resamples > 0, workspace missing where smart_sobol_workspace_bytes is not 0; SMART_E_SIZE n_base < 1 or
 * >= 2^31, n_params outside 1 .. SMART_SOBOL_MAX_PARAMS, n_rows < 1 or >= 2^31, ld < n_base * (n_params + 2),
 * n_resamples < 0 or > smart_sobol_max_resamples(), workspace_bytes too small; then SMART_E_NO_DEVICE.
 */
#define SMART_SOBOL_MAX_PARAMS 16
int smart_sobol_indices_hip(int64_t n_base, int32_t n_params, int64_t n_rows, const double *y, int64_t ld, double *s1,
                            double *st, double *moments, const uint16_t *counts, int32_t n_resamples, double *s1_std,
                            double *st_std, void *workspace, int64_t workspace_bytes, void *stream);

/* The workspace smart_sobol_indices_hip needs, in bytes, for these sizes: 0 in this version (the two kernels share only the
 * caller's moments[]); the argument is part of the entry so that a version that stages terms needs no new ABI.  A negative
 * SMART_E_SIZE for sizes the entry refuses.  Needs no device. */
int64_t smart_sobol_workspace_bytes(int64_t n_base, int32_t n_params, int64_t n_rows, int32_t n_resamples);

/* The largest n_resamples of one call (512: one lane per replicate in a workgroup of 512).  Needs no device. */
int32_t smart_sobol_max_resamples(void);

/* The largest n_base whose A and B blocks a workgroup keeps in LDS (8,192: 16 bytes per base row, 128 KiB of the 160 KiB
 * of a gfx950 compute unit).  Needs no device. */
int64_t smart_sobol_lds_capacity(void);

/*
 * Score uncertainty: the seven objective functions of an existing discharge matrix under resampling of WINDOWS of report
 * steps -- a block bootstrap over hydrological years, a leave-one-year-out jackknife (Clark et al. 2021, Water Resour.
 * Res. 57) -- for every sample: the point value, the replicates' mean, standard deviation and order statistics.
 *   sim[R][ld] sample-minor (the layout smart_run_ensemble_hip writes), obs[R] (NaN = missing), window[R] int32 with the
 *   convention of smart_objfn_windows_hip (-1 = no window, else 0 .. n_windows-1), counts[n_resamples][n_windows] uint16,
 *   point[N][SMART_OBJFN_WINDOW_COLS], stats[SMART_OBJFN_WINDOW_COLS][2 + n_probs][N] (sample-minor: stats[s][c] is a
 *   contiguous [N] vector), replicates[n_resamples][SMART_OBJFN_WINDOW_COLS][N] or NULL, workspace: device pointers;
 *   probs[n_probs]: HOST pointer, read before the call returns, each in (0, 1], n_probs <= SMART_QUANTILES_MAX_PROBS;
 *   transform / eps as for smart_objfn_windows_hip.  Asynchronous on stream; allocates nothing: the workspace is the
 *   caller's, smart_bootstrap_workspace_bytes says how much.
 * The valid rows of window w are { r : window[r] == w, obs[r] not NaN }.  Replicate b is the multiset union over w of the
 * valid rows of window w, each taken counts[b][w] times; its seven values NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE are the
 * formulas of montecarlo.py:193-209 (smart_objfn_hip's) on (f(sim), f(obs)) over that multiset, f the transform.  The
 * POINT value is the replicate with every count 1.  The entry does not know what a year is: a bootstrap and a jackknife
 * differ in counts only.  Rules:
 *   - a replicate with fewer than two rows is NaN in all seven columns, for every sample;
 *   - a (sample, window) that meets a transformed value that is not finite (smart_objfn_windows_hip's list; sums of finite
 *     values that overflow count the same way) makes NaN every replicate of that sample whose count for that window is
 *     not 0; a replicate with count 0 there is not affected;
 *   - a non-finite f(obs[r]) in window w does the same for every sample.
 * Outputs:
 *   point[n][s]                      the point value
 *   stats[s][SMART_BOOT_MEAN][n]     the mean over the n_resamples replicates
 *   stats[s][SMART_BOOT_STD][n]      their standard deviation, ddof = 1; NaN for n_resamples < 2
 *                                    (both are NaN if any replicate of that (sample, score) is NaN)
 *   stats[s][2 + k][n]               the max(1, ceil(probs[k] * n_resamples))-th smallest of the replicate values:
 *                                    numpy.quantile(..., method='inverted_cdf'), an element of the set, NaN sorts last
 *   replicates[b][s][n]              every replicate, where the caller wants them (tests, small n_resamples, the whole
 *                                    distribution); stats are the same bits with and without
 * n_resamples == 0 is allowed: point only; counts, probs and stats may be NULL and stats is not touched.
 * The matrix is read once: per (window, sample) five one-pass moments about constants of the whole launch (the mean of
 * the finite f(obs), and the sample's transformed value in the first valid row), which add across windows; a replicate is
 * counts x moments (smartpy_amd/csrc/smart_bootstrap.hip).  Mean and standard deviation accumulate in replicate order in
 * the one-pass form about the point value.  Deterministic: no floating-point atomics, every sum has one association for a
 * given (n_samples, n_reports, window array, n_resamples): two launches give the same bits, whatever ld.
 * Errors (all found before the device is touched, every output left as it was): SMART_E_NULL sim, obs, window or point
 * missing, counts, probs or stats missing with n_resamples > 0, workspace missing; SMART_E_SIZE n_samples or n_reports < 1
 * or >= 2^31, ld < n_samples, n_windows outside 1 .. smart_bootstrap_max_windows(), n_resamples outside
 * 0 .. smart_bootstrap_max_resamples(), n_probs outside 1 .. 16 or a probability outside (0, 1] with n_resamples > 0, eps
 * negative or not finite, workspace_bytes too small; SMART_E_MODE unknown transform; then SMART_E_NO_DEVICE.
 */
#define SMART_BOOT_MEAN 0
#define SMART_BOOT_STD 1
int smart_objfn_bootstrap_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                              const int32_t *window, int32_t n_windows, int32_t transform, double eps,
                              const uint16_t *counts, int32_t n_resamples, const double *probs, int32_t n_probs,
                              double *point, double *stats, double *replicates, void *workspace, int64_t workspace_bytes,
                              void *stream);

/* The workspace smart_objfn_bootstrap_hip needs, in bytes: the moments of every (window, sample), 40 * n_windows *
 * n_samples bytes, and the replicates and order statistics of one CHUNK of samples -- the entry walks the samples in chunks
 * of a multiple of 64 (at least 64, at most 16,384) whose 7 * n_resamples values per sample stay below 128 MiB, so the
 * second part does not grow with n_samples.  with_replicates (the caller passes a replicates buffer) does not change the
 * answer in this version: the chunk is where the order statistics are taken; the argument is part of the entry so that a
 * version that takes them in the caller's buffer needs no new ABI.  A negative SMART_E_SIZE for sizes the entry refuses.
 * Needs no device. */
int64_t smart_bootstrap_workspace_bytes(int64_t n_samples, int32_t n_windows, int32_t n_resamples, int32_t with_replicates);

/* The largest n_windows of smart_objfn_bootstrap_hip (64: one lane of a wavefront per window holds a replicate's counts).
 * Needs no device. */
int32_t smart_bootstrap_max_windows(void);

/* The largest n_resamples of one call (4,096, inside the sort capacity of the order statistics).  Needs no device. */
int32_t smart_bootstrap_max_resamples(void);

/*
 * Pareto selection: for every row of a score matrix, the number of rows that dominate it over n_objectives selected
 * columns, each with a direction.  0 = the row is on the Pareto front (no row beats it on every selected score at once).
 *   scores[n_rows][ld] (row-major: a row's scores together, ld > the largest selected column), eligible [n_rows] bytes
 *   or NULL, dominated_by [n_rows] int32, workspace: device pointers.  columns, direction, target [n_objectives]: HOST
 *   arrays, read before the call returns.  Asynchronous on stream; allocates nothing.
 * key[i][m], in fp64 exactly as written, from x = scores[i][columns[m]]: x for SMART_PARETO_MAX, -x for SMART_PARETO_MIN,
 * -|x - target[m]| for SMART_PARETO_TARGET (target may be NULL when no column is a TARGET).  Row i TAKES PART iff eligible
 * is NULL or eligible[i] != 0, and none of its selected scores is a NaN; columns that are not selected, and the padding of
 * ld, are never read.  Row j dominates row i iff both take part, key[j][m] >= key[i][m] for every m and key[j][m] >
 * key[i][m] for at least one m (IEEE compares: -0.0 equals +0.0, infinities take part).  Rows whose keys are all equal do
 * not dominate each other: a front keeps its duplicates.
 *   dominated_by[i] = the number of rows that dominate row i; -1 where row i does not take part.
 * The rows that take part are compacted first, so the work is E^2 pairs for E such rows, not n_rows^2.  Deterministic: the
 * results are sums of integers that no atomic touches.
 * Errors (all found before the device is touched): SMART_E_NULL scores, columns, direction or dominated_by missing, target
 * missing where a direction is TARGET, workspace missing; SMART_E_SIZE n_rows outside 1 .. 2^31 - 1, n_objectives outside
 * 1 .. SMART_PARETO_MAX_OBJECTIVES, a column negative or >= ld, a column named twice, a TARGET's target NaN or infinite,
 * workspace_bytes below smart_pareto_workspace_bytes; SMART_E_MODE an unknown direction; then SMART_E_NO_DEVICE.
 */
#define SMART_PARETO_MAX_OBJECTIVES 16
#define SMART_PARETO_MAX 0
#define SMART_PARETO_MIN 1
#define SMART_PARETO_TARGET 2
int smart_pareto_counts_hip(int64_t n_rows, const double *scores, int64_t ld, const int32_t *columns,
                            const int32_t *direction, const double *target, int32_t n_objectives, const uint8_t *eligible,
                            int32_t *dominated_by, void *workspace, int64_t workspace_bytes, void *stream);

/* The workspace smart_pareto_counts_hip needs, in bytes: a counter, the compacted keys (n_rows x 2, 4, 8 or 16 doubles),
 * the list of the rows that take part and 16 partial counts per row.  Monotone in both arguments; 0 for sizes the entry
 * refuses.  Needs no device. */
int64_t smart_pareto_workspace_bytes(int64_t n_rows, int32_t n_objectives);

/* SMART_PARETO_MAX_OBJECTIVES as the library was built.  Needs no device. */
int smart_pareto_max_objectives(void);

/*
 * Ensemble verification along the SAMPLE axis, per report step: is the predictive distribution of the (behavioural,
 * likelihood-weighted) ensemble any good against the observation.  For one report step with members x_n = sim[r][n],
 * weights w_n >= 0 (NULL: all 1) and the observation y = obs[r]: the members with w_n == 0 take no part at all -- they
 * are dropped when the step is loaded, a NaN or an infinity of weight zero decides nothing.  With the live members
 * sorted ascending x_(1) <= ... <= x_(M), W their total weight, A_i = sum of w_(j) over j <= i (prefix sums, left to
 * right), B_i = sum of w_(j) over j > i (suffix sums, right to left; never 1 - A_i / W), P_i = A_i / W, Q_i = B_i / W:
 *   SMART_ENS_CRPS      the integral of (F(x) - 1[x >= y])^2 dx = max(x_(1) - y, 0) + max(y - x_(M), 0) +
 *                       sum over i < M of (m_i - x_(i)) P_i^2 + (x_(i+1) - m_i) Q_i^2, m_i = min(max(y, x_(i)), x_(i+1))
 *   SMART_ENS_SPREAD    the integral of F (1 - F) dx = sum over i < M of (x_(i+1) - x_(i)) P_i Q_i  (= E|X - X'| / 2, so
 *                       CRPS = E|X - y| - SPREAD; computed as this sum of non-negative terms, not as that difference)
 *   SMART_ENS_PIT_LOW   sum of w over { x < y } / W         SMART_ENS_PIT_HIGH   sum of w over { x <= y } / W
 *   SMART_ENS_MEAN      sum of w x / W, added in sorted order
 * -0.0 and +0.0 are one value.  W == 0, or a live member that is a NaN or an infinity: all five NaN for that step.  An
 * observation that is not finite (missing), or obs == NULL (every one missing): CRPS and both PITs NaN; SPREAD and MEAN
 * do not depend on it.  The weights MUST be finite and >= 0: a precondition, not checked on the device.
 *   sim[R][ld] sample-minor (the layout smart_run_ensemble_hip writes), weights[N] or NULL, obs[R] or NULL,
 *   out[SMART_ENSEMBLE_SCORE_COLS][R] (every column a contiguous [R] vector): device pointers.  Asynchronous on stream;
 *   allocates nothing: the workspace is the caller's.
 * One workgroup per report step, in one of two forms (smartpy_amd/csrc/smart_ensemble_scores.hip):
 *   SMART_ENS_LDS     the step sorted in LDS, both scans and the terms in registers; no workspace;
 *                     n_samples <= smart_ensemble_scores_lds_capacity(), else SMART_E_SIZE
 *   SMART_ENS_GLOBAL  any n_samples <= 2^24: the step sorted in the workspace (long stages there, short ones block by
 *                     block in LDS); the report steps go in batches of as many as the workspace holds, one launch each
 *   SMART_ENS_AUTO    LDS within its capacity, global beyond
 * Deterministic: no floating-point atomics, every sum has one association for a given (n_samples, form), so two launches
 * give the same bits -- whatever the batches.  The two forms associate differently and agree to rounding only.
 * Errors (all found before the device is touched): SMART_E_NULL sim or out missing, the global form without a workspace;
 * SMART_E_SIZE a size < 1, ld < n_samples, n_reports >= 2^31, n_samples > 2^24, the LDS form beyond its capacity, a
 * workspace that does not hold one step; SMART_E_MODE unknown method; then SMART_E_NO_DEVICE without a HIP device.
 */
#define SMART_ENSEMBLE_SCORE_COLS 5
#define SMART_ENS_CRPS 0
#define SMART_ENS_SPREAD 1
#define SMART_ENS_PIT_LOW 2
#define SMART_ENS_PIT_HIGH 3
#define SMART_ENS_MEAN 4
#define SMART_ENS_AUTO 0
#define SMART_ENS_LDS 1
#define SMART_ENS_GLOBAL 2
int smart_ensemble_scores_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *weights,
                              const double *obs, double *out, int32_t method, void *workspace, int64_t workspace_bytes,
                              void *stream);

/* The workspace smart_ensemble_scores_hip asks for, in bytes: 0 for the LDS form (and for AUTO within its capacity); for
 * the global form one step is n_samples rounded up to a power of two (at least 4096) times 16 bytes with weights, 8
 * without, and the answer holds min(n_reports, as many steps as fit in 256 MiB, at least one).  The entry itself takes
 * any workspace that holds one step.  A negative SMART_E_* code for what the entry refuses.  Needs no device. */
int64_t smart_ensemble_scores_workspace_bytes(int64_t n_samples, int64_t n_reports, int32_t weighted, int32_t method);

/* The largest n_samples SMART_ENS_LDS takes: 8192 (10 bytes per sorted element in LDS).  Needs no device. */
int64_t smart_ensemble_scores_lds_capacity(void);

/*
 * Dynamic identifiability analysis (DYNIA, Wagener et al. 2003, Hydrol. Process. 17): WHEN in the record does the sample
 * the caller already has constrain each factor.  Inputs: sim[R][ld] sample-minor (the layout smart_run_ensemble_hip
 * writes); obs[R], a value that is not finite is missing; a half width h >= 0 in report steps, the window being
 * w = 2 h + 1 steps; 1 <= min_valid <= w; fraction in (0, 1]; a category table cat[P][N] of uint8 -- the bin of row n on
 * factor p, 255: the row takes no part in this factor (a value in n_bins .. 254 does the same) --, P <=
 * SMART_DYNIA_MAX_FACTORS, n_bins B <= SMART_DYNIA_MAX_BINS; support SMART_DYNIA_EQUAL or SMART_DYNIA_LINEAR.
 * Per report step r:
 *   1. V_r = { s : |s - r| <= h, 0 <= s < R, obs[s] finite }: the window is cut at both ends of the record.
 *      count[r] = |V_r|.
 *   2. count[r] < min_valid: the step is not assessed -- cut[r] and every share of the step are NaN, retained[r] = 0, and
 *      the step's row of err is NaN where err is asked for.
 *   3. Otherwise E[r][n] = sum over s in V_r of |sim[s][n] - obs[s]|: the window's SUM of absolute errors, not its mean --
 *      the count is the same for every sample of a step, so neither the ranks nor the normalised supports depend on it,
 *      and one rounding is saved (divide by count[r] for display).  A sim value that is not finite makes E not finite.
 *   4. The rows with a finite E[r][n] are eligible, M_r of them; M_r == 0 is treated like a step not assessed.
 *      k = max(1, (int64) ceil(fraction * (double) M_r)), in double arithmetic exactly as written.
 *   5. cut[r] = the k-th smallest eligible E (compared as order-preserving keys: -0.0 and +0.0 are one value).  Retained:
 *      every eligible row with E <= cut[r] -- every tie at the cut stays in, retained[r] >= k.
 *   6. The support of a retained row: EQUAL s_n = 1; LINEAR s_n = cut[r] - E[r][n], one subtraction, >= 0.  S = the sum of
 *      s_n over the retained rows; S == 0 (every retained row ties at the cut) falls back to s_n = 1.
 *   7. shares[r][p][b] = (the sum of s_n over the retained n with cat[p][n] == b) / S.  A factor with rows of category
 *      255 sums to less than one.
 * Outputs, device pointers: shares[R][P][B], cut[R], retained[R] and count[R] (int32), and err[R][ld_err] holding the E
 * sums, or NULL where they are not wanted.  Asynchronous on stream; allocates nothing: the workspace is the caller's.  The
 * E sums of a batch of steps live there as [batch][N] doubles (in err itself where it is given); the entry takes any
 * workspace that holds one step, n_samples * 8 bytes.
 * The window sums use additions only (no running sum that subtracts the outgoing term): time is tiled in blocks of w rows
 * at absolute positions, a window is a suffix sum of one block plus a prefix sum of the next, at most w - 1 additions of
 * non-negative terms (smartpy_amd/csrc/smart_dynia.hip).  A share adds its supports in ascending sample order.
 * Deterministic: no floating-point atomics, every sum has one association for a given (n_samples, n_reports, h), so two
 * launches give the same bits -- whatever the batches.
 * Errors (all found before the device is touched): SMART_E_NULL a required pointer missing (err alone may be NULL);
 * SMART_E_SIZE a size < 1, n_samples or n_reports >= 2^31, h beyond smart_dynia_max_half_width(), P or B beyond the
 * macros, ld or ld_err < n_samples, min_valid outside 1 .. w, fraction outside (0, 1] or NaN, a workspace that does not
 * hold one step; SMART_E_MODE unknown support; then SMART_E_NO_DEVICE without a HIP device.
 */
#define SMART_DYNIA_MAX_FACTORS 16
#define SMART_DYNIA_MAX_BINS 64
#define SMART_DYNIA_EQUAL 0
#define SMART_DYNIA_LINEAR 1
int smart_dynia_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                    int32_t half_width, int32_t min_valid, double fraction, const uint8_t *cat, int32_t n_factors,
                    int32_t n_bins, int32_t support, double *shares, double *cut, int32_t *retained, int32_t *count,
                    double *err, int64_t ld_err, void *workspace, int64_t workspace_bytes, void *stream);

/* The workspace smart_dynia_hip asks for, in bytes: one step is n_samples * 8 bytes, and the answer holds
 * min(n_reports, as many steps as fit in 256 MiB, at least one).  SMART_E_SIZE (negative) for sizes the entry refuses.
 * Needs no device. */
int64_t smart_dynia_workspace_bytes(int64_t n_samples, int64_t n_reports, int32_t half_width, int32_t n_factors,
                                    int32_t n_bins);

/* The largest half width smart_dynia_hip takes: 63 (a window of 127 steps per lane in LDS).  Needs no device. */
int32_t smart_dynia_max_half_width(void);

/* The largest n_samples whose step smart_dynia_hip keeps in LDS for the selection: 16384 (up to 2048 in a smaller
 * instance); beyond, the step is re-read from the batch's row.  Needs no device. */
int64_t smart_dynia_lds_capacity(void);

/*
 * PAWN sensitivity from the sample at hand (Pianosi & Wagener 2015, Environ. Model. Softw. 67; the given-data form, 2018,
 * Environ. Model. Softw. 108): HOW MUCH does the distribution of an output move when a factor is confined to one bin of
 * its range -- the Kolmogorov-Smirnov distance between the unconditional empirical CDF and the conditional one, per
 * output, factor and bin.  Inputs: y[R][ld] sample-minor (the discharge matrix where smart_run_ensemble_hip left it, or
 * any [M][N] table of per-row values); a category table cat[P][N] of uint8 exactly as smart_dynia_hip takes it --
 * cat[p][n] the bin of row n on factor p, 255 or any value >= B: in no bin of this factor --, P <= SMART_PAWN_MAX_FACTORS,
 * n_bins B <= SMART_PAWN_MAX_BINS, N <= 2^24.
 * Per call: counts[p][b] = the number of rows n < N with cat[p][n] == b (int32).
 * Per row r of the matrix:
 *   1. The N values sorted ascending, compared as order-preserving keys: -0.0 and +0.0 are one value.
 *   2. Position i (0-based) is an EVALUATION POINT iff i == N - 1 or key[i] != key[i + 1]: the end of a run of ties.
 *   3. For factor p and bin b with n_b = counts[p][b] > 0, c_b(i) the number of positions <= i whose row lies in bin b:
 *        num[r][p][b] = max over the evaluation points i of |(i + 1) n_b - c_b(i) N|     (integers below 2^48)
 *        ks[r][p][b]  = (double) num / ((double) N * (double) n_b)      (the product is exact: ONE correctly rounded division)
 *   4. n_b == 0: NaN.
 *   5. A value of the row that is not finite (NaN, +-inf): every ks[r][.][.] is NaN.
 * This is sup over x of |F(x) - F_b(x)| of the two right-continuous empirical CDFs: both are constant between sample
 * values, so the supremum is taken at a sample value, after all its ties.  Rows of category 255 belong to the
 * unconditional sample and to no bin.
 * Outputs, device pointers: ks[R][P][B] (double) and counts[P][B] (int32).  Asynchronous on stream; allocates nothing: the
 * workspace is the caller's.  No atomics of any kind.  Everything is integers until the one division (held exactly in
 * doubles: smartpy_amd/csrc/smart_pawn.hip), so the result does not depend on the launch, the batches or the form: the
 * two forms agree BIT FOR BIT, and with the definition as written.
 * One workgroup per row, in one of two forms:
 *   SMART_PAWN_LDS     the row sorted in LDS with 16-bit sample indices; no workspace;
 *                      n_samples <= smart_pawn_lds_capacity(), else SMART_E_SIZE
 *   SMART_PAWN_GLOBAL  any n_samples <= 2^24: (key, 32-bit index) pairs sorted in the workspace (long stages there, short
 *                      ones block by block in LDS); the rows go in batches of as many as the workspace holds
 *   SMART_PAWN_AUTO    LDS within its capacity, global beyond
 * Errors (all found before the device is touched; the first offending argument wins): SMART_E_NULL y, cat, ks or counts
 * missing; SMART_E_SIZE a size < 1, n_samples > 2^24, n_rows >= 2^31, ld < n_samples, n_factors outside 1 .. 16, n_bins
 * outside 1 .. 64; SMART_E_MODE unknown method; SMART_E_SIZE the LDS form beyond its capacity; SMART_E_NULL the global form
 * without a workspace, SMART_E_SIZE a workspace that does not hold one step; then SMART_E_NO_DEVICE without a HIP device.
 */
#define SMART_PAWN_MAX_FACTORS 16
#define SMART_PAWN_MAX_BINS 64
#define SMART_PAWN_AUTO 0
#define SMART_PAWN_LDS 1
#define SMART_PAWN_GLOBAL 2
int smart_pawn_ks_hip(int64_t n_samples, int64_t n_rows, const double *y, int64_t ld, const uint8_t *cat, int32_t n_factors,
                      int32_t n_bins, double *ks, int32_t *counts, int32_t method, void *workspace, int64_t workspace_bytes,
                      void *stream);

/* The workspace smart_pawn_ks_hip asks for, in bytes: 0 for the LDS form (and for AUTO within its capacity); for the
 * global form one step is n_samples rounded up to a power of two (at least 4096) times 12 bytes, and the answer holds
 * min(n_rows, as many steps as fit in 256 MiB, at least one).  The entry itself takes any workspace that holds one step.
 * A negative SMART_E_* code for what the entry refuses.  Needs no device. */
int64_t smart_pawn_workspace_bytes(int64_t n_samples, int64_t n_rows, int32_t method);

/* The largest n_samples SMART_PAWN_LDS takes: 8192 (10 bytes per sorted element in LDS).  Needs no device. */
int64_t smart_pawn_lds_capacity(void);

/*
 * One generation of DE-MCz -- differential evolution Markov chain with sampling from the past (ter Braak & Vrugt 2008,
 * Stat. Comput. 18), with the subspace crossover of DREAM (Vrugt 2016) and a uniform prior on the box [lo, hi] -- AROUND
 * the ensemble launch that scores the proposals: N chains in lockstep, d <= SMART_DEMCZ_MAX_DIMS varying parameters.  No
 * snooker update, no crossover adaptation, no outlier handling.  One call runs the ACCEPT phase (score given), the PROPOSE
 * phase (propose != 0) or both, in that order, as two small kernels on `stream`, one lane per chain; nothing is read
 * back, nothing is allocated, no atomics.  The archive size M and the generation g are the caller's to keep.
 *
 * Chain i of the call has the number c = chain_offset + i (below 2^32); every per-chain array is indexed by i, the
 * archive and the draws by c: a call over a part of the chains draws what the call over all of them draws.
 *
 * RANDOMNESS is Philox4x32-10 (Salmon et al. 2011), counter-based: the bits depend on (seed, chain, generation) only.
 *   words(c, g, b) = Philox with counter (c, g, b, 0) and key (seed mod 2^32, seed div 2^32).
 *   u53(w0, w1) = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53.
 *   mulhi(w, n) = (w n) >> 32 in 64-bit integers.
 *   Block 0 = (r0, r1, r2, r3): a = mulhi(r0, M); b = mulhi(r1, M - 1), then b += (b >= a); jump = r2 < J; fallback
 *     dimension = mulhi(r3, d).
 *   Block 1 = (w0, w1, ., .): the acceptance uniform of generation g, u = u53(w0, w1).  The accept phase reads it for the
 *     proposals that the propose phase of generation g made.
 *   Block 2 + j, for dimension j: dimension j is updated iff w0 < C; eps_j = scale_j (2 u53(w1, w2) - 1).
 *   If no dimension is selected, the fallback dimension alone is.
 * The host passes J = floor(p_jump 2^32) and C = floor(CR 2^32) as 64-bit integers in [0, 2^32] (jump_threshold,
 * cr_threshold), scale_j = b* (hi_j - lo_j), and a table gamma[d' - 1] = 2.38 / sqrt(2 d') for d' = 1 .. d; lo, hi, scale,
 * gamma and columns are HOST arrays of n_dims values (they travel as kernel arguments).
 *
 * ACCEPT phase of a call with generation g: the decision on the proposals of generation g - 1.  Per chain: the score
 * score[i * score_stride] gives the log-density l*:
 *   SMART_DEMCZ_SCORE_LOGP        l* = score
 *   SMART_DEMCZ_SCORE_RMSE        l* = -((n_eff / 2) ln(n_obs score^2))     the Gaussian likelihood with sigma integrated out;
 *                                 the score is read in place, e.g. the RMSE column of the [N][8] objective table, stride 8
 *   SMART_DEMCZ_SCORE_RMSE_SIGMA  l* = -(n_eff score^2) / (2 sigma^2)        for a fixed sigma
 * With u of block 1 of generation g - 1: rejected if out[i] is set or l* is NaN, else accepted iff log(u) < l* - logp[i]
 * (an IEEE compare: a NaN difference rejects).  On acceptance x[i][.] = proposal[i][.], logp[i] = l*, the payload
 * carry[i][0 .. n_carry) = carry_new[i][.] (n_carry <= SMART_DEMCZ_MAX_CARRY doubles that travel with the chain: its
 * objective functions, say) and accepted[i] += 1.  g = 1 is the INITIAL POPULATION taking its scores: x stays as the
 * caller launched it, logp[i] = l* and the payload are taken unconditionally (a NaN too), accepted is not touched, nothing
 * is drawn.  With append != 0 every chain's state, logp and payload as they are after the decision are written as archive
 * row M + c (archive[capacity][d], archive_logp[capacity], archive_carry[capacity][n_carry]).
 *
 * PROPOSE phase of a call with generation g, from M' >= 2 archive rows -- M' = archive_size, or archive_size +
 * chain_offset + n_chains where the accept phase of the same call appended (a call over a part of the chains that appends
 * proposes in a call of its own, once every part has appended).  With gamma = 1 where jump is set, else gamma[d' - 1], d'
 * the number of updated dimensions, an updated dimension j is
 *     t = z_a,j - z_b,j;  t = gamma t;  t = t + eps_j;  y = x_j + t        (each operation rounded once, no contraction)
 * then   if y < lo_j: y = 2 lo_j - y;   if y > hi_j: y = 2 hi_j - y;   y still outside [lo_j, hi_j] (or NaN): the
 * proposal is `out`.  A dimension that is not updated keeps x_j.  Outputs: proposal[i][0 .. d), out[i] (uint8), and the
 * launch matrix rows[i][columns[j]] = the proposal's j, or x_j for every j where the proposal is out (the lockstep launch
 * stays valid); the other columns of rows[N][ld] are the caller's and are not touched.
 *
 * Errors (all found before the device is touched; the first offending argument wins): SMART_E_NULL x, logp, proposal, out
 * or archive missing; SMART_E_SIZE n_chains < 1, a chain number >= 2^32, n_dims outside 1 .. 16, generation outside
 * 1 .. 2^32 - 1, capacity outside 1 .. 2^31 - 1, archive_size outside 0 .. capacity, n_carry outside 0 .. 16; SMART_E_NULL
 * neither phase asked for; accept phase: SMART_E_MODE unknown score_kind, SMART_E_SIZE score_stride < 1, n_obs < 1 (RMSE),
 * n_eff or sigma not finite and > 0 (where read), SMART_E_NULL accepted, carry / carry_new (n_carry > 0), archive_logp /
 * archive_carry (append) missing, SMART_E_SIZE an append past the capacity -- never a write past the end; SMART_E_NULL
 * append without the accept phase; propose phase: SMART_E_NULL lo, hi, scale, gamma, rows or columns missing, SMART_E_SIZE
 * M' < 2 or > capacity, a threshold outside 0 .. 2^32, ld < n_dims, a column outside 0 .. ld - 1 or named twice, bounds
 * that are not finite or lo > hi; then SMART_E_NO_DEVICE without a HIP device.
 */
#define SMART_DEMCZ_MAX_DIMS 16
#define SMART_DEMCZ_MAX_CARRY 16
#define SMART_DEMCZ_SCORE_LOGP 0
#define SMART_DEMCZ_SCORE_RMSE 1
#define SMART_DEMCZ_SCORE_RMSE_SIGMA 2
int smart_demcz_step_hip(int64_t n_chains, int64_t chain_offset, int32_t n_dims, uint64_t seed, int64_t generation,
                         int64_t archive_size, int64_t capacity, double *x, double *logp, double *carry, int32_t *accepted,
                         double *proposal, uint8_t *out, const double *score, int64_t score_stride, int32_t score_kind,
                         int64_t n_obs, double n_eff, double sigma, const double *carry_new, int32_t n_carry,
                         int32_t append, double *archive, double *archive_logp, double *archive_carry, int32_t propose,
                         const double *lo, const double *hi, const double *scale, const double *gamma,
                         int64_t jump_threshold, int64_t cr_threshold, double *rows, int64_t ld, const int32_t *columns,
                         void *stream);

/*
 * One generation of NSGA-II (Deb et al. 2002, IEEE Trans. Evol. Comput. 6) -- non-dominated sorting, crowding distance and
 * truncation over parents and offspring -- with the variation of differential evolution on that selection (NSDE, GDE3:
 * Kukkonen & Lampinen 2005), AROUND the ensemble launch that scores the offspring: N rows in lockstep, d varying parameters,
 * M objectives.  Simulated binary crossover and polynomial mutation are not built: both need pow, which is not correctly
 * rounded, and every output of this entry is defined to the bit.  One call runs the SURVIVE phase (scores given), the VARY
 * phase (vary != 0) or both, in that order, on `stream`; nothing is allocated: the workspace is the caller's.  The only
 * atomics are integer counters whose final value does not depend on the order; every output has the same bits on every
 * launch.  The generation g and which of its two population buffers is current are the caller's to keep.
 *
 * SIZES.  4 <= N = n_rows <= SMART_NSGA2_MAX_ROWS, 1 <= d = n_dims <= SMART_NSGA2_MAX_DIMS, 2 <= M = n_objectives <=
 * SMART_NSGA2_MAX_OBJECTIVES, a payload of n_carry <= SMART_NSGA2_MAX_CARRY doubles per row.  CANDIDATES e in [0, E): with
 * parents != 0, E = 2 N, e < N is parent e (row e of pop_x, pop_keys, pop_carry, pop_part) and e >= N is offspring e - N; with
 * parents == 0 (the first call: the N launched rows are the candidates) E = N and e is offspring e.  Offspring c has the
 * parameters offspring[c][0 .. d), the flag out[c], the scores scores[c * ld_scores + score_columns[m]] (read in place: the
 * [N][8] objective table of smart_run_ensemble_hip with ld_scores = 8 is the main case), eligible[c] (eligible may be NULL) and
 * the payload carry_new[c][0 .. n_carry).
 *
 * KEYS, as for smart_pareto_counts_hip: key_m = x for SMART_PARETO_MAX, -x for SMART_PARETO_MIN, -|x - target[m]| for
 * SMART_PARETO_TARGET, of x = the score in column score_columns[m]; larger keys are better.
 * TAKING PART.  An offspring takes part iff out[c] == 0, eligible is NULL or eligible[c] != 0, and none of its M selected
 * scores is a NaN.  The M keys of an offspring that does not take part are stored as the quiet NaN 0x7ff8000000000000,
 * whatever its scores are.  A parent takes part iff it did when it entered the population (pop_part).
 * DOMINANCE, exactly as for smart_pareto_counts_hip: j dominates i iff both take part, key_m(j) >= key_m(i) for every m and
 * not key_m(j) <= key_m(i) for every m (IEEE compares).  Candidates with equal keys do not dominate each other.
 * RANK.  Fronts are peeled: rank 1 are the candidates that take part and that nobody dominates, rank r + 1 those that only
 * candidates of ranks <= r dominate.  Peeling stops after the first front with which at least N candidates are ranked, or
 * when none that takes part is left.  A candidate that takes part but lies beyond the last peeled front has rank
 * SMART_NSGA2_RANK_BEYOND = 2^31 - 2, one that does not take part SMART_NSGA2_RANK_OUT = 2^31 - 1.
 * CROWDING DISTANCE, by value (it does not depend on the order a sort would leave ties in).  For candidate i of a peeled
 * front F, with min_m and max_m the smallest and largest key_m over F, dist = 0.0, then for m = 0 .. M - 1 in this order:
 *     key_m(i) == min_m or key_m(i) == max_m:   dist = +inf
 *     otherwise:   U = the smallest key_m(j) >= key_m(i), L = the largest key_m(j) <= key_m(i), over the j in F, j != i;
 *                  t = U - L;  w = max_m - min_m;  t = t / w;  dist = dist + t      (each operation rounded once)
 * Every duplicate of an extreme has +inf, a duplicate in the interior has U = L there, and on keys without ties this is
 * Deb's sorted-neighbour sum.  A candidate outside the peeled fronts has the distance 0.0.
 * SURVIVAL.  The total order is (rank ascending, distance descending, e ascending); pos(e) = the number of candidates that
 * precede e.  e survives iff pos(e) < N and becomes row p = pos(e) of the NEXT population: next_x[p][.] = its d parameters,
 * next_keys[p][0 .. M) its keys, next_carry[p][.] its payload, next_part[p] whether it takes part, rank[p], crowding[p],
 * origin[p] = e.  The population therefore lies in tournament order: a smaller row number wins the binary tournament.
 * counts[0] = the number of fronts peeled, counts[1] = the number of candidates of rank 1 (int32, left on the device).
 * next_* must not overlap pop_*: the caller keeps two population buffers and swaps them.
 *
 * VARIATION of generation g, from the population the SURVIVE phase of the same call wrote (next_x), or from pop_x in a call
 * without one (parents != 0 is required then); one lane per offspring c.  Philox4x32-10 with the counter (c, g, block, 0) and
 * the key (seed mod 2^32, seed div 2^32); u53 and mulhi as for smart_demcz_step_hip.
 *   Block 0 = (r0, r1, r2, r3): a = mulhi(r0, N); b = mulhi(r1, N - 1), then b += (b >= a); the base row t = min(a, b) --
 *     the binary tournament by rank and then crowding; p1 = mulhi(r2, N); p2 = mulhi(r3, N - 1), then p2 += (p2 >= p1).
 *   Block 1 = (w0, ., ., .): the fallback dimension mulhi(w0, d).
 *   Block 2 + j, for dimension j: j is crossed iff w0 < C, C = cr_threshold = floor(CR 2^32) in [0, 2^32];
 *     eps_j = scale_j (2 u53(w1, w2) - 1), scale_j = b* (hi_j - lo_j).  If no dimension is crossed, the fallback one alone is.
 * A crossed dimension, each operation rounded once, no contraction, x the population:
 *     s = x[p1][j] - x[p2][j];  s = f s;  s = s + eps_j;  y = x[t][j] + s
 * then   if y < lo_j: y = 2 lo_j - y;   if y > hi_j: y = 2 hi_j - y;   y still outside [lo_j, hi_j] (or NaN): the offspring
 * is `out`.  A dimension that is not crossed keeps x[t][j].  Outputs: offspring[c][0 .. d), out[c] (uint8) and the launch
 * matrix rows[c][columns[j]] = the offspring's j, or x[t][j] for every j where the offspring is out (the lockstep launch
 * stays valid); the other columns of rows[N][ld] are the caller's and are not touched.  lo, hi, scale, score_columns,
 * direction, target and columns are HOST arrays (they travel as kernel arguments).
 *
 * The SURVIVE phase peels with one small launch per front, issued in batches, and reads ONE 4-byte flag back per batch to
 * learn that the stop condition was met (16 passes in the first batch, twice as many in every further one, at most 1024): a
 * pass that finds it met returns at once.  That is the entry's only wait on the stream; the caller reads nothing.
 *
 * Errors (all found before the device is touched; the first offending argument wins): SMART_E_NULL offspring or out
 * missing; SMART_E_SIZE n_rows outside 4 .. 8192, n_dims outside 1 .. 16, n_objectives outside 2 .. 4, n_carry outside
 * 0 .. 16, generation outside 1 .. 2^32 - 1; SMART_E_NULL neither phase asked for; survive phase: SMART_E_NULL next_x,
 * next_keys, next_part, rank, crowding, origin, counts, score_columns or direction missing, pop_x, pop_keys or pop_part
 * (parents != 0), next_carry, carry_new or -- with parents -- pop_carry (n_carry > 0) missing, SMART_E_SIZE ld_scores < 1, a
 * score column outside 0 .. ld_scores - 1 or named twice, SMART_E_MODE an unknown direction, SMART_E_NULL / SMART_E_SIZE a
 * TARGET without a finite target, SMART_E_NULL no workspace, SMART_E_SIZE one of fewer than smart_nsga2_workspace_bytes
 * bytes; vary phase: SMART_E_NULL lo, hi, scale, rows or columns missing, a call without the survive phase that has no
 * parents or no pop_x, SMART_E_SIZE f not finite, cr_threshold outside 0 .. 2^32, ld < n_dims, a column outside 0 .. ld - 1
 * or named twice, bounds that are not finite or lo > hi; then SMART_E_NO_DEVICE without a HIP device.
 */
#define SMART_NSGA2_MAX_ROWS 8192
#define SMART_NSGA2_MAX_DIMS 16
#define SMART_NSGA2_MAX_OBJECTIVES 4
#define SMART_NSGA2_MAX_CARRY 16
#define SMART_NSGA2_RANK_BEYOND 2147483646
#define SMART_NSGA2_RANK_OUT 2147483647
int smart_nsga2_step_hip(int64_t n_rows, int32_t n_dims, int32_t n_objectives, int32_t n_carry, uint64_t seed,
                         int64_t generation, int32_t parents, const double *pop_x, const double *pop_keys,
                         const double *pop_carry, const uint8_t *pop_part, double *next_x, double *next_keys,
                         double *next_carry, uint8_t *next_part, int32_t *rank, double *crowding, int32_t *origin,
                         int32_t *counts, double *offspring, uint8_t *out, const double *scores, int64_t ld_scores,
                         const int32_t *score_columns, const int32_t *direction, const double *target,
                         const uint8_t *eligible, const double *carry_new, void *workspace, int64_t workspace_bytes,
                         int32_t vary, const double *lo, const double *hi, const double *scale, double f,
                         int64_t cr_threshold, double *rows, int64_t ld, const int32_t *columns, void *stream);

/* The workspace smart_nsga2_step_hip asks for, in bytes, for 2 N candidates: their padded keys, counts, ranks and
 * distances, the counters of the peel, and the bit matrix of who dominates whom, (2 N)^2 / 8 bytes (32 MiB at N = 8192; at
 * least 128 bytes per candidate: the crowding pass keeps its partial results there once the fronts are peeled).
 * SMART_E_SIZE (negative) for sizes the entry refuses.  Needs no device. */
int64_t smart_nsga2_workspace_bytes(int64_t n_rows, int32_t n_objectives);

/*
 * The residual error model of a stored discharge matrix sim[R][ld] (sample-minor): a standard deviation linear in the
 * simulated flow, and standardised residuals that follow a first-order autoregression (Schoups & Vrugt 2010, Water
 * Resour. Res. 46; the AR(1) on the STANDARDISED residuals: Evin et al. 2014, Water Resour. Res. 50).  Sample i has the
 * error parameters (sigma0, sigma1, phi) = err[i * err_ld + 0 .. 2]: err_ld >= 3 is a row stride, so three columns of a
 * wider matrix (the launch matrix of DE-MCz) are read where they lie.  With q = (1 - phi)(1 + phi), for a report step t:
 *     sigma_t = sigma0 + sigma1 sim[t][i]          a_t = (obs[t] - sim[t][i]) / sigma_t
 * each operation rounded once, no contraction.  Device pointers; stream-ordered; nothing is allocated, nothing is read
 * back, no atomics.
 *
 * smart_error_model_loglik_hip: the log-likelihood of every sample -> loglik[3][N], row 0 LOGLIK, row 1 SSQ, row 2 LOGSIG.
 * A step is OBSERVED where obs[t] is not a NaN; an observed step is a START if t = 0 or step t - 1 is not observed (a gap
 * restarts the chain with its stationary density N(0, 1 / q)), else a CONTINUATION.  With n observed steps, S of them
 * starts (both depend on obs alone):
 *     SSQ    = sum over starts of q a_t^2  +  sum over continuations of (a_t - phi a_{t-1})^2       (no negative term)
 *     LOGSIG = sum over observed steps of ln sigma_t                                                 (one log per step)
 *     LOGLIK = ((-SSQ / 2 - LOGSIG) + (S / 2) ln q) - (n / 2) ln(2 pi)
 * A sample is INVALID if |phi| >= 1, if one of its three parameters is not finite, or if at an observed step sim is not
 * finite or sigma_t <= 0: LOGLIK = -inf, SSQ = LOGSIG = NaN.  What sim holds at a step that is not observed is never looked
 * at.  n = 0: all three +0.0.
 * THE ORDER OF THE SUMS is fixed, whatever the launch: the report steps are cut into segments of SMART_ERROR_MODEL_SEGMENT
 * steps, segment s belongs to part s mod 4, a part adds the terms of its steps in ascending order, and the four parts are
 * added as ((p0 + p1) + p2) + p3.  The first step of a segment takes a_{t-1} from row t - 1 itself.
 * Errors (all found before the device is touched; the first offending argument wins): SMART_E_NULL sim, obs, err or
 * loglik missing; SMART_E_SIZE n_samples or n_reports < 1, ld < n_samples, err_ld < 3, more than 2^31 - 1 samples or
 * report steps; then SMART_E_NO_DEVICE without a HIP device.
 *
 * smart_error_model_draw_hip: realisations of the error model on top of the simulated flows -> out[R][out_ld], n_replicates
 * = K columns per sample: column c = i K + k of the call is replicate k of its sample i, C = n_samples K columns in all.
 * Along the report steps of a column, over EVERY step (observed or not):
 *     a_0 = eps_0 / sqrt(q)      a_t = phi a_{t-1} + eps_t      y = sim[t][i] + sigma_t a_t      truncate != 0: y > 0 ? y : 0
 * A sample that is invalid -- as above, judged over every report step -- gives columns of NaN.  RANDOMNESS is
 * Philox4x32-10 with u53 as for smart_demcz_step_hip: for the pair of steps (2j, 2j + 1) the words w0 .. w3 of the counter
 * (column_offset + c, j, 0, 0) under the key (seed mod 2^32, seed div 2^32) give
 *     u1 = 1 - u53(w0, w1) in (0, 1]     u2 = u53(w2, w3)     r = sqrt(-2 ln u1)     ang = 6.283185307179586 u2
 *     eps_{2j} = r cos(ang)              eps_{2j+1} = r sin(ang)
 * so a call over a part of the samples (sim, err and out moved on by that many samples and columns, column_offset = the
 * number of its first column) draws what the call over all of them draws.  Not correctly rounded by definition: ln, cos,
 * sin.
 * Errors, as above: SMART_E_NULL sim, err or out missing; SMART_E_SIZE n_samples, n_reports or n_replicates < 1, ld <
 * n_samples, err_ld < 3, out_ld < C, a column number >= 2^32 (column_offset outside 0 .. 2^32 - 1 included), more than
 * 2^31 - 1 report steps; then SMART_E_NO_DEVICE.
 */
#define SMART_ERROR_MODEL_SEGMENT 64
#define SMART_ERROR_MODEL_LOGLIK 0
#define SMART_ERROR_MODEL_SSQ 1
#define SMART_ERROR_MODEL_LOGSIG 2
int smart_error_model_loglik_hip(int64_t n_samples, int64_t n_reports, const double *sim, int64_t ld, const double *obs,
                                 const double *err, int64_t err_ld, double *loglik, void *stream);
int smart_error_model_draw_hip(int64_t n_samples, int64_t n_reports, int64_t n_replicates, const double *sim, int64_t ld,
                               const double *err, int64_t err_ld, uint64_t seed, int64_t column_offset, int32_t truncate,
                               double *out, int64_t out_ld, void *stream);

/*
 * One assimilation step of a bootstrap particle filter (Gordon et al. 1993; systematic resampling: Kitagawa 1996) AROUND the
 * ensemble launch that ran N particles over window k of the report steps: the particles are weighed by the window's
 * observations, the weights are turned into integers, and where the effective sample size falls below tau N the particles
 * are resampled and moved.  1 <= N = n_particles <= SMART_PARTICLE_MAX_PARTICLES = 2^19, d = n_dims <=
 * SMART_PARTICLE_MAX_DIMS varying parameters, k = step.  Four small kernels on `stream`; nothing is read back, nothing is
 * allocated (the workspace is the caller's), no kernel waits on another workgroup, no floating-point atomics: the same call
 * gives the same bits on every launch.  Which half of its double-buffered arrays is current is the caller's to keep: the
 * *_in arrays are read, the *_out arrays written, and they must not overlap (a parent's row is read while a child's is
 * written).
 *
 * A particle i has a row rows_in[i][0 .. ld) of the launch matrix (the d columns `columns` vary inside [lo, hi]; the others
 * are the caller's in both halves), SMART_PARTICLE_STATES = 12 states states_in[i][0 .. 12) (SmartEnsemble.initial of the
 * next window; columns 7 .. 18 of final_vars of the last) and a log-weight logw_in[i].
 *
 * WEIGH (phase SMART_PARTICLE_WEIGH).  With sim[t][i] = sim[t * ld_sim + i] the window's discharge where the launch left it,
 * t < Rw = n_reports, and obs[t] (NaN: missing), over the observed t in ascending order, each operation rounded once:
 *     sigma_t = sigma0 + sigma1 |obs_t|;   r = (sim_ti - obs_t) / sigma_t;   s = s + r r      from s = 0
 *     l_i = -0.5 s;   logw'_i = logw_i + l_i,  or -inf where sim_ti is not finite at an observed t
 * (what sim holds at a step that is not observed is never looked at).  logw' is written to logw_out.
 * QUANTISE.  m' = the largest finite logw'; q_i = rint(2^22 exp(logw'_i - m')) as an integer, 0 where logw'_i is not finite
 * (exp is the one operation here that is not correctly rounded: its last bit moves 2^22 e by far less than 1).  No finite
 * logw' at all: the flag SMART_PARTICLE_FLAG_DEGENERATE, q_i = 2^22 for every particle, the particles are kept and logw_out
 * = 0.  No observed t in the window: the flag SMART_PARTICLE_FLAG_NO_OBS; logw' = logw bit for bit and nothing is resampled.
 * The same integers q0_i are made of logw (maximum m, sum Q0; all 0 where no logw is finite).  From here on everything is
 * integers, so no order of summation can matter: Q = sum q_i <= 2^41, S2 = sum q_i^2 <= 2^63 (unsigned), C_i = the
 * inclusive prefix sums of q.  q[N] (int64) is an output: as doubles, the weights of the analysis.
 * With q_in (int64 [N], each in 0 .. 2^22) the window is not weighed: q = q_in, logw' = logw_in, DEGENERATE iff Q = 0 (q
 * stays 0), and the evidence and the two maxima are NaN.  sim and obs are not read.
 * DECIDE.  ess = fl(fl(double(Q) double(Q)) / double(S2)); resampled iff no flag is set and ess < fl(tau double(N)).
 * RESAMPLE (phase SMART_PARTICLE_RESAMPLE), systematic.  With u = u53(w0, w1) of the Philox4x32-10 words of the counter
 * (2^32 - 1, k, 0, 0) under the key (seed mod 2^32, seed div 2^32) -- u53 as for smart_demcz_step_hip --
 *     rho = min(offset >= 0 ? offset : floor(fl(u double(Q))), Q - 1);    a_j = #{i : N C_i <= j Q + rho}     (parents[j])
 * in unsigned 64-bit integers (every product stays below 2^60).  A particle with q = 0 has no child, particle i has
 * floor(N q_i / Q) or that plus one.  Without resampling a_j = j.  counts[SMART_PARTICLE_DISTINCT] = the number of
 * particles with a child.
 * MOVE (phase SMART_PARTICLE_MOVE) of child j from its parent p = a_j, resampled or not.
 *   Parameters: the jitter and the box of the generational samplers (smart_demcz_step_hip, with a difference of weight 0).
 *     For a dimension c whose scale_c is not 0, with (w0, w1, w2, w3) the words of the counter (j, k, 2 + c, 0):
 *         eps = scale_c (2 u53(w1, w2) - 1);   t = 0 + eps;   y = theta_p,c + t
 *         if y < lo_c: y = 2 lo_c - y;   if y > hi_c: y = 2 hi_c - y
 *     and where a y is still outside its [lo_c, hi_c] (or NaN) the child takes the parent's whole row.  A dimension whose
 *     scale_c is 0 is copied.  rows_out[j][columns[c]] is written for every c < d; the other columns are not touched.
 *   States, s < 12, with the words of the counter (j, k, 18 + s div 2, 0), (w0, w1) for an even s and (w2, w3) for an odd:
 *         f = 2 u53(.,.);  f = f - 1;  f = noise_s f;  f = 1 + f;  x' = x_p,s f               0 <= noise_s < 1
 *     then the six soil layers s = SMART_PARTICLE_FIRST_LAYER .. + 5 are held below their capacity (above it the model
 *     overflows): cap = ((Z' / 6) / 1e3) area_m2, x' = x' > cap ? cap : x', Z' the child's value of column z_column of the
 *     launch matrix (the parent's where that column does not vary).
 *   logw_out[j] = 0 where the step resampled or is DEGENERATE, else logw'_j.
 * THE HEADER, on the device: stats[4] (doubles) = ess, the evidence increment log(sum w_prev e^l) = (m' + ln(Q / 2^22)) -
 * (m + ln(Q0 / 2^22)), m', m; counts[8] (int64) = resampled (0 / 1), Q, distinct parents, flags, rho, S2, Q0, 0.  The
 * RESAMPLE and MOVE phases read it there.
 * PHASES.  `phases` is a mask; a call with all three is the step.  A call without WEIGH uses what an earlier call with it
 * left in the workspace, q, stats and counts (and is given the same q_in); MOVE without RESAMPLE reads parents[].
 * lo, hi, scale (d values), noise (12) and columns (d) are HOST arrays (they travel as kernel arguments).
 *
 * Errors (all found before the device is touched; the first offending argument wins): SMART_E_NULL logw_in, logw_out, q,
 * parents, stats, counts or workspace missing; SMART_E_SIZE n_particles outside 1 .. 2^19, n_dims outside 1 .. 16, step
 * outside 0 .. 2^32 - 1, SMART_E_MODE phases outside 1 .. 7; weigh phase: SMART_E_SIZE tau not finite or < 0, offset >=
 * 2^41, and without q_in SMART_E_NULL sim or obs missing, SMART_E_SIZE n_reports outside 1 .. 2^31 - 1, ld_sim < n_particles,
 * sigma0 not finite or <= 0, sigma1 not finite or < 0; move phase: SMART_E_NULL rows_in, rows_out, states_in, states_out,
 * lo, hi, scale, noise or columns missing, SMART_E_SIZE ld < n_dims, a column outside 0 .. ld - 1 or named twice, bounds that
 * are not finite or lo > hi, z_column outside 0 .. ld - 1, a scale that is not finite or < 0, a noise outside [0, 1), area_m2
 * not finite or <= 0; SMART_E_SIZE a workspace of fewer than smart_particle_workspace_bytes bytes; then SMART_E_NO_DEVICE
 * without a HIP device.
 */
#define SMART_PARTICLE_MAX_PARTICLES 524288
#define SMART_PARTICLE_MAX_DIMS 16
#define SMART_PARTICLE_STATES 12
#define SMART_PARTICLE_FIRST_LAYER 5
#define SMART_PARTICLE_WEIGH 1
#define SMART_PARTICLE_RESAMPLE 2
#define SMART_PARTICLE_MOVE 4
#define SMART_PARTICLE_FLAG_DEGENERATE 1
#define SMART_PARTICLE_FLAG_NO_OBS 2
#define SMART_PARTICLE_ESS 0
#define SMART_PARTICLE_EVIDENCE 1
#define SMART_PARTICLE_MAX 2
#define SMART_PARTICLE_MAX_PRIOR 3
#define SMART_PARTICLE_RESAMPLED 0
#define SMART_PARTICLE_Q 1
#define SMART_PARTICLE_DISTINCT 2
#define SMART_PARTICLE_FLAGS 3
#define SMART_PARTICLE_OFFSET 4
#define SMART_PARTICLE_S2 5
#define SMART_PARTICLE_Q_PRIOR 6
int smart_particle_step_hip(int64_t n_particles, int32_t n_dims, uint64_t seed, int64_t step, int32_t phases,
                            int64_t n_reports, const double *sim, int64_t ld_sim, const double *obs, double sigma0,
                            double sigma1, double tau, const int64_t *q_in, int64_t offset, const double *rows_in,
                            double *rows_out, int64_t ld, const int32_t *columns, int32_t z_column, double area_m2,
                            const double *lo, const double *hi, const double *scale, const double *noise,
                            const double *states_in, double *states_out, const double *logw_in, double *logw_out,
                            int64_t *q, int32_t *parents, double *stats, int64_t *counts, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* The workspace smart_particle_step_hip asks for, in bytes: six values per block of 256 particles for 2048 blocks, and the
 * 32-bit prefix sums of the integers inside a block (96 KiB + 4 N rounded up to blocks).  SMART_E_SIZE (negative) for an
 * n_particles the entry refuses.  Needs no device. */
int64_t smart_particle_workspace_bytes(int64_t n_particles);

/*
 * Sampling database, CSV flavour -- the rows MonteCarlo.save writes one by one (montecarlo.py:211-231): every value
 * cast to float32 and printed '%.6e', comma separated, one '\n'-terminated line per sample.  HOST pointers, no
 * device involved.  Appends n_rows lines of n_cols values (row-major float32 table: objective functions, parameters,
 * optionally the simulated series -- the caller writes the header line, montecarlo.py:122-127) to `path`.
 * n_threads <= 0: one per core, at most 16.  Characters identical to Python's '%.6e' % numpy.float32(x).
 */
int smart_db_append_rows(const char *path, const float *table, int64_t n_rows, int64_t n_cols, int32_t n_threads);

/*
 * ... and reading them back: GLUE / Best / Total take their sample from an LHS database (montecarlo.py:233-262,
 * DictReader + numpy.array(rows, dtype=float32)).  `text` = the file's bytes after the header line, `len` of them;
 * every line holds n_cols values; the n_use columns listed in `cols` (indices into the header) are parsed
 * (text -> correctly rounded double -> float32, as numpy does) into out[row][0..n_use).  Returns the number of rows
 * (<= max_rows) or a negative SMART_E_* code.
 */
int64_t smart_db_parse_rows(const char *text, int64_t len, int64_t n_cols, const int32_t *cols, int32_t n_use,
                            float *out, int64_t max_rows, int32_t n_threads);

/* The arithmetic class of ONE parameter row -- 0 regular, 1 stiff, 2 guard, 3 ill-conditioned / literal: the c of the
 * SMART_PLAN_CLASS_* bit (1 << c) its kernel answers to -- worked out on the host with the rules the kernels apply on
 * the device (smart_fast_model.h: wave_class).  params[10] as lhs.py:114 lays them out; initial12: the twelve initial
 * states of the row, or NULL (the reference's half-full soil / educated guess, structure.py:97-140); area_m2 is read with
 * initial12 only.  Pure host code, no device needed.  smart_allsteps_hip classifies its one row with it (ABI 6); a
 * caller that launches one row at a time can fill SmartEnsemble.plan the same way:
 *   plan = SMART_PLAN_VALID | (forcing bits of an earlier smart_plan_ensemble) | (1 << smart_row_class(...)).
 * The device stays authoritative: a row this call misjudges meets no kernel and raises SMART_STATUS_STALE_PLAN. */
int smart_row_class(const double *params, double delta_sec, const double *initial12, double area_m2);

/* Device bookkeeping */
int smart_device_count(void);           /* number of visible HIP devices (0 if none / no driver)      */
int smart_abi_version(void);            /* SMART_AMD_ABI_VERSION the library was built with           */
const char *smart_build_info(void);     /* the compiler that built the library, the ABI, and the stamp of the build's code lint:
                                         * "hipcc <HIP version> | clang <version> | gfx950 | ABI 7 | SMART_LINT_STAMP=pairs-ok"
                                         * (smartpy_amd.build writes the stamp into the file it has linted; "unchecked": a
                                         * build by another route -- the step loops then run without computed jumps unless
                                         * the environment says SMART_PAIR_BLOCKS=1) */
const char *smart_last_error(void);     /* text of the calling thread's last error ("" if none)       */

#ifdef __cplusplus
}
#endif
#endif /* SMART_AMD_H */
