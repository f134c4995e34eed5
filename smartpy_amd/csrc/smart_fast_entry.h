// smart_fast_entry.h -- the kernels of SMART_MATH_FAST, one __global__ per arithmetic variant.
//
// Round 1 had ONE kernel that held every variant behind a wave-uniform switch; it was allocated the registers of
// its hungriest branch (189 VGPRs, 209 spilled SGPRs: two wavefronts per SIMD for everything).  Each variant is now
// its own kernel with its own register allocation (profiles/r02_kernel_resources.txt), launched over the same grid:
// a workgroup classifies its 64 parameter rows (wave_class) and returns at once unless they belong to its kernel.
// The host launches only the kernels a call can need (report type, gap, outputs; and, with a plan from
// smart_plan_ensemble, only the classes actually present) -- concurrently, on forked streams, when there are several.
//
//   kernel                       rows / forcing it takes                                         body
//   smart_fast_intervals_exits   class 0, summary, gap >= 2, piecewise-constant forcing          interval engine, early exits
//   smart_fast_intervals         same, for launches with <= 2 blocks of 64 samples per SIMD    interval engine, straight-line
//   smart_fast_intervals_states  same, final state vector asked for                              interval engine, SPLIT
//   smart_fast_runs(_exits)      same as the two above for forcing constant over runs of k steps,  interval engine over runs
//   smart_fast_runs_states       k >= 2 a divisor of the gap (e.g. 6-hourly data, hourly steps)     ... SPLIT
//   smart_fast_steps             class 0, summary, gap >= 2, forcing varying inside the interval step loop, merged
//   smart_fast_steps_states      same, final state vector asked for                              step loop, SPLIT
//   smart_fast_steps_raw         class 0, raw reports, gap >= 2 (W, T multiples of it)           step loop, last-step routing
//   smart_fast_intervals_raw     same over piecewise-constant forcing                            interval engine, n - 1 + 1 steps
//   smart_fast_steps_every       class 0, a report every step (gap 1)                            single-step arms + report
//   smart_fast_plain             class 0, what is left: raw reports over a ragged time axis, raw   step loop (unsliced)
//                                or every-step reports with the final state vector
//   smart_fast_stiff             class 1: some k * 3600 < dt (clamps, 95 % rule reachable)        step loop, STIFF
//   smart_fast_guard             class 2: S outside [0, 0.5], C < 0 or Z <= 0                     step loop, GUARD
//   smart_fast_illcond           class 3: dt / (RK * 3600) > 2 (the river only), few blocks      literal model, one sample per
//                                                                                                 DPP row (latency form)
//   smart_fast_illcond_lanes     class 3, many blocks (round 6: chosen per launch from the load)  literal model, one sample per
//                                                                                                 lane, cached reciprocals
#pragma once

#include "smart_fast_model.h"

namespace smart {

// THE list of the fast kernels: enum id, __global__ symbol, arithmetic class (wave_class), whether the kernel belongs to a
// family of time-sliced kernels, and the workgroups it runs per block of 64 samples.  The enum, the declarations and
// (smart_capi.hip) the handles, the names smart_describe_launch prints and what a launch does with each follow from it.
#define SMART_FAST_KERNELS(X)                                                                                          \
    X(kIntervalsExits, smart_fast_intervals_exits, 0, true, 1)                                                         \
    X(kIntervals, smart_fast_intervals, 0, true, 1)                                                                    \
    X(kIntervalsStates, smart_fast_intervals_states, 0, true, 1)                                                       \
    X(kSteps, smart_fast_steps, 0, true, 1)                                                                            \
    X(kStepsStates, smart_fast_steps_states, 0, true, 1)                                                               \
    X(kPlain, smart_fast_plain, 0, false, 1)                                                                           \
    X(kStiff, smart_fast_stiff, 1, false, 1)                                                                           \
    X(kGuard, smart_fast_guard, 2, false, 1)                                                                           \
    X(kIllCond, smart_fast_illcond, 3, false, kIllCondWaves)                                                           \
    X(kRunsExits, smart_fast_runs_exits, 0, true, 1)                                                                   \
    X(kRuns, smart_fast_runs, 0, true, 1)                                                                              \
    X(kRunsStates, smart_fast_runs_states, 0, true, 1)                                                                 \
    X(kStepsRaw, smart_fast_steps_raw, 0, true, 1)                                                                     \
    X(kIntervalsRaw, smart_fast_intervals_raw, 0, true, 1)                                                             \
    X(kStepsEvery, smart_fast_steps_every, 0, true, 1)                                                                 \
    X(kIllCondLanes, smart_fast_illcond_lanes, 3, false, 1)

#define SMART_FAST_KERNEL(name)                                                                                        \
    __global__ __launch_bounds__(kWave) void name(KArgs a, const double2 *__restrict__ forcing,                        \
                                                  const double *__restrict__ obs, const double *__restrict__ ws)

enum FastKernel : int {
#define X(id, symbol, cls, sliced, waves) id,
    SMART_FAST_KERNELS(X)
#undef X
    kNumFastKernels
};

// (each kernel is defined in one of the smart_fast_*.hip units; smart_capi.hip launches them from these declarations)
#define X(id, symbol, cls, sliced, waves) SMART_FAST_KERNEL(symbol);
SMART_FAST_KERNELS(X)
#undef X

// ticket counters of the families of time-sliced kernels (workspace header, claim_work): at most one kernel of a
// family runs in a call
constexpr int kTicketIntervals = 0, kTicketSteps = 1, kTicketRuns = 2, kTicketStepsRaw = 3, kTicketIntervalsRaw = 4,
              kTicketEvery = 5;
static_assert(kHdrTicket + kTicketEvery < kHdrPlan, "the tickets end in front of the plan word of smart_plan_ensemble");

// Do this block's 64 rows belong to the kernel of class CLS?  A block whose class has no kernel in this call (the
// caller's plan is stale) is reported through the status word by whichever kernel meets it first.
template <int CLS>
__device__ __forceinline__ bool block_is_mine(const KArgs &a, const Work &w)
{
    const int cls = wave_class(a, w.block, w.c);
    if (cls == CLS)
        return true;
    if (w.seg == 0 && !((a.class_mask >> cls) & 1))
        raise_status(a, kStatusStalePlan);
    return false;
}

// Class-0 summary runs: is this catchment's forcing the kind this kernel takes?  Answered by smart_forcing_scan
// before the launch (a.fflags); without a workspace every wavefront scans the forcing itself.
template <int FORCING>
__device__ __forceinline__ bool forcing_is_mine(const KArgs &a, int fflags, const Work &w)
{
    const int kind = forcing_kind(a, fflags);
    if (kind == FORCING)
        return true;
    if (w.seg == 0 && !(a.pc_mask & pc_bit(kind)))
        raise_status(a, kStatusStalePlan);
    return false;
}

template <class Model, int FORCING, int REPORT = kReportMean>
__device__ __forceinline__ void merged_kernel(const KArgs &a, const double2 *__restrict__ forcing,
                                              const double *__restrict__ obs, const double *__restrict__ ws)
{
    constexpr int ticket = REPORT == kReportEvery  ? kTicketEvery
                           : REPORT == kReportLast ? (FORCING == kForcingIntervals ? kTicketIntervalsRaw : kTicketStepsRaw)
                           : FORCING == kForcingIntervals ? kTicketIntervals
                                                          : (FORCING == kForcingVarying ? kTicketSteps : kTicketRuns);
    const Work w = claim_work(a, ticket);
    if (!block_is_mine<0>(a, w))
        return;
    const int fflags = forcing_flags(a, forcing, w.c);
    if constexpr (REPORT == kReportLast && FORCING == kForcingVarying) {
        // the step loop of raw reports takes every forcing the interval engine does not (varying, and constant over runs
        // shorter than the report interval: there is no run engine for raw reports)
        if (forcing_kind(a, fflags) == kForcingIntervals) {
            if (w.seg == 0 && !(a.pc_mask & kPcIntervals))
                raise_status(a, kStatusStalePlan);
            return;
        }
    } else if constexpr (REPORT != kReportEvery) { // (a report every step: one kernel whatever the forcing)
        if (!forcing_is_mine<FORCING>(a, fflags, w))
            return;
    }
#ifdef SMART_SLICE_TIMELINE
    timeline_note(a, w.block, w.c, w.seg, 0, (unsigned long long)(w.seg * a.seg_blocks + w.c * a.n_blocks + w.block));
    timeline_note(a, w.block, w.c, w.seg, 1,
                  (unsigned long long)__builtin_amdgcn_s_getreg(63492) // HW_ID [31:0]
                      | (unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32); // XCC_ID [31:0]
    timeline_note(a, w.block, w.c, w.seg, 2, __builtin_amdgcn_s_memrealtime());
#endif
    run_ensemble_merged<Model, FORCING, REPORT>(a, forcing, obs, ws, w.block, w.c, w.seg, fflags);
#ifdef SMART_SLICE_TIMELINE
    timeline_note(a, w.block, w.c, w.seg, 4, __builtin_amdgcn_s_memrealtime());
#endif
}

} // namespace smart
