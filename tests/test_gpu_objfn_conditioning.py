"""The objective functions where the first report is unobserved: smart_objfn_hip, smart_objfn_windows_hip,
smart_objfn_bootstrap_hip and the fused moments of the time-loop kernels against the exact scores of
oracle/analyses/objfn.py.

Every result is held to `truth` (fractions.Fraction over the observed rows) within `bounds(..., the first observed row)`:
what any order of the kernel's float64 additions may differ by when the one-pass moments are taken about the sample's
value at the FIRST REPORT THAT CARRIES AN OBSERVATION -- of the matrix, of the window, of the launch for the bootstrap.
The pattern of NaN and of infinities is equal.  The cases and their data are the host module's, where they are held to
the conditions that make this module bite: about the first observed row every bound is below the suite's 1e-9 gate, and
about row 0 some entry of every case with r1 > 0 misses its bound a hundredfold -- a kernel that takes its constant from
an unobserved report 0 (a flood before the gauge begins, a start-up value, a NaN) fails here.

The fused moments of every time-loop kernel are held the same way, against truth on the discharge the same launch
stored (second half of the module).  The flow-duration scores are held to the same truth in
tests/test_gpu_flow_duration_truth.py: their constant is the first in-segment rank, and a constant from elsewhere fails there.

The largest used fraction of the bound per path is printed at the end of the module (and written to
$SMART_MARGINS_DIR/objfn_conditioning_margins.txt where that is set); profiles/objfn_conditioning_margins.txt is that
table."""
import os

import numpy as np
import pytest

import support
from support import Margins, margins_dir, padded, eng      # noqa: F401 (eng is a fixture)
from cases_objfn import (BIG_CASE, EPS, MATRIX_CASES, SPECIAL_CASES, WINDOW_CASES, big_columns, bootstrap_case, compared,
                         inside_and_below_the_gate, matrix_case, window_case)
from oracle.analyses.objfn import bootstrap_reference, bounds, emulate, first_observed, kappa, truth, window_reference

pytestmark = pytest.mark.gpu

PAD = 3             # ld = N + 3, the padding holds NaN
MARGINS = Margins()
PATHS = ['smart_objfn_hip', 'smart_objfn_hip, one lane per sample', 'smart_objfn_windows_hip none',
         'smart_objfn_windows_hip sqrt', 'smart_objfn_windows_hip log', 'smart_objfn_windows_hip inverse',
         'smart_objfn_bootstrap_hip point', 'smart_objfn_bootstrap_hip jackknife']


def on_device(sim):
    """[R, N] host matrix -> the [R, N] view of a device matrix with ld = N + PAD whose padding holds NaN"""
    return padded(sim, PAD)[0][:, :sim.shape[1]]


def hold(path, what, got, want, bnd):
    """the pattern of NaN and infinities equal, every finite entry within its bound; the used fraction is kept"""
    support.hold(MARGINS, path, what, got, want, bnd)


@pytest.fixture(scope='module', autouse=True)
def _print_the_margins():
    yield
    if not MARGINS:
        return
    text = ('largest |result - truth| of this run as a fraction of bounds(..., first observed row) of '
            'oracle/analyses/objfn.py (truth in fractions.Fraction; the bound is what any order of the float64 '
            'additions may differ by): path, fraction, where it was seen\n' +
            '\n'.join('%-38s %-10.3g %s' % (p, MARGINS[p][0], MARGINS[p][1])
                      for p in PATHS + sorted(set(MARGINS) - set(PATHS)) if p in MARGINS) + '\n')
    MARGINS.publish(text, margins_dir(), 'objfn_conditioning_margins.txt')


# ---- smart_objfn_hip ---------------------------------------------------------------------------------------------------
def objfn(sim, obs):
    from smartpy_amd import engine
    out = engine.objective_functions(on_device(sim), obs).cpu().numpy()
    assert out.shape == (sim.shape[1], 8) and np.isnan(out[:, 7]).all()         # no groundwater constraint was given
    return out[:, :7]


def two_pass(sim, obs):
    """[n, 7]: the scores of every column in the two-pass float64 form of oracle/objfn_oracle.py, all columns at once"""
    seen = ~np.isnan(obs)
    e, s = obs[seen][:, None], sim[seen]
    de, ds, d = e - e.mean(), s - s.mean(axis=0), s - e
    cc = (de * ds).sum(axis=0) / np.sqrt((ds * ds).sum(axis=0) * (de * de).sum())
    alpha, beta = np.sqrt((ds * ds).mean(axis=0) / (de * de).mean()), s.sum(axis=0) / e.sum()
    kge = 1.0 - np.sqrt((cc - 1.0) ** 2 + (alpha - 1.0) ** 2 + (beta - 1.0) ** 2)
    return np.stack([1.0 - (d * d).sum(axis=0) / (de * de).sum(), kge, cc, alpha, beta, 100.0 * d.sum(axis=0) / e.sum(),
                     np.sqrt((d * d).mean(axis=0))], axis=1)


@pytest.mark.parametrize('R,N,r1', MATRIX_CASES)
def test_matrix_kernel_about_the_first_observed_report(R, N, r1):
    sim, obs, _ = matrix_case(R, N, r1)
    assert first_observed(obs) == r1
    hold('smart_objfn_hip', 'R=%d N=%d r1=%d' % (R, N, r1), objfn(sim, obs), truth(sim, obs), bounds(sim, obs, r1))


@pytest.mark.parametrize('R,N,r1,row', SPECIAL_CASES)
def test_matrix_kernel_never_sees_an_unobserved_nan_inf_or_1e308(R, N, r1, row):
    sim, obs, info = matrix_case(R, N, r1, row)
    assert np.isnan(obs[row]) and sorted(info['special']) == ['1e308', 'inf', 'nan']
    want = truth(sim, obs)
    assert np.isfinite(want).all()
    hold('smart_objfn_hip', 'R=%d N=%d r1=%d, NaN, +inf, 1e308 at row %d' % (R, N, r1, row), objfn(sim, obs), want,
         bounds(sim, obs, r1))


def test_matrix_kernel_with_one_lane_per_sample():
    R, N, r1 = BIG_CASE
    sim, obs, _ = matrix_case(R, N, r1)
    cols = big_columns(N)
    got = objfn(sim, obs)
    assert np.isfinite(got).all()
    # every column against the two-pass float64 statement at the suite's gate (a lane or a workgroup that reads its
    # neighbour's column shows here), the columns of big_columns against truth within the bound
    want = two_pass(sim, obs)
    keep = np.abs(want) >= 1e-6
    assert np.max(np.abs(got - want)[keep] / np.abs(want)[keep]) < 1e-9 and keep.mean() > 0.98
    hold('smart_objfn_hip, one lane per sample', 'R=%d N=%d r1=%d, %d columns' % (R, N, r1, cols.size), got[cols],
         truth(sim[:, cols], obs), bounds(sim[:, cols], obs, r1))


# ---- smart_objfn_windows_hip -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,transform', WINDOW_CASES)
def test_windows_kernel_about_each_windows_first_observed_report(name, transform):
    from smartpy_amd import engine
    sim, obs, win, W = window_case(name, transform)
    got = engine.objective_functions_windows(on_device(sim), obs, win, n_windows=W, transform=transform,
                                             eps=EPS[transform]).cpu().numpy()
    want, bnd = window_reference(sim, obs, win, W, transform)
    assert np.isfinite(want).all()
    hold('smart_objfn_windows_hip ' + transform, '%s, W=%d' % (name, W), got, want, bnd)


# ---- smart_objfn_bootstrap_hip -----------------------------------------------------------------------------------------
def test_bootstrap_point_and_jackknife_about_the_launchs_first_valid_row():
    """The replicate that leaves out the window holding that row (replicate 0) sums no row near its constant: it is held
    to the bound that says so, the others to theirs."""
    from smartpy_amd import engine
    sim, obs, win, W = bootstrap_case()
    counts = engine.jackknife_counts(W)
    assert counts.shape == (W, W) and counts[0, 0] == 0 and counts[0, 1:].all()
    res = engine.objective_functions_bootstrap(on_device(sim), obs, win, counts, n_windows=W, replicates=True)
    every = np.concatenate([np.ones((1, W), dtype=np.int64), counts.astype(np.int64)])
    want, bnd, r0 = bootstrap_reference(sim, obs, win, every)
    assert win[r0] == 0
    what = 'R=%d N=%d W=%d' % (sim.shape[0], sim.shape[1], W)
    hold('smart_objfn_bootstrap_hip point', what, res.point.cpu().numpy(), want[0], bnd[0])
    reps = np.transpose(res.replicates.cpu().numpy(), (0, 2, 1))               # [B, 7, N] -> [B, N, 7]
    hold('smart_objfn_bootstrap_hip jackknife', what + ', without the window of row %d' % r0, reps[:1], want[1:2], bnd[1:2])
    hold('smart_objfn_bootstrap_hip jackknife', what + ', the other replicates', reps[1:], want[2:], bnd[2:])


# ---- the fused moments of the time-loop kernels ------------------------------------------------------------------------
# A storm in the first day and no warm-up; the observations begin later -- on the last quarter of the reports ('late'), or
# from report 1 on ('from_1').  Truth is taken on the discharge the SAME launch stored, so the model's arithmetic does not
# enter; the constant is the sample's value at the first observed report r1.  Every kernel that reports is reached the way
# tests/golden/make_forcing_signs.py reaches it (LAUNCHES, SLICED, DAILY_CLASSES), each launch asserting its describe().
#
# What report 0 holds, and so what follows the storm (figures of oracle/smart_oracle.py on the inputs of this module, N =
# 65, 40 and 80 days):
#   daily means and raw reports every 24 steps: the flood itself (the mean of day 0, 14 to 16 m3/s in row 0; step 23 of it,
#     34 to 39 m3/s).  No rain follows, the observed stretch is the recession: kappa about report 0 is 3.2e6 to 6.6e6 for
#     the daily means and 2.4e7 to 4.1e7 for the raw reports, and the float64 emulation of the sums about report 0 misses
#     the bound 1.7e4 to 9.6e5 times.
#   a report of ONE step (a report every step, raw reports every 7 steps, the daily classes): the start-up flow of step 0,
#     3.0 m3/s, before the storm has reached the outlet.  A recession does not stay far from that (kappa 1e3 to 6e3, a
#     miss of 3 to 42 bounds), so steady rain follows the storm there -- STEADY_RAIN, DAILY_STEADY_RAIN -- and the observed
#     stretch settles near an equilibrium far above 3.0: kappa 1.2e7 to 1.4e9 (hourly) and 1.4e7 to 8.4e9 (daily classes),
#     a miss of 1.5e4 to 1.4e8 bounds.  In the six-hourly and the varying form the steady part keeps the form's pattern at
#     RIPPLE of its size: every six hours, every step still has a value of its own, which is what picks the kernel.
# 'late' therefore sees a constant taken from report 0 in every kernel: kappa > 1e6 and a hundredfold miss of the
# emulation about report 0 are asserted on the stored discharge of every such launch, with conditions (b) and (d) of
# oracle/analyses/objfn.py.
# 'from_1' CANNOT see it and is here for the r1 = 1 control path alone -- the constant set twice, one report apart, whole
# and across slices, bit for bit with and without the stored matrix.  The series that follows report 0 at once still holds
# the flood's recession or the rise to the equilibrium: kappa about report 0 is 11 to 152 there and the emulation about it
# stays at 0.01 to 0.48 of the bound.  A value one report old does not lie a thousand spreads away from the 39 to 1,919
# reports that follow it under any forcing tried, so nothing is asserted of kappa there; it is printed.
import functools                    # noqa: E402
import importlib.util               # noqa: E402

_spec = importlib.util.spec_from_file_location(
    'make_forcing_signs', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'make_forcing_signs.py'))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

STORM_RAIN, STORM_PE = 40.0, 0.02   # mm per hour on the first day; every hour
STEADY_RAIN = 3.0                   # mm per hour after the storm where a report is one step of an hourly run
DAILY_STEADY_RAIN = 20.0            # the same for the daily classes (times 24: mm per day)
RIPPLE = 1e-3
ONE_STEP_REPORTS = ('every', 'raw7')
FUSED_N = 65
SETUPS = ('late', 'from_1')


@functools.lru_cache(maxsize=None)
def storm(form, days, steady=0.0, per_day=1.0):
    """[days * 24, 2] hourly in the three forms of make_forcing_signs.forcing (per_day = 24: [days, 2] in mm per day): the
    storm on day 0, `steady` mm per hour of rain from day 1 on.  With steady > 0 the pattern of the form -- the weights of
    the four six-hour values, the factor of every step -- is kept in full on day 0 and at RIPPLE of its size after it."""
    daily = np.zeros((days, 2))
    daily[:, 0], daily[:, 1] = steady, STORM_PE
    daily[0, 0] = STORM_RAIN
    if per_day != 1.0:
        return np.ascontiguousarray(daily * per_day)
    calm = RIPPLE if steady > 0.0 else 1.0
    f = np.repeat(daily, 24, axis=0)
    if form == 'six_hourly':
        rain_w = np.tile([0.4, 0.0, 0.35, 0.25], (days, 1))
        pe_w = np.tile([0.1, 0.4, 0.4, 0.1], (days, 1))
        rain_w[1:] = 0.25 + calm * (rain_w[1:] - 0.25)
        pe_w[1:] = 0.25 + calm * (pe_w[1:] - 0.25)
        f = np.stack([np.repeat((daily[:, 0:1] * 24 * rain_w).ravel() / 6, 6),
                      np.repeat((daily[:, 1:2] * 24 * pe_w).ravel() / 6, 6)], axis=1)
    elif form == 'varying':
        factor = np.random.default_rng(63).uniform(0.0, 2.0, (len(f), 1))
        factor[24:] = 1.0 + calm * (factor[24:] - 1.0)
        f = f * factor
    else:
        assert form == 'piecewise', form
    return np.ascontiguousarray(f)


def late_observations(R, setup, seed=0):
    """-> (obs [R], r1): a recession under log-normal noise, with 10 % of the later reports missing as well"""
    rng = np.random.default_rng(100 + seed)
    r1 = R - R // 4 if setup == 'late' else 1
    obs = (1.0 + 4.0 * np.exp(-np.arange(R) / (R / 3.0))) * np.exp(rng.normal(0.0, 0.2, R))
    gone = rng.random(R) < 0.1
    gone[[r1, R - 1]] = False
    obs[gone] = np.nan
    obs[:r1] = np.nan
    return obs, r1


def hold_fused(kernel, what, objfn, discharge, obs, r1, setup):
    """the seven scores of a launch against truth on the discharge [n, R] it stored; the conditions on that discharge"""
    sim = np.ascontiguousarray(discharge.T)
    assert first_observed(obs) == r1 and np.isfinite(sim).all()
    want, bnd = truth(sim, obs), bounds(sim, obs, r1)
    # every bound finite, below the suite's gate, at most 2 % of the entries too small to compare: (b) and (d)
    assert inside_and_below_the_gate(want, bnd, what) == want.size, what
    k0 = float(np.max(kappa(sim, obs, 0)))
    miss = float(np.max(np.where(compared(want), np.abs(emulate(sim, obs, 0) - want) / bnd, 0.0)))
    print('%s: %s: kappa about report 0 up to %.3g, about report %d up to %.3g; the emulation about report 0 at %.3g of '
          'the bound' % (kernel, what, k0, r1, float(np.max(kappa(sim, obs, r1))), miss))
    assert setup in SETUPS, setup
    if setup == 'late':
        assert k0 > 1e6, (what, k0)
        assert miss >= 100.0, (what, miss)                                                   # (c)
    hold('fused ' + kernel, what, objfn[:, :7], want, bnd)


def fused_launch(eng, name, days, setup, store, time_slices=0):
    _, form, report_kind, final, exits, kernel = cases.LAUNCH[name]
    report, gap = cases.REPORTS[report_kind]
    obs, r1 = late_observations(cases.n_reports(days * 24, report_kind), setup)
    f = storm(form, days, STEADY_RAIN if report_kind in ONE_STEP_REPORTS else 0.0)
    got, what = cases.launch(eng, cases.parameters(FUSED_N), f, 0, report, gap, exits=exits, obs=obs,
                             want_final=final, want_discharge=store, time_slices=time_slices)
    assert kernel in what and ' + ' not in what, what
    return got, obs, r1, kernel.rstrip('['), what


@pytest.mark.parametrize('name', [l[0] for l in cases.LAUNCHES])
def test_fused_moments_of_every_hourly_kernel(eng, name):
    """40 days; with the discharge stored the scores are held to truth on it, and without it they are the same bits"""
    for setup in SETUPS:
        got, obs, r1, kernel, what = fused_launch(eng, name, 40, setup, True)
        hold_fused(kernel, '%s %s: %s' % (name, setup, what), got['objfn'], got['discharge'], obs, r1, setup)
        alone, _, _, _, text = fused_launch(eng, name, 40, setup, False)
        assert 'discharge' not in alone, text
        assert np.array_equal(alone['objfn'].view(np.int64), got['objfn'].view(np.int64)), (name, setup, what, text)


@pytest.mark.parametrize('name', cases.SLICED)
def test_fused_moments_whole_and_in_time_slices(eng, name):
    """80 days (the length the library cuts): whole, in 2 and in 5 time slices, the first observed report inside a later
    slice; every one against truth, and the sliced launches the bits of the whole one"""
    for setup in SETUPS:
        whole = None
        for asked in (1, 2, 5):
            got, obs, r1, kernel, what = fused_launch(eng, name, 80, setup, True, time_slices=asked)
            assert ('[%d slices' % asked in what) == (asked > 1) and ('slices' in what) == (asked > 1), what
            hold_fused(kernel, '%s %s: %s' % (name, setup, what), got['objfn'], got['discharge'], obs, r1, setup)
            whole = got if whole is None else whole
            assert np.array_equal(got['objfn'].view(np.int64), whole['objfn'].view(np.int64)), (name, setup, what)


@pytest.mark.parametrize('literal_form', ['rows', 'lanes'])
def test_fused_moments_of_the_daily_classes(eng, literal_form):
    """dt = 86400 s, a report every step: smart_fast_steps_every, smart_fast_stiff, smart_fast_guard and the literal rows in
    both forms side by side, every row against truth on its own stored discharge"""
    params, cls = cases.daily_parameters()
    f = storm('piecewise', cases.DAILY_STEPS, DAILY_STEADY_RAIN, per_day=24.0)
    kernels = ['smart_fast_steps_every', 'smart_fast_stiff', 'smart_fast_guard',
               'smart_fast_illcond' if literal_form == 'rows' else 'smart_fast_illcond_lanes']
    for setup in SETUPS:
        obs, r1 = late_observations(cases.DAILY_STEPS, setup)
        got, what = cases.launch(eng, params, f, 0, 'summary', 1, dt=86400.0, obs=obs, literal_form=literal_form)
        assert all(k + '[' in what for k in kernels) and what.count(' + ') == 3, what
        alone, _ = cases.launch(eng, params, f, 0, 'summary', 1, dt=86400.0, obs=obs, literal_form=literal_form,
                                want_discharge=False)
        assert np.array_equal(alone['objfn'].view(np.int64), got['objfn'].view(np.int64)), (setup, what)
        for c, kernel in enumerate(kernels):
            rows = np.flatnonzero(cls == c)
            hold_fused(kernel, 'daily steps, %s rows, %s: %s' % (cases.DAILY_CLASSES[c], setup, what), got['objfn'][rows],
                       got['discharge'][rows], obs, r1, setup)


def test_fused_moments_of_two_catchments_with_different_first_reports(eng):
    """One launch, two catchments, r1 = 30 and r1 = 1: each block is what the catchment gives in a launch of its own, bit for
    bit, and is held to truth with its own r1"""
    days = 40
    fs = [storm('piecewise', days), storm('six_hourly', days)]
    setups = ('late', 'from_1')
    pairs = [late_observations(days, setup, seed=1 + c) for c, setup in enumerate(setups)]
    assert pairs[0][1] != pairs[1][1]
    both, what = cases.launch(eng, cases.parameters(FUSED_N), np.stack(fs), 0, 'summary', 24,
                              obs=np.stack([p[0] for p in pairs]))
    assert 'smart_fast_intervals[' in what and 'smart_fast_runs[' in what and what.count(' + ') == 1, what
    for c, (f, (obs, r1), kernel) in enumerate(zip(fs, pairs, ('smart_fast_intervals', 'smart_fast_runs'))):
        one, text = cases.launch(eng, cases.parameters(FUSED_N), f, 0, 'summary', 24, obs=obs)
        assert kernel + '[' in text and ' + ' not in text, text
        assert np.array_equal(one['objfn'].view(np.int64), both['objfn'][c].view(np.int64)), (c, what)
        hold_fused(kernel, 'two catchments, catchment %d: %s' % (c, what), both['objfn'][c], both['discharge'][c], obs, r1,
                   setups[c])
