"""SMART_MATH_FAST on finite forcing with the sign bit set -- negative and -0.0 rain and evaporation -- against the oracle:
every fast kernel on the path that the per-catchment flag kForcingInsane sends such forcing down, where the scalar
shortcuts ("no rain: dry", "neither: calm") are off and every interval and step takes the general excess / wet / dry
code.  Needs an MI355X.  tests/golden/make_forcing_signs.py has the table, the forms, the set-ups and the launches, and
tests/test_oracle_golden.py pins the oracle to the reference on the same inputs.

Each launch names its kernel (describe()) and leaves status 0.  Held to the reference-exact oracle at the project's gates:
  what the model computes   excess(got, want, 1e-9) on the discharge, 1e-10 with top = 1 on the groundwater ratio, 1e-8 on
                            the final row.  excess() <= 1 is the contract; the module holds itself to GATE = EXCESS_GATE,
                            a tenth of it: the largest margin of the run the gate was chosen from is 6.6e-4
                            (profiles/forcing_signs_margins.txt), far under the 0.05 that choice asks for.
  the objective functions   1e-9 relative, element by element, with the constraint flag equal: the gate itself, as
                            tests/test_gpu_parity.py and tests/test_interval_glue.py apply it (their EXCESS_GATE and FUZZ_GATE
                            are bounds on excess() margins).  The margin is recorded with the others -- 0.57 of the
                            tolerance at its largest -- and is not a measure of the kernels: a relative difference of a
                            score that is a difference of nearly equal sums.  Among 130 rows and 7 scores per launch some
                            correlation, NSE or bias passes close to zero whatever the observations are; the 0.57 is a
                            correlation of -3.5e-7, where one unit in the last place of the O(1) sums it is made of is
                            3e-10 of it, in the oracle's own numpy evaluation as much as in the kernel's one-pass moments.
                            (Observations made from a row's discharge times log-normal noise, as bench.py makes them, put
                            the bias of some row at 4e-6 of the flow instead, and the same comparison at 2.3 tolerances with
                            a discharge within 6e-5 of its own tolerance: measured once, not used.)
The margins of a run are printed at the end of the module (pytest -s, or the captured output); profiles/
forcing_signs_margins.txt is that table of the run GATE was chosen from.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

from support import Margins, bits_equal, excess, rel, eng      # noqa: F401 (eng is a fixture)
from oracle import smart_oracle as so
from oracle import objfn_oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_forcing_signs', os.path.join(HERE, 'golden', 'make_forcing_signs.py'))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

REL_FAST = 1e-9
EXCESS_GATE, FUZZ_GATE = 0.1, 0.5       # the two gates of tests/test_gpu_parity.py on a support.excess()
GATE = EXCESS_GATE                      # (the module docstring has the measurement behind the choice)
MARGINS = Margins()  # (quantity, kernel) -> (largest margin seen in this run, the launch it was seen in)


def hold(quantity, kernel, tag, margin, gate=None):
    """record the margin, print it, then hold it to the gate (None: GATE, looked up now)"""
    gate = GATE if gate is None else gate
    if margin >= MARGINS.get((quantity, kernel), (-1.0, ''))[0]:
        MARGINS[quantity, kernel] = (margin, tag)
    print('%-10s %-32s %.3g  %s' % (quantity, kernel, margin, tag))
    assert np.isfinite(margin) and margin <= gate, (quantity, kernel, tag, margin)


def against_the_oracle(got, want, obs, kernel, tag, rows=slice(None)):
    """the outputs of a launch ({field: array}) against the oracle's (discharge, gw, final) on `rows`"""
    dis, gw, fin = (a[rows] for a in want)
    assert np.isfinite(dis).all() and np.isfinite(gw).all() and np.isfinite(fin).all(), tag
    if 'discharge' in got:
        assert got['discharge'][rows].shape == dis.shape, tag
        hold('discharge', kernel, tag, excess(got['discharge'][rows], dis, REL_FAST))
    hold('gw', kernel, tag, excess(got['gw'][rows], gw, 1e-10, top=1.0))
    if 'final_vars' in got:
        hold('final', kernel, tag, excess(got['final_vars'][rows], fin, 1e-8))
    if 'objfn' in got:
        scores = objfn_oracle.objective_matrix(dis, obs, gw, cases.GW_OBS)
        assert np.isfinite(scores).all(), tag
        assert np.array_equal(got['objfn'][rows][:, 7], scores[:, 7]), tag
        hold('scores', kernel, tag, rel(got['objfn'][rows][:, :7], scores[:, :7]) / 1e-9, gate=1.0)


@pytest.fixture(scope='module', autouse=True)
def _print_the_margins():
    yield
    if not MARGINS:
        return
    lines = ['%-10s %-32s %-9.3g %s' % (q, k, m, tag) for (q, k), (m, tag) in
             sorted(MARGINS.items(), key=lambda kv: (kv[0][0], -kv[1][0]))]
    worst = {q: max(m for (q1, _), (m, _) in MARGINS.items() if q1 == q) for q, _ in MARGINS}
    text = ('margins of this run against the reference-exact oracle (1.0 = the tolerance; discharge, gw and final are held to '
            '%.2g, the scores to 1): quantity, kernel, largest margin, the launch it was seen in\n' % GATE + '\n'.join(lines) +
            '\nlargest by quantity: ' + ', '.join('%s %.3g' % kv for kv in sorted(worst.items())) + '\n')
    MARGINS.publish(text)


@functools.lru_cache(maxsize=None)
def hourly_forcing(form, days, which):
    return cases.forcing(form, days, which)


@functools.lru_cache(maxsize=None)
def oracle(n, days, warm_days, form, report_kind, which='table', literal=False):
    """(discharge [n, R], gw [n], final [n, 19]): the reference-exact oracle, or (literal) the one configured as the
    literal kernel computes; once per set-up, shared by the launches"""
    report, gap = cases.REPORTS[report_kind]
    kw = dict(pow_mode=so.POW_MUL, sum_mode=so.SUM_GPU) if literal else {}
    out = cases.oracle_run(so, hourly_forcing(form, days, which), warm_days * 24, cases.parameters(n), report, gap, **kw)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def daily_oracle(literal=False):
    kw = dict(pow_mode=so.POW_MUL, sum_mode=so.SUM_GPU) if literal else {}
    out = cases.oracle_run(so, cases.daily_forcing(), cases.DAILY_WARM, cases.daily_parameters()[0], 'summary', 1,
                           dt=86400.0, **kw)
    for a in out:
        a.setflags(write=False)
    return out


def run_hourly(eng, name, n, days, warm_days, store, which='table', time_slices=0):
    """One launch of cases.LAUNCHES by name: stored discharge goes with observations whose first report is missing,
    objectives alone with ones whose last is -> (got, observations, kernel, tag, the launch's description)"""
    _, form, report_kind, final, exits, kernel = cases.LAUNCH[name]
    report, gap = cases.REPORTS[report_kind]
    obs = cases.observations('nan_first' if store else 'nan_last', cases.n_reports(days * 24, report_kind))
    got, what = cases.launch(eng, cases.parameters(n), hourly_forcing(form, days, which), warm_days * 24, report, gap,
                             exits=exits, obs=obs, gw_obs=cases.GW_OBS, want_final=final,
                             want_discharge=store, time_slices=time_slices)
    tag = '%s %s N=%d T=%d W=%d %s: %s' % (name, which, n, days * 24, warm_days * 24,
                                           'stored' if store else 'objectives only', what)
    assert kernel in what and ' + ' not in what, tag
    assert ('discharge' in got) == store and ('final_vars' in got) == final and 'objfn' in got, tag
    return got, obs, kernel.rstrip('['), tag, what


def test_what_the_cases_claim_about_their_forcing():
    t = cases.TABLE
    assert t.shape == (16, 2) and np.isfinite(t).all()
    neg_zero = np.signbit(t) & (t == 0)
    assert neg_zero[:, 0].sum() == 2 and neg_zero[:, 1].sum() == 2 and (t < 0).sum() == 6
    assert ((t[:, 0] == 0) & ~np.signbit(t[:, 0]) & (t[:, 1] < 0)).sum() == 1      # the day a missed flag gets wrong
    for n, _ in cases.SETUPS:
        T = cases.parameters(n)[:, 0]
        assert n % 64 in (1, 2)
        pad = np.concatenate([T, np.full((-n) % 64, T[-1])]).reshape(-1, 64)
        ex = t[None, None, :, 0] * pad[:, :, None] - t[None, None, :, 1]            # [block, lane, day]
        mixed = ~(ex >= 0).all(1) & ~(ex < 0).all(1)
        assert mixed[:n // 64, 8].all() and mixed[:n // 64, 12].all()               # the sign changes inside full blocks
        assert (ex[:, :, 4] > 0).all() and (ex[:, :, 6] < 0).all()
    for form in cases.FORMS:
        f = cases.forcing(form)
        assert f.shape == (cases.DAYS * 24, 2) and np.isfinite(f).all() and np.signbit(f).any()
        assert np.allclose(f.reshape(cases.DAYS, 24, 2).sum(1), t * 24, atol=1e-12) or form == 'varying'
    six = cases.forcing('six_hourly')
    assert (np.signbit(six) & (six == 0) & (np.repeat(t, 24, axis=0) < 0)).any()    # zero weight x negative total: -0.0
    for which, day in cases.PLACEMENTS.items():
        f, sane = cases.forcing('piecewise', which=which), cases.forcing('piecewise', which='sane')
        assert not np.signbit(sane).any()
        assert np.flatnonzero(np.signbit(f).any(1)).tolist() == list(range(day * 24, day * 24 + 24))
    assert cases.PLACEMENTS['step_63'] * 24 <= 63 < cases.PLACEMENTS['step_63'] * 24 + 24
    p, cls = cases.daily_parameters()
    k = p[:, 6:10] * 3600.0
    assert ((k >= 86400.0).all(1) == (cls != 1) & (cls != 3)).all() and ((p[:, 4] > 0.5) == (cls == 2)).all()
    assert ((k[:, 3] < 43200.0) == (cls == 3)).all() and (k[cls == 1, 3] >= 86400.0).all()
    assert np.signbit(cases.daily_forcing()).any() and cases.daily_forcing().shape == (cases.DAILY_STEPS, 2)


@pytest.mark.parametrize('n, warm_days', cases.SETUPS)
def test_every_hourly_kernel_against_the_oracle(eng, n, warm_days):
    """smart_fast_intervals / _exits / _states, smart_fast_runs / _states, smart_fast_steps / _states,
    smart_fast_intervals_raw, smart_fast_steps_raw, smart_fast_steps_every and smart_fast_plain on the table in its three
    forms: with the discharge stored and without, observations with a NaN first and last, gw_obs, the final row where
    the kernel takes it"""
    for name, form, report_kind, final, exits, kernel in cases.LAUNCHES:
        for store in (True, False):
            got, obs, kernel, tag, _ = run_hourly(eng, name, n, cases.DAYS, warm_days, store)
            against_the_oracle(got, oracle(n, cases.DAYS, warm_days, form, report_kind), obs, kernel, tag)


def test_time_slices_over_eighty_days(eng):
    """The one length the library cuts: every sliceable kernel whole, in 3 slices and in one slice per day asked for, which
    the library makes one per four intervals (20) under daily reports and leaves at 82 under a report every step -- against
    the oracle, and the sliced launches the bits of the whole one"""
    n, warm_days = cases.LONG_SETUP
    days = cases.LONG_DAYS
    n_all = days + warm_days
    for name in cases.SLICED:
        _, form, report_kind, final, exits, kernel = cases.LAUNCH[name]
        per = 24 // cases.REPORTS[report_kind][1]        # report intervals per day
        for store in (True, False):
            whole = None
            for asked, n_slices in ((1, 1), (3, 3), (n_all, min(n_all, n_all * per // 4))):
                got, obs, kernel, tag, what = run_hourly(eng, name, n, days, warm_days, store, time_slices=asked)
                assert ('[%d slices' % n_slices in what) == (n_slices > 1) and ('slices' in what) == (n_slices > 1), tag
                against_the_oracle(got, oracle(n, days, warm_days, form, report_kind), obs, kernel, tag)
                if whole is None:
                    whole = got
                for field, a in got.items():
                    assert bits_equal(a, whole[field]), (tag, field)


@pytest.mark.parametrize('which', list(cases.PLACEMENTS))
def test_one_bad_day_in_a_sane_series(eng, which):
    """One day of (0.0, -0.05) in the sane table of tests/test_interval_glue.py -- the first day, the last, the one that
    holds step 63, the warm-up part: a flag scan that misses an end of the series runs that day dry"""
    for n, warm_days in cases.SETUPS:
        if which == 'warm_up_part' and warm_days == 0:
            continue
        assert which != 'warm_up_part' or cases.PLACEMENTS[which] < warm_days
        for name in ('intervals', 'intervals_states', 'runs', 'steps', 'intervals_raw', 'steps_raw', 'steps_every_piecewise',
                     'plain_varying'):
            _, form, report_kind, final, exits, kernel = cases.LAUNCH[name]
            got, obs, kernel, tag, _ = run_hourly(eng, name, n, cases.DAYS, warm_days, True, which=which)
            want = oracle(n, cases.DAYS, warm_days, form, report_kind, which)
            against_the_oracle(got, want, obs, kernel, tag)


@pytest.mark.parametrize('final', [False, True])
def test_three_catchments_with_a_flag_each(eng, final):
    """One launch over the sane table, the table above on every hour and the table above as 6-hourly values: every
    catchment's block is what the catchment gives in a launch of its own, bit for bit (the flag is per catchment)"""
    n, warm_days = 130, 2
    fs = [hourly_forcing('piecewise', cases.DAYS, 'sane'), hourly_forcing('piecewise', cases.DAYS, 'table'),
          hourly_forcing('six_hourly', cases.DAYS, 'table')]
    obs = cases.observations('nan_first', cases.DAYS)
    kw = dict(obs=obs, gw_obs=cases.GW_OBS, want_final=final)
    both, what = cases.launch(eng, cases.parameters(n), np.stack(fs), warm_days * 24, 'summary', 24, **kw)
    tail = '_states[' if final else '['
    assert 'smart_fast_intervals' + tail in what and 'smart_fast_runs' + tail in what and what.count(' + ') == 1, what
    assert both['discharge'].shape == (3, n, cases.DAYS)
    for c, (f, kernel) in enumerate(zip(fs, ('smart_fast_intervals', 'smart_fast_intervals', 'smart_fast_runs'))):
        one, text = cases.launch(eng, cases.parameters(n), f, warm_days * 24, 'summary', 24, **kw)
        assert kernel + tail in text and ' + ' not in text, text
        assert sorted(one) == sorted(both)
        for field, a in one.items():
            assert bits_equal(both[field][c], a), (c, field, what)
    # (each block against the oracle as well: the launch of its own is held to it above, the sane one here)
    against_the_oracle({k: v[0] for k, v in both.items()}, oracle(n, cases.DAYS, warm_days, 'piecewise', 'summary24', 'sane'),
                       obs, 'smart_fast_intervals' + tail.rstrip('['), 'three catchments, the sane one: ' + what)


@pytest.mark.parametrize('literal_form, want_final', [('rows', False), ('lanes', False), ('rows', True), ('lanes', True)])
def test_daily_steps_on_every_class_of_rows(eng, literal_form, want_final):
    """dt = 86400 s, a report every step: smart_fast_steps_every (with the final row: smart_fast_plain), smart_fast_stiff,
    smart_fast_guard and smart_fast_illcond / _lanes side by side, the rows grouped by the engine.  Every row against the
    oracle; the ill-conditioned rows the bits of the literal launch as well"""
    params, cls = cases.daily_parameters()
    f = cases.daily_forcing()
    obs = cases.observations('nan_first', cases.DAILY_STEPS)
    kw = dict(dt=86400.0, obs=obs, gw_obs=cases.GW_OBS, want_final=want_final)
    got, what = cases.launch(eng, params, f, cases.DAILY_WARM, 'summary', 1, literal_form=literal_form, **kw)
    kernels = ['smart_fast_plain' if want_final else 'smart_fast_steps_every', 'smart_fast_stiff', 'smart_fast_guard',
               'smart_fast_illcond' if literal_form == 'rows' else 'smart_fast_illcond_lanes']
    assert all(k + '[' in what for k in kernels) and what.count(' + ') == 3, what
    lit, text = cases.launch(eng, params, f, cases.DAILY_WARM, 'summary', 1, math_mode='literal', **kw)
    assert text == 'smart_ensemble_literal'
    for c, kernel in enumerate(kernels):
        rows = np.flatnonzero(cls == c)
        tag = 'daily steps, %s rows, final row %s: %s' % (cases.DAILY_CLASSES[c], want_final, what)
        against_the_oracle(got, daily_oracle(), obs, kernel, tag, rows)
        if c == 3:
            for field in ('discharge', 'gw') + (('final_vars',) if want_final else ()):
                assert bits_equal(got[field][rows], lit[field][rows]), (tag, field)
    # the literal launch: every output the bits of the oracle configured as that kernel computes
    dis, gw, fin = daily_oracle(literal=True)
    assert bits_equal(lit['discharge'], dis) and bits_equal(lit['gw'], gw), what
    if want_final:
        assert bits_equal(lit['final_vars'], fin)


@pytest.mark.parametrize('form', cases.FORMS)
def test_literal_mode_on_the_same_forcing_bit_for_bit(eng, form):
    """math_mode='literal' against the oracle with the product chain for s' ** i and the kernel's summation orders: the
    same bits (every output is finite: the sign of a NaN plays no part)"""
    for n, warm_days in ((130, 2), (65, 0)):
        for report_kind, (report, gap) in cases.REPORTS.items():
            got, what = cases.launch(eng, cases.parameters(n), hourly_forcing(form, cases.DAYS, 'table'), warm_days * 24,
                                     report, gap, math_mode='literal', want_final=True)
            assert what == 'smart_ensemble_literal'
            dis, gw, fin = oracle(n, cases.DAYS, warm_days, form, report_kind, literal=True)
            tag = (form, report_kind, n, warm_days)
            assert np.isfinite(dis).all() and np.isfinite(gw).all() and np.isfinite(fin).all(), tag
            assert bits_equal(got['discharge'], dis), tag
            assert bits_equal(got['gw'], gw), tag
            assert bits_equal(got['final_vars'], fin), tag
