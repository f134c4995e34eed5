"""Finite forcing with the sign bit set -- negative and -0.0 rain and evaporation -- as cases that tests/test_gpu_forcing_signs.py
runs on the GPU and tests/test_oracle_golden.py pins to the reference, and the generator of that pin:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_forcing_signs.py <directory of the reference> [out.npz]

imports the reference (pure Python, never copied) and stores what its structure.run() computes -- the discharge, the
groundwater ratio and the final row of run_all_steps -- for PIN_ROWS rows of the cases below -> tests/golden/
forcing_signs.npz: numbers and names only.  Nothing but main() touches the reference; the cases and how a launch is made
live here so that the fixture, the CPU pin and the GPU tests speak of the same inputs.

SMART_MATH_FAST takes any finite forcing (include/smart_amd.h).  The fast kernels' shortcuts -- "no rain: the wavefront is
dry, demand PE", "neither: calm" -- are tests on the BITS of the forcing and hold for values >= +0 only, so one flag per
catchment (kForcingInsane: some value has its sign bit set) turns them off and every interval and step goes through the
general excess / wet / dry code.  A flag that is missed does not fail loudly: a rainless interval with PE < 0 is wet
(excess +|PE|) and would be run as a dry one with a negative demand.

TABLE, one (rain, PE) pair per day in mm per hour, visits what that path has to get right; T spans 0.9 .. 1.1 in every
wavefront (N = 65 and 130 rows of lhs_oracle.lhs_params: the last block has one or two live lanes), so the days whose
excess rain * T - PE changes sign at T = 0.95 and at 1.07 split a wavefront between the wet and the dry side.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location('make_interval_glue_parent', os.path.join(HERE, 'make_interval_glue_parent.py'))
glue = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(glue)

FIXTURE = os.path.join(HERE, 'forcing_signs.npz')
AREA, EXTRA, GW_OBS = glue.AREA, glue.EXTRA, glue.GW_OBS
TABLE = np.array([(0.5, 0.05),      # wet for every lane
                  (-0.0, 0.08),     # rainless by value, not by bits
                  (0.0, -0.0),      # calm by value, not by bits
                  (0.02, 0.1),      # dry for every lane
                  (0.0, -0.05),     # no rain, NEGATIVE PE: wet, excess +0.05 -- the day a missed flag gets wrong
                  (0.1, -0.02),     # rain and negative PE
                  (-0.05, 0.0),     # negative rain alone: dry, demand 0.05 T
                  (0.8, 0.02),      # wet
                  (-0.2, -0.19),    # both negative: the sign of rain * T - PE changes at T = 0.95, inside a wavefront
                  (-0.0, -0.0),
                  (-0.05, 0.1),
                  (5e-324, 0.0),    # the smallest subnormal rain: bits set, value positive
                  (0.1, 0.107),     # the sign changes at T = 1.07
                  (0.0, 0.12),      # rainless, sane
                  (0.3, 0.0),       # rain without PE
                  (0.0, 0.0)])      # calm, sane
BAD_DAY = (0.0, -0.05)              # the single value of the placements
FORMS = ('piecewise', 'six_hourly', 'varying')
# report kinds of an hourly run: name -> (report, gap)
REPORTS = {'summary24': ('summary', 24), 'raw24': ('raw', 24), 'every': ('summary', 1), 'raw7': ('raw', 7)}
DAYS, LONG_DAYS = 16, 80
# (samples, days of warm-up) of the 16-day set-ups; the 80-day one (the only length the library cuts into time slices:
# no run under 64 intervals is cut, plan_time_slices) has 65 samples and two days of warm-up
SETUPS = [(65, 0), (65, 2), (130, 0), (130, 2)]
LONG_SETUP = (65, 2)
# where ONE bad day goes into the sane table of make_interval_glue_parent.DAILY: name -> day.  The first and the last day
# of the series, the day that holds step 63 (the last lane of the flag scan's first sweep over the series), and the last
# day of the warm-up part (set-ups with warm-up only)
PLACEMENTS = {'first_day': 0, 'last_day': DAYS - 1, 'step_63': 63 // 24, 'warm_up_part': 1}
# daily steps: dt = 86400 s, a report every step, the table times 24 (mm per day) ten times over
DAILY_STEPS, DAILY_WARM, DAILY_N = 160, 16, 130
DAILY_CLASSES = ('regular', 'stiff', 'guard', 'illcond')
# what a fast launch of an hourly run is asked for: (name, form, report kind, want_final, SMART_EXITS (None: unset), the kernel
# describe() has to name).  A raw or every-step report with the final row is smart_fast_plain's, as is a ragged raw one.
LAUNCHES = [('intervals', 'piecewise', 'summary24', False, None, 'smart_fast_intervals['),
            ('intervals_exits', 'piecewise', 'summary24', False, '1', 'smart_fast_intervals_exits['),
            ('intervals_states', 'piecewise', 'summary24', True, None, 'smart_fast_intervals_states['),
            ('runs', 'six_hourly', 'summary24', False, None, 'smart_fast_runs['),
            ('runs_states', 'six_hourly', 'summary24', True, None, 'smart_fast_runs_states['),
            ('steps', 'varying', 'summary24', False, None, 'smart_fast_steps['),
            ('steps_states', 'varying', 'summary24', True, None, 'smart_fast_steps_states['),
            ('intervals_raw', 'piecewise', 'raw24', False, None, 'smart_fast_intervals_raw['),
            ('steps_raw', 'varying', 'raw24', False, None, 'smart_fast_steps_raw['),
            ('steps_raw_six_hourly', 'six_hourly', 'raw24', False, None, 'smart_fast_steps_raw[')]
LAUNCHES += [('steps_every_' + _f, _f, 'every', False, None, 'smart_fast_steps_every[') for _f in FORMS]
SLICED = [_l[0] for _l in LAUNCHES]         # every kernel above is one the library cuts into time slices
LAUNCHES += [('plain_' + _f, _f, 'raw7', True, None, 'smart_fast_plain[') for _f in FORMS]
LAUNCH = {_l[0]: _l for _l in LAUNCHES}
PIN_ROWS = 6


def table_of(which, days):
    """[days, 2]: TABLE repeated, or -- which = a name of PLACEMENTS -- the sane table with that one day replaced"""
    base = TABLE if which == 'table' else (glue.DAILY if which == 'sane' else None)
    if base is not None:
        return np.resize(base, (days, 2)).copy()        # (rows repeated in order)
    t = np.resize(glue.DAILY, (days, 2)).copy()
    t[PLACEMENTS[which]] = BAD_DAY
    return t


def forcing(form, days=DAYS, which='table'):
    """[days * 24, 2], hourly: the daily value on each of its 24 hours (piecewise); the day's totals as four 6-hour values
    with the weights of make_interval_glue_parent.forcing (a zero weight times a negative total leaves a -0.0); the
    piecewise form times a seeded uniform(0, 2) per step (varying)"""
    daily = table_of(which, days)
    f = np.repeat(daily, 24, axis=0)
    if form == 'six_hourly':
        rain_w, pe_w = np.array([0.4, 0.0, 0.35, 0.25]), np.array([0.1, 0.4, 0.4, 0.1])
        f = np.stack([np.repeat((daily[:, 0:1] * 24 * rain_w).ravel() / 6, 6),
                      np.repeat((daily[:, 1:2] * 24 * pe_w).ravel() / 6, 6)], axis=1)
    elif form == 'varying':
        f = f * np.random.default_rng(63).uniform(0.0, 2.0, (len(f), 1))
    else:
        assert form == 'piecewise', form
    return np.ascontiguousarray(f)


def daily_forcing():
    """[DAILY_STEPS, 2] in mm per day"""
    return np.ascontiguousarray(np.resize(TABLE * 24.0, (DAILY_STEPS, 2)))


def parameters(n):
    return glue.parameters(n)


def daily_parameters():
    """([DAILY_N, 10], the class of every row as an index of DAILY_CLASSES), the classes interleaved -- the engine groups
    them: regular (every residence time >= 24 h), stiff (SK < 24 h), guard (S = 0.7) and ill-conditioned (RK < 12 h)"""
    from oracle import lhs_oracle
    p = lhs_oracle.lhs_params(DAILY_N, seed=19)
    p[:, 6:10] = np.maximum(p[:, 6:10], 30.0)
    cls = np.arange(DAILY_N) % 4
    p[cls == 1, 6] = np.linspace(1.5, 23.0, int((cls == 1).sum()))
    p[cls == 2, 4] = 0.7
    p[cls == 3, 9] = np.linspace(1.0, 11.5, int((cls == 3).sum()))
    return p, cls


def observations(kind, n):
    """n reports, the series of make_interval_glue_parent.observations: a NaN at the front (and one inside) or at the end"""
    obs = np.abs(np.random.default_rng(21).normal(2.0, 1.0, n))
    if kind == 'nan_first':
        obs[0] = np.nan
        obs[5] = np.nan
    else:
        assert kind == 'nan_last', kind
        obs[-1] = np.nan
    return obs


def n_reports(n_steps, report_kind):
    report, gap = REPORTS[report_kind]
    return n_steps // gap if report == 'summary' else -(-n_steps // gap)


def oracle_run(so, f, n_warm, params, report, gap, dt=3600.0, **kw):
    """so: oracle.smart_oracle -> (discharge [n, R], gw [n], final [n, 19]); kw: pow_mode / sum_mode"""
    code = so.REPORT_RAW if report == 'raw' else so.REPORT_SUMMARY
    return so.run_batch(AREA, dt, f.shape[0], n_warm, f[:, 0].copy(), f[:, 1].copy(), params, EXTRA, code, gap,
                        want_final=True, **kw)


def launch(eng, params, f, n_warm, report, gap, dt=3600.0, exits=None, **kw):
    """one launch, with SMART_EXITS set to `exits` (None: unset) while the launch is decided; -> ({field: array}, describe())"""
    before = os.environ.pop('SMART_EXITS', None)
    try:
        if exits is not None:
            os.environ['SMART_EXITS'] = exits
        prepared = eng.prepare_ensemble(params, f, AREA, dt, n_warm, gap, extra=EXTRA, report=report, **kw)
        out = prepared.launch()
        what = prepared.describe()
        assert prepared.status() == 0, what
    finally:
        os.environ.pop('SMART_EXITS', None)
        if before is not None:
            os.environ['SMART_EXITS'] = before
    got = {'gw': out.gw.cpu().numpy()}
    for field in ('discharge', 'objfn', 'final_vars'):
        if getattr(out, field) is not None:
            got[field] = getattr(out, field).cpu().numpy()
    return got, what


# ---- the pin to the reference --------------------------------------------------------------------------------------
def pin_rows(n=130):
    """PIN_ROWS rows of parameters(n) by T: the ends of the range and the rows on either side of the two thresholds"""
    T = parameters(n)[:, 0]
    order = np.argsort(T)
    below = lambda x: int(order[np.searchsorted(T[order], x) - 1])     # noqa: E731
    above = lambda x: int(order[np.searchsorted(T[order], x)])         # noqa: E731
    return [int(order[0]), below(0.95), above(0.95), below(1.07), above(1.07), int(order[-1])]


def daily_pin_rows():
    """a regular, two stiff, a guard and two ill-conditioned rows of daily_parameters()"""
    cls = daily_parameters()[1]
    first = lambda c, k=0: int(np.flatnonzero(cls == c)[k])            # noqa: E731
    return [first(0), first(1), first(1, -1), first(2), first(3), first(3, -1)]


def pin_cases():
    """(key, forcing, dt, steps of warm-up, parameters [PIN_ROWS, 10], report, gap) of every pinned run: the three hourly
    forms under a daily summary after a 48-step warm-up, raw reports of gap 24, a report every step and ragged raw
    reports of gap 7; the daily steps"""
    p = parameters(130)[pin_rows()]
    for form in FORMS:
        for kind, (report, gap) in REPORTS.items():
            yield '%s|%s' % (form, kind), forcing(form), 3600.0, 48 if kind == 'summary24' else 0, p, report, gap
    yield 'daily_steps', daily_forcing(), 86400.0, DAILY_WARM, daily_parameters()[0][daily_pin_rows()], 'summary', 1


def load_fixture(path=FIXTURE):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def main(reference, path):
    sys.dont_write_bytecode = True
    sys.path.insert(0, reference)
    from datetime import timedelta
    from smartpy import structure                   # the reference
    assert not structure.smart_in_cpp, 'the pure-Python path is the reference'
    out, finals, orig = {}, [], structure.run_all_steps

    def recording(*a):
        r = orig(*a)
        finals.append(r[2])
        return r
    structure.run_all_steps = recording             # (run() drops the final row: structure.py:143-146)
    try:
        for key, f, dt, n_warm, params, report, gap in pin_cases():
            T = f.shape[0]
            R = T // gap                            # run() takes the gap from the lengths of its two time axes (:75)
            assert T // R == gap
            dis, gw, fin = [], [], []
            for row in params:
                d, g = structure.run(AREA, timedelta(seconds=dt), f[:, 0].copy(), f[:, 1].copy(), row.copy(), EXTRA,
                                     list(range(T + 1)), list(range(R + 1)), report, warm_up=n_warm * dt / 86400.0)
                dis.append(np.array(d, dtype=np.float64))
                gw.append(float(g))
                fin.append(np.array(finals[-1], dtype=np.float64))
            out[key + '|discharge'], out[key + '|gw'], out[key + '|final'] = np.array(dis), np.array(gw), np.array(fin)
            assert np.isfinite(out[key + '|discharge']).all() and np.isfinite(out[key + '|final']).all()
    finally:
        structure.run_all_steps = orig
    np.savez_compressed(path, **out)
    print('%d arrays, %d bytes -> %s' % (len(out), os.path.getsize(path), path))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else FIXTURE)
