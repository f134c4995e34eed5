"""Tapered time slices (smartpy_amd/csrc/smart_slice_cuts.h) change where a sliced launch cuts the time axis and nothing
else: every sliced kernel family, with the taper, without it (SMART_SLICE_TAPER=0) and unsliced, bit for bit; the tapered
result against the oracle; the same describe() text either way.  Needs an MI355X.

The axis is 90 intervals long (10 days of warm-up, 80 days of reports, hourly steps, daily reports), 130 samples make
three blocks of which the last is partial.  Forced slice counts:
   2   under eight slices: never tapered
   8   tapered: slices of 12 13 13 13 13 13 8 5 intervals -- the warm-up is 10 intervals, so its end lies inside slice 0
       (untapered: slices of 11 or 12), and the last slice is five reports
  10   tapered: eight slices of 10 intervals, then 6 and 4 -- slice 0 is exactly the warm-up (one more count than the
       four first asked for: see 16)
  16   ninety intervals are too few for sixteen tapered slices (the last would be under one interval; under four the
       cuts fall back to the equal ones, slices of five or six intervals, the first of them wholly in the warm-up): the
       fall-back, where the host must not ask the kernels for a taper
  22   the n_all / 4 cap on a forced count: the fall-back again, slices of four or five intervals
A report every step runs 10 + 2 days (288 steps, each its own interval): tapered at 8 and 10 slices (the last slice 15
and 12 steps), equal at 2, 16 and 22.
"""
import numpy as np
import pytest

from support import rel, tensors_same_bits
from oracle import smart_oracle as so
from oracle import objfn_oracle, lhs_oracle

pytestmark = pytest.mark.gpu

REL_FAST = 1e-9         # tests/test_gpu_parity.py: discharge and objective functions of the fast mode against the oracle
GW_ABS = 1e-10          # ... and the groundwater ratio
FLOOR = 1e-290          # magnitudes that are not above it carry no relative precision: rel(..., floor=FLOOR) skips them
N, DAYS, WARM_DAYS = 130, 80, 10
SLICES = [2, 8, 10, 16, 22]

#: name -> (forcing kind, report, gap, want_discharge, want_final, kernel named by describe())
KERNELS = {
    'intervals_stored': ('daily_spread', 'summary', 24, True, False, 'smart_fast_intervals['),
    'intervals_lean': ('daily_spread', 'summary', 24, False, False, 'smart_fast_intervals['),
    'runs_of_six': ('six_hourly', 'summary', 24, True, False, 'smart_fast_runs['),
    'step_loop': ('varying', 'summary', 24, True, False, 'smart_fast_steps['),
    'raw_reports': ('daily_spread', 'raw', 24, True, False, 'smart_fast_intervals_raw['),
    'every_step': ('varying', 'summary', 1, True, False, 'smart_fast_steps_every['),
    'split_final': ('daily_spread', 'summary', 24, True, True, '_states['),
}


def outputs(res):
    return [None if t is None else t.clone() for t in (res.discharge, res.gw, res.objfn, res.final_vars)]


_CASES = {}


def case(name):
    """Inputs, the unsliced launch and the oracle's results of one kernel family: made once, shared by its slice counts."""
    if name in _CASES:
        return _CASES[name]
    import bench
    from smartpy_amd import engine
    kind, report, gap, want_dis, want_final, kernel = KERNELS[name]
    days = 10 if gap == 1 else DAYS
    warm = 2 * 24 if gap == 1 else WARM_DAYS * 24
    base = bench.synthetic_forcing(2, hourly=True)[0][24 * 100:24 * (100 + days)]
    f = {'daily_spread': lambda x: x, 'six_hourly': bench.six_hourly_forcing,
         'varying': bench.hourly_varying_forcing}[kind](base)
    f = np.ascontiguousarray(f)
    T, R = f.shape[0], f.shape[0] // gap
    params = lhs_oracle.lhs_params(N, seed=57)
    rng = np.random.default_rng(12)
    obs = np.abs(rng.normal(2.0, 1.0, R))
    obs[rng.random(R) < 0.12] = np.nan
    obs[0] = np.nan                                     # the first report is not observed
    kw = dict(extra=bench.EXTRA, obs=obs, gw_obs=0.2, report=report, want_discharge=want_dis, want_final=want_final)
    args = (params, f, bench.AREA, 3600.0, warm, gap)
    whole = engine.prepare_ensemble(*args, time_slices=1, **kw)
    assert kernel in whole.describe() and ' + ' not in whole.describe(), whole.describe()    # every row of class 0
    res = whole.launch()
    assert whole.status() == 0
    code = so.REPORT_RAW if report == 'raw' else so.REPORT_SUMMARY
    dis, gwo, fin = so.run_batch(bench.AREA, 3600.0, T, warm, f[:, 0].copy(), f[:, 1].copy(), params, bench.EXTRA, code,
                                 gap, want_final=True)
    oracle = (dis, gwo, objfn_oracle.objective_matrix(dis, obs, gwo, 0.2), fin)
    _CASES[name] = (engine, args, kw, kernel, outputs(res), oracle, (warm // gap + R))
    return _CASES[name]


@pytest.mark.parametrize('n_slices', SLICES)
@pytest.mark.parametrize('name', list(KERNELS))
def test_tapered_slices_are_bit_identical_and_match_the_oracle(monkeypatch, name, n_slices):
    engine, args, kw, kernel, whole, oracle, n_all = case(name)
    assert n_all == (288 if name == 'every_step' else 90)
    monkeypatch.delenv('SMART_TIME_SLICES', raising=False)
    got, text = {}, {}
    for taper in ('on', 'off'):
        if taper == 'off':
            monkeypatch.setenv('SMART_SLICE_TAPER', '0')
        else:
            monkeypatch.delenv('SMART_SLICE_TAPER', raising=False)
        cut = engine.prepare_ensemble(*args, time_slices=n_slices, **kw)
        text[taper] = cut.describe()
        res = cut.launch()
        assert cut.status() == 0, (taper, text[taper])
        got[taper] = outputs(res)
    assert text['on'] == text['off'] and kernel + '%d slices x 3 blocks' % n_slices in text['on'], text
    assert tensors_same_bits(got['on'], got['off']), 'tapered and equal slices differ: %s' % text['on']
    assert tensors_same_bits(got['on'], whole), 'sliced and unsliced launches differ: %s' % text['on']
    dis, gw, obj, fin = [None if t is None else t.cpu().numpy() for t in got['on']]
    d_want, g_want, o_want, f_want = oracle
    if dis is not None:
        assert rel(dis, d_want, floor=FLOOR) < REL_FAST
    assert float(np.max(np.abs(gw - g_want))) < GW_ABS
    assert rel(obj[:, :7], o_want[:, :7], floor=FLOOR) < REL_FAST and np.array_equal(obj[:, 7], o_want[:, 7])
    if fin is not None:
        assert rel(fin, f_want, floor=FLOOR) <= REL_FAST
