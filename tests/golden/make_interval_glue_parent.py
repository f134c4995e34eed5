"""The interval engine's outputs on the cases of tests/test_interval_glue.py, bit for bit, as the PARENT commit's library
computes them -> tests/golden/interval_glue_parent.npz.  Needs an MI355X; run once, with the parent's library selected:

    bash tools/build_rev_variant.sh <parent rev> parent
    SMART_AMD_LIB=$PWD/tools/variants/libsmart_amd_parent.so python tests/golden/make_interval_glue_parent.py [out.npz]

The change the fixture was made for rewrote the compiled code around the interval engine's asm loops (counters, pointers,
the loads of the observations, the report) and no arithmetic: every kernel of the engine has to give the parent's bits.
The cases and how a case is run live here, so that the test runs exactly what the fixture recorded.

Shapes: N = 65 and 130 (the last block of 64 has one or two live lanes), hourly steps, daily reports, 12 days, without
and with two days of warm-up.  The library cuts no run of fewer than 64 intervals into time slices, and no slice
shorter than four intervals (plan_time_slices, smart_capi.hip): the 12-day cases ask for 1, 3 and one slice per
interval and run whole; the same 12 days six times over (N = 65, two days of warm-up: 74 intervals) are cut into 3 and
into 18 slices, the first of which holds the warm-up and the first reports.

The forcing visits every branch of the code around the loops: days that are wet for every lane, dry for every lane, rainless (decided on the scalar unit), with neither rain nor evaporation, rain without
evaporation, and three days on which rain x T - PE changes sign inside the range of T a wavefront holds (T in 0.9 .. 1.1;
thresholds 0.95, 1.0 and 1.07 -- the last one between the two lanes of N = 130's last block).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'interval_glue_parent.npz')
AREA = 175.46e6
EXTRA = {'aar': 1200, 'r-o_ratio': 0.45, 'r-o_split': (0.10, 0.15, 0.15, 0.30, 0.30)}
GAP = 24
GW_OBS = 0.2
# (rain, PE) in mm per hour, one pair per day
DAILY = np.array([(0.5, 0.05),      # wet for every lane
                  (0.0, 0.08),      # rainless
                  (0.0, 0.0),       # neither rain nor PE
                  (0.02, 0.1),      # rain, and dry for every lane (T < 5)
                  (0.1, 0.1),       # the sign changes at T = 1.0
                  (0.1, 0.107),     # ... at T = 1.07
                  (0.8, 0.02),      # wet
                  (0.0, 0.12),      # rainless
                  (0.2, 0.19),      # the sign changes at T = 0.95
                  (0.0, 0.0),       # calm
                  (0.01, 0.09),     # dry for every lane
                  (0.3, 0.0)])      # rain without PE
# (samples, days, days of warm-up)
SETUPS = [(65, 12, 0), (65, 12, 2), (130, 12, 0), (130, 12, 2), (65, 72, 2)]
OBS_KINDS = ('nan_first', 'nan_last', 'all_nan')
# what a launch is asked for: (name, forcing, report, want_final, time_slices (None: one interval per slice),
# SMART_EXITS (None: unset), observations, discharge stored)
MODES = []
for _kind, _forcing, _report, _final in (('summary', 'daily', 'summary', False), ('states', 'daily', 'summary', True),
                                         ('runs6', 'six_hourly', 'summary', False), ('raw', 'daily', 'raw', False)):
    for _slices in (1, 3, None):
        MODES.append(('%s_slices_%s' % (_kind, _slices or 'all'), _forcing, _report, _final, _slices, None, True, True))
MODES += [('summary_exits_0', 'daily', 'summary', False, 0, '0', True, True),
          ('summary_exits_1', 'daily', 'summary', False, 0, '1', True, True),
          ('runs6_exits_1', 'six_hourly', 'summary', False, 0, '1', True, True),
          ('summary_no_obs', 'daily', 'summary', False, 3, None, False, True),
          ('raw_no_obs', 'daily', 'raw', False, 3, None, False, True),
          ('summary_objectives_only', 'daily', 'summary', False, 3, None, True, False)]
KERNEL_OF = {'summary': 'smart_fast_intervals[', 'states': 'smart_fast_intervals_states[', 'runs6': 'smart_fast_runs[',
             'raw': 'smart_fast_intervals_raw[', 'summary_exits_0': 'smart_fast_intervals[',
             'summary_exits_1': 'smart_fast_intervals_exits[', 'runs6_exits_1': 'smart_fast_runs_exits[',
             'summary_no_obs': 'smart_fast_intervals[', 'raw_no_obs': 'smart_fast_intervals_raw[',
             'summary_objectives_only': 'smart_fast_intervals['}


def forcing(kind, days):
    """[days * 24, 2]: the daily values on every hour of their day, or the same daily totals as four 6-hour values"""
    daily = np.tile(DAILY, (days // len(DAILY), 1))
    f = np.repeat(daily, 24, axis=0)
    if kind == 'six_hourly':
        rain_w, pe_w = np.array([0.4, 0.0, 0.35, 0.25]), np.array([0.1, 0.4, 0.4, 0.1])
        f = np.stack([np.repeat((daily[:, 0:1] * 24 * rain_w).ravel() / 6, 6),
                      np.repeat((daily[:, 1:2] * 24 * pe_w).ravel() / 6, 6)], axis=1)
    return np.ascontiguousarray(f)


def observations(kind, days):
    obs = np.abs(np.random.default_rng(21).normal(2.0, 1.0, days))
    if kind == 'nan_first':
        obs[0] = np.nan
        obs[5] = np.nan
    elif kind == 'nan_last':
        obs[-1] = np.nan
    else:
        obs[:] = np.nan
    return obs


def parameters(n):
    from oracle import lhs_oracle
    return lhs_oracle.lhs_params(n, seed=9)


def kernel_of(mode_name):
    return KERNEL_OF.get(mode_name, KERNEL_OF.get(mode_name.split('_slices_')[0]))


def slices_run(slices, days, warm_days):
    """the time slices a launch that asks for `slices` (None: one per interval) is cut into: plan_time_slices"""
    n_all = warm_days + days
    want = n_all if slices is None else slices
    return 1 if want == 1 or n_all < 64 else min(want, n_all // 4)


def run_mode(eng, mode, n, days, warm_days, obs_kind):
    """one launch -> ({field: array}, the launch's description)"""
    name, fkind, report, final, slices, exits, with_obs, store = mode
    n_all = warm_days + days
    kw = dict(extra=EXTRA, report=report, want_final=final, time_slices=n_all if slices is None else slices,
              want_discharge=store)
    if with_obs:
        kw.update(obs=observations(obs_kind, days), gw_obs=GW_OBS)
    before = os.environ.pop('SMART_EXITS', None)
    try:
        if exits is not None:
            os.environ['SMART_EXITS'] = exits
        prepared = eng.prepare_ensemble(parameters(n), forcing(fkind, days), AREA, 3600.0, warm_days * 24, GAP, **kw)
        out = prepared.launch()
        what = prepared.describe()
        assert prepared.status() == 0, what
    finally:
        os.environ.pop('SMART_EXITS', None)
        if before is not None:
            os.environ['SMART_EXITS'] = before
    got = {'gw': out.gw.cpu().numpy()}
    if store:
        got['discharge'] = out.discharge.cpu().numpy()
    if with_obs:
        got['objfn'] = out.objfn.cpu().numpy()
    if final:
        got['final_vars'] = out.final_vars.cpu().numpy()
    return got, what


def key(mode_name, n, days, warm_days, obs_kind, field):
    return '%s|N%d|T%d|W%d|%s|%s' % (mode_name, n, days, warm_days, obs_kind, field)


def load_fixture(path=FIXTURE):
    """{key: array of doubles} (arrays with the same bytes are stored once)"""
    z = np.load(path, allow_pickle=False)
    return {str(k): z['a%d' % r] for k, r in zip(z['keys'], z['refs'])}


def main(path):
    import torch
    from smartpy_amd import _lib, engine
    assert torch.cuda.is_available(), 'the fixture is made on the GPU'
    print('library:', _lib.LIB_PATH)
    arrays, index, keys, refs = [], {}, [], []
    for mode in MODES:
        for n, days, warm_days in SETUPS:
            for obs_kind in OBS_KINDS:
                got, what = run_mode(engine, mode, n, days, warm_days, obs_kind)
                assert kernel_of(mode[0]) in what, (mode[0], what)
                for field, a in got.items():
                    a = np.ascontiguousarray(a, dtype=np.float64)
                    sig = (a.shape, a.tobytes())
                    if sig not in index:
                        index[sig] = len(arrays)
                        arrays.append(a)
                    keys.append(key(mode[0], n, days, warm_days, obs_kind, field))
                    refs.append(index[sig])
    np.savez_compressed(path, keys=np.array(keys), refs=np.array(refs, dtype=np.int32),
                        **{'a%d' % i: a for i, a in enumerate(arrays)})
    print('%d entries, %d distinct arrays, %d bytes -> %s' % (len(keys), len(arrays), os.path.getsize(path), path))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
