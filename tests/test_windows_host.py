"""Split-sample objective functions, host side: evaluation_windows against plain datetime arithmetic, the C entry's
validation without a device, the engine's refusals, the Monte-Carlo surface and the header of the `.windows` file.

`statement` is the truth of tests/test_gpu_objfn_windows.py as well: apply f, mask by window and missing observation,
oracle.objfn_oracle.objective_functions(...)[:7], and the entry's two rules (fewer than two rows -> NaN; a transformed
value that is not finite -> NaN)."""
import inspect
import os
from datetime import datetime, timedelta

import numpy as np
import pytest

import support
from conftest import GOLDEN
from oracle import objfn_oracle
from oracle.analyses.windows import TRANSFORMS, statement
from support import E_MODE, E_NO_DEVICE, E_NULL, E_SIZE, FAKE


def test_statement_is_the_oracle_on_one_window_and_applies_the_two_rules():
    rng = np.random.default_rng(3)
    R = 60
    obs = np.abs(rng.normal(3.0, 1.5, R))
    obs[[4, 17]] = np.nan
    sim = rng.random((R, 3)) * 6 + 0.01
    win = np.zeros(R, dtype=np.int32)
    one = statement(sim, obs, win, 1)
    assert np.array_equal(one[0], objfn_oracle.objective_matrix(sim.T, obs)[:, :7])
    win[:30], win[30:] = 0, 1
    win[50:] = -1
    two = statement(sim, obs, win, 3, 'sqrt')
    keep = ~np.isnan(obs)
    assert np.array_equal(two[1, 2], objfn_oracle.objective_functions(np.sqrt(sim[30:50, 2]), np.sqrt(obs[30:50]))[:7])
    assert keep[:30].sum() == 28 and np.isnan(two[2]).all()              # window 2 never occurs
    sim[7, 1] = -1.0
    bad = statement(sim, obs, win, 2, 'log', 0.05)
    assert np.isnan(bad[0, 1]).all() and not np.isnan(bad[0, 0]).any() and not np.isnan(bad[1, 1]).any()
    obs[3] = 0.0
    assert np.isnan(statement(sim, obs, win, 2, 'log', 0.0)[0]).all()
    obs[:] = np.nan
    obs[31] = 1.0
    assert np.isnan(statement(sim, obs, win, 2)).all()                   # one valid observation, none


# ---- evaluation_windows ---------------------------------------------------------------------------------------------
def daily(start, days):
    return [start + timedelta(days=k) for k in range(days)]


def numbered(keys, label=str):
    present = sorted(set(keys))
    return np.array([present.index(k) for k in keys], dtype=np.int32), [label(k) for k in present]


def check(got, want):
    ids, labels = got
    assert isinstance(ids, np.ndarray) and ids.dtype == np.int32 and ids.shape == want[0].shape
    assert np.array_equal(ids, want[0]) and labels == want[1] and all(isinstance(x, str) for x in labels)


TEN_YEARS = daily(datetime(1990, 3, 15, 9), 3653)           # a first and a last partial hydrological year
TWO_YEARS_HOURLY = [datetime(2006, 11, 30, 0) + timedelta(hours=k) for k in range(2 * 365 * 24)]


@pytest.mark.parametrize('stamps', [TEN_YEARS, TWO_YEARS_HOURLY], ids=['daily', 'hourly'])
def test_windows_by_calendar(stamps):
    from smartpy_amd.windows import evaluation_windows
    check(evaluation_windows(stamps, by='all'), (np.zeros(len(stamps), dtype=np.int32), ['all']))
    check(evaluation_windows(stamps, by='year'), numbered([s.year for s in stamps]))
    hydro = numbered([s.year + 1 if s.month >= 10 else s.year for s in stamps])
    check(evaluation_windows(stamps), hydro)
    check(evaluation_windows(stamps, by='hydro_year', start_month=10), hydro)
    check(evaluation_windows(stamps, by='hydro_year', start_month=1), evaluation_windows(stamps, by='year'))
    check(evaluation_windows(stamps, by='hydro_year', start_month=4),
          numbered([s.year + 1 if s.month >= 4 else s.year for s in stamps]))
    check(evaluation_windows(stamps, by='month'), numbered([s.month for s in stamps], lambda m: '%02d' % m))
    season = {12: 0, 1: 0, 2: 0, 3: 1, 4: 1, 5: 1, 6: 2, 7: 2, 8: 2, 9: 3, 10: 3, 11: 3}
    ids, labels = evaluation_windows(stamps, by='season')
    check((ids, labels), (np.array([season[s.month] for s in stamps], dtype=np.int32), ['DJF', 'MAM', 'JJA', 'SON']))
    assert sorted(set(ids.tolist())) == [0, 1, 2, 3]
    assert np.count_nonzero(np.diff(ids)) >= 7                 # interleaved along the run, not four blocks


def test_hydrological_years_partial_at_both_ends_and_seasons_across_new_year():
    from smartpy_amd.windows import evaluation_windows
    ids, labels = evaluation_windows(TEN_YEARS)
    assert labels == [str(y) for y in range(1990, 2001)]        # 15 March 1990 .. 14 March 2000: eleven, two partial
    assert TEN_YEARS[-1] == datetime(2000, 3, 14, 9)
    assert np.count_nonzero(ids == 0) == 200 and np.count_nonzero(ids == 10) == 166      # 15/03 - 30/09; 01/10 - 14/03
    assert np.count_nonzero(ids == 2) == 366                    # 1 October 1991 - 30 September 1992
    at = {s: i for s, i in zip(TEN_YEARS, evaluation_windows(TEN_YEARS, by='season')[0])}
    assert at[datetime(1994, 12, 31, 9)] == 0 and at[datetime(1995, 1, 1, 9)] == 0 and at[datetime(1995, 3, 1, 9)] == 1
    # a short run numbers only what occurs, in the order DJF, MAM, JJA, SON
    check(evaluation_windows(daily(datetime(2001, 7, 1), 120), by='season'),
          (np.array([0] * 62 + [1] * 58, dtype=np.int32), ['JJA', 'SON']))
    check(evaluation_windows(daily(datetime(2001, 11, 1), 40), by='month'),
          (np.array([0] * 30 + [1] * 10, dtype=np.int32), ['11', '12']))


def test_windows_by_split():
    from smartpy_amd.windows import evaluation_windows
    stamps = daily(datetime(2000, 1, 1, 9), 100)
    fmt = '%Y-%m-%d %H:%M:%S'

    def span(a, b):
        return '%s..%s' % (stamps[a].strftime(fmt), stamps[b].strftime(fmt))
    # one boundary equal to a stamp: that stamp opens the second window (half-open on the right)
    check(evaluation_windows(stamps, by='split', split=stamps[40]),
          (np.array([0] * 40 + [1] * 60, dtype=np.int32), [span(0, 39), span(40, 99)]))
    # three boundaries, the first before the run: its empty window is not numbered; one between two stamps
    cuts = [datetime(1999, 6, 1), stamps[10], stamps[70] + timedelta(hours=3)]
    check(evaluation_windows(stamps, by='split', split=cuts),
          (np.array([0] * 10 + [1] * 61 + [2] * 29, dtype=np.int32), [span(0, 9), span(10, 70), span(71, 99)]))
    check(evaluation_windows(stamps, by='split', split=[datetime(2100, 1, 1)]),
          (np.zeros(100, dtype=np.int32), [span(0, 99)]))


def test_window_argument_errors():
    from smartpy_amd.windows import evaluation_windows
    stamps = daily(datetime(2000, 1, 1), 10)
    with pytest.raises(Exception, match="'decade' is not recognised"):
        evaluation_windows(stamps, by='decade')
    for month in (0, 13, -1, 2.5):
        with pytest.raises(Exception, match='between 1 and 12'):
            evaluation_windows(stamps, by='hydro_year', start_month=month)
    with pytest.raises(Exception, match='need the date'):
        evaluation_windows(stamps, by='split')
    with pytest.raises(Exception, match='need the date'):
        evaluation_windows(stamps, by='split', split=[])
    with pytest.raises(Exception, match='ascending order'):
        evaluation_windows(stamps, by='split', split=[stamps[5], stamps[2]])
    with pytest.raises(Exception, match='ascending order'):
        evaluation_windows(stamps, by='split', split=[stamps[5], stamps[5]])
    with pytest.raises(Exception, match='at least one report stamp'):
        evaluation_windows([], by='year')


# ---- the C entry ----------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_the_header_states_the_rules():
    binding, L = support.binding()
    assert 'smart_objfn_windows_hip' in binding.SYMBOLS and 'smart_objfn_max_windows' in binding.SYMBOLS
    assert L.smart_objfn_max_windows() >= 1024 and L.smart_abi_version() == 7
    assert binding.TRANSFORMS == TRANSFORMS
    from smartpy_amd import engine
    assert engine.objfn_max_windows() == L.smart_objfn_max_windows()
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'smart_amd.h')).read()
    for word, code in (('NONE', 0), ('SQRT', 1), ('LOG', 2), ('INVERSE', 3)):
        assert '#define SMART_TRANSFORM_%s %d' % (word, code) in header
    assert '#define SMART_OBJFN_WINDOW_COLS 7' in header
    assert 'fewer than two rows' in header and 'not finite' in header


def test_validation_comes_before_the_device():
    binding, L = support.binding()
    cap = L.smart_objfn_max_windows()

    def call(n=100, r=50, sim=FAKE, ld=None, obs=FAKE, window=FAKE, w=3, transform=0, eps=0.0, out=FAKE):
        rc = L.smart_objfn_windows_hip(n, r, sim, n if ld is None else ld, obs, window, w, transform, eps, out, None)
        return rc, L.smart_last_error().decode()

    for name in ('sim', 'obs', 'window'):
        rc, text = call(**{name: None})
        assert rc == E_NULL and 'smart_objfn_windows_hip' in text and '(%s is NULL)' % name in text, name
    rc, text = call(out=None)
    assert rc == E_NULL and '(objfn is NULL)' in text
    for kw, word in ((dict(n=0), 'n_samples'), (dict(n=-2), 'n_samples'), (dict(r=0), 'n_reports'), (dict(w=0), 'n_windows'),
                     (dict(ld=99), 'ld'), (dict(w=cap + 1), 'n_windows'), (dict(eps=-1e-300), 'eps'),
                     (dict(eps=float('inf')), 'eps'), (dict(eps=float('nan')), 'eps')):
        rc, text = call(**kw)
        assert rc == E_SIZE and 'smart_objfn_windows_hip' in text and word in text, kw
    for t in (-1, 4, 99):
        rc, text = call(transform=t)
        assert rc == E_MODE and 'transform' in text, t
    # the order: NULL before SIZE before MODE
    assert call(sim=None, n=0, transform=9)[0] == E_NULL
    assert call(n=0, transform=9)[0] == E_SIZE and call(eps=-1.0, transform=9)[0] == E_SIZE
    if L.smart_device_count() == 0:
        # a well-formed call gets as far as the device, and no further: there is no CPU fallback
        for kw in (dict(), dict(w=cap), dict(w=1, transform=3, eps=0.5), dict(transform=2)):
            assert call(**kw)[0] in (E_NO_DEVICE,), kw


# ---- engine and Monte-Carlo surface ---------------------------------------------------------------------------------
def test_engine_refuses_before_any_device_call():
    from smartpy_amd import engine
    sim, obs = np.ones((6, 4)), np.ones(6)
    with pytest.raises(engine.SmartEngineError, match="transform 'cube' unknown") as e:
        engine.objective_functions_windows(sim, obs, np.zeros(6, dtype=np.int32), transform='cube')
    assert e.value.code == E_MODE
    for ids, n_windows, count in (([0, 1, 2, -2, 0, 0], None, 1), ([0, 1, 2, 0, 3, 3], 3, 2), ([-1, -5, -2, 0, 0, 0], 1, 2),
                                  ([0, 0, 1, 1, 2, 2], 1, 4)):
        with pytest.raises(engine.SmartEngineError, match='%d of the 6 window ids' % count) as e:
            engine.objective_functions_windows(sim, obs, np.array(ids), n_windows=n_windows)
        assert e.value.code == E_SIZE
    with pytest.raises(engine.SmartEngineError, match='2 of the 6 window ids') as e:
        import torch
        engine.objective_functions_windows(sim, obs, torch.tensor([0, 1, 7, 0, -3, 1]), n_windows=2)
    assert e.value.code == E_SIZE
    with pytest.raises(engine.SmartEngineError, match='5 window ids for a matrix of shape'):
        engine.objective_functions_windows(sim, obs, np.zeros(5, dtype=np.int64))


def test_every_workflow_has_window_objective_functions():
    from smartpy_amd.montecarlo import LHS, GLUE, Best, Total
    from smartpy_amd.montecarlo.montecarlo import MonteCarlo
    for cls in (LHS, GLUE, Best, Total):
        assert cls.window_objective_functions is MonteCarlo.window_objective_functions
    sig = inspect.signature(MonteCarlo.window_objective_functions)
    assert list(sig.parameters) == ['self', 'windows', 'transform', 'eps', 'start_month', 'split', 'write']
    defaults = {k: p.default for k, p in sig.parameters.items() if k != 'self'}
    assert defaults == dict(windows='hydro_year', transform='none', eps=None, start_month=10, split=None, write=False)


def test_header_line_of_the_windows_file_and_default_eps(tmp_path):
    from smartpy_amd import windows
    from smartpy_amd.montecarlo.analyses import _write_windows_file
    names = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE']
    assert windows.OBJ_FN_NAMES == names
    assert windows.header_line(['1994', '1995'], 'log') == \
        ','.join(['%s:log@1994' % f for f in names] + ['%s:log@1995' % f for f in names]) + '\n'
    assert windows.header_line(['DJF'], 'none') == ','.join('%s@DJF' % f for f in names) + '\n'
    obs = np.array([1.0, np.nan, 4.0, 7.0])
    assert windows.default_eps('none', obs) == 0.0 and windows.default_eps('sqrt', obs) == 0.0
    assert windows.default_eps('log', obs) == 0.04 and windows.default_eps('inverse', obs) == 0.04
    # the function write=True calls: header + one line per sample, window by window, float32 '%.6e'
    values = np.arange(2 * 3 * 7, dtype=np.float64).reshape(2, 3, 7) / 7.0
    values[1, 2, 4] = np.nan
    path = str(tmp_path / 'x.windows')
    _write_windows_file(path, ['a', 'b'], 'sqrt', values)
    lines = open(path).read().split('\n')
    assert lines[0] + '\n' == windows.header_line(['a', 'b'], 'sqrt') and lines[-1] == '' and len(lines) == 5
    for n in range(3):
        want = ['%.6e' % np.float32(v) for w in range(2) for v in values[w, n]]
        assert lines[1 + n].split(',') == want
    r = windows.WindowObjectives(['a', 'b'], 'sqrt', 0.0, values, None, path)
    assert r.names == names and r.labels == ['a', 'b'] and r.file == path and r.values is values
