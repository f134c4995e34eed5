"""Hydrological signatures, host side: the statement of smart_signatures_hip (oracle/analyses/signatures.py, the truth of
tests/test_gpu_signatures.py as well) against a series worked by hand, the C entry's validation
without a device, the engine's refusals, the Monte-Carlo surface, the default thresholds and alpha, and the `.signatures`
file."""
import inspect
import os

import numpy as np
import pytest

import support
from conftest import ROOT
from oracle.analyses.signatures import (statement, X8, NAMES, PAIR_COLUMNS, MEAN, BFI, FLASHINESS, AC1, RLD, RECESSION, PEAK, PEAK_ROW,
                                       HIGH_COUNT, HIGH_DURATION, LOW_COUNT, LOW_DURATION)
from support import E_NO_DEVICE, E_NULL, E_SIZE, FAKE


# ---- the statement ---------------------------------------------------------------------------------------------------
def test_statement_on_a_series_worked_by_hand():
    """Eight rows, the observation of row 4 missing: valid rows 0 1 2 3 5 6 7 (m = 7), pairs at 1 2 3 6 7 (p = 5).
    alpha = 0.5, so the filter's gain (1 + alpha) / 2 is 0.75; lo = 3.5, hi = 2."""
    sim = np.array(X8).reshape(8, 1)
    obs = np.ones(8)
    obs[4] = np.nan
    got = statement(sim, obs, None, 1, 0.5, [(3.5, 2.0)])[0, :, 0]
    # f: 0 | 0.75 * 2 = 1.5 | 0.75 + 0.75 = 1.5 | 0.75 - 1.5 < 0 -> 0 | (gap) 0 | -1.5 -> 0 | 0.75: sum f = 3.75
    assert got[MEAN] == 19.0 / 7.0 and got[BFI] == (19.0 - 3.75) / 19.0
    assert got[FLASHINESS] == (2.0 + 1.0 + 2.0 + 2.0 + 1.0) / (3.0 + 4.0 + 2.0 + 2.0 + 3.0)
    # the pairs (1,3) (3,4) (4,2) (4,2) (2,3): both means 2.8; covariance sum -2.2, variance sums 6.8 and 2.8
    assert abs(got[AC1] - (-2.2 / np.sqrt(6.8 * 2.8))) < 1e-15
    assert got[RLD] == 2.0 / 3.0                                        # rising at 1, 2 and 7; limbs start at 1 and at 7
    assert got[RECESSION] == np.log(0.5)                                # 4 -> 2 at row 3 and at row 6
    assert got[PEAK] == 4.0 and got[PEAK_ROW] == 2.0                    # the 9 has no observation; 4 again at row 5
    assert got[HIGH_COUNT] == 3.0 and got[HIGH_DURATION] == 4.0 / 3.0   # above 2: rows 1 2 | 5 (after the gap) | 7
    assert got[LOW_COUNT] == 3.0 and got[LOW_DURATION] == 5.0 / 3.0     # below 3.5: rows 0 1 | 3 | 6 7
    # strict comparisons: a threshold equal to a value neither is above nor below it
    exact = statement(sim, obs, None, 1, 0.5, [(2.0, 4.0)])[0, :, 0]
    assert exact[HIGH_COUNT] == 0.0 and np.isnan(exact[HIGH_DURATION]) and exact[LOW_COUNT] == 1.0 and exact[LOW_DURATION] == 1.0
    # without observations the 9 of row 4 is a value like any other
    free = statement(sim, None, None, 1, 0.5, None)[0, :, 0]
    assert free[PEAK] == 9.0 and free[PEAK_ROW] == 4.0 and free[MEAN] == 28.0 / 8.0 and np.isnan(free[HIGH_COUNT:]).all()
    assert free[RLD] == 3.0 / 4.0                                       # rising at 1 2 | 4 | 7


def test_statement_windows_and_rules():
    sim = np.array([X8, [0.0] * 8, [2.5] * 8, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]]).T.copy()
    win = np.array([0, 0, 0, 0, 1, 1, -1, 1], dtype=np.int32)
    got = statement(sim, None, win, 3, 0.5, [(3.5, 2.0), (np.nan, 2.0), (3.5, 2.0)])
    assert np.isnan(got[2]).all()                                       # a window that never occurs
    assert got[0, MEAN, 0] == 2.5 and got[1, MEAN, 0] == 16.0 / 3.0 and got[1, PEAK_ROW, 0] == 4.0
    assert got[1, FLASHINESS, 0] == 5.0 / 4.0                           # one pair (rows 4, 5); row 7 stands alone
    assert np.isnan(got[1, AC1, 0]) and np.isnan(got[1, LOW_COUNT:, 0]).all() and got[1, HIGH_COUNT, 0] == 2.0
    assert np.isnan(got[0, [BFI, FLASHINESS, AC1, RLD, RECESSION], 1]).all() and got[0, MEAN, 1] == 0.0   # all zero
    assert got[0, FLASHINESS, 2] == 0.0 and np.isnan(got[0, [AC1, RLD, RECESSION], 2]).all()              # constant
    assert got[0, BFI, 2] == 1.0 and got[0, PEAK_ROW, 2] == 0.0
    assert got[0, RLD, 3] == 1.0 / 3.0 and np.isnan(got[0, RECESSION, 3])                                 # one limb
    # r % 2: no pair anywhere
    alone = statement(sim, None, np.arange(8, dtype=np.int32) % 2, 2, 0.5, [(3.5, 2.0)] * 2)
    assert np.isnan(alone[:, PAIR_COLUMNS]).all() and not np.isnan(alone[:, [MEAN, PEAK, PEAK_ROW], :]).any()
    assert np.array_equal(alone[:, BFI, 0], [1.0, 1.0]) and np.isnan(alone[:, BFI, 1]).all()
    # a value that is not finite empties its (window, column), and no other
    bad = sim.copy()
    bad[5, 0], bad[6, 3] = np.nan, np.inf
    got = statement(bad, None, win, 2, 0.5, None)
    assert np.isnan(got[1, :, 0]).all() and not np.isnan(got[0, :PEAK_ROW + 1, 0]).any()
    assert not np.isnan(got[:, MEAN, 3]).any()                          # row 6 belongs to no window


# ---- the C entry -----------------------------------------------------------------------------------------------------
def test_symbols_and_columns():
    binding, L = support.binding()
    assert 'smart_signatures_hip' in binding.SYMBOLS and 'smart_signature_cols' in binding.SYMBOLS
    assert L.smart_signature_cols() == 12 == binding.SIGNATURE_COLS and L.smart_abi_version() == 7
    assert binding.SIGNATURE_NAMES == NAMES
    header = open(os.path.join(ROOT, 'include', 'smart_amd.h')).read()
    assert '#define SMART_SIGNATURE_COLS 12' in header
    for k, name in enumerate(NAMES):
        assert '#define SMART_SIG_%s %d\n' % (name, k) in header
    assert 'int smart_signatures_hip(' in header and 'int32_t smart_signature_cols(void);' in header
    assert 'three-pass form' in header and 'second matrix' in header
    from smartpy_amd import analysis, engine, windows
    assert engine.signatures is analysis.signatures and engine.SIGNATURE_NAMES == NAMES == windows.SIGNATURE_NAMES
    from smartpy_amd import build
    assert build.UNITS['smart_signatures.hip'] == []


def test_validation_comes_before_the_device():
    binding, L = support.binding()
    max_windows = L.smart_objfn_max_windows()

    def call(n=100, r=50, sim=FAKE, ld=None, obs=FAKE, window=FAKE, w=3, alpha=0.925, pulse=FAKE, sig=FAKE):
        rc = L.smart_signatures_hip(n, r, sim, n if ld is None else ld, obs, window, w, alpha, pulse, sig, None)
        return rc, L.smart_last_error().decode()

    for name in ('sim', 'sig'):
        rc, text = call(**{name: None})
        assert rc == E_NULL and 'smart_signatures_hip' in text and '(%s is NULL)' % name in text, name
    for kw, word in ((dict(n=0), 'n_samples'), (dict(n=-2), 'n_samples'), (dict(r=0), 'n_reports'), (dict(w=0), 'n_windows'),
                     (dict(ld=99), 'ld'), (dict(r=2 ** 31), 'n_reports'), (dict(w=max_windows + 1), 'n_windows'),
                     (dict(window=None, w=2), 'n_windows'), (dict(alpha=0.0), 'alpha'), (dict(alpha=1.0), 'alpha'),
                     (dict(alpha=-0.5), 'alpha'), (dict(alpha=1.5), 'alpha'), (dict(alpha=float('nan')), 'alpha'),
                     (dict(alpha=float('inf')), 'alpha')):
        rc, text = call(**kw)
        assert rc == E_SIZE and 'smart_signatures_hip' in text and word in text, (kw, text)
    # the order: NULL before SIZE
    assert call(sim=None, n=0)[0] == E_NULL and call(sig=None, alpha=2.0)[0] == E_NULL
    if L.smart_device_count() == 0:
        # a well-formed call gets as far as the device, and no further: there is no CPU fallback
        for kw in (dict(), dict(window=None, w=1, obs=None, pulse=None), dict(obs=None), dict(pulse=None),
                   dict(w=max_windows), dict(alpha=1e-300), dict(alpha=0.5), dict(r=2 ** 31 - 1), dict(ld=101)):
            rc, text = call(**kw)
            assert rc == E_NO_DEVICE and text, kw


# ---- engine and Monte-Carlo surface ----------------------------------------------------------------------------------
def test_engine_refuses_before_it_touches_the_library(monkeypatch):
    from smartpy_amd import engine, _lib as binding

    def untouched():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(binding, 'lib', untouched)
    sim, obs = np.ones((6, 4)), np.ones(6)
    for alpha in (0.0, 1.0, -0.1, 1.5, float('nan'), float('inf')):
        with pytest.raises(engine.SmartEngineError, match='alpha') as e:
            engine.signatures(sim, obs, alpha=alpha)
        assert e.value.code == E_SIZE
    for bad in (np.ones((2, 2)), np.ones(2), np.ones((1, 3)), np.ones((1, 2, 1))):
        with pytest.raises(engine.SmartEngineError, match=r'thresholds must be \(lo, hi\) per window') as e:
            engine.signatures(sim, obs, thresholds=bad)
        assert e.value.code == E_SIZE
    with pytest.raises(engine.SmartEngineError, match=r'shape \(3, 2\)'):
        engine.signatures(sim, obs, windows=np.array([0, 1, 2, 0, 1, 2]), thresholds=np.ones((2, 2)))
    with pytest.raises(engine.SmartEngineError, match='signatures: 2 of the 6 window ids') as e:
        engine.signatures(sim, obs, windows=np.array([0, 1, 2, 0, 3, 3]), n_windows=3)
    assert e.value.code == E_SIZE
    with pytest.raises(engine.SmartEngineError, match='windows must be integers'):
        engine.signatures(sim, obs, windows=np.zeros(6))
    with pytest.raises(engine.SmartEngineError, match='5 window ids for a matrix of shape'):
        engine.signatures(sim, obs, windows=np.zeros(5, dtype=np.int64))
    with pytest.raises(engine.SmartEngineError, match='n_windows = 2 without windows'):
        engine.signatures(sim, obs, n_windows=2)
    with pytest.raises(engine.SmartEngineError, match=r'a matrix \[R, N\] is needed'):
        engine.signatures(np.ones(6), obs)
    sig = inspect.signature(engine.signatures)
    assert list(sig.parameters) == ['discharge_report_major', 'obs', 'windows', 'n_windows', 'alpha', 'thresholds']
    assert sig.parameters['alpha'].default == 0.925 and sig.parameters['thresholds'].default is None


def test_every_workflow_has_hydrological_signatures():
    from smartpy_amd.montecarlo import LHS, GLUE, Best, Total
    from smartpy_amd.montecarlo.montecarlo import MonteCarlo
    for cls in (LHS, GLUE, Best, Total):
        assert cls.hydrological_signatures is MonteCarlo.hydrological_signatures
    sig = inspect.signature(MonteCarlo.hydrological_signatures)
    assert list(sig.parameters) == ['self', 'windows', 'alpha', 'high', 'low', 'thresholds', 'start_month', 'split', 'write']
    defaults = {k: p.default for k, p in sig.parameters.items() if k != 'self'}
    assert defaults == dict(windows='all', alpha=None, high=3.0, low=0.2, thresholds=None, start_month=10, split=None,
                            write=False)
    assert MonteCarlo.signatures_file.fget.__doc__.startswith('`<out>/<catchment>.SMART.<func>.signatures`')


def test_default_alpha_and_thresholds():
    from smartpy_amd import windows
    assert windows.default_alpha(1.0) == 0.925 and windows.default_alpha(0.5) == 0.925 ** 0.5
    assert windows.default_alpha(1.0 / 24.0) == 0.925 ** (1.0 / 24.0) and 0.0 < windows.default_alpha(30.0) < 0.925
    obs = np.array([1.0, 2.0, np.nan, 9.0, 4.0, np.nan, 6.0, 2.0, np.nan])
    ids = np.array([0, 0, 0, 0, 1, 1, 1, -1, 2], dtype=np.int32)
    got = windows.pulse_thresholds(obs, ids, 4)
    assert got.shape == (4, 2) and got.dtype == np.float64
    assert got[0].tolist() == [0.2 * 4.0, 3.0 * 2.0]                    # lo = 0.2 x mean(1, 2, 9), hi = 3 x median
    assert got[1].tolist() == [0.2 * 5.0, 3.0 * 5.0]
    assert np.isnan(got[2:]).all()                                      # every observation missing; a window that never occurs
    assert windows.pulse_thresholds(obs, ids, 2, high=2.0, low=0.5)[0].tolist() == [2.0, 4.0]


def test_the_signatures_file_and_the_result(tmp_path):
    from smartpy_amd import windows
    from smartpy_amd.montecarlo.analyses import _write_signatures_file
    from smartpy_amd.montecarlo.selection import as_stored
    assert windows.signatures_header_line(['2007', '2008']) == \
        ','.join(['%s@2007' % f for f in NAMES] + ['%s@2008' % f for f in NAMES]) + '\n'
    W, n = 2, 5
    values = (np.arange(W * 12 * n, dtype=np.float64).reshape(W, 12, n) - 7.0) / 3.0
    values[1, AC1, 2] = values[0, RLD, 4] = np.nan
    path = str(tmp_path / 'x.signatures')
    _write_signatures_file(path, ['a', 'b'], values)
    lines = open(path).read().split('\n')
    assert lines[0] + '\n' == windows.signatures_header_line(['a', 'b']) and lines[0].startswith('MEAN@a,BFI@a,')
    assert lines[-1] == '' and len(lines) == n + 2
    table = values.transpose(2, 0, 1).reshape(n, W * 12)
    for c in range(n):
        assert lines[1 + c].split(',') == ['%.6e' % np.float32(values[w, k, c]) for w in range(W) for k in range(12)]
    back = np.array([[float(v) for v in line.split(',')] for line in lines[1:-1]], dtype=np.float32)
    assert np.array_equal(back, as_stored(table), equal_nan=True)      # the round trip of the sampling database
    observed = values[:, :, 0] * 2.0
    thresholds = np.array([[0.5, 3.0], [0.25, np.nan]])
    r = windows.Signatures(['a', 'b'], 0.925, thresholds, values, None, observed, path)
    assert r.names == NAMES and r.labels == ['a', 'b'] and r.alpha == 0.925 and r.path == path
    assert r.values is values and r.device_values is None and r.observed is observed
    assert np.array_equal(r.thresholds, thresholds, equal_nan=True)
    want = (values - observed[:, :, None]) / np.abs(observed[:, :, None])
    assert np.array_equal(r.relative_error(), want, equal_nan=True) and r.relative_error().shape == (W, 12, n)
    # an empty sample: the header alone
    _write_signatures_file(path, ['a'], np.empty((1, 12, 0)))
    assert open(path).read() == windows.signatures_header_line(['a'])
