"""Flow duration curves, host side: the numpy statement of smart_flow_duration_hip (the truth of
tests/test_gpu_flow_duration.py as well), that statement against numpy's own 'inverted_cdf', the C entry's validation
without a device, the capacity and workspace functions, the engine's refusals, the Monte-Carlo surface, the exceedance ->
non-exceedance conversion and the `.fdc` file."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import support
from cases_flow_duration import CAPACITY
from conftest import GOLDEN
from oracle import objfn_oracle
from oracle.analyses.flow_duration import rank_of, statement
from support import E_MODE, E_NO_DEVICE, E_NULL, E_SIZE, FAKE


# ---- the statement ---------------------------------------------------------------------------------------------------
def test_statement_is_numpy_inverted_cdf():
    rng = np.random.default_rng(12)
    checked = 0
    for m in (1, 2, 3, 7, 8, 64, 100, 365, 1000, 4097):
        x = rng.normal(size=(m, 2))
        x[rng.integers(0, m, m // 3)] = 1.5                  # ties
        probs = [0.0, 1.0, 0.5, 0.25, 0.125, 1.0 / 3.0, 0.01, 0.99, 1.0 / m, (m - 1.0) / m, 0.3, 0.7]
        quant, scores = statement(x, probs)
        assert scores is None and quant.shape == (1, len(probs), 2)
        for k, q in enumerate(probs):
            want = np.quantile(x, q, axis=0, method='inverted_cdf')
            assert np.array_equal(quant[0, k], want), (m, q)
            checked += 1
    assert checked == 120
    assert rank_of(0.0, 10) == 1 and rank_of(1.0, 10) == 10 and rank_of(0.5, 10) == 5 and rank_of(0.51, 10) == 6


def test_statement_windows_missing_observations_and_nan_order():
    R = 12
    sim = np.arange(R, dtype=np.float64)[::-1].reshape(R, 1).copy()      # 11, 10, ... 0
    obs = np.ones(R)
    obs[[0, 5]] = np.nan
    win = np.array([0] * 6 + [1] * 6, dtype=np.int32)
    win[11] = -1
    quant, _ = statement(sim, [0.0, 0.5, 1.0], obs, win, 3)
    assert quant[0, :, 0].tolist() == [7.0, 8.0, 10.0]                    # rows 1 .. 4: 10, 9, 8, 7; rank ceil(0.5 * 4) = 2
    assert quant[1, :, 0].tolist() == [1.0, 3.0, 5.0]                     # rows 6 .. 10: 5 .. 1; rank ceil(2.5) = 3
    assert np.isnan(quant[2]).all()                                       # window 2 never occurs
    sim[2, 0], sim[3, 0] = np.nan, np.inf
    quant, _ = statement(sim, [0.5, 0.75, 1.0], obs, win, 2)
    assert quant[0, 0, 0] == 10.0 and quant[0, 1, 0] == np.inf and np.isnan(quant[0, 2, 0])      # 7, 10, inf, NaN


def test_statement_objective_functions_segments_and_rules():
    rng = np.random.default_rng(4)
    R = 200
    obs = np.abs(rng.normal(3.0, 1.5, R)) + 0.1
    obs[[3, 50]] = np.nan
    sim = rng.random((R, 3)) * 6 + 0.01
    keep = ~np.isnan(obs)
    _, whole = statement(sim, [0.5], obs, None, 1, objfn=True)
    want = objfn_oracle.objective_functions(np.sort(sim[keep, 1]), np.sort(obs[keep]))[:7]
    assert np.array_equal(whole[0, 1], want)
    _, top = statement(sim, [0.5], obs, None, 1, 'log', 0.05, (0.98, 1.0), objfn=True)
    m = int(keep.sum())
    assert m == 198                                                       # 0.98 * 198 = 194.04: ranks 195 .. 197
    want = objfn_oracle.objective_functions(np.log(np.sort(sim[keep, 2])[195:] + 0.05), np.log(np.sort(obs[keep])[195:] + 0.05))
    assert np.array_equal(top[0, 2], want[:7])
    _, low = statement(sim, [0.5], obs, None, 1, 'sqrt', 0.0, (0.0, 0.3), objfn=True)
    want = objfn_oracle.objective_functions(np.sqrt(np.sort(sim[keep, 0])[:60]), np.sqrt(np.sort(obs[keep])[:60]))   # 59.4
    assert np.array_equal(low[0, 0], want[:7])
    # the two rules, on the pairs that take part
    _, few = statement(sim, [0.5], obs, None, 1, segment=(0.99, 1.0), objfn=True)      # 196.02 <= i: one rank
    assert np.isnan(few).all()
    bad = sim.copy()
    bad[7, 1] = -1.0                                                      # the smallest value of column 1
    _, a = statement(bad, [0.5], obs, None, 1, 'log', 0.05, (0.0, 0.3), objfn=True)
    _, b = statement(bad, [0.5], obs, None, 1, 'log', 0.05, (0.98, 1.0), objfn=True)
    assert np.isnan(a[0, 1]).all() and not np.isnan(a[0, [0, 2]]).any() and not np.isnan(b).any()
    bad[7, 1] = np.nan                                                    # ... now the largest
    _, a = statement(bad, [0.5], obs, None, 1, 'none', 0.0, (0.0, 0.3), objfn=True)
    _, b = statement(bad, [0.5], obs, None, 1, 'none', 0.0, (0.98, 1.0), objfn=True)
    assert not np.isnan(a).any() and np.isnan(b[0, 1]).all() and not np.isnan(b[0, [0, 2]]).any()
    zero = obs.copy()
    zero[9] = 0.0
    _, a = statement(sim, [0.5], zero, None, 1, 'log', 0.0, (0.0, 0.3), objfn=True)
    _, b = statement(sim, [0.5], zero, None, 1, 'log', 0.0, (0.5, 1.0), objfn=True)
    assert np.isnan(a).all() and not np.isnan(b).any()


# ---- the C entry -----------------------------------------------------------------------------------------------------
def test_symbols_capacity_and_workspace():
    binding, L = support.binding()
    for name in ('smart_flow_duration_hip', 'smart_flow_duration_workspace_bytes', 'smart_flow_duration_sort_capacity'):
        assert name in binding.SYMBOLS
    assert L.smart_abi_version() == 7
    assert L.smart_flow_duration_sort_capacity() == CAPACITY
    assert binding.FDC_METHODS == {'auto': 0, 'sort': 1, 'select': 2}
    from smartpy_amd import engine
    assert engine.flow_duration_sort_capacity() == CAPACITY
    ws = L.smart_flow_duration_workspace_bytes
    assert ws(3653, 10, 0) == 0 and ws(1, 1, 0) == 0
    for r, w in ((1, 1), (501, 7), (3653, 10), (CAPACITY, 1024)):
        need = ws(r, w, 1)
        assert need % 256 == 0 and 0 <= need - w * (8 + r) * 8 < 256, (r, w)
    assert ws(0, 1, 1) == E_SIZE and ws(5, 0, 1) == E_SIZE and ws(2 ** 31, 1, 0) == E_SIZE
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'smart_amd.h')).read()
    for word, code in (('AUTO', 0), ('SORT', 1), ('SELECT', 2)):
        assert '#define SMART_FDC_%s %d' % (word, code) in header
    assert "method='inverted_cdf'" in header and 'fewer than two pairs' in header and 'not finite' in header


def test_validation_comes_before_the_device():
    binding, L = support.binding()
    max_windows = L.smart_objfn_max_windows()
    half = (ctypes.c_double * 16)(*([0.5] * 16))

    def call(n=100, r=50, sim=FAKE, ld=None, obs=FAKE, window=FAKE, w=3, probs=half, k=3, quant=FAKE, transform=0, eps=0.0,
             lo=0.0, hi=1.0, objfn=None, work=None, work_bytes=0, method=0):
        rc = L.smart_flow_duration_hip(n, r, sim, n if ld is None else ld, obs, window, w, probs, k, quant, transform, eps,
                                       lo, hi, objfn, work, work_bytes, method, None)
        return rc, L.smart_last_error().decode()

    def probs_of(*values):
        return (ctypes.c_double * len(values))(*values)

    for name in ('sim', 'probs', 'quant'):
        rc, text = call(**{name: None})
        assert rc == E_NULL and 'smart_flow_duration_hip' in text and '(%s is NULL)' % name in text, name
    rc, text = call(objfn=FAKE, obs=None, work=FAKE, work_bytes=1 << 20)
    assert rc == E_NULL and 'objfn needs obs' in text
    rc, text = call(objfn=FAKE, work=None)
    assert rc == E_NULL and 'workspace is NULL' in text
    need = L.smart_flow_duration_workspace_bytes(50, 3, 1)
    for kw, word in ((dict(n=0), 'n_samples'), (dict(n=-2), 'n_samples'), (dict(r=0), 'n_reports'), (dict(w=0), 'n_windows'),
                     (dict(k=0), 'n_probs'), (dict(ld=99), 'ld'), (dict(r=2 ** 31), 'n_reports'),
                     (dict(w=max_windows + 1), 'n_windows'), (dict(window=None, w=2), 'n_windows'), (dict(k=17), 'n_probs'),
                     (dict(probs=probs_of(0.5, -1e-9, 0.5)), 'probability 1'), (dict(probs=probs_of(0.5, 0.5, 1.0000001)), 'probability 2'),
                     (dict(probs=probs_of(float('nan'), 0.5, 0.5)), 'probability 0'), (dict(probs=probs_of(float('inf'), 0.5, 0.5)), 'probability 0'),
                     (dict(eps=-1e-300), 'eps'), (dict(eps=float('inf')), 'eps'), (dict(eps=float('nan')), 'eps'),
                     (dict(lo=-0.1), 'segment'), (dict(lo=0.5, hi=0.5), 'segment'), (dict(lo=0.6, hi=0.5), 'segment'),
                     (dict(hi=1.5), 'segment'), (dict(lo=float('nan')), 'segment'), (dict(hi=float('nan')), 'segment'),
                     (dict(objfn=FAKE, work=FAKE, work_bytes=need - 1), 'workspace_bytes'),
                     (dict(r=CAPACITY + 1, method=1), 'sort form takes at most %d' % CAPACITY),
                     (dict(r=CAPACITY + 1, objfn=FAKE, work=FAKE, work_bytes=1 << 30), 'take at most %d' % CAPACITY),
                     (dict(r=CAPACITY + 1, objfn=FAKE, work=FAKE, work_bytes=1 << 30, method=1), 'at most %d' % CAPACITY)):
        rc, text = call(**kw)
        assert rc == E_SIZE and 'smart_flow_duration_hip' in text and word in text, (kw, text)
    for t in (-1, 4, 99):
        rc, text = call(transform=t)
        assert rc == E_MODE and 'transform' in text, t
    for how in (-1, 3, 99):
        rc, text = call(method=how)
        assert rc == E_MODE and 'method' in text, how
    rc, text = call(objfn=FAKE, work=FAKE, work_bytes=need, method=2)
    assert rc == E_MODE and 'select form' in text
    # the order: NULL before SIZE before MODE
    assert call(sim=None, n=0, transform=9)[0] == E_NULL
    assert call(n=0, transform=9)[0] == E_SIZE and call(eps=-1.0, method=9)[0] == E_SIZE
    # probabilities 0 and 1 are inside, and so are eps 0 and the whole curve
    if L.smart_device_count() == 0:
        # a well-formed call gets as far as the device, and no further: there is no CPU fallback
        for kw in (dict(), dict(probs=probs_of(0.0, 1.0, 0.5)), dict(window=None, w=1, obs=None), dict(k=16),
                   dict(objfn=FAKE, work=FAKE, work_bytes=need, transform=2, eps=0.5, lo=0.98), dict(r=CAPACITY + 1),
                   dict(r=CAPACITY + 1, method=2), dict(r=CAPACITY, method=1, w=max_windows)):
            assert call(**kw)[0] == E_NO_DEVICE, kw


# ---- engine and Monte-Carlo surface ----------------------------------------------------------------------------------
def test_engine_refuses_before_any_device_call():
    from smartpy_amd import engine
    sim, obs = np.ones((6, 4)), np.ones(6)
    with pytest.raises(engine.SmartEngineError, match="transform 'cube' unknown") as e:
        engine.flow_duration(sim, [0.5], transform='cube')
    assert e.value.code == E_MODE
    with pytest.raises(engine.SmartEngineError, match="method 'heap' unknown") as e:
        engine.flow_duration(sim, [0.5], method='heap')
    assert e.value.code == E_MODE
    with pytest.raises(engine.SmartEngineError, match='need obs') as e:
        engine.flow_duration(sim, [0.5], objfn=True)
    assert e.value.code == E_NULL
    with pytest.raises(engine.SmartEngineError, match='flow_duration: 2 of the 6 window ids') as e:
        engine.flow_duration(sim, [0.5], obs, windows=np.array([0, 1, 2, 0, 3, 3]), n_windows=3)
    assert e.value.code == E_SIZE
    with pytest.raises(engine.SmartEngineError, match='5 window ids for a matrix of shape'):
        engine.flow_duration(sim, [0.5], obs, windows=np.zeros(5, dtype=np.int64))
    with pytest.raises(engine.SmartEngineError, match='n_windows = 2 without windows'):
        engine.flow_duration(sim, [0.5], obs, n_windows=2)
    sig = inspect.signature(engine.flow_duration)
    assert list(sig.parameters) == ['discharge_report_major', 'probs', 'obs', 'windows', 'n_windows', 'transform', 'eps',
                                    'segment', 'objfn', 'method']


def test_every_workflow_has_flow_duration_curves():
    from smartpy_amd.montecarlo import LHS, GLUE, Best, Total
    from smartpy_amd.montecarlo.montecarlo import MonteCarlo
    for cls in (LHS, GLUE, Best, Total):
        assert cls.flow_duration_curves is MonteCarlo.flow_duration_curves
    sig = inspect.signature(MonteCarlo.flow_duration_curves)
    assert list(sig.parameters) == ['self', 'exceedance', 'windows', 'transform', 'eps', 'segment', 'start_month', 'split',
                                    'write']
    defaults = {k: p.default for k, p in sig.parameters.items() if k != 'self'}
    assert defaults == dict(exceedance=(0.01, 0.05, 0.1, 0.2, 0.5, 0.8, 0.9, 0.95, 0.99), windows='all', transform='none',
                            eps=None, segment=(0.0, 1.0), start_month=10, split=None, write=False)
    assert 'q = 1 - p' in MonteCarlo.flow_duration_curves.__doc__


def test_exceedance_becomes_non_exceedance_on_the_host():
    from smartpy_amd import windows
    p = (0.01, 0.05, 0.5, 0.95, 0.99, 0.0, 1.0)
    q = windows.non_exceedance(p)
    assert q.dtype == np.float64 and q.tolist() == [1.0 - x for x in p] and q[-2] == 1.0 and q[-1] == 0.0
    assert windows.non_exceedance(0.25).tolist() == [0.75]
    for bad in ((-0.1,), (1.1, 0.5), (float('nan'),), ()):
        with pytest.raises(Exception, match='between 0 and 1'):
            windows.non_exceedance(bad)
    # Q1 (exceeded 1 % of the time) is a HIGH flow: the 99th of 100 ascending values
    obs = np.arange(1.0, 101.0)
    obs[17] = np.nan
    ids = np.zeros(100, dtype=np.int32)
    ids[90:] = 1
    got = windows.observed_duration(obs, ids, 3, windows.non_exceedance((0.01, 0.5, 1.0)))
    x0 = np.sort(obs[:90][~np.isnan(obs[:90])])
    assert got.shape == (3, 3) and got[0].tolist() == [x0[rank_of(0.99, 89) - 1], x0[rank_of(0.5, 89) - 1], x0[0]]
    assert got[0, 0] == 90.0 and got[1].tolist() == [100.0, 95.0, 91.0] and np.isnan(got[2]).all()
    want, _ = statement(obs.reshape(100, 1), windows.non_exceedance((0.01, 0.5, 1.0)), obs, ids, 3)
    assert np.array_equal(got, want[:, :, 0], equal_nan=True)


def test_the_fdc_file(tmp_path):
    from smartpy_amd import windows
    from smartpy_amd.montecarlo.analyses import _write_fdc_file
    names = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE']
    assert windows.fdc_header_line((0.01, 0.5), ['2007', '2008'], 'log') == \
        ','.join(['Q0.01@2007', 'Q0.5@2007', 'Q0.01@2008', 'Q0.5@2008'] + ['%s:log@2007' % f for f in names]
                 + ['%s:log@2008' % f for f in names]) + '\n'
    assert windows.fdc_header_line((0.95,), ['all']) == ','.join(['Q0.95@all'] + ['%s@all' % f for f in names]) + '\n'
    W, K, n = 2, 3, 4
    curves = (np.arange(W * K * n, dtype=np.float64).reshape(W, K, n) + 0.5) / 3.0
    values = np.arange(W * n * 7, dtype=np.float64).reshape(W, n, 7) / 7.0
    values[1, 2, 4] = np.nan
    curves[0, 1, 3] = np.nan
    path = str(tmp_path / 'x.fdc')
    _write_fdc_file(path, (0.1, 0.5, 0.9), ['a', 'b'], 'sqrt', curves, values)
    lines = open(path).read().split('\n')
    assert lines[0] + '\n' == windows.fdc_header_line((0.1, 0.5, 0.9), ['a', 'b'], 'sqrt')
    assert lines[-1] == '' and len(lines) == n + 2 and len(lines[0].split(',')) == W * K + W * 7
    for c in range(n):
        want = ['%.6e' % np.float32(curves[w, k, c]) for w in range(W) for k in range(K)]
        want += ['%.6e' % np.float32(v) for w in range(W) for v in values[w, c]]
        assert lines[1 + c].split(',') == want
    r = windows.FlowDuration((0.1, 0.5, 0.9), ['a', 'b'], curves, np.zeros((W, K)), 'sqrt', 0.0, (0.0, 1.0), values, None, path)
    assert r.names == names and r.labels == ['a', 'b'] and r.exceedance == [0.1, 0.5, 0.9] and r.file == path
    assert r.curves is curves and r.values is values and r.device_values is None and r.segment == (0.0, 1.0)
    assert r.observed.shape == (W, K) and r.transform == 'sqrt' and r.eps == 0.0
    # an empty sample: the header alone
    _write_fdc_file(path, (0.5,), ['a'], 'none', np.empty((1, 1, 0)), np.empty((1, 0, 7)))
    assert open(path).read() == windows.fdc_header_line((0.5,), ['a'])
