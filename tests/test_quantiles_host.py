"""Weighted ensemble quantiles (the GLUE prediction bounds), host side: the definition as a numpy statement -- what
tests/test_gpu_quantiles.py holds the kernels against --, the C entry's validation (done before the device is touched,
so a machine without a GPU can test it), and the part of GLUE that needs no launch."""
import ctypes
import inspect
import json
import math
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

E_NULL, E_SIZE, E_NO_DEVICE, E_MODE = -1, -2, -6, -7
DYADIC = (0.0625, 0.5, 0.9375, 1.0)


def weighted_quantile(x, w, q):
    """THE DEFINITION for one report step: the smallest value v among x with sum(w[x <= v]) >= q * sum(w); NaN sorts
    last (numpy.sort), a total weight of zero gives NaN; w = None: equal weights."""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(x.size) if w is None else np.asarray(w, dtype=np.float64)
    order = np.argsort(x, kind='stable')
    cum = np.cumsum(w[order])
    if not cum[-1] > 0.0:
        return float('nan')
    first = np.searchsorted(cum, q * cum[-1], side='left')     # the first position with cum >= q * W
    return float(x[order][first])


def statement(matrix, w, probs):
    """weighted_quantile for every row of a [R, N] matrix -> [K, R]."""
    return np.array([[weighted_quantile(row, w, q) for row in np.asarray(matrix)] for q in probs])


def band_violations(x, w, q, v):
    """What a weighted quantile computed in ANY summation order must satisfy for general (inexact) weights: v is an
    element of the row, sum(w[x < v]) <= qW (1 + eps) and sum(w[x <= v]) >= qW (1 - eps) with eps = N * 2**-52 (the
    sums taken exactly here).  -> list of what fails (empty: fine)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    eps = x.size * 2.0 ** -52
    t = q * math.fsum(w)
    below, upto = math.fsum(w[x < v]), math.fsum(w[x <= v])
    problems = []
    if not np.any(x == v):
        problems.append('%r is no element of the row' % v)
    if not below <= t * (1 + eps):
        problems.append('q=%g: sum(w[x < v]) = %r > %r' % (q, below, t * (1 + eps)))
    if not upto >= t * (1 - eps):
        problems.append('q=%g: sum(w[x <= v]) = %r < %r' % (q, upto, t * (1 - eps)))
    return problems


# ---- the statement itself -----------------------------------------------------------------------------------------
def test_statement_is_numpys_inverted_cdf_with_weights():
    rng = np.random.default_rng(20240607)
    for n in (1, 2, 7, 64, 65, 301):
        x = rng.normal(size=n)
        if n > 10:
            x[::5] = x[1]                                   # ties
        w = rng.integers(0, 6, size=n).astype(np.float64)
        w[0] = 3.0                                          # (a total above zero)
        for q in DYADIC:
            assert weighted_quantile(x, w, q) == np.quantile(x, q, method='inverted_cdf', weights=w), (n, q)
            assert weighted_quantile(x, None, q) == np.quantile(x, q, method='inverted_cdf'), (n, q)


def test_statement_edge_cases():
    nan, inf = float('nan'), float('inf')
    x = np.array([3.0, nan, -1.0, inf, 2.0])
    w = np.array([1.0, 1.0, 1.0, 1.0, 0.0])
    assert weighted_quantile(x, w, 0.25) == -1.0 and weighted_quantile(x, w, 0.5) == 3.0
    assert weighted_quantile(x, w, 0.75) == inf and math.isnan(weighted_quantile(x, w, 1.0))
    assert math.isnan(weighted_quantile(x, np.zeros(5), 0.5))
    # weight zero never decides: the smallest and the largest value carry none
    assert weighted_quantile([1.0, 2.0, 3.0], [0.0, 1.0, 0.0], 0.0625) == 2.0
    assert weighted_quantile([1.0, 2.0, 3.0], [0.0, 1.0, 0.0], 1.0) == 2.0
    assert weighted_quantile([0.0, -0.0, 5e-324, -5e-324], None, 0.5) == 0.0
    assert statement([[1.0, 2.0], [4.0, 3.0]], None, [0.5, 1.0]).tolist() == [[1.0, 3.0], [2.0, 4.0]]


def test_statement_meets_the_band_for_general_weights():
    """The band tests/test_gpu_quantiles.py holds the kernels to for uniform float weights is not vacuous: the statement
    (sequential sums) lies inside it, a neighbouring element of the row does not."""
    rng = np.random.default_rng(5)
    for n in (65, 1000, 8257):
        x, w = rng.normal(size=n), rng.uniform(size=n)
        ranked = np.sort(x)
        for q in (0.05, 0.5, 0.95):
            v = weighted_quantile(x, w, q)
            assert band_violations(x, w, q, v) == []
            at = int(np.searchsorted(ranked, v))
            assert band_violations(x, w, q, ranked[at - 1]) and band_violations(x, w, q, ranked[at + 1])


# ---- the C entry ----------------------------------------------------------------------------------------------------
def _lib():
    from smartpy_amd import _lib as binding
    return binding, binding.lib()


def test_symbols_are_bound_and_capacity_needs_no_device():
    binding, L = _lib()
    assert 'smart_weighted_quantiles_hip' in binding.SYMBOLS and 'smart_quantiles_sort_capacity' in binding.SYMBOLS
    cap = L.smart_quantiles_sort_capacity()
    assert cap >= 1024
    from smartpy_amd import engine
    assert engine.quantiles_sort_capacity() == cap and callable(engine.weighted_quantiles)
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'smart_amd.h')).read()
    assert 'inverted_cdf' in header and 'finite and >= 0' in header


def test_validation_comes_before_the_device():
    binding, L = _lib()
    cap = L.smart_quantiles_sort_capacity()
    fake = 4096                         # a non-NULL address that is never followed: every call below is refused first

    def call(n=100, r=5, sim=fake, ld=None, w=None, probs=(0.05, 0.5, 0.95), k=None, out=fake, method=0):
        q = None if probs is None else (ctypes.c_double * len(probs))(*probs)
        rc = L.smart_weighted_quantiles_hip(n, r, sim, n if ld is None else ld, w, q,
                                            (len(probs) if probs is not None else 3) if k is None else k, out, method,
                                            None)
        return rc, L.smart_last_error().decode()

    for kw in (dict(sim=None), dict(probs=None), dict(out=None)):
        rc, text = call(**kw)
        assert rc == E_NULL and 'smart_weighted_quantiles_hip' in text, kw
    for kw in (dict(n=0), dict(r=0), dict(k=0), dict(n=-3), dict(ld=99), dict(probs=(0.5, 0.0)), dict(probs=(1.5,)),
               dict(probs=(-0.25,)), dict(probs=(float('nan'),)), dict(probs=(0.5,) * 17),
               dict(n=cap + 1, method=1)):
        rc, text = call(**kw)
        assert rc == E_SIZE and 'smart_weighted_quantiles_hip' in text, kw
    assert call(probs=(0.5,) * 16, method=7)[0] == E_MODE and call(method=-1)[0] == E_MODE
    assert 'method' in call(method=3)[1]
    if L.smart_device_count() == 0:
        # a well-formed call gets as far as the device, and no further: there is no CPU fallback
        for kw in (dict(), dict(n=cap, method=1), dict(n=cap + 1, method=2), dict(n=cap + 1), dict(probs=(1.0,))):
            assert call(**kw)[0] == E_NO_DEVICE, kw
    else:
        import torch
        sim, out = torch.rand(5, 100, dtype=torch.float64, device='cuda'), torch.empty(3, 5, dtype=torch.float64,
                                                                                       device='cuda')
        assert call(sim=sim.data_ptr(), out=out.data_ptr())[0] == 0
        torch.cuda.synchronize()


# ---- GLUE -----------------------------------------------------------------------------------------------------------
NAMES = ['T', 'C', 'H', 'D', 'S', 'Z', 'SK', 'FK', 'GK', 'RK']
OBJ = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE', 'GW']


@pytest.fixture()
def root(tmp_path):
    r = str(tmp_path / 'data')
    shutil.copytree(os.path.join(GOLDEN, 'data', 'in'), os.path.join(r, 'in'))
    with open(os.path.join(r, 'in', 'Catchment', 'Catchment.short.sttngs'), 'w') as f:
        f.write('ARGUMENT,VALUE\ncatchment_area_km2,175.46\ngauged_area_km2,175.97\nstart_datetime,01/01/2007 09:00:00\n'
                'end_datetime,01/03/2007 09:00:00\nsimu_timedelta_min,60\nreport_timedelta_min,1440\nwarm_up_days,10\n'
                'gw_constraint,0.12667\n')
    return r


def test_glue_has_prediction_bounds_and_its_constructor_is_what_it_was(root):
    from smartpy_amd.montecarlo import GLUE
    assert list(inspect.signature(GLUE.prediction_bounds).parameters) == ['self', 'quantiles', 'likelihood', 'write']
    defaults = {k: p.default for k, p in inspect.signature(GLUE.prediction_bounds).parameters.items()}
    assert defaults['quantiles'] == (0.05, 0.5, 0.95) and defaults['likelihood'] is None and defaults['write'] is False
    # without the database of a sampling run there is nothing to condition: the reader's error, as before
    with pytest.raises(FileNotFoundError, match='Catchment.SMART.lhs'):
        GLUE('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (0.5,))},
             settings_filename='Catchment.short.sttngs')


def test_behavioural_objective_functions_follow_the_mask_on_the_file_path(root):
    """KAT-12 (the fixtures of tests/test_montecarlo_golden.py): GLUE built from a database file keeps, next to the
    behavioural parameter rows, the sampling run's objective functions of those same rows."""
    from smartpy_amd.montecarlo import GLUE
    from smartpy_amd.montecarlo.database import SamplingCsv
    z = load_golden('kat12_selection.npz')
    with open(os.path.join(GOLDEN, 'kat12_selection.json')) as fh:
        cases = json.load(fh)
    params, fns = z['params'], z['obj_fns']
    os.makedirs(os.path.join(root, 'out', 'Catchment'), exist_ok=True)
    db = SamplingCsv(os.path.join(root, 'out', 'Catchment', 'Catchment.SMART.lhs'), OBJ, NAMES).create(len(params))
    db.write_table(fns, params)
    db.close()
    for c in cases['glue']:
        cond = {OBJ[col]: (kind, tuple(val)) for col, kind, val in zip(c['columns'], c['kinds'], c['values'])}
        glue = GLUE('Catchment', root, 'csv', 'csv', conditioning=cond, settings_filename='Catchment.short.sttngs')
        assert [int(v) for v in glue.behavioural_params[:, 0]] == c['rows'], c
        assert glue.behavioural_obj_fns.dtype == np.float32
        assert np.array_equal(glue.behavioural_obj_fns, fns[c['rows']], equal_nan=True), c
        # the weights prediction_bounds would use, and the ones it refuses (no launch is made for either)
        if len(c['rows']):
            by_name = glue._likelihood_weights('KGEa')
            assert by_name.dtype == np.float64 and np.array_equal(by_name, fns[c['rows'], 3].astype(np.float64))
            with pytest.raises(Exception, match='negative or not finite'):
                glue.prediction_bounds(likelihood=-np.ones(len(c['rows'])))
            with pytest.raises(Exception, match='negative or not finite'):
                glue.prediction_bounds(likelihood=np.full(len(c['rows']), np.nan))
            with pytest.raises(Exception, match='one value per behavioural set'):
                glue.prediction_bounds(likelihood=np.ones(len(c['rows']) + 1))
            with pytest.raises(Exception, match="'Nash'"):
                glue.prediction_bounds(likelihood='Nash')
        else:
            out = glue.prediction_bounds(quantiles=(0.25, 0.75))       # nothing behavioural: nothing is launched
            assert out.bounds.shape == (2, len(glue.model.timeseries_report) - 1) and np.isnan(out.bounds).all()
            assert math.isnan(out.containment) and list(out.quantiles) == [0.25, 0.75]
            assert out.datetime == glue.model.timeseries_report[1:]
