"""Weighted ensemble quantiles (the GLUE prediction bounds), host side: the definition as a numpy statement -- what
tests/test_gpu_quantiles.py holds the kernels against --, the C entry's validation (done before the device is touched,
so a machine without a GPU can test it), and the part of GLUE that needs no launch."""
import ctypes
import inspect
import json
import math
import os

import numpy as np
import pytest

import support
from conftest import GOLDEN, load_golden
from oracle.analyses.quantiles import (DYADIC, HUGE, NAN_BITS, NAN_SHARE, SUBNORMAL, THRESHOLD_SIZES, band_violations,
                                       distinct_rows, is_power_of_two, many_nan_rows, mixed_nans, power_of_two_weights,
                                       statement, statement_rows, threshold_probs, weighted_quantile,
                                       weightless_successor)
from support import E_MODE, E_NO_DEVICE, E_NULL, E_SIZE, FAKE, example_root, same_bits, settings_file


# ---- the statement itself -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', THRESHOLD_SIZES)
def test_threshold_constructions_are_sound(n):
    """power_of_two_weights and threshold_probs against the statement: the three probabilities around sixteen partial
    sums give exactly the values the construction names (also where the successor weighs nothing), and a power-of-two
    scale of the weights changes nothing.  With 2**-1060 every weight and W itself are subnormal: the partial sums stay
    exact (multiples of 2**-1070), and so does q * W for a dyadic q; for a q one ulp off a partial sum the product
    rounds ONTO that sum down there, so the ulp-neighbours are scaled up only."""
    rng = np.random.default_rng(4000 + n)
    w = power_of_two_weights(rng, n)
    assert w.shape == (n,) and (w > 0).all() and np.array_equal(w * 1024.0, np.round(w * 1024.0))
    assert is_power_of_two(w.sum()) and is_power_of_two(math.fsum(w)) and w.sum() == math.fsum(w)
    x = distinct_rows(rng, 1, n)[0]
    positions = rng.choice(n - 1, size=16, replace=False)
    probs, values = threshold_probs(x, w, positions)
    assert len(probs) == 48 and len(set(probs)) == 48
    got = statement([x], w, probs)[:, 0]
    assert np.array_equal(got, values), (n, positions)
    ranked = np.sort(x)
    at = np.searchsorted(ranked, values)
    assert np.array_equal(at[0::3], positions) and np.array_equal(at[1::3], positions + 1)
    assert np.array_equal(at[2::3], positions)
    # ... the successor of one position without weight: one ulp above skips it
    w0, j = weightless_successor(x, w, rng)
    assert is_power_of_two(w0.sum()) and w0.sum() == w.sum() and np.count_nonzero(w0 == 0.0) == 1
    p0, v0 = threshold_probs(x, w0, [j])
    assert v0.tolist() == [ranked[j], ranked[j + 2], ranked[j]]
    assert np.array_equal(statement([x], w0, p0)[:, 0], v0)
    # ... the scale of the weights
    assert (w * SUBNORMAL > 0).all() and (w * SUBNORMAL < 2.0 ** -1022).all() and w.sum() * SUBNORMAL < 2.0 ** -1022
    assert np.array_equal(w * SUBNORMAL / SUBNORMAL, w) and np.array_equal(w * HUGE / HUGE, w)
    rows = rng.normal(size=(2, n))
    want = statement(rows, w, DYADIC)
    assert same_bits(statement(rows, w * SUBNORMAL, DYADIC), want) and same_bits(statement(rows, w * HUGE, DYADIC), want)
    assert not np.isnan(want).any()
    assert np.array_equal(statement([x], w * HUGE, probs)[:, 0], values)
    assert np.array_equal(statement([x], w0 * HUGE, p0)[:, 0], v0)


def test_statement_on_rows_where_nans_decide():
    """numpy sorts every NaN last, whatever its sign and payload: with two fifths of a row NaN (and weights that give
    them between a sixteenth and a half of the total) the upper quantiles are NaN and the lower ones are not."""
    assert np.isnan(NAN_BITS.view(np.float64)).all() and len(set(NAN_BITS.tolist())) == len(NAN_BITS)
    assert np.signbit(NAN_BITS.view(np.float64)).sum() == 4
    rng = np.random.default_rng(99)
    for n in (64, 65, 1025, 8192, 8257):
        x = many_nan_rows(rng, rng.normal(size=(5, n)))
        assert (np.isnan(x).sum(axis=1) == math.ceil(NAN_SHARE * n)).all() and np.isnan(x).mean() > 1 / 3
        assert len(set(x[np.isnan(x)].view(np.uint64).tolist())) == len(NAN_BITS)
        assert np.isnan(np.sort(x, axis=1)[:, -int(NAN_SHARE * n):]).all()
        w = rng.integers(1, 2 ** 20, size=n).astype(np.float64) / 1024.0
        want = statement(x, w, DYADIC)                                   # DYADIC = (0.0625, 0.5, 0.9375, 1.0)
        assert np.isnan(want[2:]).all() and not np.isnan(want[:2]).any(), n
        assert np.array_equal(want, statement(np.where(np.isnan(x), np.nan, x), w, DYADIC), equal_nan=True)
        assert np.isnan(statement(mixed_nans(rng, (2, n)), w, DYADIC)).all()
        # without weight the NaNs decide nothing: the row without them answers the same
        x[:] = rng.normal(size=(5, n))
        cols = rng.permutation(n)[:int(NAN_SHARE * n)]
        w[cols] = 0.0
        want = statement(np.delete(x, cols, axis=1), np.delete(w, cols), DYADIC)
        x[:, cols] = mixed_nans(rng, (5, cols.size))
        assert same_bits(statement(x, w, DYADIC), want) and not np.isnan(want).any()


def test_statement_rows_is_the_statement():
    rng = np.random.default_rng(12)
    for n, w in ((1, None), (3, np.array([0.25, 0.5, 0.25])), (3, np.zeros(3)), (7, rng.integers(0, 4, size=7) / 4.0)):
        x = rng.integers(0, 5, size=(50, n)).astype(np.float64)
        x[rng.random(size=x.shape) < 0.1] = np.nan
        probs = (0.0625, 0.5, 0.75, 1.0)
        assert same_bits(statement_rows(x, w, probs), statement(x, w, probs)), n


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
def test_symbols_are_bound_and_capacity_needs_no_device():
    binding, L = support.binding()
    assert 'smart_weighted_quantiles_hip' in binding.SYMBOLS and 'smart_quantiles_sort_capacity' in binding.SYMBOLS
    cap = L.smart_quantiles_sort_capacity()
    assert cap >= 1024
    from smartpy_amd import engine
    assert engine.quantiles_sort_capacity() == cap and callable(engine.weighted_quantiles)
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'smart_amd.h')).read()
    assert 'inverted_cdf' in header and 'finite and >= 0' in header


def test_validation_comes_before_the_device():
    binding, L = support.binding()
    cap = L.smart_quantiles_sort_capacity()

    def call(n=100, r=5, sim=FAKE, ld=None, w=None, probs=(0.05, 0.5, 0.95), k=None, out=FAKE, method=0):
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
    r = example_root(tmp_path)
    settings_file(r, 'Catchment.short.sttngs', '01/01/2007', '01/03/2007', 10)
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
