"""Weighted ensemble quantiles on the GPU (smartpy_amd/csrc/smart_quantiles.hip) against the numpy statement of the
definition in tests/test_quantiles_host.py: both forms, every size at which the code takes another path, the C entry
with its own leading dimension, the engine and GLUE.prediction_bounds on top."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from test_quantiles_host import statement, band_violations, DYADIC

pytestmark = pytest.mark.gpu

AUTO, SORT, SELECT = 0, 1, 2
EXTRA = {'aar': 1200, 'r-o_ratio': 0.45, 'r-o_split': (0.10, 0.15, 0.15, 0.30, 0.30)}
# the 'min' threshold on the sampling run's NSE in the GLUE test: between 10 and 200 of the 256 seeded rows pass
NSE_MIN = 0.2


def capacity():
    from smartpy_amd import engine
    return engine.quantiles_sort_capacity()


def launch(matrix, weights, probs, method, pad=0, junk=np.nan):
    """The C entry on a [R, N] host matrix laid out with ld = N + pad (the padding holds `junk`) -> numpy [K, R]."""
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    matrix = np.asarray(matrix, dtype=np.float64)
    R, N = matrix.shape
    host = np.full((R, N + pad), junk)
    host[:, :N] = matrix
    sim = torch.from_numpy(host).cuda()
    w = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).cuda()
    q = (ctypes.c_double * len(probs))(*probs)
    out = torch.full((len(probs), R), -7.0, dtype=torch.float64, device='cuda')
    _lib.check(L.smart_weighted_quantiles_hip(N, R, sim.data_ptr(), N + pad, None if w is None else w.data_ptr(), q,
                                              len(probs), out.data_ptr(), method,
                                              torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


def same(a, b):
    """`==` everywhere (so -0.0 is 0.0), NaN where NaN."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def exact_weights(rng, n):
    """Integer multiples of 2**-10 below 2**10: every partial sum is exact in any order."""
    return rng.integers(1, 2 ** 20, size=n).astype(np.float64) / 1024.0


def contents(kind, rng, R, N):
    """-> (matrix [R, N], weights [N] or None)."""
    w = exact_weights(rng, N)
    x = rng.normal(size=(R, N))
    if kind == 'random':
        pass
    elif kind == 'equal':
        x[:] = 2.5
    elif kind == 'ties':
        x = rng.integers(0, 8, size=(R, N)).astype(np.float64)
    elif kind == 'zero_third':
        w[rng.permutation(N)[:N // 3]] = 0.0
        w[np.argmin(x[0])] = w[np.argmax(x[0])] = 0.0           # the ends of the first step carry no weight
    elif kind == 'one_nan':
        x[np.arange(R), rng.integers(0, N, size=R)] = np.nan
    elif kind == 'inf':
        x[rng.random(size=(R, N)) < 0.2] = np.inf
        x[rng.random(size=(R, N)) < 0.1] = -np.inf
        x[:, -1] = np.inf
    elif kind == 'tiny':
        x = rng.choice(np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.3e-308, -2.3e-308]), size=(R, N))
    elif kind == 'zero_weights':
        w[:] = 0.0
    elif kind == 'none':
        w = None
    else:
        raise AssertionError(kind)
    return x, w


KINDS = ['random', 'equal', 'ties', 'zero_third', 'one_nan', 'inf', 'tiny', 'zero_weights', 'none']
SIZES = ['1', '2', '63', '64', '65', '1000', 'cap', 'cap+1', 'cap+65']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('size', SIZES)
def test_exact_cases(size, kind):
    cap = capacity()
    N = eval(size, {'cap': cap})
    rng = np.random.default_rng(1000 * SIZES.index(size) + KINDS.index(kind))
    for R in (1, 5):
        x, w = contents(kind, rng, R, N)
        want = statement(x, w, DYADIC)
        if kind == 'one_nan':
            assert np.isnan(want[-1]).all()                     # q = 1.0 reaches the NaN ...
            if N >= 63:
                assert not np.isnan(want[:-1]).any()            # ... the lower quantiles do not
        if kind == 'zero_weights':
            assert np.isnan(want).all()
        if kind == 'none':
            assert same(want, statement(x, np.ones(N), DYADIC))
        for pad in (0, 3):
            got = {m: launch(x, w, DYADIC, m, pad) for m in ((SORT, SELECT) if N <= cap else (SELECT,))}
            if N in (cap, cap + 1):
                got[AUTO] = launch(x, w, DYADIC, AUTO, pad)
            for m, g in got.items():
                assert same(g, want), (size, kind, R, pad, m, g, want)
            if kind == 'none':
                for m in got:
                    assert same(launch(x, np.ones(N), DYADIC, m, pad), want), (size, R, pad, m)


def test_sort_form_refuses_what_is_beyond_its_capacity():
    from smartpy_amd._lib import SmartEngineError
    cap = capacity()
    with pytest.raises(SmartEngineError, match='at most %d samples' % cap) as err:
        launch(np.zeros((1, cap + 1)), None, DYADIC, SORT)
    assert err.value.code == -2


@pytest.mark.parametrize('size', ['65', '1000', 'cap', 'cap+65'])
def test_general_weights_stay_within_the_band(size):
    cap = capacity()
    N = eval(size, {'cap': cap})
    rng = np.random.default_rng(77 + N)
    x, w = rng.normal(size=(3, N)), rng.uniform(size=N)
    x[:, ::7] = x[:, 1:2]                                       # some ties
    probs = (0.05, 0.5, 0.95)
    for m in ((SORT, SELECT) if N <= cap else (SELECT,)):
        got = launch(x, w, probs, m, pad=3)
        problems = [p for k, q in enumerate(probs) for r in range(3) for p in band_violations(x[r], w, q, got[k, r])]
        assert not problems, (m, problems)


def test_two_launches_give_the_same_bits():
    cap = capacity()
    rng = np.random.default_rng(3)
    for N, methods in ((1000, (SORT, SELECT)), (cap, (SORT,)), (cap + 65, (SELECT,))):
        x, w = rng.normal(size=(5, N)), rng.uniform(size=N)
        for m in methods:
            a, b = launch(x, w, (0.05, 0.5, 0.95), m), launch(x, w, (0.05, 0.5, 0.95), m)
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (N, m)


def test_engine_takes_the_matrix_a_launch_stored_on_its_stream(example):
    """200 rows x 30 daily steps: the quantiles of the sample-minor matrix run_ensemble itself has written, with the
    stride of that tensor, queued behind the launch on a stream that is not the default one."""
    import torch
    from smartpy_amd import engine
    rng = np.random.default_rng(8)
    params = np.asarray(example['params'], dtype=np.float64)[None, :] * rng.uniform(0.8, 1.2, size=(200, 10))
    forcing = np.stack([example['rain_daily'][:30], example['peva_daily'][:30]], axis=1)
    w = exact_weights(rng, 200)
    probs = (0.05, 0.5, 0.95, 1.0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = engine.run_ensemble(params, forcing, example['area'], 86400.0, 0, 1, want_discharge=True)
        stored = out.discharge_report_major
        assert stored.shape == (30, 200) and stored.stride(1) == 1
        got = {m: engine.weighted_quantiles(stored, probs, w, method=m) for m in ('auto', 'sort', 'select')}
        equal = engine.weighted_quantiles(stored, probs)
        from_host = engine.weighted_quantiles(stored.cpu().numpy(), probs, w)
    stream.synchronize()
    dis = out.discharge.cpu().numpy()
    assert dis.shape == (200, 30)
    want = statement(dis.T, w, probs)
    for m, g in got.items():
        assert g.is_cuda and g.dtype == torch.float64 and g.shape == (4, 30)
        assert same(g.cpu().numpy(), want), m
    assert same(equal.cpu().numpy(), statement(dis.T, None, probs)) and same(from_host.cpu().numpy(), want)
    bad = w.copy()
    bad[3], bad[5] = -1.0, np.inf
    with pytest.raises(engine.SmartEngineError, match='2 of the 200 weights'):
        engine.weighted_quantiles(stored, probs, bad)
    with pytest.raises(engine.SmartEngineError, match="method 'median' unknown"):
        engine.weighted_quantiles(stored, probs, w, method='median')


def _settings(root, name, start, end, warm):
    with open(os.path.join(root, 'in', 'Catchment', name), 'w') as f:
        f.write('ARGUMENT,VALUE\ncatchment_area_km2,175.46\ngauged_area_km2,175.97\nstart_datetime,%s 09:00:00\n'
                'end_datetime,%s 09:00:00\nsimu_timedelta_min,60\nreport_timedelta_min,1440\nwarm_up_days,%d\n'
                'gw_constraint,0.12667\n' % (start, end, warm))


def test_glue_prediction_bounds_end_to_end(tmp_path):
    from smartpy_amd.montecarlo import LHS, GLUE
    root = str(tmp_path / 'data')
    shutil.copytree(os.path.join(GOLDEN, 'data', 'in'), os.path.join(root, 'in'))
    _settings(root, 'Catchment.sampling.sttngs', '01/01/2007', '31/12/2007', 180)
    _settings(root, 'Catchment.evaluating.sttngs', '01/01/2008', '30/06/2008', 90)
    np.random.seed(2024)
    lhs = LHS('Catchment', root, 'csv', 'csv', sample_size=256, settings_filename='Catchment.sampling.sttngs')
    lhs.model.extra = EXTRA
    lhs.run()
    glue = GLUE('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (NSE_MIN,))}, sampling=lhs,
                settings_filename='Catchment.evaluating.sttngs')
    glue.model.extra = EXTRA
    n = glue.behavioural_params.shape[0]
    print('behavioural rows: %d of 256 with NSE >= %g; NSE of the sample, sorted: %s'
          % (n, NSE_MIN, np.sort(lhs.obj_fns[:, 0])[::-1][:210:10]))
    assert 10 <= n <= 200
    nse = glue.behavioural_obj_fns[:, 0].astype(np.float64)
    assert nse.shape == (n,) and (nse >= NSE_MIN).all()         # NSE_MIN >= 0: the name can be the likelihood
    # ... the same numbers the file-based constructor reads back from the sampling run's database
    from_file = GLUE('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (NSE_MIN,))},
                     settings_filename='Catchment.evaluating.sttngs')
    assert np.array_equal(from_file.behavioural_obj_fns, glue.behavioural_obj_fns, equal_nan=True)
    quantiles = (0.05, 0.5, 0.95)
    pb = glue.prediction_bounds(likelihood='NSE', write=True)
    R = len(glue.model.timeseries_report) - 1
    assert pb.bounds.shape == (3, R) and pb.bounds.dtype == np.float64 and tuple(pb.quantiles) == quantiles
    assert pb.datetime == glue.model.timeseries_report[1:]
    out = glue.model.simulate_ensemble(glue._sample, save_discharge=True, math_mode=glue.math_mode)
    dis = out.discharge.cpu().numpy()
    assert dis.shape == (n, R)
    assert same(pb.bounds, statement(dis.T, nse, quantiles))
    assert (pb.bounds[0] <= pb.bounds[1]).all() and (pb.bounds[1] <= pb.bounds[2]).all()
    obs = np.asarray(glue.model.nd_flow, dtype=np.float64)
    there = ~np.isnan(obs)
    assert there.sum() > 0
    inside = there & (pb.bounds[0] <= obs) & (obs <= pb.bounds[-1])
    assert pb.containment == inside.sum() / there.sum()
    # the file: the dates and the '%e' of the modelled flow file, one column per quantile
    assert pb.file == os.path.join(glue.model.out_f, 'Catchment.SMART.glue.bounds')
    lines = open(pb.file, newline='').read().split('\r\n')
    assert lines[0] == 'DateTime,q0.05,q0.5,q0.95' and len(lines) == R + 2 and lines[-1] == ''
    assert [ln.split(',')[0] for ln in lines[1:-1]] == [str(dt) for dt in pb.datetime]
    assert [ln.split(',')[1:] for ln in lines[1:-1]] == [['%e' % v for v in col] for col in pb.bounds.T]
    parsed = np.array([[float(v) for v in ln.split(',')[1:]] for ln in lines[1:-1]]).T
    assert np.allclose(parsed, pb.bounds, rtol=5e-7, atol=0)    # seven significant digits
    # equal weights and an explicit array go the same way
    flat = glue.prediction_bounds(quantiles=(0.5,))
    assert flat.file is None and same(flat.bounds, statement(dis.T, None, (0.5,)))
    shifted = glue.prediction_bounds(likelihood=nse - nse.min())
    assert same(shifted.bounds, statement(dis.T, nse - nse.min(), quantiles))
