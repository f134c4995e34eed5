"""Weighted ensemble quantiles on the GPU (smartpy_amd/csrc/smart_quantiles.hip) against the numpy statement of the
definition in oracle/analyses/quantiles.py: both forms, the C entry with its own leading dimension, the engine and
GLUE.prediction_bounds on top.  launch_quantiles chooses among seven kernel instances; each is reached here by
(instance, chosen when, and below it the tests with the N or K that reach it)

    smart_quantiles_sort<1024, 512>    sort, N <= 1024
        test_exact_cases N = 1 ... 1000, 1024; test_every_probability_count N = 1 ... 1000
    smart_quantiles_sort<2048, 1024>   sort, 1025 <= N <= 2048
        test_exact_cases N = 1025, 2048; test_thresholds_to_the_ulp N = 1025; the engine test with 1,500 rows
    smart_quantiles_sort<4096, 1024>   sort, 2049 <= N <= 4096
        test_exact_cases N = 2049, 4096; test_every_probability_count N = 2049; the engine test with 3,000 rows
    smart_quantiles_sort<8192, 1024>   sort, 4097 <= N <= capacity
        test_exact_cases N = 4097, cap; test_thresholds_to_the_ulp N = 4097, cap
    smart_quantiles_select<4>          select, K <= 4
        test_exact_cases (K = 4); test_every_probability_count K = 1, 4
    smart_quantiles_select<8>          select, 5 <= K <= 8
        test_every_probability_count K = 5, 8; the K = 7 runs of the band, two-launches and engine tests
    smart_quantiles_select<16>         select, 9 <= K <= 16
        test_every_probability_count K = 9, 16; test_thresholds_to_the_ulp (K = 15);
        test_weights_at_the_ends_of_the_exponent_range and test_select_form_on_an_ensemble_of_1e5 (K = 16)

AUTO takes the sort form up to the capacity: test_exact_cases launches it on both sides of every boundary (1024 | 1025,
2048 | 2049, 4096 | 4097, cap | cap + 1).  Everything but test_general_weights_stay_within_the_band compares with
`same`: bit for bit, NaN for NaN."""
import ctypes
import os

import numpy as np
import pytest

from oracle.analyses.quantiles import (statement, statement_rows, band_violations, DYADIC, power_of_two_weights, threshold_probs,
                                       distinct_rows, weightless_successor, many_nan_rows, mixed_nans, is_power_of_two,
                                       NAN_SHARE, SUBNORMAL, HUGE)
from support import EXTRA, NSE_MIN, SENTINEL, example_root, filled, padded, ptr, same, settings_file, to_device

pytestmark = pytest.mark.gpu

AUTO, SORT, SELECT = 0, 1, 2
SEVEN = (0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975)


def capacity():
    from smartpy_amd import engine
    return engine.quantiles_sort_capacity()


def launch(matrix, weights, probs, method, pad=0, junk=np.nan, spare=0):
    """The C entry on a [R, N] host matrix laid out with ld = N + pad (the padding holds `junk`) -> numpy [K, R]
    (with `spare` more rows below, as they were before the call: SENTINEL)."""
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    R, N = np.shape(matrix)
    sim, ld = padded(matrix, pad, junk)
    w = to_device(weights)
    q = (ctypes.c_double * len(probs))(*probs)
    out = filled((len(probs) + spare, R))
    _lib.check(L.smart_weighted_quantiles_hip(N, R, sim.data_ptr(), ld, ptr(w), q, len(probs), out.data_ptr(), method,
                                              torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


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
    elif kind == 'many_nan':
        x = many_nan_rows(rng, x)
    elif kind == 'all_nan':
        x = mixed_nans(rng, (R, N))
    elif kind == 'nan_weightless':
        cols = rng.permutation(N)[:int(NAN_SHARE * N)]
        x[:, cols] = mixed_nans(rng, (R, cols.size))
        w[cols] = 0.0
    else:
        raise AssertionError(kind)
    return x, w


KINDS = ['random', 'equal', 'ties', 'zero_third', 'one_nan', 'inf', 'tiny', 'zero_weights', 'none']
BOUNDARIES = ['1024', '1025', '2048', '2049', '4096', '4097']     # the sort form changes its instance between each pair
SIZES = ['1', '2', '63', '64', '65', '1000', 'cap', 'cap+1', 'cap+65'] + BOUNDARIES


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
            if N in (cap, cap + 1) or size in BOUNDARIES:
                got[AUTO] = launch(x, w, DYADIC, AUTO, pad)
            for m, g in got.items():
                assert same(g, want), (size, kind, R, pad, m, g, want)
            if kind == 'none':
                for m in got:
                    assert same(launch(x, np.ones(N), DYADIC, m, pad), want), (size, R, pad, m)


# dyadic probabilities (multiples of 1/32) in no order; 1.0 is among the first three
THIRTY_SECONDS = (24, 3, 32, 16, 31, 1, 20, 8, 12, 29, 2, 17, 30, 5, 9)


def probs_of(K):
    """K probabilities: the first K - 1 of THIRTY_SECONDS, then the second one (3/32) once more."""
    m = THIRTY_SECONDS[:1] if K == 1 else THIRTY_SECONDS[:K - 1] + THIRTY_SECONDS[1:2]
    return tuple(v / 32.0 for v in m)


@pytest.mark.parametrize('kind', ['random', 'equal', 'zero_third', 'inf'])
@pytest.mark.parametrize('size', ['1', '2', '65', '1000', '2049', 'cap', 'cap+65'])
@pytest.mark.parametrize('K', [1, 4, 5, 8, 9, 16])
def test_every_probability_count(K, size, kind):
    """Both sides of the K at which the select form changes its instance (and its workgroup width), in both forms:
    row k of the result belongs to probability k, and nothing is written below row K - 1.  'equal' makes the select form
    do no round at all, 'inf' (-inf ... +inf in the row) all 64."""
    cap = capacity()
    N = eval(size, {'cap': cap})
    probs = probs_of(K)
    assert len(probs) == K and (K < 4 or 1.0 in probs) and (K == 1 or (probs[1] == probs[-1] and len(set(probs)) == K - 1))
    assert K < 3 or list(probs) != sorted(probs)
    rng = np.random.default_rng(100000 + 1000 * K + 10 * N + len(kind))
    x, w = contents(kind, rng, 5, N)
    want = statement(x, w, probs)
    for m in ((SORT, SELECT) if N <= cap else (SELECT,)):
        got = launch(x, w, probs, m, pad=3, spare=1)
        assert got.shape == (K + 1, 5)
        assert same(got[:K], want), (K, size, kind, m, got, want)
        assert same(got[1], got[K - 1]) or K == 1
        assert (got[K] == SENTINEL).all(), (K, size, kind, m, got[K])


THRESHOLD_CASES = [('65', SORT), ('65', SELECT), ('1025', SORT), ('1025', SELECT), ('2049', SORT), ('2049', SELECT),
                   ('4097', SORT), ('4097', SELECT), ('cap', SORT), ('cap', SELECT), ('cap+65', SELECT)]


@pytest.mark.parametrize('size,method', THRESHOLD_CASES)
def test_thresholds_to_the_ulp(size, method):
    """`cum >= q * W` with q * W ON a partial sum, one ulp above and one ulp below it (threshold_probs: W is a power of
    two and every sum exact, so the three products are what they say): the element at the sum, the next one that
    carries weight, the element at the sum.  Three independent permutations per launch, five positions of one of them
    (its own probabilities, K = 15) per launch; the second pass takes the weight off one position's successor."""
    cap = capacity()
    N = eval(size, {'cap': cap})
    rng = np.random.default_rng(31000 + N + method)
    x = distinct_rows(rng, 3, N)
    full = power_of_two_weights(rng, N)
    for weightless in (False, True):
        for r in range(3):
            draw = [int(v) for v in rng.choice(N - 1, size=7, replace=False)]
            w, positions = full, draw[:5]
            if weightless:
                w, j = weightless_successor(x[r], full, rng)
                positions = [j] + [v for v in draw if v not in (j, j + 1)][:4]
            assert is_power_of_two(w.sum()) and w.sum() == full.sum()
            probs, values = threshold_probs(x[r], w, positions)
            assert len(probs) == 15
            ranked = np.sort(x[r])
            if weightless:
                assert values[:3].tolist() == [ranked[j], ranked[j + 2], ranked[j]]
            want = statement(x, w, probs)
            assert np.array_equal(want[:, r], values)
            got = launch(x, w, probs, method, pad=3)
            print(size, method, weightless, r, 'positions', list(positions), 'differ at', np.argwhere(got != want).tolist())
            assert same(got[:, r], values), (size, method, weightless, r, got[:, r], values)
            assert same(got, want), (size, method, weightless, r)


@pytest.mark.parametrize('size,method', THRESHOLD_CASES)
def test_weights_at_the_ends_of_the_exponent_range(size, method):
    """Weights times 2**-1060 (every weight and W itself subnormal: flushed to zero they would make every bound NaN) and
    times 2**900 give the bits of the unscaled weights: every partial sum and every q * W scales exactly."""
    cap = capacity()
    N = eval(size, {'cap': cap})
    rng = np.random.default_rng(52000 + N + method)
    x, w = rng.normal(size=(3, N)), power_of_two_weights(rng, N)
    want = statement(x, w, DYADIC)
    assert not np.isnan(want).any()
    got = launch(x, w, DYADIC, method, pad=3)
    assert same(got, want), (size, method)
    for scale in (SUBNORMAL, HUGE):
        scaled = w * scale
        assert np.array_equal(scaled / scale, w) and (scale > 1 or scaled.sum() < 2.0 ** -1022)
        assert same(statement(x, scaled, DYADIC), want)
        g = launch(x, scaled, DYADIC, method, pad=3)
        assert not np.isnan(g).any(), (size, method, scale)
        assert np.array_equal(g.view(np.int64), got.view(np.int64)), (size, method, scale, g, got)
    # sixteen probabilities (the widest select instance), the same claim
    probs = probs_of(16)
    want = statement(x, w, probs)
    for scale in (1.0, SUBNORMAL, HUGE):
        assert same(launch(x, w * scale, probs, method, pad=3), want), (size, method, scale)


@pytest.mark.parametrize('kind', ['many_nan', 'all_nan', 'nan_weightless'])
@pytest.mark.parametrize('size', ['64', '65', '1025', 'cap', 'cap+65'])
def test_rows_where_nans_decide(size, kind):
    """NaNs of either sign, quiet and signalling, with payloads: all of them sort above +inf, and a quantile is NaN
    exactly where the statement's is."""
    cap = capacity()
    N = eval(size, {'cap': cap})
    rng = np.random.default_rng(7000 + 10 * N + len(kind))
    x, w = contents(kind, rng, 5, N)
    want = statement(x, w, DYADIC)
    if kind == 'many_nan':
        assert np.isnan(x).mean() >= NAN_SHARE
        assert np.isnan(want[2:]).all() and not np.isnan(want[:2]).any()    # 0.9375 and 1.0 reach the NaNs
    elif kind == 'all_nan':
        assert np.isnan(x).all() and np.isnan(want).all()
    else:
        assert np.isnan(x).mean() > 1 / 3 and not np.isnan(want).any()
    for m in ((SORT, SELECT) if N <= cap else (SELECT,)):
        for pad in (0, 3):
            got = launch(x, w, DYADIC, m, pad)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (size, kind, m, pad)
            assert same(got, want), (size, kind, m, pad, got, want)


@pytest.mark.parametrize('method', [SORT, SELECT])
def test_more_report_steps_than_65535(method):
    """A grid wider than 65,535 workgroups: 70,001 steps of three samples, the values of step r inside [4r, 4r + 2] and
    permuted by r, so that a result stored for the wrong step cannot pass."""
    R = 70001
    perms = np.array([[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]], dtype=np.float64)
    x = 4.0 * np.arange(R)[:, None] + perms[np.arange(R) % 6]
    w = np.array([0.25, 0.5, 0.25])
    probs = (0.5, 1.0)
    want = statement_rows(x, w, probs)
    assert same(want[:, :600], statement(x[:600], w, probs)) and same(want[:, -7:], statement(x[-7:], w, probs))
    assert np.array_equal(want[1], 4.0 * np.arange(R) + 2.0) and np.array_equal(want[0] // 4, np.arange(R))
    assert len(set((want[0, :6] % 4).tolist())) > 1
    got = launch(x, w, probs, method, pad=1)
    assert same(got, want), np.argwhere(got != want)[:10]


@pytest.mark.parametrize('K', [3, 16])
def test_select_form_on_an_ensemble_of_1e5(K):
    rng = np.random.default_rng(100003 + K)
    N = 100003
    x, w = rng.normal(size=(2, N)), exact_weights(rng, N)
    x[:, ::9] = x[:, 4:5]                                       # ties
    assert w.sum() < 2.0 ** 27
    probs = DYADIC[:3] if K == 3 else probs_of(16)
    got = launch(x, w, probs, SELECT, pad=3)
    assert same(got, statement(x, w, probs))


def test_sort_form_refuses_what_is_beyond_its_capacity():
    from smartpy_amd._lib import SmartEngineError
    cap = capacity()
    with pytest.raises(SmartEngineError, match='at most %d samples' % cap) as err:
        launch(np.zeros((1, cap + 1)), None, DYADIC, SORT)
    assert err.value.code == -2


@pytest.mark.parametrize('size', ['65', '1000', 'cap', 'cap+65', '1025', '2049', '4097'])
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
    if size == 'cap+65':
        got = launch(x, w, SEVEN, SELECT, pad=3)
        problems = [p for k, q in enumerate(SEVEN) for r in range(3) for p in band_violations(x[r], w, q, got[k, r])]
        assert not problems, problems


def test_two_launches_give_the_same_bits():
    cap = capacity()
    rng = np.random.default_rng(3)
    for N, methods in ((1000, (SORT, SELECT)), (cap, (SORT,)), (cap + 65, (SELECT,))):
        x, w = rng.normal(size=(5, N)), rng.uniform(size=N)
        for m in methods:
            a, b = launch(x, w, (0.05, 0.5, 0.95), m), launch(x, w, (0.05, 0.5, 0.95), m)
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (N, m)
    for N, m, probs in ((2049, SORT, (0.05, 0.5, 0.95)), (4096, SORT, (0.05, 0.5, 0.95)), (cap + 65, SELECT, SEVEN),
                        (cap + 65, SELECT, tuple((k + 1) / 17.0 for k in range(16)))):
        x, w = rng.normal(size=(5, N)), rng.uniform(size=N)
        a, b = launch(x, w, probs, m), launch(x, w, probs, m)
        assert a.shape == (len(probs), 5) and not np.isnan(a).any()
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), (N, m, len(probs))


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


@pytest.mark.parametrize('rows', [1500, 3000])
def test_engine_on_ensembles_of_a_few_thousand_rows(example, rows):
    """An ordinary behavioural set (1,025 ... 4,096 rows: 'auto' takes the sort form's middle instances) with seven
    quantiles (the select form's instance for 5 ... 8): the matrix run_ensemble stored, every method."""
    import torch
    from smartpy_amd import engine
    rng = np.random.default_rng(rows)
    params = np.asarray(example['params'], dtype=np.float64)[None, :] * rng.uniform(0.8, 1.2, size=(rows, 10))
    forcing = np.stack([example['rain_daily'][:30], example['peva_daily'][:30]], axis=1)
    w = exact_weights(rng, rows)
    out = engine.run_ensemble(params, forcing, example['area'], 86400.0, 0, 1, want_discharge=True)
    stored = out.discharge_report_major
    assert stored.shape == (30, rows) and stored.stride(1) == 1
    got = {m: engine.weighted_quantiles(stored, SEVEN, w, method=m) for m in ('auto', 'sort', 'select')}
    equal = engine.weighted_quantiles(stored, SEVEN)
    torch.cuda.synchronize()
    dis = out.discharge.cpu().numpy()
    assert dis.shape == (rows, 30) and np.array_equal(stored.cpu().numpy(), dis.T)
    want = statement(dis.T, w, SEVEN)
    assert not np.isnan(want).any() and (want[0] < want[-1]).any()
    for m, g in got.items():
        assert g.is_cuda and g.dtype == torch.float64 and g.shape == (7, 30)
        assert same(g.cpu().numpy(), want), m
    assert same(equal.cpu().numpy(), statement(dis.T, None, SEVEN))


def test_glue_prediction_bounds_end_to_end(tmp_path):
    from smartpy_amd.montecarlo import LHS, GLUE
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sampling.sttngs', '01/01/2007', '31/12/2007', 180)
    settings_file(root, 'Catchment.evaluating.sttngs', '01/01/2008', '30/06/2008', 90)
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
    # seven quantiles (more than four: another instance of the select form, should the set outgrow the sort form)
    seven = glue.prediction_bounds(quantiles=SEVEN, likelihood='NSE', write=True)
    assert tuple(seven.quantiles) == SEVEN and seven.bounds.shape == (7, R) and seven.file == pb.file
    assert same(seven.bounds, statement(dis.T, nse, SEVEN))
    assert same(seven.bounds[3], pb.bounds[1]) and (np.diff(seven.bounds, axis=0) >= 0).all()
    lines = open(seven.file, newline='').read().split('\r\n')
    assert lines[0] == 'DateTime,q0.025,q0.05,q0.25,q0.5,q0.75,q0.95,q0.975' and len(lines) == R + 2 and lines[-1] == ''
    assert [ln.split(',')[0] for ln in lines[1:-1]] == [str(dt) for dt in seven.datetime]
    assert [ln.split(',')[1:] for ln in lines[1:-1]] == [['%e' % v for v in col] for col in seven.bounds.T]
