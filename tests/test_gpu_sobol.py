"""smart_sobol_indices_hip on the GPU against the numpy statement of oracle/analyses/sobol.py (sums in math.fsum).

The tolerance of every comparison is not a chosen number: sobol_statement(..., bounds=True) computes from the data what
ANY order of additions may differ by -- (m - 1) 2^-53 sum|c t| per sum of m terms, carried through the quotients, plus 4
ulp; sqrt(2) times the largest replicate bound for a standard deviation -- and every test asserts as well that this bound
is below the project's 1e-9 gate on the inputs it uses (a seed that fails that is changed, not the gate).

Shapes stand on both sides of every switch: the point kernel's LDS instances (n <= 1,024, <= capacity, beyond), its 1,024
threads (n = 1,023 / 1,025), the wavefront (63 / 64 / 65), the bootstrap's tile of 128 base rows, its replicate groups of
64 (B = 63 / 64 / 65 / 130 / the cap) and its three instances (k <= 4, 10, 16).  ld = N + 3 with NaN in the padding; the
outputs lie inside buffers of sentinels with a spare row behind them."""
import os

import numpy as np
import pytest

from oracle.analyses.sobol import sobol_statement, design_values
from support import EXTRA, GATE, Guarded, bits_equal, example_root, padded, ptr, settings_file

pytestmark = pytest.mark.gpu


def launch(y, n, k, counts=None, pad=3):
    """The C entry on a host matrix laid out with ld = N + pad (NaN in the padding) -> dict of numpy arrays like
    sobol_statement's.  Every output lies support.GUARD doubles inside a buffer of support.SENTINEL with a spare row behind it; what the
    call does not own is checked to be as it was (without counts: both buffers of standard deviations entirely)."""
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    y = np.atleast_2d(y)
    M, N = y.shape
    assert N == n * (k + 2)
    d_y, ld = padded(y, pad)
    B = 0 if counts is None else counts.shape[1]
    d_c = None if not B else torch.from_numpy(np.ascontiguousarray(counts).view(np.int16)).cuda()
    sizes = {'S1': k, 'ST': k, 'moments': 2, 'S1_std': k, 'ST_std': k}
    buf = {name: Guarded(M * w, tail=w) for name, w in sizes.items()}
    rc = L.smart_sobol_indices_hip(n, k, M, d_y.data_ptr(), ld, buf['S1'].ptr(), buf['ST'].ptr(), buf['moments'].ptr(),
                                   ptr(d_c), B, buf['S1_std'].ptr(null=not B), buf['ST_std'].ptr(null=not B), None, 0,
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _lib.check(rc)
    out = {}
    for name, w in sizes.items():
        own = M * w if (B or not name.endswith('_std')) else 0
        flat, intact = buf[name].read(own)
        assert intact, name
        out[name] = flat.reshape(M, w) if own else None
    out['mu'], out['V'] = out['moments'][:, 0], out['moments'][:, 1]
    return out


def compare(got, want, names, what):
    worst = 0.0
    for name in names:
        g, w, b = got[name], want[name], want['bound_' + name]
        assert g.shape == w.shape, (what, name)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, name, g, w)
        if (~nan).any():
            assert np.all(b[~nan] < GATE), (what, name, float(np.max(b[~nan])))
            excess = np.abs(g - w)[~nan] - b[~nan]
            ratio = float(np.max(np.abs(g - w)[~nan] / b[~nan])) if np.all(b[~nan] > 0) else 0.0
            worst = max(worst, ratio)
            assert np.all(excess <= 0.0), (what, name, float(np.max(excess)), ratio)
    print('%s: largest |got - want| / bound = %.3f' % (what, worst))


POINT = ('S1', 'ST', 'mu', 'V')
ALL = POINT + ('S1_std', 'ST_std')


def _capacity():
    from smartpy_amd import _lib
    return int(_lib.lib().smart_sobol_lds_capacity())


@pytest.mark.parametrize('n,k,R', [(1, 1, 2), (2, 3, 1), (63, 10, 2), (64, 16, 1), (65, 1, 257), (255, 3, 2), (256, 10, 1),
                                   (257, 16, 2), (1023, 3, 257), (1025, 10, 2), (0, 3, 2), (-1, 3, 2)])
def test_point_estimates_at_every_shape(n, k, R):
    if n <= 0:
        n = _capacity() + (1 if n else 0)           # the last resident size, the first streamed one
    y = design_values(1000 * k + n, n, k, R)
    got = launch(y, n, k)
    compare(got, sobol_statement(y, n, k, bounds=True), POINT, 'n %d k %d R %d' % (n, k, R))
    assert got['S1_std'] is None and got['ST_std'] is None


@pytest.mark.parametrize('B,n,k', [(0, 257, 3), (1, 257, 3), (2, 257, 3), (63, 257, 3), (64, 129, 3), (65, 300, 10),
                                   (130, 200, 16), (-1, 128, 3), (64, 1, 1), (5, 2, 16)])
def test_resamples(B, n, k):
    from smartpy_amd import engine
    if B < 0:
        B = engine.sobol_max_resamples()
    y = design_values(7 * B + n, n, k, 2)
    counts = engine.sobol_counts(n, B, seed=B) if B else None
    got = launch(y, n, k, counts)
    want = sobol_statement(y, n, k, counts, bounds=True)
    compare(got, want, ALL if B else POINT, 'B %d n %d k %d' % (B, n, k))
    if B == 1:
        assert np.isnan(got['S1_std']).all() and np.isnan(got['ST_std']).all()
    # the point estimates do not know about the bootstrap, and a second launch gives the same bits
    plain, again = launch(y, n, k), launch(y, n, k, counts)
    for name in POINT:
        assert bits_equal(plain[name], got[name]), name
    for name in (ALL if B else POINT):
        assert bits_equal(again[name], got[name]), name


def test_inert_parameter_and_the_all_ones_replicate():
    n, k, B = 300, 3, 70
    y = design_values(5, n, k, 3, inert=1)
    counts = np.ones((n, B), dtype=np.uint16)
    got = launch(y, n, k, counts)
    want = sobol_statement(y, n, k, counts, bounds=True)
    for name in ('S1', 'ST', 'S1_std', 'ST_std'):
        assert bits_equal(got[name][:, 1], np.zeros(3)), name                # +0.0, not -0.0, not 1e-17
    compare(got, want, ALL, 'all counts 1')
    assert np.all(got['S1_std'] == 0.0) and np.all(got['ST_std'] == 0.0)    # every replicate IS the point estimate
    # ... which one replicate of ones among drawn ones reproduces within the bound: its value is behind the std of two
    from smartpy_amd import engine
    drawn = engine.sobol_counts(n, 64, seed=1)
    drawn[:, 0] = 1
    compare(launch(y, n, k, drawn), sobol_statement(y, n, k, drawn, bounds=True), ALL, 'one replicate of ones')


def test_poisoned_and_constant_rows():
    n, k, B = 200, 4, 33
    from smartpy_amd import engine
    y = design_values(9, n, k, 8)
    counts = engine.sobol_counts(n, B, seed=2)
    clean = launch(y, n, k, counts)
    bad = y.copy()
    bad[1, 17] = np.nan                 # block A
    bad[3, n + 5] = np.inf              # block B
    bad[5, (2 + 2) * n + 199] = -np.inf     # block AB_2
    bad[7, :] = 2.5                     # no variance
    got = launch(bad, n, k, counts)
    for name in ALL:
        for r in (1, 3, 5):
            assert np.isnan(got[name][r]).all(), (name, r)
        for r in (0, 2, 4, 6):
            assert bits_equal(got[name][r], clean[name][r]), (name, r)
    for name in ('S1', 'ST', 'S1_std', 'ST_std'):
        assert np.isnan(got[name][7]).all(), name
    assert got['mu'][7] == 2.5 and got['V'][7] == 0.0
    compare(got, sobol_statement(bad, n, k, counts, bounds=True), ALL, 'poisoned rows')


def test_engine_surface_honours_the_leading_dimension():
    import torch
    from smartpy_amd import engine
    n, k = 100, 3
    y = design_values(3, n, k, 4)
    wide = torch.full((4, n * (k + 2) + 11), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :n * (k + 2)] = torch.from_numpy(y).cuda()
    counts = engine.sobol_counts(n, 16, seed=0)
    res = engine.sobol_indices(wide[:, :n * (k + 2)], n, k, counts=counts)
    want = sobol_statement(y, n, k, counts, bounds=True)
    got = {'S1': res.S1.cpu().numpy(), 'ST': res.ST.cpu().numpy(), 'mu': res.moments[:, 0].cpu().numpy(),
           'V': res.moments[:, 1].cpu().numpy(), 'S1_std': res.S1_std.cpu().numpy(), 'ST_std': res.ST_std.cpu().numpy()}
    compare(got, want, ALL, 'engine, device view')
    host = engine.sobol_indices(y[2], n, k)                     # one row from the host, no bootstrap
    assert host.S1_std is None and bits_equal(host.S1.cpu().numpy()[0], got['S1'][2])


def test_through_the_model(tmp_path):
    from smartpy_amd import engine
    from smartpy_amd.montecarlo import Sobol
    from smartpy_amd.montecarlo.sobol import normal_quantile, series_header_line, INDICES_HEADER
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sobol.sttngs', '01/01/2007', '19/07/2007', 60)       # two hundred report steps
    n = 64
    sob = Sobol('Catchment', root, 'csv', 'csv', base_size=n, settings_filename='Catchment.sobol.sttngs', seed=4)
    sob.model.extra = EXTRA
    with pytest.raises(Exception, match='run\\(\\) has to come first'):
        sob.sensitivity()
    sob.run()
    assert sob.vary == sob.param_names and sob._sample.shape == (n * 12, 10) and sob.obj_fns.shape == (n * 12, 8)
    assert os.path.normpath(sob.db_file) == os.path.join(root, 'out', 'Catchment', 'Catchment.SMART.sobol')
    z = normal_quantile(0.95)
    res = sob.sensitivity(resamples=64, seed=8, write=True)
    names = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE']
    assert res.targets == names and res.parameters == sob.param_names and res.S1.shape == (7, 10)
    counts = engine.sobol_counts(n, 64, seed=8)
    want = sobol_statement(sob.obj_fns[:, :7].T, n, 10, counts, bounds=True)
    got = {'S1': res.S1, 'ST': res.ST, 'mu': res.mean, 'V': res.variance, 'S1_std': res.S1_conf / z, 'ST_std': res.ST_conf / z}
    for name in ('S1_std', 'ST_std'):
        want['bound_' + name] = want['bound_' + name] + 4 * 2.0 ** -52 * np.abs(want[name])    # times z, over z
    compare(got, want, ALL, 'objective functions through the model')
    assert res.device.S1.is_cuda and bits_equal(res.device.S1.cpu().numpy(), res.S1)
    # targets as an array are the same call by name; 'GW' is one
    by_array = sob.sensitivity(targets=sob.obj_fns[:, 1], resamples=64, seed=8)
    by_name = sob.sensitivity(targets=['KGE'], resamples=64, seed=8)
    assert by_array.targets == ['target0'] and by_name.targets == ['KGE']
    for name in ('S1', 'ST', 'S1_conf', 'ST_conf', 'mean', 'variance'):
        assert bits_equal(getattr(by_array, name), getattr(by_name, name)), name
        assert bits_equal(getattr(by_name, name)[0], getattr(res, name)[1]), name
    assert sob.sensitivity(targets='GW', resamples=0).S1_conf is None
    # the .indices file: the characters of '%.6e' of the float32
    assert res.file == sob.indices_file and res.file.endswith('Catchment.SMART.sobol.indices')
    lines = open(res.file).read().split('\n')
    assert lines[0] + '\n' == INDICES_HEADER and len(lines) == 7 * 10 + 2 and lines[-1] == ''
    kept = np.stack([res.S1, res.S1_conf, res.ST, res.ST_conf], axis=2).reshape(70, 4).astype(np.float32)
    assert [line.split(',')[2:] for line in lines[1:-1]] == [['%.6e' % v for v in row] for row in kept]
    assert [line.split(',')[:2] for line in lines[1:-1]] == [[t, p] for t in names for p in sob.param_names]
    back = np.array([[float(v) for v in line.split(',')[2:]] for line in lines[1:-1]], dtype=np.float32)
    assert np.allclose(back, kept, rtol=1e-6, atol=0, equal_nan=True)
    # time-varying sensitivity: every report step a row, against the statement on the discharge the engine returns
    ser = sob.sensitivity_series(resamples=0, write=True)
    sim = sob.model.simulate_ensemble(sob._sample, save_discharge=True, math_mode=sob.math_mode).discharge_report_major.cpu().numpy()
    R = sim.shape[0]
    assert R == len(sob.model.timeseries_report) - 1 == 200
    assert ser.S1.shape == (R, 10) and ser.variance.shape == (R,) and len(ser.datetime) == R and ser.S1_conf is None
    want = sobol_statement(sim, n, 10, bounds=True)
    compare({'S1': ser.S1, 'ST': ser.ST, 'mu': ser.mean, 'V': ser.variance}, want, POINT, 'discharge per report step')
    lines = open(ser.file).read().split('\n')
    assert ser.file.endswith('Catchment.SMART.sobol.series') and lines[0] + '\n' == series_header_line(sob.param_names)
    assert len(lines) == R + 2
    kept = np.concatenate([ser.S1, ser.ST], axis=1).astype(np.float32)
    assert [line.split(',')[1:] for line in lines[1:-1]] == [['%.6e' % v for v in row] for row in kept]
    assert lines[1].split(',')[0] == ser.datetime[0].strftime('%Y-%m-%d %H:%M:%S')
    # three parameters vary: N = 5 n rows, and the database has that many lines
    three = Sobol('Catchment', root, 'csv', 'csv', base_size=n, settings_filename='Catchment.sobol.sttngs', seed=4,
                  vary=['T', 'SK', 'RK'], fixed={'C': 1.0})
    three.model.extra = EXTRA
    three.run()
    assert three._sample.shape == (5 * n, 10) and set(three._sample[:, 1].tolist()) == {1.0}
    assert len(open(three.db_file).read().split('\n')) == 5 * n + 2
    small = three.sensitivity(targets=['NSE', 'GW'], resamples=16, seed=1)
    assert small.S1.shape == (2, 3) and small.parameters == ['T', 'SK', 'RK']
