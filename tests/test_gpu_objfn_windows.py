"""smart_objfn_windows_hip on the GPU against the numpy statement of oracle/analyses/windows.py (apply f, mask by window
and missing observation, oracle.objfn_oracle.objective_functions(...)[:7], the entry's two rules).

The kernel has ONE geometry (grid = 64-sample blocks x windows, eight wavefronts per workgroup; chunks of 1,024 report
steps), so there is no size switch to straddle; R = 501 keeps every chunk partial, R = 2 * max_windows = 2,048 takes two
full chunks.  The gate is the one the suite holds smart_objfn_hip to against the same restatement: rel < 1e-9 with
|want| floored at 1e-12; every compared |want| is asserted to be above 1e-6, so that no entry sits on a cancellation
(a seed that fails this is changed, not the gate)."""
import os

import numpy as np
import pytest

from cases_objfn import EPS
from oracle.analyses.windows import statement, TRANSFORMS
from support import (EXTRA, GATE, SENTINEL, bits_equal, columns, data, example_root, filled, padded, rel_to_want,
                     settings_file, to_device, window_arrays)

pytestmark = pytest.mark.gpu


def launch(sim, obs, win, W, transform, eps, pad=0, junk=np.nan, spare=1):
    """The C entry on a [R, N] host matrix laid out with ld = N + pad (the padding holds `junk`) -> numpy
    [W + spare, N, 7]; the spare windows are as they were before the call (SENTINEL)."""
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    R, N = sim.shape
    d_sim, ld = padded(sim, pad, junk)
    d_obs, d_win = to_device(obs), to_device(win, np.int32)
    out = filled((W + spare, N, 7))
    _lib.check(L.smart_objfn_windows_hip(N, R, d_sim.data_ptr(), ld, d_obs.data_ptr(), d_win.data_ptr(), W,
                                         TRANSFORMS[transform], float(eps), out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def compare(got, sim, obs, win, W, transform, eps, cols, what):
    want = statement(sim[:, cols], obs, win, W, transform, eps)
    finite = want[~np.isnan(want)]
    err = rel_to_want(got[:W][:, cols], want)
    print('%s: rel %.3e, smallest |want| %.3e, NaN entries %d' % (what, err, np.min(np.abs(finite)) if finite.size else -1,
                                                                  int(np.isnan(want).sum())))
    assert finite.size == 0 or np.min(np.abs(finite)) > 1e-6, what      # (change the seed, not the gate)
    assert err < GATE, what
    return want


@pytest.mark.parametrize('n,ld', [(1, 1), (63, 64), (64, 64), (65, 128), (1000, 1000), (4097, 4160)])
def test_geometries_windows_and_transforms(n, ld):
    R = 501
    rng, obs, sim = data(1000 + n, R, n, obs_plus=0.0)
    cols = columns(rng, n, 12)
    for W, win in window_arrays(rng, R, 'zeros'):
        for transform in ('none', 'sqrt', 'log', 'inverse'):
            got = launch(sim, obs, win, W, transform, EPS[transform], pad=ld - n)
            assert got.shape == (W + 1, n, 7) and np.all(got[W] == SENTINEL)
            want = compare(got, sim, obs, win, W, transform, EPS[transform], cols, 'n=%d W=%d %s' % (n, W, transform))
            assert not np.isnan(want).any()
            assert not np.isnan(got[:W]).any()


def test_as_many_windows_as_one_call_takes():
    from smartpy_amd import engine
    W = engine.objfn_max_windows()
    R, n = 2 * W, 65
    rng, obs, sim = data(77, R, n, obs_plus=0.0)
    win = (np.arange(R) // 2).astype(np.int32)      # two report steps each: a window that misses one of them is NaN
    cols = columns(rng, n, 12)
    for transform in ('none', 'log'):
        got = launch(sim, obs, win, W, transform, EPS[transform])
        want = compare(got, sim, obs, win, W, transform, EPS[transform], cols, 'W=%d %s' % (W, transform))
        empty = np.isnan(want[:, 0, 0])
        assert 0.2 * W < empty.sum() < 0.4 * W                          # 1 - 0.85^2 of the windows
        assert np.isnan(got[:W][empty]).all() and not np.isnan(got[:W][~empty]).any() and np.all(got[W] == SENTINEL)


def test_the_two_rules():
    R, n, W = 501, 130, 6
    rng, obs, sim = data(5, R, n, obs_plus=0.0)
    win = (np.arange(R) * 5 // R).astype(np.int32)                     # 0 .. 4 occur, window 5 never does
    obs[win == 1] = np.nan                                              # every observation missing
    two = np.flatnonzero(win == 2)
    obs[two] = np.nan
    obs[two[7]] = 2.5                                                   # exactly one valid observation
    cols = np.arange(n)
    for transform in ('none', 'sqrt', 'log', 'inverse'):
        got = launch(sim, obs, win, W, transform, EPS[transform])
        compare(got, sim, obs, win, W, transform, EPS[transform], cols, 'few rows, %s' % transform)
        assert np.isnan(got[[1, 2, 5]]).all() and not np.isnan(got[[0, 3, 4]]).any()
    # one sample with a single negative flow in window 3: NaN in that (window, sample) only
    rows3 = np.flatnonzero((win == 3) & ~np.isnan(obs))
    bad = sim.copy()
    bad[rows3[11], 70] = -1.0
    for transform in ('sqrt', 'log'):
        got = launch(bad, obs, win, W, transform, EPS[transform])
        compare(got, bad, obs, win, W, transform, EPS[transform], cols, 'negative flow, %s' % transform)
        nan = np.isnan(got[:W]).all(axis=2)
        expect = np.zeros((W, n), dtype=bool)
        expect[[1, 2, 5]] = True
        expect[3, 70] = True
        assert np.array_equal(nan, expect)
    # ... also when it is the sample's first in-window value (the shift) or a NaN / infinity in the matrix
    for value, column in ((-1.0, 3), (np.nan, 64), (np.inf, 129)):
        bad = sim.copy()
        bad[rows3[0], column] = value
        got = launch(bad, obs, win, W, 'sqrt', 0.0)
        compare(got, bad, obs, win, W, 'sqrt', 0.0, cols, 'first value %r' % value)
        assert np.isnan(got[3, column]).all() and not np.isnan(got[3, column - 1]).any()
    # an observation 0.0 under ln with eps = 0: the whole window NaN, the others as the statement has them
    zero = obs.copy()
    zero[np.flatnonzero((win == 4) & ~np.isnan(obs))[5]] = 0.0
    got = launch(sim, zero, win, W, 'log', 0.0)
    compare(got, sim, zero, win, W, 'log', 0.0, cols, 'ln(0)')
    assert np.isnan(got[4]).all() and not np.isnan(got[[0, 3]]).any()


def test_one_definition_two_kernels():
    import torch
    from smartpy_amd import engine
    R, n = 501, 4097
    rng, obs, sim = data(11, R, n, obs_plus=0.0)
    d_sim = torch.from_numpy(sim).cuda()
    whole = engine.objective_functions(d_sim, obs).cpu().numpy()[:, :7]
    mine = engine.objective_functions_windows(d_sim, obs, np.zeros(R, dtype=np.int64))
    assert mine.shape == (1, n, 7) and mine.dtype == torch.float64 and mine.is_cuda
    err = rel_to_want(mine.cpu().numpy()[0], whole)
    print('windows kernel against smart_objfn_hip, %d columns: rel %.3e' % (n, err))
    assert err < GATE
    # the engine's other inputs: a device tensor of ids, a padded view, n_windows beyond the largest id
    wide = torch.full((R, n + 63), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :n] = d_sim
    ids = torch.from_numpy((np.arange(R) % 3).astype(np.int32)).cuda()
    a = engine.objective_functions_windows(wide[:, :n], torch.from_numpy(obs).cuda(), ids, n_windows=4,
                                           transform='sqrt').cpu().numpy()
    b = launch(sim, obs, np.arange(R) % 3, 4, 'sqrt', 0.0, spare=0)
    assert a.shape == (4, n, 7) and bits_equal(a, b) and np.isnan(a[3]).all() and not np.isnan(a[:3]).any()
    with pytest.raises(engine.SmartEngineError, match='1 of the 501 window ids'):
        bad = ids.clone()
        bad[17] = 3
        engine.objective_functions_windows(d_sim, obs, bad, n_windows=3)


def test_determinism_and_bounds():
    R, n = 501, 1000
    rng, obs, sim = data(23, R, n, obs_plus=0.0)
    for W, win in window_arrays(rng, R, 'zeros'):
        for transform in ('none', 'log'):
            first = launch(sim, obs, win, W, transform, EPS[transform])
            again = launch(sim, obs, win, W, transform, EPS[transform])
            assert bits_equal(first, again)
            assert np.all(first[W] == SENTINEL)                         # the spare window is untouched
            wide = launch(sim, obs, win, W, transform, EPS[transform], pad=37, junk=np.nan)
            assert bits_equal(first, wide)                              # NaN in the columns [n, ld) changes nothing


def test_through_the_model(tmp_path):
    import torch
    from smartpy_amd.montecarlo import LHS, GLUE
    from smartpy_amd.montecarlo.selection import condition_mask
    from smartpy_amd.windows import evaluation_windows, header_line
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sampling.sttngs', '01/01/2007', '31/12/2007', 180)
    settings_file(root, 'Catchment.evaluating.sttngs', '01/01/2008', '30/06/2008', 90)
    np.random.seed(2024)
    lhs = LHS('Catchment', root, 'csv', 'csv', sample_size=64, settings_filename='Catchment.sampling.sttngs')
    lhs.model.extra = EXTRA
    lhs.run()
    n = 64
    obs = np.asarray(lhs.model.nd_flow, dtype=np.float64)
    sim = lhs.model.simulate_ensemble(lhs._sample, save_discharge=True, math_mode=lhs.math_mode).discharge.cpu().numpy().T
    ids, labels = evaluation_windows(lhs.model.timeseries_report[1:], by='hydro_year')
    assert labels == ['2007', '2008']
    res = lhs.window_objective_functions('hydro_year')
    assert res.labels == labels and res.transform == 'none' and res.eps == 0.0 and res.file is None
    assert res.values.shape == (2, n, 7) and res.device_values.is_cuda and res.names[0] == 'NSE'
    assert bits_equal(res.values, res.device_values.cpu().numpy())
    err = rel_to_want(res.values, statement(sim, obs, ids, 2))
    print('hydrological years against the statement: rel %.3e' % err)
    assert err < GATE
    whole = lhs.window_objective_functions('all')
    err = rel_to_want(whole.values[0], lhs.obj_fns[:, :7])
    print("'all' against the fused moments of run(): rel %.3e" % err)
    assert whole.labels == ['all'] and err < GATE
    # eps=None: one hundredth of the mean observation for 'log', and the value is reported
    logs = lhs.window_objective_functions((ids, labels), transform='log', write=True)
    assert logs.eps == float(np.mean(obs[~np.isnan(obs)])) / 100.0 and logs.eps > 0.0
    err = rel_to_want(logs.values, statement(sim, obs, ids, 2, 'log', logs.eps))
    print('log flows against the statement: rel %.3e' % err)
    assert err < GATE
    assert logs.file == lhs.windows_file and os.path.normpath(logs.file) == os.path.join(root, 'out', 'Catchment', 'Catchment.SMART.lhs.windows')
    lines = open(logs.file).read().split('\n')
    assert len(lines) == n + 2 and lines[-1] == '' and lines[0] + '\n' == header_line(labels, 'log')
    # '%.6e' keeps seven significant digits of a float32 that needs up to nine: the characters are exactly those of the
    # float32 of `values`, and what they parse back to lies within half a unit of the seventh digit of it
    kept = logs.values.astype(np.float32).transpose(1, 0, 2).reshape(n, 14)
    assert [line.split(',') for line in lines[1:-1]] == [['%.6e' % v for v in row] for row in kept]
    back = np.array([[float(v) for v in line.split(',')] for line in lines[1:-1]])
    assert back.shape == (n, 14) and rel_to_want(back, kept.astype(np.float64)) <= 5.0e-7
    # GLUE from that run, conditioned per window of its own period
    threshold = float(np.median(lhs.obj_fns[:, 0]))
    glue = GLUE('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (threshold,))}, sampling=lhs,
                settings_filename='Catchment.evaluating.sttngs')
    glue.model.extra = EXTRA
    nb = glue.behavioural_params.shape[0]
    assert 2 <= nb < n
    monthly = glue.window_objective_functions('month', transform='sqrt')
    W = len(monthly.labels)
    assert monthly.labels[0] == '01' and W >= 3 and monthly.values.shape == (W, nb, 7)
    assert tuple(monthly.device_values.shape) == (W, nb, 7)
    both_d, both_h = None, None
    for w in range(W):
        level = float(np.median(monthly.values[w][:, 0]))
        on_device = condition_mask(monthly.device_values[w][:, [0]], [(level,)], ['min'])
        on_host = condition_mask(monthly.values[w][:, [0]], [(level,)], ['min'])
        assert np.array_equal(on_device.cpu().numpy(), on_host) and 0 < on_host.sum() <= nb
        both_d = on_device if both_d is None else both_d & on_device
        both_h = on_host if both_h is None else both_h & on_host
    assert isinstance(both_d, torch.Tensor) and np.array_equal(both_d.cpu().numpy(), both_h)
