"""smart_flow_duration_hip on the GPU against the numpy statement of oracle/analyses/flow_duration.py.

Shapes straddle every switch: the sort form has five instances chosen from R (1,024 x 16 columns, 2,048 x 8, 4,096 x 4,
8,192 x 2, 16,384 x 1), so R in {1, 2, 501, 1024 | 1025 | 4096 | 4097 | 16384} runs each at its first and its full size
and R = 16385 takes 'auto' to the select form; the N of every R leave the last workgroup of that instance's COLS partial
(and N = 65 a second, partial wavefront of the select form).  ld = N + pad with NaN in the padding; the outputs lie inside
a larger buffer of sentinels with a spare window behind them.

Order statistics must be BIT-EQUAL to the statement (a zero is compared by value: both zeros are one key).  The objective
functions are held to the gate the suite holds smart_objfn_hip and the windows kernel to against the same restatement: rel
< 1e-9 with |want| floored at 1e-12, every compared |want| asserted above 1e-6 (a seed that fails this is changed, not the
gate)."""
import os

import numpy as np
import pytest

from cases_flow_duration import CAPACITY, EPS, launch
from oracle.analyses.flow_duration import rank_of, statement
from support import (EXTRA, E_SIZE, GATE, bits_equal, columns, data, example_root, rel_to_want, same_values, settings_file,
                     window_arrays)

pytestmark = pytest.mark.gpu

# R -> the N it is run with (COLS of the instance: 16, 16, 16, 16, 8, 4, 2, 1; select beyond)
SHAPES = {1: (1, 17, 65), 2: (1, 15, 65), 501: (1, 15, 17, 1000), 1024: (5, 63), 1025: (3, 15, 17, 65), 4096: (3, 4, 5, 63),
          4097: (1, 3, 5, 65), 16384: (1, 3, 17), 16385: (5, 65)}


def probabilities(obs, win, W):
    """0, 1, binary fractions (q * m an integer for every m that is a multiple of 8), thirds, the tails, and j / m for the
    m of the first window that has rows"""
    probs = [0.0, 1.0, 0.5, 0.25, 0.125, 1.0 / 3.0, 0.01, 0.99]
    for w in range(W):
        m = int(((win == w) & (~np.isnan(obs) if obs is not None else True)).sum())
        if m:
            probs += [1.0 / m, (m - 1.0) / m, (m // 2) / float(m)]
            break
    return probs


@pytest.mark.parametrize('R', sorted(SHAPES))
def test_order_statistics_are_the_statement_bit_for_bit(R):
    for n in SHAPES[R]:
        rng, obs, sim = data(100 * R + n, R, n, obs_plus=0.05)
        variants = window_arrays(rng, R, 'zeros')
        for W, win in variants:
            for with_obs in (obs, None):
                if R > CAPACITY and with_obs is None and W != 16:
                    continue                                            # (a pass of the select form over 16,385 rows by one
                                                                        # wavefront, ~60 times: once per window array is enough)
                probs = probabilities(with_obs, win, W)
                want, _ = statement(sim, probs, with_obs, win, W)
                got, none = launch(sim, probs, with_obs, win, W, pad=3)
                assert none is None and same_values(got, want), 'R=%d n=%d W=%d obs=%s' % (R, n, W, with_obs is not None)
                if R <= CAPACITY and (R <= 1025 or W == 16):
                    # the two forms on the same inputs, and each of them twice (a long single window costs the select
                    # form ~R x 60 dependent passes of one wavefront: the long columns go there split over 16 windows)
                    assert bits_equal(got, launch(sim, probs, with_obs, win, W, pad=3, method='sort')[0])
                    picked = launch(sim, probs, with_obs, win, W, method='select')[0]
                    assert bits_equal(got, picked) and bits_equal(picked, launch(sim, probs, with_obs, win, W, method='select')[0])
        # no window array: one window holding every row
        probs = probabilities(obs, np.zeros(R, dtype=np.int32), 1)
        assert same_values(launch(sim, probs, obs)[0], statement(sim, probs, obs)[0])
        if R <= 4097:
            assert same_values(launch(sim, probs, method='select')[0], statement(sim, probs)[0])


def test_empty_windows_ties_zeros_and_values_that_are_not_finite():
    R, n, W = 501, 37, 5
    rng, obs, sim = data(9, R, n, obs_plus=0.05)
    win = (np.arange(R) * 4 // R).astype(np.int32)                      # 0 .. 3 occur, window 4 never does
    obs[win == 1] = np.nan                                              # every observation missing: empty as well
    sim[:, 0] = 2.5                                                     # an all-equal column
    sim[:, 1] = rng.integers(0, 4, R).astype(np.float64)                # many ties
    sim[:, 2] = rng.choice([0.0, -0.0, 1.0, -1.0], R)                   # both zeros in one column
    sim[rng.integers(0, R, 40), 3] = np.nan
    sim[rng.integers(0, R, 40), 4] = np.inf
    sim[rng.integers(0, R, 40), 4] = -np.inf
    sim[rng.integers(0, R, 25), 5] = np.nan
    sim[:, 6] = np.nan                                                  # nothing but NaN
    sim[:, 7] = -rng.random(R) * 1e-300                                 # denormal neighbourhood, negative
    probs = [0.0, 1.0, 0.5, 0.9, 0.95, 0.99, 0.05, 0.1]
    want, _ = statement(sim, probs, obs, win, W)
    assert np.isnan(want[[1, 4]]).all() and np.isnan(want[0, 1, 3]) and want[0, 0, 4] == -np.inf and want[0, 1, 4] == np.inf
    for method in ('sort', 'select'):
        got, _ = launch(sim, probs, obs, win, W, method=method, pad=2)
        assert same_values(got, want), method
        assert np.array_equal(got[:, :, 2], want[:, :, 2], equal_nan=True)          # ... and the zeros by value
    free, _ = statement(sim, probs, None, win, W)
    assert not np.isnan(free[1, :, 0]).any()
    assert same_values(launch(sim, probs, None, win, W)[0], free)


def compare(got, want, what):
    finite = want[~np.isnan(want)]
    err = rel_to_want(got, want)
    print('%s: rel %.3e, smallest |want| %.3e, NaN entries %d' % (what, err, np.min(np.abs(finite)) if finite.size else -1,
                                                                  int(np.isnan(want).sum())))
    assert finite.size == 0 or np.min(np.abs(finite)) > 1e-6, what      # (change the seed, not the gate)
    assert err < GATE, what


@pytest.mark.parametrize('R,n', [(501, 17), (1025, 15), (2049, 5), (4097, 5), (16384, 3)])
def test_objective_functions_of_the_curve(R, n):
    rng, obs, sim = data(7000 + R, R, n, obs_plus=0.05)
    cols = columns(rng, n, 10)
    probs = [0.05, 0.5, 0.95]
    for W, win in window_arrays(rng, R, 'zeros')[:3] if R > 501 else window_arrays(rng, R, 'zeros'):
        for transform in ('none', 'sqrt', 'log', 'inverse'):
            for segment in ((0.0, 1.0), (0.98, 1.0), (0.0, 0.3), (0.3, 0.7)):
                if R * (segment[1] - segment[0]) / W < 4:
                    continue                                            # (the rule for short segments has its own test)
                want_q, want = statement(sim[:, cols], probs, obs, win, W, transform, EPS[transform], segment, objfn=True)
                got_q, got = launch(sim, probs, obs, win, W, transform, EPS[transform], segment, objfn=True, pad=1)
                assert same_values(got_q[:, :, cols], want_q)
                compare(got[:, cols], want, 'R=%d n=%d W=%d %s %r' % (R, n, W, transform, segment))
                assert not np.isnan(want).any() and not np.isnan(got).any()
    again = launch(sim, probs, obs, win, W, transform, EPS[transform], segment, objfn=True, pad=1)[1]
    assert bits_equal(got, again)                                       # two launches, the same bits


def test_the_two_rules_of_the_curve():
    R, n, W = 501, 20, 4
    rng, obs, sim = data(31, R, n, obs_plus=0.05)
    win = (np.arange(R) * 3 // R).astype(np.int32)                      # 0 .. 2 occur, window 3 never does
    one = np.flatnonzero(win == 1)
    obs[one] = np.nan
    obs[one[[5, 9, 40]]] = [2.5, 1.5, 3.5]                              # three valid observations: (0.98, 1) keeps no rank, (0, 0.3) one
    probs = [0.5]
    for segment, nan_windows in (((0.0, 1.0), [3]), ((0.98, 1.0), [1, 3]), ((0.0, 0.3), [1, 3])):
        want_q, want = statement(sim, probs, obs, win, W, 'sqrt', 0.0, segment, objfn=True)
        got_q, got = launch(sim, probs, obs, win, W, 'sqrt', 0.0, segment, objfn=True)
        assert same_values(got_q, want_q)
        compare(got, want, 'few ranks %r' % (segment,))
        others = [w for w in range(W) if w not in nan_windows]
        assert np.isnan(got[nan_windows]).all() and not np.isnan(got[others]).any()
    # a negative flow under ln sorts to the bottom: it spoils the low segment of its (window, sample) and no other
    rows0 = np.flatnonzero((win == 0) & ~np.isnan(obs))
    bad = sim.copy()
    bad[rows0[11], 7] = -1.0
    for segment, spoilt in (((0.0, 0.3), True), ((0.0, 1.0), True), ((0.98, 1.0), False)):
        want = statement(bad, probs, obs, win, W, 'log', 0.05, segment, objfn=True)[1]
        got = launch(bad, probs, obs, win, W, 'log', 0.05, segment, objfn=True)[1]
        compare(got, want, 'negative flow %r' % (segment,))
        assert bool(np.isnan(got[0, 7]).all()) == spoilt and not np.isnan(got[0, [6, 8]]).any() and not np.isnan(got[2, 7]).any()
    # a NaN in the column sorts to the top: it spoils the segments that reach the top rank
    bad = sim.copy()
    bad[rows0[3], 16] = np.nan
    for segment, spoilt in (((0.0, 0.3), False), ((0.0, 1.0), True), ((0.98, 1.0), True)):
        want = statement(bad, probs, obs, win, W, 'none', 0.0, segment, objfn=True)[1]
        got = launch(bad, probs, obs, win, W, 'none', 0.0, segment, objfn=True)[1]
        compare(got, want, 'NaN in the column %r' % (segment,))
        assert bool(np.isnan(got[0, 16]).all()) == spoilt and not np.isnan(got[0, [15, 17]]).any()
    # an observation 0.0 under ln with eps = 0: every sample of the window whose segment holds it
    zero = obs.copy()
    zero[rows0[5]] = 0.0
    for segment, spoilt in (((0.0, 0.3), True), ((0.5, 1.0), False)):
        want = statement(sim, probs, zero, win, W, 'log', 0.0, segment, objfn=True)[1]
        got = launch(sim, probs, zero, win, W, 'log', 0.0, segment, objfn=True)[1]
        compare(got, want, 'ln(0) %r' % (segment,))
        assert bool(np.isnan(got[0]).all()) == spoilt and not np.isnan(got[2]).any()


def test_beyond_the_capacity_is_refused_not_rerouted():
    R, n = CAPACITY + 1, 3
    rng, obs, sim = data(5, R, n, obs_plus=0.05)
    win = (np.arange(R) % 16).astype(np.int32)
    text = launch(sim, [0.5], obs, win, 16, objfn=True, expect=E_SIZE)
    assert str(CAPACITY) in text and 'objective functions' in text
    text = launch(sim, [0.5], obs, win, 16, method='sort', expect=E_SIZE)
    assert str(CAPACITY) in text and 'sort form' in text
    from smartpy_amd import engine
    with pytest.raises(engine.SmartEngineError, match=str(CAPACITY)) as e:
        engine.flow_duration(sim, [0.5], obs, win, objfn=True)
    assert e.value.code == E_SIZE


def test_engine_surface():
    import torch
    from smartpy_amd import engine
    R, n = 501, 130
    rng, obs, sim = data(41, R, n, obs_plus=0.05)
    ids = (np.arange(R) % 3).astype(np.int32)
    probs = [0.1, 0.5, 0.9]
    want_q, want = statement(sim, probs, obs, ids, 4, 'sqrt', 0.0, (0.0, 0.3), objfn=True)
    wide = torch.full((R, n + 63), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :n] = torch.from_numpy(sim).cuda()
    quant, scores = engine.flow_duration(wide[:, :n], probs, torch.from_numpy(obs).cuda(), torch.from_numpy(ids).cuda(),
                                         n_windows=4, transform='sqrt', segment=(0.0, 0.3), objfn=True)
    assert quant.is_cuda and quant.dtype == torch.float64 and tuple(quant.shape) == (4, 3, n)
    assert scores.is_cuda and tuple(scores.shape) == (4, n, 7)
    assert same_values(quant.cpu().numpy(), want_q) and np.isnan(want_q[3]).all()
    compare(scores.cpu().numpy(), want, 'engine, strided view')
    quant, scores = engine.flow_duration(sim, 0.5)                       # host matrix, one probability, nothing else
    assert scores is None and same_values(quant.cpu().numpy(), statement(sim, [0.5])[0])
    picked, _ = engine.flow_duration(sim, 0.5, method='select')
    assert bits_equal(quant.cpu().numpy(), picked.cpu().numpy())
    empty_q, empty_s = engine.flow_duration(torch.empty((R, 0), dtype=torch.float64, device='cuda'), probs, obs, objfn=True)
    assert tuple(empty_q.shape) == (1, 3, 0) and tuple(empty_s.shape) == (1, 0, 7)
    with pytest.raises(engine.SmartEngineError, match='1 of the 501 window ids'):
        bad = torch.from_numpy(ids).cuda()
        bad[17] = 3
        engine.flow_duration(sim, probs, obs, bad, n_windows=3)


def test_a_matrix_without_a_report_step_is_refused_in_the_entrys_own_words():
    """smart_flow_duration_workspace_bytes refuses n_reports = 0, and so does the entry: the sentence is the entry's, not
    whatever the thread's last failure left -- and it is about the size, though torch gives such a matrix no address."""
    import torch
    from smartpy_amd import _lib, engine
    assert _lib.lib().smart_objfn_hip(1, 1, None, 1, None, None, 0.0, None, None) == -1      # leaves another entry's text
    sim = torch.empty((0, 4), dtype=torch.float64, device='cuda')
    with pytest.raises(engine.SmartEngineError) as e:
        engine.flow_duration(sim, 0.5)
    assert e.value.code == E_SIZE
    assert str(e.value).startswith('smart_flow_duration_hip: need n_samples, n_reports'), str(e.value)


def test_through_the_model(tmp_path):
    from smartpy_amd.montecarlo import LHS
    from smartpy_amd.montecarlo.selection import condition_mask
    from smartpy_amd.windows import evaluation_windows, fdc_header_line, non_exceedance, observed_duration
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sampling.sttngs', '01/01/2007', '31/12/2007', 180)
    np.random.seed(2025)
    n = 256
    lhs = LHS('Catchment', root, 'csv', 'csv', sample_size=n, settings_filename='Catchment.sampling.sttngs')
    lhs.model.extra = EXTRA
    lhs.run()
    obs = np.asarray(lhs.model.nd_flow, dtype=np.float64)
    sim = lhs.model.simulate_ensemble(lhs._sample, save_discharge=True, math_mode=lhs.math_mode).discharge.cpu().numpy().T
    ids, labels = evaluation_windows(lhs.model.timeseries_report[1:], by='hydro_year')
    assert labels == ['2007', '2008']
    res = lhs.flow_duration_curves(windows='hydro_year', write=True)
    p = [0.01, 0.05, 0.1, 0.2, 0.5, 0.8, 0.9, 0.95, 0.99]
    q = non_exceedance(p)
    assert res.exceedance == p and res.labels == labels and res.transform == 'none' and res.eps == 0.0
    assert res.segment == (0.0, 1.0) and res.names[0] == 'NSE' and res.device_values.is_cuda
    assert res.curves.shape == (2, 9, n) and res.values.shape == (2, n, 7) and res.observed.shape == (2, 9)
    want_q, want = statement(sim, q, obs, ids, 2, objfn=True)
    assert same_values(res.curves, want_q)
    assert np.all(res.curves[:, 0] >= res.curves[:, -1])                # Q1 is the high flow
    compare(res.values, want, 'hydrological years through the model')
    assert bits_equal(res.values, res.device_values.cpu().numpy())
    assert np.array_equal(res.observed, observed_duration(obs, ids, 2, q))
    for w in range(2):
        x = np.sort(obs[(ids == w) & ~np.isnan(obs)])
        assert res.observed[w].tolist() == [x[rank_of(qk, x.size) - 1] for qk in q]
    level = float(np.median(res.values[0][:, 0]))
    on_device = condition_mask(res.device_values[0][:, [0]], [(level,)], ['min'])
    assert np.array_equal(on_device.cpu().numpy(), condition_mask(res.values[0][:, [0]], [(level,)], ['min']))
    # the file: the characters are those of '%.6e' of the float32 of curves / values, and parse back to it within half a
    # unit of the seventh digit (seven printed digits do not round-trip a float32)
    assert res.file == lhs.fdc_file and os.path.normpath(res.file) == os.path.join(root, 'out', 'Catchment', 'Catchment.SMART.lhs.fdc')
    lines = open(res.file).read().split('\n')
    assert len(lines) == n + 2 and lines[-1] == '' and lines[0] + '\n' == fdc_header_line(p, labels)
    kept = np.concatenate([res.curves.astype(np.float32).transpose(2, 0, 1).reshape(n, 18),
                           res.values.astype(np.float32).transpose(1, 0, 2).reshape(n, 14)], axis=1)
    assert [line.split(',') for line in lines[1:-1]] == [['%.6e' % v for v in row] for row in kept]
    back = np.array([[float(v) for v in line.split(',')] for line in lines[1:-1]])
    assert back.shape == (n, 32) and rel_to_want(back, kept.astype(np.float64)) <= 5.0e-7
    # a low-flow score: ln(Q + eps) over the bottom 30 % of the ranks, eps from the observations
    low = lhs.flow_duration_curves(exceedance=(0.7, 0.95), windows='all', transform='log', segment=(0.0, 0.3))
    assert low.file is None and low.labels == ['all'] and low.eps == float(np.mean(obs[~np.isnan(obs)])) / 100.0
    want_q, want = statement(sim, non_exceedance((0.7, 0.95)), obs, None, 1, 'log', low.eps, (0.0, 0.3), objfn=True)
    assert same_values(low.curves, want_q)
    compare(low.values, want, 'low flows through the model')
