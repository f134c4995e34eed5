"""smart_objfn_bootstrap_hip on the GPU against the yardstick of oracle/analyses/bootstrap.py (`truth`: direct resampling
in np.longdouble).

Shapes are the smallest at which the kernels can go wrong.  R: 1, 2 (fewer than two rows, and exactly two), 9, 501, 1025
(one compaction chunk of 1,024 rows plus a row), 4097.  N: 1, 63, 65, 257, 300 (and 700 for the chunks).  W: 1, 2, 11, 16 and the cap (64).  B: 0, 1
(STD is NaN), 2, 63, 65, 257 and the cap (4,096).  The cap lies inside flow_duration_sort_capacity() (16,384), so the select
form of the order statistics is NOT reachable from this entry and no case asks for it.  The chunking over the samples: at
B = the cap a chunk is 576 samples (smart_bootstrap_workspace_bytes: 7 B doubles per sample stay below 128 MiB), so N = 700
is a full chunk and a partial one -- the host test of the workspace entry shows that its answer stops growing there.
'none' runs at every shape, the other three transforms at one shape each (eps = 0.01).  ld = N + pad with NaN in the
padding; every output lies 64 doubles inside a buffer of sentinels.

Counts (oracle.analyses.bootstrap.make_counts): random draws; row 0 all ones (bit-equal to `point` in `replicates`), row 1 all
zeros (NaN for every sample), row 2 a single window W times, row 3 with 65,535 somewhere -- as many of them as B has room
for.  With R = 1 every replicate has fewer than two rows or repeats one row, whose scores are 0 / 0: the case keeps to
B = 2 (ones, zeros), all NaN.

Data: the generator of tests/cases_signatures.py; windows arange(R) * W // R with 10 % of the rows in no window.

Gates.  The pattern of NaN (and of infinities) is equal everywhere; point, replicates, MEAN and STD are held to `truth` at
relative 1e-9 with |want| floored at 1e-12, every compared |want| asserted to be 0 or above 1e-6 (a seed that fails this
is changed, not the gate), STD only where truth's STD is above 1e-6; the quantile rows are the elements
np.quantile(replicates from the GPU, method='inverted_cdf') names, bit for bit (a zero against a zero of either sign, which
the order keys hold to be one value); point against smart_objfn_windows_hip with every windowed row in one window at the
same gate.  The largest margin per column is printed at the end of the module (and written to
$SMART_MARGINS_DIR/bootstrap_margins.txt where that is set); profiles/bootstrap_margins.txt is that table."""
import os

import numpy as np
import pytest

from cases_signatures import data
from oracle.analyses.bootstrap import truth, inverted_cdf, windows_of, make_counts, worst, assert_comparable, NAMES
from support import (EXTRA, E_SIZE, GATE, Guarded, Margins, bits_equal, example_root, margins_dir, padded, same_values,
                     settings_file, to_device, workspace)

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
MARGINS = Margins()     # column name -> (largest margin as a fraction of the gate, where it was seen)
CAP_W, CAP_B = 64, 4096
# (R, N, W, B, transform)
CASES = [(1, 65, 1, 2, 'none'), (2, 63, 1, 63, 'none'), (2, 257, 2, 1, 'none'), (9, 1, 2, 0, 'none'),
         (9, 700, 2, CAP_B, 'none'), (501, 65, 11, 65, 'none'), (501, 65, 11, 65, 'sqrt'), (501, 63, 16, 257, 'log'),
         (1025, 257, 16, 63, 'inverse'), (1025, 257, 16, 63, 'none'), (1025, 65, CAP_W, 2, 'none'),
         (4097, 65, 11, 65, 'none'), (501, 300, 16, 257, 'none')]


def launch(sim, obs, win, W, counts, transform='none', eps=0.0, probs=PROBS, pad=3, with_reps=True, expect=0, **over):
    """The C entry on a [R, N] host matrix laid out with ld = N + pad (the padding holds NaN) -> (point [N, 7], stats
    [7, 2 + K, N] or None, replicates [B, 7, N] or None) as numpy.  Every output lies support.GUARD doubles inside a buffer of
    support.SENTINEL; everything around what the call owns is checked to be as it was.  over: arguments of the entry to replace."""
    import ctypes
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    R, N = sim.shape
    counts = np.ascontiguousarray(counts, dtype=np.uint16).reshape(-1, W)
    B, K = counts.shape[0], len(probs)
    d_sim, ld = padded(sim, pad)
    d_obs, d_win = to_device(obs), to_device(win, np.int32)
    d_counts = torch.from_numpy(counts.view(np.int16).copy()).cuda() if B else None
    q = (ctypes.c_double * max(K, 1))(*probs)
    sizes = [N * 7, 7 * (2 + K) * N if B else 0, B * 7 * N if with_reps else 0]
    bufs = [Guarded(s) for s in sizes]
    need = int(L.smart_bootstrap_workspace_bytes(N, min(W, CAP_W), min(B, CAP_B), 1 if with_reps else 0))
    work = workspace(need, least=256)
    a = dict(n=N, r=R, ld=ld, w=W, b=B, k=K, transform=_lib.TRANSFORMS.get(transform, transform), eps=float(eps),
             ws_bytes=need)
    a.update(over)
    rc = L.smart_objfn_bootstrap_hip(a['n'], a['r'], d_sim.data_ptr(), a['ld'], d_obs.data_ptr(), d_win.data_ptr(), a['w'],
                                     a['transform'], a['eps'], d_counts.data_ptr() if B else None, a['b'], q, a['k'],
                                     bufs[0].ptr(), bufs[1].ptr(null=not B), bufs[2].ptr(null=not (with_reps and B)),
                                     work.data_ptr(), a['ws_bytes'], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, (rc, L.smart_last_error().decode())
        assert all(b.untouched() for b in bufs)
        return L.smart_last_error().decode()
    _lib.check(rc)
    out = []
    for buf in bufs:
        own, intact = buf.read()
        assert intact
        out.append(own)
    return (out[0].reshape(N, 7), out[1].reshape(7, 2 + K, N) if B else None,
            out[2].reshape(B, 7, N) if with_reps and B else None)


def hold(got, want, what, probs=PROBS):
    """every gate of the module's docstring on one launch; got and want are (point, stats, replicates)"""
    (point, stats, reps), (w_point, w_stats, w_reps) = got, want
    assert_comparable(w_point, what)
    assert_comparable(w_reps, what)
    for s, name in enumerate(NAMES):
        pairs = [('point', point[:, s], w_point[:, s])]
        if stats is not None:
            std_ok = w_stats[s, 1] > 1e-6
            assert np.array_equal(np.isnan(stats[s, 1]), np.isnan(w_stats[s, 1])), what + ': the pattern of NaN in STD'
            pairs += [('MEAN', stats[s, 0], w_stats[s, 0]), ('STD', stats[s, 1][std_ok], w_stats[s, 1][std_ok])]
            if reps is not None:
                pairs.append(('replicates', reps[:, s], w_reps[:, s]))
            else:                   # (a caller that keeps no replicates: the quantiles against truth's, at the gate)
                pairs.append(('quantiles', stats[s, 2:], w_stats[s, 2:]))
        for kind, g, w in pairs:
            err = worst(g, w)
            print('%s %s %s %.3e' % (what, name, kind, err))
            MARGINS.note(name, err / GATE, what + ' ' + kind)
            assert err < GATE, '%s: %s of %s off by %.3e' % (what, kind, name, err)
    if stats is not None and reps is not None:
        got_q = np.transpose(stats[:, 2:], (1, 0, 2))                   # [K, 7, N]
        assert same_values(got_q, inverted_cdf(reps, probs), any_nan=True), what + ': the quantiles'
        clean = ~np.isnan(reps).any(axis=0)                             # (numpy gives NaN for a column that holds one)
        if clean.any():
            numpy_says = np.quantile(reps, probs, axis=0, method='inverted_cdf')
            assert same_values(got_q[:, clean], numpy_says[:, clean], any_nan=True), what + ': np.quantile'


@pytest.fixture(scope='module', autouse=True)
def _print_the_margins():
    yield
    if not MARGINS:
        return
    text = ('largest error of this run against truth (direct resampling in longdouble), as a fraction of the gate (relative '
            '1e-9 with |want| floored at 1e-12), over point, replicates, MEAN and STD: column, margin, where it was seen\n' +
            '\n'.join('%-6s %-10.3g %s' % (name, MARGINS[name][0], MARGINS[name][1]) for name in NAMES if name in MARGINS) +
            '\nquantiles: the elements np.quantile(method=inverted_cdf) names on the replicates, bit for bit\n')
    MARGINS.publish(text, margins_dir(), 'bootstrap_margins.txt')


def case_inputs(R, n, W, B):
    rng, obs, sim = data(1000 * R + 7 * n + W, R, n)
    if R <= 2:
        obs = sim[:, 0] * np.array([1.1, 0.8])[:R] + 0.01            # (two rows: both observed)
    return sim, obs, windows_of(rng, R, W), make_counts(rng, W, B)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'R%d-N%d-W%d-B%d-%s' % c)
def test_bootstrap_is_the_truth(case):
    from smartpy_amd import engine
    assert (engine.bootstrap_max_windows(), engine.bootstrap_max_resamples()) == (CAP_W, CAP_B)
    assert CAP_B <= engine.flow_duration_sort_capacity()            # the select form is not reachable (docstring)
    R, n, W, B, transform = case
    sim, obs, win, counts = case_inputs(R, n, W, B)
    eps = 0.0 if transform == 'none' else 0.01
    what = 'R=%d n=%d W=%d B=%d %s' % case
    want = truth(sim, obs, win, W, counts, transform, eps, PROBS)
    got = launch(sim, obs, win, W, counts, transform, eps)
    hold(got, want, what)
    point, stats, reps = got
    if B >= 1:
        assert bits_equal(reps[0].T, point), what + ': a row of ones is the point value'
    if B >= 2:
        assert np.isnan(reps[1]).all() and np.isnan(stats[:, :2]).all(), what + ': a row of zeros'
    if B == 1:
        assert np.isnan(stats[:, 1]).all() and not np.isnan(stats[:, 0]).any()
    if 3 <= B <= 300:
        # the row of zeros makes MEAN and STD NaN for every sample: without it they are numbers, held to truth
        keep = counts[np.arange(B) != 1]
        some = launch(sim, obs, win, W, keep, transform, eps, pad=0)
        hold(some, truth(sim, obs, win, W, keep, transform, eps, PROBS), what + ' without the row of zeros')
        assert not np.isnan(some[1][:, 0]).all() and bits_equal(some[2], reps[np.arange(B) != 1])
    if R == 1:
        assert np.isnan(point).all()
    # without the caller's replicates the statistics are the same bits
    bare = launch(sim, obs, win, W, counts, transform, eps, with_reps=False)
    assert bits_equal(bare[0], point) and bare[2] is None
    if B:
        assert bits_equal(bare[1], stats)
    # the point value is what the windowed objective functions give with every windowed row in one window
    one = engine.objective_functions_windows(sim, obs, np.where(win >= 0, 0, -1).astype(np.int32), n_windows=1,
                                             transform=transform, eps=eps).cpu().numpy()[0]
    err = worst(point, one)
    MARGINS.note('point', err / GATE, what + ' against smart_objfn_windows_hip')
    assert err < GATE, what


def test_planted_columns():
    R, n, W = 501, 65, 3
    rng, obs, sim = data(5, R, n)
    win = (np.arange(R) * 2 // R).astype(np.int32)                      # 0 and 1 occur, window 2 never does
    valid = ~np.isnan(obs)
    counts = np.array([[1, 1, 1], [0, 0, 0], [0, 2, 5], [3, 0, 65535], [1, 2, 0], [2, 0, 0], [0, 1, 1]], dtype=np.uint16)
    draws0, draws1 = counts[:, 0] > 0, counts[:, 1] > 0
    sim[:, 0] = 2.5                                                     # constant
    sim[np.flatnonzero(valid & (win == 1))[7], 5] = np.nan              # a NaN in a valid row of window 1
    sim[np.flatnonzero(valid & (win == 0))[9], 6] = np.inf              # an infinity in a valid row of window 0
    sim[np.flatnonzero(~valid), 7] = np.nan                             # NaN only in rows that are not valid
    clean = sim.copy()
    overflow = sim.copy()
    overflow[:, 8] *= 1e154                                             # squares that overflow: a non-finite sum
    want = truth(sim, obs, win, W, counts)
    point, stats, reps = got = launch(sim, obs, win, W, counts, pad=5)
    hold(got, want, 'planted columns')
    assert np.isnan(reps[:, 2, 0][counts.sum(axis=1) > 0]).all() and np.all(reps[:, 3, 0][counts.sum(axis=1) > 0] == 0.0)
    assert np.isnan(point[0, 2]) and point[0, 3] == 0.0                 # KGEc NaN and KGEa 0, as finish_objectives gives
    assert np.isnan(reps[draws1][:, :, 5]).all() and not np.isnan(reps[~draws1 & draws0][:, :, 5]).any()
    assert np.isnan(reps[draws0][:, :, 6]).all() and not np.isnan(reps[~draws0 & draws1][:, :, 6]).any()
    assert np.isnan(stats[:, :2, 5]).all() and np.isnan(point[[5, 6]]).all()
    clean[:, 7] = 1.0
    clean[valid, 7] = sim[valid, 7]
    again = launch(clean, obs, win, W, counts, pad=5)
    assert not np.isnan(reps[draws0 | draws1][:, :, 7]).any()
    assert bits_equal(got[0][7], again[0][7]) and bits_equal(got[1][..., 7], again[1][..., 7]) and \
        bits_equal(got[2][..., 7], again[2][..., 7])                    # nothing changes
    big = launch(overflow, obs, win, W, counts, pad=5)
    assert np.isnan(big[0][8]).all() and np.isnan(big[2][:, :, 8]).all() and np.isnan(big[1][:, :2, 8]).all()
    assert bits_equal(got[0][9:], big[0][9:]) and bits_equal(got[1][..., 9:], big[1][..., 9:]) and \
        bits_equal(got[2][..., 9:], big[2][..., 9:])
    # an observation that makes ln non-finite under 'log': every sample, for the replicates that draw its window
    bad = obs.copy()
    bad[np.flatnonzero(valid & (win == 1))[3]] = -1.0
    want = truth(sim[:, 9:], bad, win, W, counts, 'log', 0.01)
    point, stats, reps = got = launch(sim[:, 9:], bad, win, W, counts, 'log', 0.01)
    hold(got, want, 'planted observation')
    assert np.isnan(reps[draws1]).all() and not np.isnan(reps[~draws1 & draws0]).any() and np.isnan(point).all()


def test_two_launches_give_the_same_bits():
    R, n, W, B = 1025, 300, 16, 65
    sim, obs, win, counts = case_inputs(R, n, W, B)
    first = launch(sim, obs, win, W, counts, pad=1)
    for pad in (1, 70):                                                 # ... whatever the leading dimension
        assert all(bits_equal(a, b) for a, b in zip(first, launch(sim, obs, win, W, counts, pad=pad)))


def test_an_error_return_leaves_the_outputs_untouched():
    R, n, W, B = 9, 5, 2, 4
    sim, obs, win, counts = case_inputs(R, n, W, B)
    assert 'n_windows' in launch(sim, obs, win, W, counts, expect=E_SIZE, w=CAP_W + 1)
    assert 'n_resamples' in launch(sim, obs, win, W, counts, expect=E_SIZE, b=CAP_B + 1)
    assert 'workspace_bytes' in launch(sim, obs, win, W, counts, expect=E_SIZE, ws_bytes=64)
    assert 'ld' in launch(sim, obs, win, W, counts, expect=E_SIZE, ld=n - 1)
    assert 'probability' in launch(sim, obs, win, W, counts, probs=(0.5, 0.0, 0.9), expect=E_SIZE)
    assert 'transform' in launch(sim, obs, win, W, counts, expect=-7, transform=4)


def test_engine_surface():
    import torch
    from smartpy_amd import engine
    from smartpy_amd.montecarlo.selection import pareto_rows, condition_mask
    R, n, W, B = 501, 130, 4, 33
    rng, obs, sim = data(41, R, n)
    ids = np.minimum(np.arange(R) * 3 // R, 2).astype(np.int32)         # 0, 1, 2 occur; window 3 never does
    counts = engine.bootstrap_counts(W, B, seed=5, eligible=[1, 1, 1, 0])
    want = truth(sim, obs, ids, W, counts, 'sqrt', 0.0, (0.1, 0.9))
    wide = torch.full((R, n + 63), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :n] = torch.from_numpy(sim).cuda()
    res = engine.objective_functions_bootstrap(wide[:, :n], torch.from_numpy(obs).cuda(), torch.from_numpy(ids).cuda(),
                                               counts, probs=(0.1, 0.9), n_windows=W, transform='sqrt', replicates=True)
    assert res.point.is_cuda and tuple(res.point.shape) == (n, 7) and tuple(res.stats.shape) == (7, 4, n)
    assert tuple(res.replicates.shape) == (B, 7, n) and res.stats[1, 2].is_contiguous()
    got = (res.point.cpu().numpy(), res.stats.cpu().numpy(), res.replicates.cpu().numpy())
    hold(got, want, 'engine, strided view', (0.1, 0.9))
    # host arrays and counts on the device; no replicates
    on_device = torch.from_numpy(counts.view(np.int16).copy()).cuda()
    bare = engine.objective_functions_bootstrap(sim, obs, ids, on_device, probs=(0.1, 0.9), n_windows=W, transform='sqrt')
    assert bare.replicates is None and bits_equal(bare.stats.cpu().numpy(), got[1]) and bits_equal(bare.point.cpu().numpy(), got[0])
    # a row of stats goes to the selection as it is
    low = res.stats[1, 2]
    assert tuple(low.shape) == (n,)
    rows, ranks = pareto_rows(torch.stack([low, res.stats[0, 2]], dim=1), ['max', 'max'])
    h_rows, h_ranks = pareto_rows(np.stack([got[1][1, 2], got[1][0, 2]], axis=1), ['max', 'max'])
    assert np.array_equal(rows.cpu().numpy(), h_rows) and len(h_rows) >= 1
    mask = condition_mask(low.reshape(-1, 1), [(0.0,)], ['min'])
    assert mask.is_cuda and np.array_equal(mask.cpu().numpy(), condition_mask(got[1][1, 2].reshape(-1, 1), [(0.0,)], ['min']))
    none = engine.objective_functions_bootstrap(sim, obs, ids, counts[:0], n_windows=W)
    assert none.stats is None and none.replicates is None
    assert worst(none.point.cpu().numpy(), truth(sim, obs, ids, W, counts[:0])[0]) < GATE
    empty = engine.objective_functions_bootstrap(torch.empty((R, 0), dtype=torch.float64, device='cuda'), obs, ids, counts,
                                                 n_windows=W, replicates=True)
    assert tuple(empty.point.shape) == (0, 7) and tuple(empty.stats.shape) == (7, 5, 0) and tuple(empty.replicates.shape) == (B, 7, 0)


def test_through_the_model(tmp_path):
    from smartpy_amd import engine, windows as swin
    from smartpy_amd.montecarlo import LHS
    from smartpy_amd.montecarlo.selection import as_stored
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sampling.sttngs', '01/01/2007', '31/12/2010', 180)
    np.random.seed(2025)
    n = 70
    lhs = LHS('Catchment', root, 'csv', 'csv', sample_size=n, settings_filename='Catchment.sampling.sttngs')
    lhs.model.extra = EXTRA
    obs = np.asarray(lhs.model.nd_flow, dtype=np.float64)
    sim = lhs.model.simulate_ensemble(lhs._sample, save_discharge=True, math_mode=lhs.math_mode).discharge.cpu().numpy().T
    ids, labels = swin.evaluation_windows(lhs.model.timeseries_report[1:], by='hydro_year')
    assert labels == ['2007', '2008', '2009', '2010', '2011']
    eligible, least = swin.eligible_windows(obs, ids, 5)
    assert eligible.tolist() == [False, True, True, True, False]       # the two partial years are left out
    res = lhs.score_uncertainty(resamples=64, seed=7, write=True)
    assert res.names == NAMES and res.labels == labels and res.eligible.tolist() == eligible.tolist()
    assert res.seed == 7 and res.resamples == 64 and res.probs == [0.05, 0.5, 0.95] and res.min_steps == least
    assert res.device_stats.is_cuda and tuple(res.device_stats.shape) == (7, 5, n)
    used = np.where(eligible[ids], ids, -1)
    boot = engine.bootstrap_counts(5, 64, seed=7, eligible=eligible)
    jack = engine.jackknife_counts(5, eligible=eligible)
    want = truth(sim, obs, used, 5, boot)
    hold((res.point, res.device_stats.cpu().numpy(), None), want, 'hydrological years through the model')
    assert bits_equal(res.mean, res.device_stats.cpu().numpy()[:, 0]) and bits_equal(res.se_boot, res.device_stats.cpu().numpy()[:, 1])
    assert bits_equal(res.quantiles, res.device_stats.cpu().numpy()[:, 2:])
    theta = truth(sim, obs, used, 5, jack)[2]                           # [3, 7, n]: the leave-one-year-out values
    identity = np.sqrt(2.0 / 3.0 * ((theta - theta.mean(axis=0)) ** 2).sum(axis=0))
    assert worst(res.se_jack, identity) < 1e-6 and res.se_jack.shape == (7, n)
    # the file: header and float32 rows
    assert res.path == lhs.uncertainty_file and \
        os.path.normpath(res.path) == os.path.join(root, 'out', 'Catchment', 'Catchment.SMART.lhs.uncertainty')
    lines = open(res.path).read().split('\n')
    assert len(lines) == n + 2 and lines[-1] == '' and lines[0] + '\n' == swin.uncertainty_header_line(res.probs)
    assert lines[0].startswith('NSE,NSE_se,NSE_jse,NSE_q0.05,NSE_q0.5,NSE_q0.95,KGE,')
    back = np.array([[float(v) for v in line.split(',')] for line in lines[1:-1]], dtype=np.float32)
    table = np.concatenate([res.point[:, :, None], res.se_boot.T[:, :, None], res.se_jack.T[:, :, None],
                            np.transpose(res.quantiles, (2, 0, 1))], axis=2).reshape(n, 7 * 6)
    assert np.array_equal(back, as_stored(table), equal_nan=True)
    with pytest.raises(Exception, match='at least three windows'):
        lhs.score_uncertainty(resamples=8, min_steps=360)
    with pytest.raises(Exception, match='at least three windows'):
        lhs.score_uncertainty(windows='year', resamples=8, min_steps=366)
