"""Score uncertainty (block bootstrap and jackknife of the objective functions), host side: the yardstick, the kernel's
pooled-moment formula held to it, the counts, the C entry's validation without a device, the engine's refusals, the
jackknife identity and the Monte-Carlo surface."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import support
from cases_signatures import data
from conftest import GOLDEN
from oracle.analyses.bootstrap import assert_comparable, make_counts, pooled, truth, windows_of, worst
from support import E_MODE, E_NO_DEVICE, E_NULL, E_SIZE, FAKE, GATE

TRANSFORM_NAMES = ['none', 'sqrt', 'log', 'inverse']


# ---- the yardstick and the formula --------------------------------------------------------------------------------
def test_truth_is_the_oracle_on_unit_counts_and_resamples_directly():
    from oracle import objfn_oracle
    rng, obs, sim = data(7, 120, 5)
    win = windows_of(rng, 120, 3)
    counts = np.array([[1, 1, 1], [2, 0, 1], [0, 0, 0], [0, 3, 0]], dtype=np.uint16)
    point, stats, reps = truth(sim, obs, win, 3, counts)
    rows = (win >= 0) & ~np.isnan(obs)
    want = np.array([objfn_oracle.objective_functions(sim[rows, n], obs[rows])[:7] for n in range(5)])
    assert worst(point, want) < 1e-11 and np.array_equal(point, reps[0].T)
    # replicate 1 is the rows of window 0 twice and those of window 2 once, gathered for real
    take = np.concatenate([np.flatnonzero(rows & (win == 0))] * 2 + [np.flatnonzero(rows & (win == 2))])
    want = np.array([objfn_oracle.objective_functions(sim[take, n], obs[take])[:7] for n in range(5)])
    assert worst(reps[1].T, want) < 1e-11
    assert np.isnan(reps[2]).all() and np.isnan(stats[:, :2]).all()          # an empty replicate; MEAN and STD follow it
    clean = truth(sim, obs, win, 3, counts[[0, 1, 3]])[1]
    reps3 = reps[[0, 1, 3]]
    assert worst(clean[:, 0], reps3.mean(axis=0)) < 1e-12 and worst(clean[:, 1], reps3.std(axis=0, ddof=1)) < 1e-9
    assert np.array_equal(clean[:, 2:], np.transpose(np.quantile(reps3, [0.05, 0.5, 0.95], axis=0, method='inverted_cdf'),
                                                     (1, 0, 2)))
    assert np.isnan(truth(sim, obs, win, 3, counts[:1])[1][:, 1]).all()      # B == 1: no standard deviation
    assert truth(sim, obs, win, 3, counts[:0])[1] is None
    # the rules: a bad value spoils the replicates that draw its window, and no other
    sim[np.flatnonzero(rows & (win == 1))[2], 3] = np.nan
    _, _, bad = truth(sim, obs, win, 3, counts)
    assert np.isnan(bad[[0, 3], :, 3]).all() and not np.isnan(bad[1, :, 3]).any() and not np.isnan(bad[0, :, 2]).any()
    obs[np.flatnonzero(rows & (win == 0))[0]] = -1.0
    _, _, bad = truth(sim, obs, win, 3, counts, 'log', 0.01)
    assert np.isnan(bad[[0, 1]]).all() and not np.isnan(bad[3, :, :3]).any()


@pytest.mark.parametrize('shape', [(9, 63, 2), (501, 65, 11), (1025, 257, 16), (3653, 65, 11)], ids=str)
def test_pooled_moments_are_the_truth(shape):
    R, n, W = shape
    rng, obs, sim = data(31 * R + n, R, n)
    win = windows_of(rng, R, W)
    counts = make_counts(rng, W, 10)
    for transform in TRANSFORM_NAMES:
        what = 'R=%d n=%d W=%d %s' % (R, n, W, transform)
        want_point, _, want = truth(sim, obs, win, W, counts, transform, 0.01)
        assert_comparable(want, what)
        point, got = pooled(sim, obs, win, W, counts, transform, 0.01)
        assert worst(got, want) < GATE / 5 and worst(point, want_point) < GATE / 5, (what, worst(got, want))
        assert np.array_equal(got[0].T, point) and np.isnan(got[1]).all()


def test_pooled_keeps_a_bad_window_out_of_the_replicates_that_do_not_draw_it():
    R, n, W = 501, 9, 3
    rng, obs, sim = data(5, R, n)
    win = (np.arange(R) * 2 // R).astype(np.int32)
    valid = ~np.isnan(obs)
    sim[np.flatnonzero(valid & (win == 1))[7], 1] = np.nan
    sim[np.flatnonzero(valid & (win == 0))[9], 2] = np.inf
    counts = np.array([[1, 1, 1], [2, 0, 5], [0, 2, 0]], dtype=np.uint16)
    want = truth(sim, obs, win, W, counts)[2]
    got = pooled(sim, obs, win, W, counts)[1]
    assert worst(got, want) < GATE
    assert np.isnan(got[[0, 2], :, 1]).all() and not np.isnan(got[1, :, 1]).any()
    assert np.isnan(got[[0, 1], :, 2]).all() and not np.isnan(got[2, :, 2]).any()


# ---- the counts ---------------------------------------------------------------------------------------------------
def test_bootstrap_counts_are_the_documented_draws():
    from smartpy_amd import engine
    a = engine.bootstrap_counts(11, 64, seed=7)
    assert a.dtype == np.uint16 and a.shape == (64, 11) and a.flags.c_contiguous
    assert np.array_equal(a, engine.bootstrap_counts(11, 64, seed=7))
    assert not np.array_equal(a, engine.bootstrap_counts(11, 64, seed=8))
    draws = np.random.Generator(np.random.PCG64(7)).integers(11, size=(64, 11))
    assert np.array_equal(a, np.array([np.bincount(d, minlength=11) for d in draws]))
    assert np.all(a.sum(axis=1) == 11)
    mask = np.array([0, 1, 1, 0, 1, 1, 1, 0], dtype=bool)
    b = engine.bootstrap_counts(8, 33, seed=3, eligible=mask)
    draws = np.random.Generator(np.random.PCG64(3)).integers(5, size=(33, 5))
    want = np.zeros((33, 8), dtype=np.int64)
    for r in range(33):
        want[r, np.flatnonzero(mask)] = np.bincount(draws[r], minlength=5)
    assert np.array_equal(b, want) and np.all(b.sum(axis=1) == 5) and np.all(b[:, ~mask] == 0)
    assert engine.bootstrap_counts(4, 0).shape == (0, 4)
    for kw, word in ((dict(n_windows=0, resamples=1), 'n_windows'), (dict(n_windows=3, resamples=-1), 'resamples'),
                     (dict(n_windows=3, resamples=engine.bootstrap_max_resamples() + 1), 'resamples'),
                     (dict(n_windows=3, resamples=2, eligible=[0, 0, 0]), 'eligible'),
                     (dict(n_windows=3, resamples=2, eligible=[1, 1]), 'eligible'),
                     (dict(n_windows=65536, resamples=1), 'uint16')):
        with pytest.raises(engine.SmartEngineError, match=word):
            engine.bootstrap_counts(**kw)


def test_jackknife_counts():
    from smartpy_amd import engine
    j = engine.jackknife_counts(4)
    assert j.dtype == np.uint16 and np.array_equal(j, 1 - np.eye(4, dtype=np.uint16))
    mask = np.array([1, 0, 1, 1, 0], dtype=bool)
    j = engine.jackknife_counts(5, eligible=mask)
    assert np.array_equal(j, [[0, 0, 1, 1, 0], [1, 0, 0, 1, 0], [1, 0, 1, 0, 0]])
    with pytest.raises(engine.SmartEngineError, match='eligible'):
        engine.jackknife_counts(5, eligible=[1, 1])


def test_jackknife_standard_error_identity():
    from smartpy_amd import windows
    rng = np.random.default_rng(11)
    for E in (3, 4, 10, 37):
        theta = rng.normal(0.7, 0.05, (E, 7, 5))
        want = np.sqrt((E - 1.0) / E * ((theta - theta.mean(axis=0)) ** 2).sum(axis=0))
        got = windows.jackknife_factor(E) * theta.std(axis=0, ddof=1)
        assert np.max(np.abs(got - want) / want) < 1e-14
        assert windows.jackknife_factor(E) == np.sqrt((E - 1.0) ** 2 / E)


# ---- the C entry --------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_the_caps_answer_without_a_device():
    binding, L = support.binding()
    for name in ('smart_objfn_bootstrap_hip', 'smart_bootstrap_workspace_bytes', 'smart_bootstrap_max_windows',
                 'smart_bootstrap_max_resamples'):
        assert name in binding.SYMBOLS and getattr(L, name) is not None
    assert L.smart_bootstrap_max_windows() >= 32 and L.smart_bootstrap_max_resamples() >= 1024
    assert L.smart_abi_version() == 7
    from smartpy_amd import engine
    assert engine.bootstrap_max_windows() == L.smart_bootstrap_max_windows()
    assert engine.bootstrap_max_resamples() == L.smart_bootstrap_max_resamples()
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'smart_amd.h')).read()
    assert '#define SMART_BOOT_MEAN 0' in header and '#define SMART_BOOT_STD 1' in header
    assert binding.BOOT_MEAN == 0 and binding.BOOT_STD == 1
    assert 'fewer than two rows' in header and 'count 0 there is not affected' in header


def test_workspace_bytes():
    _, L = support.binding()
    ws = L.smart_bootstrap_workspace_bytes
    capW, capB = L.smart_bootstrap_max_windows(), L.smart_bootstrap_max_resamples()
    for bad in ((0, 3, 10, 0), (10, 0, 10, 0), (10, capW + 1, 10, 0), (10, 3, -1, 0), (10, 3, capB + 1, 0), (2 ** 31, 3, 1, 0)):
        assert ws(*bad) == E_SIZE, bad
    assert ws(100, 3, 0, 0) >= 100 * 3 * 5 * 8 and ws(100, 3, 0, 0) % 256 == 0
    assert ws(100, 3, 64, 0) >= ws(100, 3, 0, 0) + 64 * 7 * 100 * 8
    assert ws(100, 3, 64, 1) == ws(100, 3, 64, 0)
    # the samples are walked in chunks: what the replicates take stops growing with n_samples
    grow = ws(10 ** 6, 3, capB, 0) - ws(10 ** 5, 3, capB, 0)
    assert abs(grow - 9 * 10 ** 5 * 3 * 5 * 8) < 1024
    assert ws(700, 2, capB, 0) - ws(576, 2, capB, 0) < 1 << 20      # (at the cap a chunk is 576 samples)
    assert ws(576, 2, capB, 0) - ws(288, 2, capB, 0) > 60 << 20


def test_validation_comes_before_the_device():
    _, L = support.binding()
    capW, capB = L.smart_bootstrap_max_windows(), L.smart_bootstrap_max_resamples()
    good = (ctypes.c_double * 3)(0.05, 0.5, 0.95)

    def call(n=100, r=50, sim=FAKE, ld=None, obs=FAKE, window=FAKE, w=3, transform=0, eps=0.0, counts=FAKE, b=10,
             probs=good, k=3, point=FAKE, stats=FAKE, reps=None, ws=FAKE, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = max(0, L.smart_bootstrap_workspace_bytes(n, w, b, 0))
        rc = L.smart_objfn_bootstrap_hip(n, r, sim, n if ld is None else ld, obs, window, w, transform, eps, counts, b,
                                         probs, k, point, stats, reps, ws, ws_bytes, None)
        return rc, L.smart_last_error().decode()

    for name in ('sim', 'obs', 'window', 'point', 'counts', 'probs', 'stats'):
        rc, text = call(**{name: None})
        assert rc == E_NULL and 'smart_objfn_bootstrap_hip' in text and '(%s is NULL)' % name in text, name
    rc, text = call(ws=None)
    assert rc == E_NULL and 'workspace is NULL' in text
    out = (ctypes.c_double * 17)(*([0.5] * 17))
    for kw, word in ((dict(n=0), 'n_samples'), (dict(r=0), 'n_reports'), (dict(r=2 ** 31), 'n_reports'),
                     (dict(w=0), 'n_windows'), (dict(w=capW + 1), 'n_windows'), (dict(b=-1), 'n_resamples'),
                     (dict(b=capB + 1), 'n_resamples'), (dict(k=0), 'n_probs'), (dict(k=17, probs=out), 'n_probs'),
                     (dict(ld=99), 'ld'), (dict(eps=-1.0), 'eps'), (dict(eps=float('nan')), 'eps'),
                     (dict(ws_bytes=L.smart_bootstrap_workspace_bytes(100, 3, 10, 0) - 1), 'workspace_bytes')):
        rc, text = call(**kw)
        assert rc == E_SIZE and 'smart_objfn_bootstrap_hip' in text and word in text, (kw, text)
    for q in (0.0, -0.1, 1.0000001, float('nan')):
        rc, text = call(probs=(ctypes.c_double * 3)(0.5, q, 0.9))
        assert rc == E_SIZE and 'probability 1' in text and '(0, 1]' in text, q
    for t in (-1, 4):
        rc, text = call(transform=t)
        assert rc == E_MODE and 'transform' in text, t
    assert call(sim=None, n=0, transform=9)[0] == E_NULL and call(n=0, transform=9)[0] == E_SIZE
    if L.smart_device_count() == 0:
        # a well-formed call gets as far as the device, and no further; B == 0 needs neither counts nor probs nor stats
        for kw in (dict(), dict(w=capW, b=capB), dict(b=0, counts=None, probs=None, stats=None, k=0), dict(reps=FAKE),
                   dict(probs=(ctypes.c_double * 1)(1.0), k=1, transform=3, eps=0.5)):
            assert call(**kw)[0] == E_NO_DEVICE, kw


# ---- engine and Monte-Carlo surface ---------------------------------------------------------------------------------
def test_engine_refuses_before_any_device_call():
    from smartpy_amd import engine
    sim, obs, win = np.ones((6, 4)), np.ones(6), np.array([0, 0, 1, 1, 2, 2], dtype=np.int32)
    counts = engine.jackknife_counts(3)
    call = engine.objective_functions_bootstrap
    with pytest.raises(engine.SmartEngineError, match="transform 'cube' unknown") as e:
        call(sim, obs, win, counts, transform='cube')
    assert e.value.code == E_MODE
    with pytest.raises(engine.SmartEngineError, match='1 of the 6 window ids'):
        call(sim, obs, np.array([0, 0, 1, 1, 2, 3]), counts, n_windows=3)
    with pytest.raises(engine.SmartEngineError, match='5 window ids for a matrix of shape'):
        call(sim, obs, win[:5], counts, n_windows=3)
    capW, capB = engine.bootstrap_max_windows(), engine.bootstrap_max_resamples()
    with pytest.raises(engine.SmartEngineError, match='%d windows, at most %d' % (capW + 1, capW)):
        call(sim, obs, win, np.zeros((2, capW + 1), dtype=np.uint16), n_windows=capW + 1)
    for bad in (counts.astype(np.int64), counts.astype(np.float64), counts[:, :2], counts.reshape(-1), [[1, 1, 1]]):
        with pytest.raises(engine.SmartEngineError, match='counts must be uint16') as e:
            call(sim, obs, win, bad)
        assert e.value.code == E_SIZE
    with pytest.raises(engine.SmartEngineError, match='%d resamples, at most %d' % (capB + 1, capB)):
        call(sim, obs, win, np.ones((capB + 1, 3), dtype=np.uint16))
    for probs in ((), [0.5] * 17, (0.0, 0.5), (0.5, 1.5), (float('nan'),)):
        with pytest.raises(engine.SmartEngineError, match='probabilities'):
            call(sim, obs, win, counts, probs=probs)
    with pytest.raises(engine.SmartEngineError, match='eps'):
        call(sim, obs, win, counts, eps=-1.0)


def test_every_workflow_has_score_uncertainty():
    from smartpy_amd.montecarlo import LHS, GLUE, Best, Total, Sobol, Pareto
    from smartpy_amd.montecarlo.montecarlo import MonteCarlo
    for cls in (LHS, GLUE, Best, Total, Sobol, Pareto):
        assert cls.score_uncertainty is MonteCarlo.score_uncertainty
    sig = inspect.signature(MonteCarlo.score_uncertainty)
    defaults = {k: p.default for k, p in sig.parameters.items() if k != 'self'}
    assert list(defaults) == ['windows', 'resamples', 'seed', 'quantiles', 'transform', 'eps', 'min_steps', 'start_month',
                              'split', 'write']
    assert defaults == dict(windows='hydro_year', resamples=1000, seed=None, quantiles=(0.05, 0.5, 0.95), transform='none',
                            eps=None, min_steps=None, start_month=10, split=None, write=False)


def test_eligible_windows_and_the_uncertainty_file(tmp_path):
    from smartpy_amd import windows
    from smartpy_amd.montecarlo.analyses import _write_uncertainty_file
    obs = np.ones(1230)
    ids = np.repeat(np.arange(5), [100, 365, 366, 330, 69]).astype(np.int32)
    obs[120:140] = np.nan                                               # window 1 keeps 345 of 365
    mask, least = windows.eligible_windows(obs, ids, 5)
    assert least == 0.9 * 366 and mask.tolist() == [False, True, True, True, False]
    assert windows.eligible_windows(obs, ids, 5, min_steps=70)[0].tolist() == [True, True, True, True, False]
    few, least = windows.eligible_windows(obs[:465], ids[:465], 2)
    assert few.tolist() == [True, True] and least == 1.0
    assert windows.uncertainty_header_line((0.05, 0.5)).startswith('NSE,NSE_se,NSE_jse,NSE_q0.05,NSE_q0.5,KGE,KGE_se,')
    n, K = 3, 2
    rng = np.random.default_rng(1)
    point, se, jse, quant = rng.random((n, 7)), rng.random((7, n)), rng.random((7, n)), rng.random((7, K, n))
    quant[4, 1, 2] = np.nan
    path = str(tmp_path / 'x.uncertainty')
    _write_uncertainty_file(path, (0.05, 0.5), point, se, jse, quant)
    lines = open(path).read().split('\n')
    assert lines[0] + '\n' == windows.uncertainty_header_line((0.05, 0.5)) and lines[-1] == '' and len(lines) == n + 2
    for i in range(n):
        want = ['%.6e' % np.float32(v) for s in range(7) for v in [point[i, s], se[s, i], jse[s, i]] + list(quant[s, :, i])]
        assert lines[1 + i].split(',') == want
