"""Score uncertainty (block bootstrap and jackknife of the objective functions), host side: the yardstick, the kernel's
pooled-moment formula held to it, the counts, the C entry's validation without a device, the engine's refusals, the
jackknife identity and the Monte-Carlo surface.

`truth` is the yardstick of tests/test_gpu_bootstrap.py as well: direct resampling in np.longdouble.  For every replicate
the valid rows of the windows it draws are taken with their multiplicities (a row drawn c times enters every sum c times:
the sums run over (row, multiplicity) pairs, so that a count of 65,535 costs what a count of 1 costs), two-pass means,
variances and covariance, the seven formulas, rounded to float64 at the end; MEAN and STD (ddof = 1) over the replicates in
longdouble; quantiles np.quantile(method='inverted_cdf') on the float64 replicate values with NaN last.  The transform
itself is applied in float64, as the kernel applies it, before anything is widened.

`pooled` is the kernel's formulation in plain float64 numpy: per-window one-pass moments about the launch-wide constants g
and c_n, a replicate as counts x moments, finish_objectives.  It is held to `truth` at the suite's usual gate -- relative
1e-9 with |want| floored at 1e-12, every compared |want| asserted to be 0 or above 1e-6 (a seed that fails this is changed,
not the gate) -- which tells a wrong formula from a rounding difference before a GPU is involved."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_windows_host import transformed, E_NULL, E_SIZE, E_NO_DEVICE, E_MODE
from test_signatures_truth_host import data

LD = np.longdouble
GATE = 1e-9
NAMES = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE']
TRANSFORM_NAMES = ['none', 'sqrt', 'log', 'inverse']


def _seven(s, e, m):
    """s [rows, n], e [rows], m [rows] multiplicities, all longdouble -> [7, n] longdouble: two-pass moments of the
    multiset, the formulas of montecarlo.py:193-209"""
    with np.errstate(all='ignore'):
        cnt = m.sum()
        mc = m[:, None]
        me, ms = (m * e).sum() / cnt, (mc * s).sum(axis=0) / cnt
        de, ds = e - me, s - ms
        var_e, var_s = (m * de * de).sum() / cnt, (mc * ds * ds).sum(axis=0) / cnt
        cov = (mc * ds * de[:, None]).sum(axis=0) / cnt
        d = s - e[:, None]
        A, B, se = (mc * d).sum(axis=0), (mc * d * d).sum(axis=0), (m * e).sum()
        cc = cov / np.sqrt(var_s * var_e)
        cc = np.where(np.isnan(cc), cc, np.clip(cc, -1.0, 1.0))
        alpha = np.sqrt(var_s / var_e)
        beta = 1.0 + A / se
        kge = 1.0 - np.sqrt((cc - 1.0) ** 2 + (alpha - 1.0) ** 2 + (beta - 1.0) ** 2)
        return np.stack([1.0 - B / (var_e * cnt), kge, cc, alpha, beta, 100.0 * (A / se), np.sqrt(B / cnt)])


def inverted_cdf(reps, probs):
    """reps [B, ...] float64 -> [K, ...]: the max(1, ceil(q B))-th smallest along axis 0, NaN last (np.sort puts it there);
    np.quantile(method='inverted_cdf') wherever the column holds no NaN (asserted by the host tests)"""
    B = reps.shape[0]
    ordered = np.sort(reps, axis=0)
    return np.stack([ordered[max(1, int(np.ceil(q * B))) - 1] for q in probs])


def truth(sim, obs, win, W, counts, transform='none', eps=0.0, probs=(0.05, 0.5, 0.95)):
    """-> (point [n, 7], stats [7, 2 + K, n] or None for B == 0, replicates [B, 7, n]), float64"""
    sim, obs, win = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64), np.asarray(win)
    counts = np.asarray(counts).reshape(-1, W).astype(np.int64)
    R, n = sim.shape
    valid = (win >= 0) & (win < W) & ~np.isnan(obs)
    fe64, fs64 = transformed(transform, np.where(valid, obs, 1.0), eps), transformed(transform, sim, eps)
    fe, fs = fe64.astype(LD), fs64.astype(LD)

    def replicate(c):
        m = np.where(valid, c[np.clip(win, 0, W - 1)], 0)
        rows = m > 0
        out = np.full((7, n), np.nan)
        if m.sum() < 2 or not np.isfinite(fe64[rows]).all():
            return out
        clean = np.isfinite(fs64[rows]).all(axis=0)
        if clean.any():
            out[:, clean] = _seven(fs[rows][:, clean], fe[rows], m[rows].astype(LD)).astype(np.float64)
        return out

    point = replicate(np.ones(W, dtype=np.int64)).T.copy()
    B = counts.shape[0]
    reps = np.full((B, 7, n), np.nan)
    for b in range(B):
        reps[b] = replicate(counts[b])
    if B == 0:
        return point, None, reps
    with np.errstate(all='ignore'):
        wide = reps.astype(LD)
        mean = wide.sum(axis=0) / B
        std = np.sqrt(((wide - mean) ** 2).sum(axis=0) / (B - 1)) if B > 1 else np.full((7, n), np.nan)
    stats = np.concatenate([mean.astype(np.float64)[:, None], np.asarray(std, dtype=np.float64)[:, None],
                            np.transpose(inverted_cdf(reps, probs), (1, 0, 2))], axis=1)
    return point, stats, reps


def pooled(sim, obs, win, W, counts, transform='none', eps=0.0):
    """The kernel's formulation in float64 -> (point [n, 7], replicates [B, 7, n])"""
    sim, obs, win = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64), np.asarray(win)
    counts = np.asarray(counts).reshape(-1, W).astype(np.int64)
    R, n = sim.shape
    valid = (win >= 0) & (win < W) & ~np.isnan(obs)
    with np.errstate(all='ignore'):
        fe, fs = transformed(transform, np.where(valid, obs, 1.0), eps), transformed(transform, sim, eps)
        fin = valid & np.isfinite(fe)
        g = fe[fin].sum() / fin.sum() if fin.any() else 0.0
        shift = np.zeros(n)
        if valid.any():
            shift = fs[np.flatnonzero(valid)[0]].copy()
            shift[~np.isfinite(shift)] = 0.0
        ow, mom = np.zeros((W, 4)), np.zeros((W, 5, n))
        for w in range(W):
            rows = valid & (win == w)
            e, s = fe[rows], fs[rows]
            d, u = s - e[:, None], s - shift
            ow[w] = [rows.sum(), e.sum(), (e - g).sum(), ((e - g) ** 2).sum()]
            mom[w] = [d.sum(axis=0), (d * d).sum(axis=0), u.sum(axis=0), (u * u).sum(axis=0),
                      ((e - g)[:, None] * u).sum(axis=0)]

        def replicate(c):
            rn = se = s1 = s2 = 0.0
            acc = np.zeros((5, n))
            for w in range(W):
                if c[w]:                            # a count of 0 does not touch the window's sums (0 x inf)
                    rn, se, s1, s2 = (x + c[w] * y for x, y in zip((rn, se, s1, s2), ow[w]))
                    acc = acc + float(c[w]) * mom[w]
            if rn < 2 or not (np.isfinite(se) and np.isfinite(s2)):
                return np.full((7, n), np.nan)
            A, B, C1, C2, C3 = acc
            see, m1 = s2 - s1 * s1 / rn, C1 / rn
            var_s, var_e, cov = C2 / rn - m1 * m1, see / rn, (C3 - s1 * m1) / rn
            cc = cov / np.sqrt(var_s * var_e)
            cc = np.where(np.isnan(cc), cc, np.clip(cc, -1.0, 1.0))
            alpha, beta = np.sqrt(var_s / var_e), 1.0 + A / se
            out = np.stack([1.0 - B / see, 1.0 - np.sqrt((cc - 1.0) ** 2 + (alpha - 1.0) ** 2 + (beta - 1.0) ** 2), cc,
                            alpha, beta, 100.0 * (A / se), np.sqrt(B / rn)])
            out[:, ~np.isfinite(acc).all(axis=0)] = np.nan
            return out
        point = replicate(np.ones(W, dtype=np.int64)).T.copy()
        reps = np.stack([replicate(c) for c in counts]) if len(counts) else np.empty((0, 7, n))
    return point, reps


def windows_of(rng, R, W):
    """arange(R) * W // R with 10 % of the rows in no window (every row in its window for R < 8)"""
    win = (np.arange(R) * W // R).astype(np.int32)
    if R >= 8:
        win[rng.random(R) < 0.10] = -1
    return win


def make_counts(rng, W, B):
    """[B, W] uint16: random draws (every row sums to W); row 0 all ones, row 1 all zeros, row 2 one window W times, row 3
    with 65,535 somewhere -- as many of the four as B has room for"""
    counts = np.zeros((B, W), dtype=np.int64)
    for b in range(B):
        counts[b] = np.bincount(rng.integers(W, size=W), minlength=W)
    special = [np.ones(W), np.zeros(W), np.where(np.arange(W) == W // 2, W, 0),
               np.where(np.arange(W) == W - 1, 65535, counts[min(3, B - 1)] if B else 0)]
    for b, row in enumerate(special[:B]):
        counts[b] = row
    return counts.astype(np.uint16)


def worst(got, want, floor=1e-12):
    """max |got - want| / max(|want|, floor) over the finite entries of want; the pattern of NaN and the infinities are
    required to be the same (else inf)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return float('inf')
    special = np.isinf(want) | np.isinf(got)
    if not np.array_equal(got[special], want[special]):
        return float('inf')
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), floor)))


def assert_comparable(want, what):
    """every compared |want| is 0 or above 1e-6 (a seed that fails this is changed, not the gate)"""
    x = np.asarray(want, dtype=np.float64)
    x = x[np.isfinite(x)]
    assert x.size == 0 or np.all((x == 0.0) | (np.abs(x) > 1e-6)), what


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
def _lib():
    from smartpy_amd import _lib as binding
    return binding, binding.lib()


def test_symbols_are_bound_and_the_caps_answer_without_a_device():
    binding, L = _lib()
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
    _, L = _lib()
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
    _, L = _lib()
    capW, capB = L.smart_bootstrap_max_windows(), L.smart_bootstrap_max_resamples()
    fake = 4096                         # a non-NULL address that is never followed: every call below is refused first
    good = (ctypes.c_double * 3)(0.05, 0.5, 0.95)

    def call(n=100, r=50, sim=fake, ld=None, obs=fake, window=fake, w=3, transform=0, eps=0.0, counts=fake, b=10,
             probs=good, k=3, point=fake, stats=fake, reps=None, ws=fake, ws_bytes=None):
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
        for kw in (dict(), dict(w=capW, b=capB), dict(b=0, counts=None, probs=None, stats=None, k=0), dict(reps=fake),
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
