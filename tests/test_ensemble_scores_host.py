"""Ensemble verification (CRPS, spread, PIT, mean per report step), host side: the exact yardstick and the float64
statement of oracle/analyses/ensemble_scores.py (which tests/test_gpu_ensemble_scores.py holds the kernels against);
why the integral form and not the pair form; the aggregates of smartpy_amd/verification.py on hand-worked cases; and the C
entries' validation, done before the device is touched, so a machine without a GPU can test it."""
import math
from fractions import Fraction

import numpy as np
import pytest

import support
from oracle.analyses.ensemble_scores import (CRPS, SPREAD, PIT_LOW, PIT_HIGH, MEAN, as_floats, far_member, float_scores,
                                             gamma_ensemble, observations_around, pair_form, pair_form_sorted, rel_bound,
                                             shares, statement, yardstick)
from support import E_MODE, E_NO_DEVICE, E_NULL, E_SIZE, FAKE


# ---- the float statement against the yardstick --------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 65, 1000, 4096])
@pytest.mark.parametrize('kind', ['gamma', 'far', 'equal_weights'])
def test_float_statement_within_the_bound(kind, n):
    rng = np.random.default_rng(100 * n + len(kind))
    x, w = far_member(rng, n) if kind == 'far' and n >= 3 else gamma_ensemble(rng, n)
    if kind == 'equal_weights':
        w = None
    worst = {}
    for y in observations_around(x, rng):
        got, exact = float_scores(x, w, y), yardstick(x, w, y)
        for name, s in shares(got, exact, x, w).items():
            worst[name] = max(worst.get(name, 0.0), s)
    print(kind, n, 'largest share of the tolerance:', worst)
    assert max(worst.values()) <= 1.0, worst
    if n == 4096:       # the statement is far inside: 1.1e-14 relative was seen against the bound of 1.8e-12
        assert worst['CRPS'] < 0.05 and worst['SPREAD'] < 0.05


def test_yardstick_by_hand():
    """Members 1, 2, 4 with weights 1/4, 1/2, 1/4 and y = 3: F is 1/4 on [1, 2), 3/4 on [2, 4).
    CRPS = 1 * (1/4)^2 + (3 - 2) * (3/4)^2 + (4 - 3) * (1/4)^2 = 11/16; SPREAD = 1 * 3/16 + 2 * 3/16 = 9/16."""
    cols = yardstick([4.0, 1.0, 2.0], [0.25, 0.25, 0.5], 3.0)
    assert cols == [Fraction(11, 16), Fraction(9, 16), Fraction(3, 4), Fraction(3, 4), Fraction(9, 4)]
    assert np.array_equal(float_scores([4.0, 1.0, 2.0], [0.25, 0.25, 0.5], 3.0), as_floats(cols))
    # y on a member: the PITs part; y outside: the distance comes on top, the PITs are 0 or 1
    assert yardstick([4.0, 1.0, 2.0], [0.25, 0.25, 0.5], 2.0)[2:4] == [Fraction(1, 4), Fraction(3, 4)]
    below = yardstick([4.0, 1.0, 2.0], [0.25, 0.25, 0.5], 0.0)
    # E|X - 0| - SPREAD = 9/4 - 9/16
    assert below[0] == Fraction(9, 4) - Fraction(9, 16) and below[2:4] == [0, 0]
    above = yardstick([4.0, 1.0, 2.0], [0.25, 0.25, 0.5], 6.0)
    assert above[0] == (6 - Fraction(9, 4)) - Fraction(9, 16) and above[2:4] == [1, 1]
    # one member; all members equal: no spread, CRPS = |x - y|
    assert yardstick([2.5], None, 4.0) == [Fraction(3, 2), 0, 1, 1, Fraction(5, 2)]
    assert yardstick([2.5] * 7, None, 1.0) == [Fraction(3, 2), 0, 0, 0, Fraction(5, 2)]


def test_special_cases_of_the_definitions():
    nan, inf = float('nan'), float('inf')
    x, w = [1.0, nan, 2.0, inf, -inf, 4.0], [0.25, 0.0, 0.5, 0.0, 0.0, 0.25]
    assert yardstick(x, w, 3.0) == yardstick([4.0, 1.0, 2.0], [0.25, 0.25, 0.5], 3.0)      # weight zero: no part at all
    assert np.array_equal(float_scores(x, w, 3.0), float_scores([1.0, 2.0, 4.0], [0.25, 0.5, 0.25], 3.0))
    assert yardstick(x, None, 3.0) == [None] * 5 and np.isnan(float_scores(x, None, 3.0)).all()    # a live NaN
    assert yardstick([1.0, inf], None, 3.0) == [None] * 5 and np.isnan(float_scores([1.0, -inf], None, 3.0)).all()
    assert yardstick(x, [0.0] * 6, 3.0) == [None] * 5 and np.isnan(float_scores(x, np.zeros(6), 3.0)).all()    # W == 0
    for y in (nan, inf, -inf):          # a missing observation: SPREAD and MEAN are still there
        cols = yardstick(x, w, y)
        assert cols[:1] + cols[2:4] == [None] * 3 and cols[1] == Fraction(9, 16) and cols[4] == Fraction(9, 4)
        got = float_scores(x, w, y)
        assert np.isnan(got[[0, 2, 3]]).all() and got[1] == 9 / 16 and got[4] == 9 / 4
    # -0.0 and +0.0 are one value: among the members and as the observation
    a = yardstick([0.0, -0.0, 1.0, -1.0], None, -0.0)
    assert a == yardstick([0.0, 0.0, 1.0, -1.0], None, 0.0) and a[2:4] == [Fraction(1, 4), Fraction(3, 4)]
    assert np.array_equal(float_scores([0.0, -0.0, 1.0, -1.0], None, -0.0), as_floats(a))
    assert not np.signbit(float_scores([-0.0, -0.0], None, 0.0)[MEAN])


@pytest.mark.parametrize('n', [2, 17, 512])
def test_pair_form_agrees_on_well_spread_ensembles(n):
    rng = np.random.default_rng(7 + n)
    x, w = gamma_ensemble(rng, n)
    for y in observations_around(x, rng):
        if not np.isfinite(y):
            continue
        crps, spread = pair_form(x, w, y)
        got = float_scores(x, w, y)
        fast = pair_form_sorted(x, w, y)
        assert abs(fast[0] - got[CRPS]) <= 1e-12 * got[CRPS] and abs(fast[1] - got[SPREAD]) <= 1e-12 * got[SPREAD]
        assert abs(crps - got[CRPS]) <= 1e-12 * abs(got[CRPS]) and abs(spread - got[SPREAD]) <= 1e-12 * got[SPREAD]
        exact = yardstick(x, w, y)
        assert abs(Fraction(crps) - exact[CRPS]) <= Fraction(1e-12) * exact[CRPS]


def test_tight_ensemble_far_from_zero_is_why_the_integral_form():
    """Members 1e6 +- 1e-3.  The pair form as it is usually evaluated (sorted members, sum p x (2 P - p - 1)) adds terms
    near 1e6, each rounded to 1e-10, for a result near 3e-4: it keeps about six digits where the integral form keeps
    fifteen.  (Evaluated pair by pair, O(N^2), the differences x_i - x_j are exact and nothing is lost -- but that is no
    kernel for 1e5 members.)"""
    rng = np.random.default_rng(11)
    n = 400
    x, w = 1e6 + rng.uniform(-1e-3, 1e-3, size=n), rng.uniform(0.1, 1.0, size=n)
    y = 1e6 + 2.5e-4
    exact = yardstick(x, w, y)
    got = float_scores(x, w, y)

    def rel(v, c):
        return float(abs(Fraction(float(v)) - exact[c]) / exact[c])
    err = {'integral': (rel(got[CRPS], CRPS), rel(got[SPREAD], SPREAD)),
           'pairs one by one': tuple(rel(v, c) for v, c in zip(pair_form(x, w, y), (CRPS, SPREAD))),
           'pairs, sorted': tuple(rel(v, c) for v, c in zip(pair_form_sorted(x, w, y), (CRPS, SPREAD)))}
    print('relative error of (CRPS, SPREAD):', err)
    assert max(err['integral']) <= rel_bound(n)
    assert max(err['pairs one by one']) <= 1e-12
    assert min(err['pairs, sorted']) > 1e-10 and min(err['pairs, sorted']) > 1e4 * max(err['integral'])


# ---- the aggregates -------------------------------------------------------------------------------------------------
def test_reliable_pit_gives_alpha_one_and_a_flat_histogram():
    from smartpy_amd import verification as v
    n = 200
    p = np.arange(1, n + 1) / (n + 1.0)
    rng = np.random.default_rng(0)
    p = p[rng.permutation(n)]
    assert abs(v.reliability(p, p) - 1.0) <= 1.0 / n
    hist = v.pit_histogram(p, p, 10)
    assert hist.shape == (10,) and hist.sum() == n and np.abs(hist - n / 10).max() <= 1.0
    # a PIT that is always 1/2: alpha = 1 - 2 * mean |1/2 - i / (n + 1)| = 1/2 up to 1/n
    assert abs(v.reliability(np.full(n, 0.5), np.full(n, 0.5)) - 0.5) <= 1.0 / n
    assert math.isnan(v.reliability([], [])) and math.isnan(v.reliability([np.nan], [np.nan]))


def test_pit_histogram_spreads_a_step_over_its_interval():
    from smartpy_amd import verification as v
    # [0.2, 0.6] has the width of two of five bins and of four of ten: the step's mass goes to them in equal shares
    five = v.pit_histogram([0.2], [0.6], 5)
    assert np.allclose(five, [0, 0.5, 0.5, 0, 0], atol=1e-15) and five.sum() == 1.0
    ten = v.pit_histogram([0.2], [0.6], 10)
    assert np.allclose(ten, [0, 0, 0.25, 0.25, 0.25, 0.25, 0, 0, 0, 0], atol=1e-15) and abs(ten.sum() - 1.0) < 1e-15
    # an interval that cuts bins: [0.1, 0.5] at 5 bins is a quarter, a half, a quarter
    assert np.allclose(v.pit_histogram([0.1], [0.5], 5), [0.25, 0.5, 0.25, 0, 0], atol=1e-15)
    # points: p = 1 goes to the last bin, p = 0 to the first, an edge to the bin it opens
    assert v.pit_histogram([1.0, 0.0, 0.5], [1.0, 0.0, 0.5], 4).tolist() == [1.0, 0.0, 1.0, 1.0]
    # steps without PITs do not count
    mixed = v.pit_histogram([0.0, np.nan, 0.3], [1.0, np.nan, 0.3], 10)
    assert abs(mixed.sum() - 2.0) < 1e-14 and np.allclose(mixed, [0.1] * 3 + [1.1] + [0.1] * 6, atol=1e-15)


def test_climatological_crps_against_the_yardstick():
    from smartpy_amd import verification as v
    rng = np.random.default_rng(3)
    obs = rng.gamma(2.0, 2.0, size=60)
    obs[[4, 17]] = np.nan
    obs[30] = obs[31]                                           # a tie
    got = v.crps_climatology(obs)
    clim = obs[np.isfinite(obs)]
    assert got.shape == (58,)
    for y, g in zip(np.sort(clim), got):
        exact = yardstick(clim, None, y)[CRPS]
        assert abs(Fraction(float(g)) - exact) <= Fraction(rel_bound(58)) * exact
    at = np.array([-1.0, 100.0, np.nan, clim[5], 0.5 * (clim[5] + clim[6])])
    got = v.crps_climatology(obs, at)
    assert np.isnan(got[2])
    for y, g in zip(at, got):
        if np.isfinite(y):
            exact = yardstick(clim, None, y)[CRPS]
            assert abs(Fraction(float(g)) - exact) <= Fraction(rel_bound(58)) * exact
    assert np.isnan(v.crps_climatology([np.nan, np.nan], [1.0])).all()


def test_verification_object_on_a_small_run():
    from smartpy_amd import verification as v
    rng = np.random.default_rng(5)
    R, N = 40, 30
    sim = rng.gamma(2.0, 2.0, size=(R, N))
    obs = rng.gamma(2.0, 2.0, size=R)
    obs[[3, 9]] = np.nan
    sim[12, 4] = np.nan                                         # a step that has no scores at all
    scores = statement(sim, None, obs)
    ev = v.EnsembleVerification(scores, obs, stamps=list(range(R)), bins=5)
    valid = np.isfinite(scores[CRPS])
    assert ev.n_valid == valid.sum() == R - 3 and ev.file is None and ev.datetime == list(range(R))
    assert np.array_equal(ev.crps, scores[CRPS], equal_nan=True) and np.array_equal(ev.mean, scores[MEAN], equal_nan=True)
    assert ev.mean_crps == scores[CRPS][valid].mean() and ev.mean_spread == scores[SPREAD][valid].mean()
    clim = v.crps_climatology(obs, obs[valid])
    assert np.array_equal(ev.crps_climatology[valid], clim) and np.isnan(ev.crps_climatology[~valid]).all()
    assert ev.skill == 1.0 - ev.mean_crps / clim.mean()
    assert ev.pit_histogram.shape == (5,) and abs(ev.pit_histogram.sum() - ev.n_valid) < 1e-12
    assert ev.reliability == v.reliability(scores[PIT_LOW][valid], scores[PIT_HIGH][valid])
    # nothing valid: every aggregate NaN, an empty histogram
    none = v.EnsembleVerification(np.full((5, R), np.nan), obs, bins=5)
    assert none.n_valid == 0 and math.isnan(none.mean_crps) and math.isnan(none.skill) and math.isnan(none.reliability)
    assert none.pit_histogram.tolist() == [0.0] * 5 and np.isnan(none.crps_climatology).all()


# ---- the C entries ----------------------------------------------------------------------------------------------------
def test_capacity_and_workspace_need_no_device():
    binding, L = support.binding()
    for name in ('smart_ensemble_scores_hip', 'smart_ensemble_scores_workspace_bytes', 'smart_ensemble_scores_lds_capacity'):
        assert name in binding.SYMBOLS
    cap = L.smart_ensemble_scores_lds_capacity()
    assert cap == 8192
    from smartpy_amd import analysis, engine
    assert engine.ensemble_scores_lds_capacity() == analysis.ensemble_scores_lds_capacity() == cap
    assert engine.ensemble_scores is analysis.ensemble_scores
    assert engine.ENSEMBLE_SCORE_NAMES == ['CRPS', 'SPREAD', 'PIT_LOW', 'PIT_HIGH', 'MEAN']
    ws = L.smart_ensemble_scores_workspace_bytes
    AUTO, LDS, GLOBAL = 0, 1, 2
    # the LDS form needs none, and neither does AUTO within the capacity
    assert ws(1000, 3653, 1, LDS) == 0 and ws(cap, 3653, 0, LDS) == 0 and ws(cap, 3653, 1, AUTO) == 0
    # the global form: a step is N rounded up to a power of two (at least 4096) times 16 bytes with weights, 8 without;
    # min(R, as many steps as fit in 256 MiB, at least one) of them
    assert ws(1, 5, 1, GLOBAL) == 5 * 4096 * 16 and ws(1, 5, 0, GLOBAL) == 5 * 4096 * 8
    assert ws(cap + 1, 7, 1, AUTO) == ws(cap + 1, 7, 1, GLOBAL) == 7 * 16384 * 16
    assert ws(100000, 3653, 1, GLOBAL) == 128 * 131072 * 16 == 256 << 20
    assert ws(100000, 3653, 0, GLOBAL) == 256 * 131072 * 8 and ws(100000, 100, 0, GLOBAL) == 100 * 131072 * 8
    assert ws(2 ** 24, 3653, 1, GLOBAL) == 2 ** 24 * 16 and ws(2 ** 24, 3653, 0, GLOBAL) == 2 * 2 ** 24 * 8
    assert ws(2 ** 24 + 1, 1, 1, GLOBAL) == E_SIZE and ws(0, 1, 1, GLOBAL) == E_SIZE and ws(5, 0, 1, AUTO) == E_SIZE
    assert ws(5, 2 ** 31, 1, AUTO) == E_SIZE and ws(cap + 1, 5, 1, LDS) == E_SIZE and ws(5, 5, 1, 3) == E_MODE


def test_validation_comes_before_the_device():
    binding, L = support.binding()
    cap = L.smart_ensemble_scores_lds_capacity()
    entry = 'smart_ensemble_scores_hip: '

    def call(n=100, r=5, sim=FAKE, ld=None, w=FAKE, obs=FAKE, out=FAKE, method=0, ws=None, ws_bytes=0):
        rc = L.smart_ensemble_scores_hip(n, r, sim, n if ld is None else ld, w, obs, out, method, ws, ws_bytes, None)
        return rc, L.smart_last_error().decode()

    assert call(sim=None) == (E_NULL, entry + 'sim and out are required (sim is NULL)')
    assert call(out=None) == (E_NULL, entry + 'sim and out are required (out is NULL)')
    assert call(n=0) == (E_SIZE, entry + 'need n_samples, n_reports >= 1 (got 0, 5)')
    assert call(r=-2) == (E_SIZE, entry + 'need n_samples, n_reports >= 1 (got 100, -2)')
    assert call(ld=99) == (E_SIZE, entry + 'ld 99 is less than n_samples 100')
    assert call(r=2 ** 31) == (E_SIZE, entry + 'n_reports 2147483648 is more than one launch takes (2^31 - 1)')
    assert call(n=2 ** 24 + 1, method=2, ws=FAKE, ws_bytes=2 ** 40) == \
        (E_SIZE, entry + 'n_samples 16777217, at most 16777216 (2^24)')
    assert call(n=cap + 1, method=1) == (E_SIZE, entry + 'the LDS form takes at most 8192 samples, not 8193')
    assert call(method=3) == (E_MODE, entry + "method '3' unknown.") and call(method=-1)[0] == E_MODE
    need = 4096 * 16
    assert call(method=2) == (E_NULL, entry + 'a workspace of %d bytes is needed (workspace is NULL)' % need)
    assert call(method=2, ws=FAKE, ws_bytes=need - 1) == (E_SIZE, entry + 'workspace_bytes %d, need %d' % (need - 1, need))
    assert call(method=2, w=None, ws=FAKE, ws_bytes=4096 * 8 - 1)[0] == E_SIZE
    assert call(n=cap + 1) == (E_NULL, entry + 'a workspace of %d bytes is needed (workspace is NULL)' % (16384 * 16))
    # two rules broken at once: the missing pointer is named before the size, the size before the method, the method
    # before the workspace
    assert call(sim=None, n=0)[0] == E_NULL and call(n=0, method=9)[0] == E_SIZE
    assert call(method=9, ld=99) == (E_MODE, entry + "method '9' unknown.")
    assert call(ld=99, method=2)[1] == entry + 'ld 99 is less than n_samples 100'
    if L.smart_device_count() == 0:
        # a well-formed call gets as far as the device, and no further: there is no CPU fallback
        for kw in (dict(), dict(w=None, obs=None), dict(n=cap, method=1), dict(method=2, ws=FAKE, ws_bytes=need),
                   dict(n=cap + 1, ws=FAKE, ws_bytes=16384 * 16), dict(n=2 ** 24, method=2, ws=FAKE, ws_bytes=2 ** 28)):
            assert call(**kw)[0] == E_NO_DEVICE, kw
    else:
        import torch
        sim = torch.rand(5, 100, dtype=torch.float64, device='cuda')
        out = torch.empty(5, 5, dtype=torch.float64, device='cuda')
        assert call(sim=sim.data_ptr(), w=None, obs=None, out=out.data_ptr())[0] == 0
        torch.cuda.synchronize()


def test_python_layer_refuses_before_the_launch():
    import inspect
    from smartpy_amd import engine
    from smartpy_amd.montecarlo import GLUE
    assert list(inspect.signature(engine.ensemble_scores).parameters) == ['discharge_report_major', 'obs', 'weights', 'method']
    assert list(inspect.signature(GLUE.ensemble_verification).parameters) == ['self', 'likelihood', 'bins', 'write']
    defaults = {k: p.default for k, p in inspect.signature(GLUE.ensemble_verification).parameters.items()}
    assert defaults['likelihood'] is None and defaults['bins'] == 10 and defaults['write'] is False
    with pytest.raises(engine.SmartEngineError, match="method 'sort' unknown"):
        engine.ensemble_scores(np.zeros((3, 4)), method='sort')
