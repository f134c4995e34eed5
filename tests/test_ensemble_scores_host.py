"""Ensemble verification (CRPS, spread, PIT, mean per report step), host side: the five definitions of
include/smart_amd.h (smart_ensemble_scores_hip) as an exact statement in fractions.Fraction -- THE YARDSTICK -- and as a
float64 numpy statement with prefix and suffix sums, which tests/test_gpu_ensemble_scores.py holds the kernels against;
why the integral form and not the pair form; the aggregates of smartpy_amd/verification.py on hand-worked cases; and the C
entries' validation, done before the device is touched, so a machine without a GPU can test it.

TOLERANCE.  Every term of CRPS and SPREAD is a product of non-negative factors, each with a relative error of at most
(N + 1) u (a sum of at most N non-negative numbers in any association, and a quotient; u = 2**-53), three factors and at most
N additions of non-negative terms: 4 (N + 4) u relative covers a float64 evaluation in ANY order of association."""
import bisect
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

E_NULL, E_SIZE, E_NO_DEVICE, E_MODE = -1, -2, -6, -7
CRPS, SPREAD, PIT_LOW, PIT_HIGH, MEAN = range(5)
U = 2.0 ** -53


def rel_bound(n):
    return 4 * (n + 4) * U


# ---- the yardstick --------------------------------------------------------------------------------------------------
def _scaled(values):
    """doubles -> (integers, unit): value = integer / unit, unit a power of two"""
    ratios = [float(v).as_integer_ratio() for v in values]
    unit = max(d for _, d in ratios)
    return [n * (unit // d) for n, d in ratios], unit


def yardstick(x, w, y, trace=None):
    """The five columns of ONE report step, exactly -> list of five Fractions, None where the column is NaN.  x: the
    members, w: the weights or None (all 1), y: the observation (not finite: missing).  The members of weight zero are
    dropped first; the rest is put in order by a stable sort of the doubles (-0.0 == 0.0 there).  Doubles are integers
    over a power of two: the sums run in integers (sum of gap * A^2 over W^2 and so on), one division at the end.  With
    `trace` a list, every intermediate that a float64 evaluation forms is appended to it as (name, Fraction)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(x.size) if w is None else np.asarray(w, dtype=np.float64)
    live = w > 0
    xs, ws = x[live], w[live]
    if xs.size == 0 or not np.isfinite(xs).all():
        return [None] * 5
    order = np.argsort(xs, kind='stable')
    have_y = bool(np.isfinite(y))
    scaled, xu = _scaled(list(xs[order]) + ([y] if have_y else []))
    X, Y = (scaled[:-1], scaled[-1]) if have_y else (scaled, None)
    Wt, wu = _scaled(ws[order])
    M = len(X)
    A = list(itertools.accumulate(Wt))
    W = A[-1]                                           # B_i = W - A_i, exactly: the suffix sum in integers
    note = (lambda name, v: trace.append((name, v))) if trace is not None else None
    crps_n = spread_n = 0                               # numerators over xu * W * W
    for i in range(M - 1):
        gap = X[i + 1] - X[i]
        if gap == 0:
            continue
        a, b = A[i], W - A[i]
        spread_n += gap * a * b
        if have_y:
            m = min(max(Y, X[i]), X[i + 1])
            crps_n += (m - X[i]) * a * a + (X[i + 1] - m) * b * b
        if note:
            P, Q, g = Fraction(a, W), Fraction(b, W), Fraction(gap, xu)
            note('P', P), note('Q', Q), note('gap*P', g * P), note('gap*P*Q', g * P * Q)
            note('spread', Fraction(spread_n, xu * W * W))
            if have_y:
                lo, hi = Fraction(m - X[i], xu), Fraction(X[i + 1] - m, xu)
                for name, v in (('P*P', P * P), ('Q*Q', Q * Q), ('(m-x)*P', lo * P), ('(x-m)*Q', hi * Q),
                                ('t1', lo * P * P), ('t2', hi * Q * Q), ('t1+t2', lo * P * P + hi * Q * Q),
                                ('crps', Fraction(crps_n, xu * W * W))):
                    note(name, v)
    spread = Fraction(spread_n, xu * W * W)
    wx = sum(a * b for a, b in zip(Wt, X))
    mean = Fraction(wx, xu * W)
    if note:
        note('W', Fraction(W, wu)), note('sum w x', Fraction(wx, xu * wu)), note('mean', mean)
        note('sum w |x|', Fraction(sum(a * abs(b) for a, b in zip(Wt, X)), xu * wu))
    crps = low = high = None
    if have_y:
        crps = Fraction(max(X[0] - Y, 0) + max(Y - X[-1], 0), xu) + Fraction(crps_n, xu * W * W)
        below, upto = bisect.bisect_left(X, Y), bisect.bisect_right(X, Y)
        low = Fraction(A[below - 1] if below else 0, W)
        high = Fraction(A[upto - 1] if upto else 0, W)
        if note:
            note('pit_low', low), note('pit_high', high)
    return [crps, spread, low, high, mean]


def representable(v):
    """a Fraction that is a float64, exactly"""
    return Fraction(float(v)) == v


def assert_all_exact(x, w, y):
    """What the exact cases of the GPU tests claim: every prefix, quotient, product and sum of the step is a float64.
    The prefix and suffix sums are multiples of the smallest weight unit below 2**53 of them (so every partial sum, in
    any order, is exact); the quotients, the products and the running sums are looked at one by one."""
    trace = []
    cols = yardstick(x, w, y, trace)
    w = np.ones(len(x)) if w is None else np.asarray(w, dtype=np.float64)
    unit = max(float(v).as_integer_ratio()[1] for v in w)
    named = dict(trace)
    assert named['W'] * unit < 2 ** 53 and (named['W'] * unit).denominator == 1
    assert named['sum w |x|'].denominator * named['sum w |x|'] < 2 ** 53        # every partial sum of w x as well
    for name, v in trace:
        assert representable(v), (name, v)
    # the terms of a sum are multiples of one power of two, fewer than 2**53 of them in the whole sum: every partial sum,
    # in any order, is exact
    for total, terms in ((cols[CRPS], ('t1', 't2')), (cols[SPREAD], ('gap*P*Q',))):
        units = [v.denominator for name, v in trace if name in terms]
        if total is not None and units:
            assert total * max(units) < 2 ** 53, terms
    for v in cols:
        assert v is None or representable(v)
    return cols


def as_floats(cols):
    return np.array([np.nan if v is None else float(v) for v in cols])


def yardstick_rows(matrix, w, obs):
    """yardstick for every row of a [R, N] matrix -> list of R lists of five"""
    obs = np.full(len(matrix), np.nan) if obs is None else obs
    return [yardstick(row, w, y) for row, y in zip(np.asarray(matrix), obs)]


# ---- the float statement ----------------------------------------------------------------------------------------------
def float_scores(x, w, y, dtype=np.float64):
    """The same five definitions in floating point: prefix sums left to right, suffix sums right to left (never 1 - P),
    non-negative terms only -> array [5] of `dtype` (np.longdouble: the reference where Fractions are too slow)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(x.size) if w is None else np.asarray(w, dtype=np.float64)
    out = np.full(5, np.nan, dtype=dtype)
    live = w > 0
    xs, ws = x[live], w[live]
    if xs.size == 0 or not np.isfinite(xs).all():
        return out
    order = np.argsort(xs, kind='stable')
    X, Wt = xs[order].astype(dtype) + dtype(0.0), ws[order].astype(dtype)
    A = np.cumsum(Wt)
    B = np.concatenate((np.cumsum(Wt[::-1])[::-1][1:], [dtype(0.0)]))
    W = A[-1]
    P, Q = A[:-1] / W, B[:-1] / W
    out[SPREAD] = np.sum((X[1:] - X[:-1]) * P * Q)
    out[MEAN] = np.sum(Wt * X) / W
    if np.isfinite(y):
        y = dtype(y)
        m = np.minimum(np.maximum(y, X[:-1]), X[1:])
        out[CRPS] = max(X[0] - y, dtype(0.0)) + max(y - X[-1], dtype(0.0)) + np.sum((m - X[:-1]) * P * P + (X[1:] - m) * Q * Q)
        below, upto = np.count_nonzero(X < y), np.count_nonzero(X <= y)
        out[PIT_LOW] = (A[below - 1] if below else dtype(0.0)) / W
        out[PIT_HIGH] = (A[upto - 1] if upto else dtype(0.0)) / W
    return out


def statement(matrix, w, obs, dtype=np.float64):
    """float_scores for every row of a [R, N] matrix -> [5, R]"""
    matrix = np.asarray(matrix)
    obs = np.full(len(matrix), np.nan) if obs is None else obs
    return np.stack([float_scores(row, w, y, dtype) for row, y in zip(matrix, obs)], axis=1)


def pair_form(x, w, y):
    """The textbook form E|X - y| - E|X - X'| / 2, O(N^2), float64 -> (crps, spread)"""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(x.size) if w is None else np.asarray(w, dtype=np.float64)
    p = w / w.sum()
    spread = 0.5 * np.sum(p[:, None] * p[None, :] * np.abs(x[:, None] - x[None, :]))
    return np.sum(p * np.abs(x - y)) - spread, spread


def pair_form_sorted(x, w, y):
    """The same pair form the way it is usually evaluated, O(N log N): E|X - X'| / 2 = sum p_(i) x_(i) (2 P_i - p_(i) - 1)
    over the sorted members -- terms of the size of the members, not of their differences -> (crps, spread)"""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(x.size) if w is None else np.asarray(w, dtype=np.float64)
    order = np.argsort(x, kind='stable')
    xs, p = x[order], w[order] / w.sum()
    spread = np.sum(p * xs * (2.0 * np.cumsum(p) - p - 1.0))
    return np.sum(p * np.abs(xs - y)) - spread, spread


def shares(got, exact, x, w):
    """How much of each column's tolerance `got` (five floats) uses against the reference `exact` (five Fractions with
    None for NaN, or five longdoubles) -> dict name: share; the tolerances: CRPS and SPREAD 4 (N + 4) u relative, the
    PITs N u absolute, MEAN N u times sum w |x| / W."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    live = w > 0
    scale = math.fsum(w[live] * np.abs(x[live])) / math.fsum(w[live]) if live.any() else 0.0
    out = {}
    for c, name in enumerate(('CRPS', 'SPREAD', 'PIT_LOW', 'PIT_HIGH', 'MEAN')):
        ref = exact[c]
        if ref is None or (not isinstance(ref, Fraction) and np.isnan(ref)):
            assert np.isnan(got[c]), (name, got[c])
            continue
        assert np.isfinite(got[c]), (name, got[c])
        if isinstance(ref, Fraction):
            err, size = float(abs(Fraction(float(got[c])) - ref)), float(abs(ref))
        else:
            err, size = float(abs(np.longdouble(got[c]) - ref)), float(abs(ref))
        tol = rel_bound(n) * size if c in (CRPS, SPREAD) else n * U * scale if c == MEAN else n * U
        out[name] = 0.0 if err == 0.0 else (err / tol if tol > 0.0 else float('inf'))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------
def gamma_ensemble(rng, n):
    return rng.gamma(2.0, 3.0, size=n), rng.uniform(0.1, 1.0, size=n)


def far_member(rng, n):
    """a tight ensemble and one member far away that weighs next to nothing"""
    x, w = rng.normal(5.0, 0.5, size=n), rng.uniform(0.5, 1.0, size=n)
    x[n // 3], w[n // 3] = 1e9, 1e-12
    return x, w


def observations_around(x, rng):
    """below all members, above all, equal to a member, in between, and missing"""
    ranked = np.sort(x[np.isfinite(x)])
    third = ranked.size // 3
    return [ranked[0] - 1.5, ranked[-1] + 2.5, ranked[ranked.size // 2],
            0.5 * (ranked[third] + ranked[min(third + 1, ranked.size - 1)]), float(rng.uniform(ranked[0], ranked[-1])),
            float('nan')]


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
def _lib():
    from smartpy_amd import _lib as binding
    return binding, binding.lib()


def test_capacity_and_workspace_need_no_device():
    binding, L = _lib()
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
    binding, L = _lib()
    cap = L.smart_ensemble_scores_lds_capacity()
    fake = 4096                         # a non-NULL address that is never followed: every call below is refused first
    entry = 'smart_ensemble_scores_hip: '

    def call(n=100, r=5, sim=fake, ld=None, w=fake, obs=fake, out=fake, method=0, ws=None, ws_bytes=0):
        rc = L.smart_ensemble_scores_hip(n, r, sim, n if ld is None else ld, w, obs, out, method, ws, ws_bytes, None)
        return rc, L.smart_last_error().decode()

    assert call(sim=None) == (E_NULL, entry + 'sim and out are required (sim is NULL)')
    assert call(out=None) == (E_NULL, entry + 'sim and out are required (out is NULL)')
    assert call(n=0) == (E_SIZE, entry + 'need n_samples, n_reports >= 1 (got 0, 5)')
    assert call(r=-2) == (E_SIZE, entry + 'need n_samples, n_reports >= 1 (got 100, -2)')
    assert call(ld=99) == (E_SIZE, entry + 'ld 99 is less than n_samples 100')
    assert call(r=2 ** 31) == (E_SIZE, entry + 'n_reports 2147483648 is more than one launch takes (2^31 - 1)')
    assert call(n=2 ** 24 + 1, method=2, ws=fake, ws_bytes=2 ** 40) == \
        (E_SIZE, entry + 'n_samples 16777217, at most 16777216 (2^24)')
    assert call(n=cap + 1, method=1) == (E_SIZE, entry + 'the LDS form takes at most 8192 samples, not 8193')
    assert call(method=3) == (E_MODE, entry + "method '3' unknown.") and call(method=-1)[0] == E_MODE
    need = 4096 * 16
    assert call(method=2) == (E_NULL, entry + 'a workspace of %d bytes is needed (workspace is NULL)' % need)
    assert call(method=2, ws=fake, ws_bytes=need - 1) == (E_SIZE, entry + 'workspace_bytes %d, need %d' % (need - 1, need))
    assert call(method=2, w=None, ws=fake, ws_bytes=4096 * 8 - 1)[0] == E_SIZE
    assert call(n=cap + 1) == (E_NULL, entry + 'a workspace of %d bytes is needed (workspace is NULL)' % (16384 * 16))
    # two rules broken at once: the missing pointer is named before the size, the size before the method, the method
    # before the workspace
    assert call(sim=None, n=0)[0] == E_NULL and call(n=0, method=9)[0] == E_SIZE
    assert call(method=9, ld=99) == (E_MODE, entry + "method '9' unknown.")
    assert call(ld=99, method=2)[1] == entry + 'ld 99 is less than n_samples 100'
    if L.smart_device_count() == 0:
        # a well-formed call gets as far as the device, and no further: there is no CPU fallback
        for kw in (dict(), dict(w=None, obs=None), dict(n=cap, method=1), dict(method=2, ws=fake, ws_bytes=need),
                   dict(n=cap + 1, ws=fake, ws_bytes=16384 * 16), dict(n=2 ** 24, method=2, ws=fake, ws_bytes=2 ** 28)):
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
