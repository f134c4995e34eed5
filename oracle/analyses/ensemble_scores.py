"""Ensemble verification (CRPS, spread, PIT, mean per report step): the five definitions of include/smart_amd.h
(smart_ensemble_scores_hip) as an exact statement in fractions.Fraction -- THE YARDSTICK -- and as a float64 numpy
statement with prefix and suffix sums.  TEST INFRASTRUCTURE ONLY.

TOLERANCE.  Every term of CRPS and SPREAD is a product of non-negative factors, each with a relative error of at most
(N + 1) u (a sum of at most N non-negative numbers in any association, and a quotient; u = 2**-53), three factors and at most
N additions of non-negative terms: 4 (N + 4) u relative covers a float64 evaluation in ANY order of association."""
import bisect
import itertools
import math
from fractions import Fraction

import numpy as np

from oracle.exact import U

CRPS, SPREAD, PIT_LOW, PIT_HIGH, MEAN = range(5)


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
    assert named['W'] * unit < 2 ** 53 and (named['W'] * unit).denominator == 1, 'W = %s is no sum of doubles' % named['W']
    assert named['sum w |x|'].denominator * named['sum w |x|'] < 2 ** 53, \
        'sum w |x| = %s is not exact in float64' % named['sum w |x|']           # every partial sum of w x as well
    for name, v in trace:
        assert representable(v), '%s = %s is not representable' % (name, v)
    # the terms of a sum are multiples of one power of two, fewer than 2**53 of them in the whole sum: every partial sum,
    # in any order, is exact
    for total, terms in ((cols[CRPS], ('t1', 't2')), (cols[SPREAD], ('gap*P*Q',))):
        units = [v.denominator for name, v in trace if name in terms]
        if total is not None and units:
            assert total * max(units) < 2 ** 53, 'a sum over %s is not exact in float64' % (terms,)
    for v in cols:
        assert v is None or representable(v), 'the column %s is not representable' % v
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
            assert np.isnan(got[c]), '%s is NaN in the yardstick, %r in the statement' % (name, got[c])
            continue
        assert np.isfinite(got[c]), '%s is finite in the yardstick, %r in the statement' % (name, got[c])
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
