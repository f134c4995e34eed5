"""Weighted ensemble quantiles (the GLUE prediction bounds): the definition as a numpy statement, what any summation
order must satisfy, and inputs whose thresholds are known to the bit.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

DYADIC = (0.0625, 0.5, 0.9375, 1.0)


def weighted_quantile(x, w, q):
    """THE DEFINITION for one report step: the smallest value v among x with sum(w[x <= v]) >= q * sum(w); NaN sorts
    last (numpy.sort), a total weight of zero gives NaN; w = None: equal weights."""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(x.size) if w is None else np.asarray(w, dtype=np.float64)
    order = np.argsort(x, kind='stable')
    cum = np.cumsum(w[order])
    if not cum[-1] > 0.0:
        return float('nan')
    first = np.searchsorted(cum, q * cum[-1], side='left')     # the first position with cum >= q * W
    return float(x[order][first])


def statement(matrix, w, probs):
    """weighted_quantile for every row of a [R, N] matrix -> [K, R]."""
    return np.array([[weighted_quantile(row, w, q) for row in np.asarray(matrix)] for q in probs])


def band_violations(x, w, q, v):
    """What a weighted quantile computed in ANY summation order must satisfy for general (inexact) weights: v is an
    element of the row, sum(w[x < v]) <= qW (1 + eps) and sum(w[x <= v]) >= qW (1 - eps) with eps = N * 2**-52 (the
    sums taken exactly here).  -> list of what fails (empty: fine)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    eps = x.size * 2.0 ** -52
    t = q * math.fsum(w)
    below, upto = math.fsum(w[x < v]), math.fsum(w[x <= v])
    problems = []
    if not np.any(x == v):
        problems.append('%r is no element of the row' % v)
    if not below <= t * (1 + eps):
        problems.append('q=%g: sum(w[x < v]) = %r > %r' % (q, below, t * (1 + eps)))
    if not upto >= t * (1 - eps):
        problems.append('q=%g: sum(w[x <= v]) = %r < %r' % (q, upto, t * (1 - eps)))
    return problems


def statement_rows(matrix, w, probs):
    """statement, all rows at once (for a matrix of very many short rows): the same stable order, the same left-to-right
    sums, the same single product q * W and the same `cum >= q * W` -> [K, R]."""
    x = np.asarray(matrix, dtype=np.float64)
    w = np.ones(x.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    order = np.argsort(x, axis=1, kind='stable')
    cum = np.cumsum(w[order], axis=1)
    ranked = np.take_along_axis(x, order, axis=1)
    out = np.full((len(probs), x.shape[0]), np.nan)
    live = cum[:, -1] > 0.0
    for k, q in enumerate(probs):
        first = (cum < (q * cum[:, -1])[:, None]).sum(axis=1)          # cum is non-decreasing: the count IS the position
        out[k, live] = ranked[live, first[live]]
    return out


# ---- inputs whose thresholds are known to the bit (tests/test_gpu_quantiles.py launches them) -------------------------
def power_of_two_weights(rng, n):
    """n weights, integer multiples of 2**-10, all > 0, whose sum W is an exact power of two: integers in [1, 2**10), the
    last one raised until the total is a power of two, all divided by 1024.  Every partial sum is exact in any order
    (an integer below 2**34 times 2**-10), W / 2**m is exact, and so is cum / W."""
    units = rng.integers(1, 2 ** 10, size=n)
    total = int(units.sum())
    units[-1] += (1 << (total - 1).bit_length()) - total
    return units.astype(np.float64) / 1024.0


def is_power_of_two(v):
    m, _ = math.frexp(v)
    return v > 0.0 and m == 0.5


def threshold_probs(x, w, positions):
    """For a row x of DISTINCT values, weights with exact partial sums and a power-of-two total W, and sorted positions
    j: the probabilities p_j = cum[j] / W (exact), nextafter(p_j, 2) and nextafter(p_j, 0), and what the definition
    gives for them -- x_sorted[j]; the next element of POSITIVE weight (x_sorted[j + 1] unless that one weighs nothing:
    p * W is then above cum[j] by less than one weight unit, and an element of weight zero does not move cum); and
    x_sorted[j] again (p * W is below cum[j] by less than a unit, so above cum[j - 1]).
    Every position must carry weight, lie before the last one (j < n - 1) and have weight after it (p_j < 1), so that
    all probabilities stay inside (0, 1].  -> (probs [3 * len(positions)], values [3 * len(positions)])."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    order = np.argsort(x, kind='stable')
    ranked, wr = x[order], w[order]
    assert np.all(ranked[1:] > ranked[:-1]), 'the values of the row must be distinct'
    cum = np.cumsum(wr)
    W = cum[-1]
    assert is_power_of_two(W), 'the total weight %r is no power of two' % W
    probs, values = [], []
    for j in positions:
        assert 0 <= j < x.size - 1 and wr[j] > 0.0 and cum[j] < W, 'position %d carries no weight or has none after it' % j
        p = cum[j] / W
        assert p * W == cum[j], 'p W is not exact at position %d' % j
        after = j + 1
        while wr[after] == 0.0:
            after += 1
        probs += [p, np.nextafter(p, 2.0), np.nextafter(p, 0.0)]
        values += [ranked[j], ranked[after], ranked[j]]
    assert all(0.0 < p <= 1.0 for p in probs), 'a probability outside (0, 1]: %r' % (probs,)
    return tuple(float(p) for p in probs), np.array(values)


def distinct_rows(rng, R, n):
    """R independent random permutations of n distinct values."""
    return np.stack([rng.permutation(n).astype(np.float64) * 0.25 - n / 8.0 for _ in range(R)])


def weightless_successor(x, w, rng):
    """Take the weight off one element of the row x (not its largest, not its smallest) and give it to the row's largest
    element, so the total stays what it was -> (weights, j): sorted position j is followed by an element of weight zero."""
    order = np.argsort(x, kind='stable')
    j = int(rng.integers(0, x.size - 2))
    w = w.copy()
    w[order[-1]] += w[order[j + 1]]
    w[order[j + 1]] = 0.0
    return w, j


# the NaNs a row may hold: quiet and signalling, either sign, with and without a payload
NAN_BITS = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000abc, 0xfff8000000000001,
                     0x7ff0000000000001, 0xfff4000000000000, 0x7fffffffffffffff, 0xffffffffffffffff], dtype=np.uint64)
NAN_SHARE = 0.4
THRESHOLD_SIZES = (65, 1025, 2048, 2049, 4096, 4097, 8192)
SUBNORMAL, HUGE = 2.0 ** -1060, 2.0 ** 900


def mixed_nans(rng, size):
    return rng.choice(NAN_BITS, size=size).view(np.float64)


def many_nan_rows(rng, x):
    """Puts NaNs of every kind on ceil(NAN_SHARE * N) random places of every row of x (its own places per row)."""
    R, N = x.shape
    count = math.ceil(NAN_SHARE * N)
    for r in range(R):
        x[r, rng.permutation(N)[:count]] = mixed_nans(rng, count)
    return x
