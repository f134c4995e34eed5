"""PAWN sensitivity from the sample at hand: the numpy statement of the per-step KS statistics in int64, and a brute-force
supremum it is held to.  TEST INFRASTRUCTURE ONLY."""
import math
from fractions import Fraction

import numpy as np

def pawn_counts(cat, B):
    cat = np.asarray(cat)
    return np.stack([np.bincount(row[row < B].astype(np.int64), minlength=B)[:B] for row in cat]).astype(np.int32)


def pawn_statement(y, cat, B):
    """The definition as written, in numpy -> (ks [R, P, B] float64, counts [P, B] int32): a stable argsort of the row, the
    ends of the runs of ties, the cumulative one-hot counts of every bin at those ends, int64 until the one division."""
    y, cat = np.asarray(y, dtype=np.float64), np.asarray(cat)
    R, N = y.shape
    P = len(cat)
    counts = pawn_counts(cat, B)
    ks = np.full((R, P, B), np.nan)
    bins = np.arange(B)
    for r in range(R):
        if not np.isfinite(y[r]).all():
            continue
        order = np.argsort(y[r], kind='stable')
        s = y[r][order]
        ev = np.ones(N, dtype=bool)
        ev[:-1] = s[:-1] != s[1:]                                   # (-0.0 == +0.0: one run)
        at = np.arange(1, N + 1, dtype=np.int64)[ev]                # i + 1 at the evaluation points
        for p in range(P):
            n_b = counts[p].astype(np.int64)
            c = np.cumsum(cat[p][order][:, None] == bins[None, :], axis=0, dtype=np.int64)[ev]
            num = np.abs(at[:, None] * n_b[None, :] - c * np.int64(N)).max(axis=0)
            assert num.max() < 2 ** 48, 'a product of counts of %d does not fit the int64 statement' % num.max()
            with np.errstate(invalid='ignore', divide='ignore'):
                ks[r, p] = np.where(n_b > 0, num.astype(np.float64) / (np.float64(N) * n_b.astype(np.float64)), np.nan)
    return ks, counts


def pawn_brute(y, cat, B):
    """sup over x of |F(x) - F_b(x)| by counting, in exact arithmetic, x running over every sample value -> ks [R, P, B],
    the float of the exact rational (one correctly rounded division)"""
    y, cat = np.asarray(y, dtype=np.float64), np.asarray(cat)
    R, N = y.shape
    P = len(cat)
    ks = np.full((R, P, B), np.nan)
    for r in range(R):
        if not all(math.isfinite(v) for v in y[r]):
            continue
        for p in range(P):
            for b in range(B):
                inside = y[r][cat[p] == b]
                if not len(inside):
                    continue
                best = Fraction(0)
                for x in y[r]:
                    F = Fraction(int((y[r] <= x).sum()), N)
                    Fb = Fraction(int((inside <= x).sum()), len(inside))
                    best = max(best, abs(F - Fb))
                ks[r, p, b] = float(best)
    return ks


def random_case(rng, i):
    N = int(rng.integers(1, 65))
    R, P, B = 3, 2, int(rng.integers(1, 7))
    if i % 2 == 0:
        y = rng.integers(0, 8, size=(R, N)).astype(np.float64)      # ties everywhere
        if N > 2:
            y[0, :2] = (-0.0, 0.0)
    else:
        y = np.exp(rng.normal(0.0, 2.0, size=(R, N)))
    cat = rng.integers(0, B + 1, size=(P, N)).astype(np.uint8)      # B: a value beyond the bins
    cat[cat == B] = 255
    if B > 1:
        cat[1][cat[1] == B - 1] = 0                                  # an empty bin
    return y, cat, B
