"""Dynamic identifiability analysis: the numpy statement of smart_dynia_hip, and its sums and shares in exact arithmetic.
TEST INFRASTRUCTURE ONLY."""
import math
from fractions import Fraction

import numpy as np

EQUAL, LINEAR = 0, 1


def window(r, R, h, obs):
    """V_r: the observed steps of the window, ascending"""
    return [s for s in range(max(0, r - h), min(R - 1, r + h) + 1) if math.isfinite(obs[s])]


def dynia_statement(sim, obs, cat, n_bins, h, min_valid, fraction, support, err=None):
    """Steps 1 .. 7 of smart_dynia_hip step by step, in float64 -> dict: count [R], E [R, N] (NaN rows where the step is
    not assessed), k [R] (0 where not assessed), cut [R], retained [R], rows (the retained sets, lists), shares [R, P, B].
    Plain loops over the steps, the rows of a window and the factors; the samples of a row are taken together (every
    sample's sum is its own: the rows of the window added in ascending order), and a sum over retained rows adds them one
    by one in ascending sample order.  With `err` ([R, N]) the sums are taken from there instead
    of being formed: stage two on a given stage one."""
    sim, obs = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    cat = np.asarray(cat)
    R, N = sim.shape
    P = len(cat)
    count, ks, kept = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int32)
    E, cut = np.full((R, N), np.nan), np.full(R, np.nan)
    shares, rows = np.full((R, P, n_bins), np.nan), [[] for _ in range(R)]

    def in_order(values):
        return float(np.cumsum(values)[-1]) if len(values) else 0.0

    for r in range(R):
        V = window(r, R, h, obs)
        count[r] = len(V)
        if len(V) < min_valid:
            continue
        if err is not None:
            E[r] = err[r]
        else:
            total = np.zeros(N)
            for s in V:
                total = total + np.abs(sim[s] - obs[s])
            E[r] = total
        eligible = np.flatnonzero(np.isfinite(E[r]))
        M = len(eligible)
        if M == 0:
            continue
        k = max(1, int(math.ceil(fraction * float(M))))
        ks[r] = k
        c = float(np.sort(E[r, eligible])[k - 1])
        cut[r] = c
        keep = eligible[E[r, eligible] <= c]
        rows[r] = keep.tolist()
        kept[r] = len(keep)
        s = np.ones(len(keep)) if support == EQUAL else c - E[r, keep]
        S = in_order(s)
        if S == 0.0:
            s = np.ones(len(keep))
            S = float(len(keep))
        for p in range(P):
            acc = np.zeros(256)
            np.add.at(acc, cat[p, keep], s)         # unbuffered: every bin adds its rows one by one, in ascending order
            shares[r, p] = acc[:n_bins] / S
    return dict(count=count, E=E, k=ks, cut=cut, retained=kept, rows=rows, shares=shares)


def exact_sums(sim, obs, h, min_valid=1):
    """E[r][n] in exact arithmetic -> R lists of N Fractions; None where the sum is not finite or the step not assessed"""
    sim, obs = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    R, N = sim.shape
    out = []
    for r in range(R):
        V = window(r, R, h, obs)
        row = []
        for n in range(N):
            if len(V) < min_valid or not all(math.isfinite(sim[s, n]) for s in V):
                row.append(None)
            else:
                # |sim - obs| is ONE rounded subtraction in the definition; the sum of those doubles is what is exact here
                row.append(sum((Fraction(abs(float(sim[s, n]) - float(obs[s]))) for s in V), Fraction(0)))
        out.append(row)
    return out


def exact_shares(E_row, cat, n_bins, fraction, support):
    """Steps 4 .. 7 on one step's doubles E_row with exact sums and an exact quotient (s_n = cut - E is one rounded
    subtraction, as defined) -> (cut, the retained rows, [P][B] Fractions), or None where no row is eligible"""
    eligible = [n for n in range(len(E_row)) if math.isfinite(E_row[n])]
    if not eligible:
        return None
    k = max(1, int(math.ceil(fraction * float(len(eligible)))))
    c = sorted(float(E_row[n]) for n in eligible)[k - 1]
    rows = [n for n in eligible if E_row[n] <= c]
    s = {n: Fraction(1) if support == EQUAL else Fraction(c - float(E_row[n])) for n in rows}
    S = sum(s.values(), Fraction(0))
    if S == 0:
        s, S = {n: Fraction(1) for n in rows}, Fraction(len(rows))
    return c, rows, [[sum((s[n] for n in rows if cat[p][n] == b), Fraction(0)) / S for b in range(n_bins)]
                     for p in range(len(cat))]
