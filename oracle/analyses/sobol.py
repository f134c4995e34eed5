"""Sobol sensitivity indices: the numpy statement of smart_sobol_indices_hip, sums in math.fsum.  TEST INFRASTRUCTURE ONLY.

`sobol_statement(y, n, k, counts)`: per row mu = fsum(A u B) / 2n, u = y - mu, V = fsum(u^2) / 2n - (fsum(u) / 2n)^2 (the
population variance, in the form that does not depend on the last bit of mu), S1_j = fsum(uB (yAB_j - yA)) / (n V),
ST_j = fsum((yA - yAB_j)^2) / (2n V); a value that is not finite or V == 0 -> NaN; replicates weight every sum by their
counts and keep mu; the standard deviation has ddof = 1."""
import math

import numpy as np

from oracle.exact import U


def sobol_statement(y, n, k, counts=None, bounds=False):
    """y [M, >= n (k + 2)] or [N]; counts [n, B] or None -> dict of S1, ST [M, k], mu, V [M], S1_std, ST_std [M, k] or
    None.  bounds=True adds under 'bound_<name>' what a computation of the same sums in ANY order of additions may differ
    by: (m - 1) 2^-53 sum|c t| for a sum of m terms, the same rule for mu (whose error moves the numerator of S1 by
    |d mu| sum|c d|; V and ST do not depend on it), carried through the quotient as (|d num| + |S| |d den|) / |den|, plus
    4 ulp; for a standard deviation sqrt(2) times the largest replicate bound, plus its own two sums of B terms."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    M, B = y.shape[0], 0 if counts is None else counts.shape[1]
    out = {name: np.full((M, k), np.nan) for name in ('S1', 'ST', 'bound_S1', 'bound_ST')}
    for name in ('mu', 'V', 'bound_mu', 'bound_V'):
        out[name] = np.full(M, np.nan)
    for name in ('S1_std', 'ST_std', 'bound_S1_std', 'bound_ST_std'):
        out[name] = np.full((M, k), np.nan) if B else None
    two_n = 2.0 * n

    def indices(uA, uB, d, ad, c, dmu):
        """-> (V, [k] S1, [k] ST, bound V, [k] bound S1, [k] bound ST) of one weighting c; with sum(c) = n the form of V
        is the same number for mu and for mu + d mu, so an error of mu reaches the numerator of S1 alone"""
        sq, su = c * (uA * uA + uB * uB), c * (uA + uB)
        P, Q = math.fsum(sq), math.fsum(su)
        V = P / two_n - (Q / two_n) ** 2
        dq = (2 * n - 1) * U * math.fsum(np.abs(su)) / two_n            # of Q / 2n; V does not move with mu (docstring)
        dV = (2 * n - 1) * U * P / two_n + 2.0 * abs(Q) / two_n * dq + dq * dq
        S1, ST, b1, bt = (np.full(k, np.nan) for _ in range(4))
        for j in range(k):
            t1, tt = c * uB * d[j], c * d[j] * d[j]
            for S, bnd, num, dnum, den in ((S1, b1, math.fsum(t1), (n - 1) * U * math.fsum(np.abs(t1)) + dmu * math.fsum(c * ad[j]), n * V),
                                           (ST, bt, math.fsum(tt), (n - 1) * U * math.fsum(tt), two_n * V)):
                if V != 0.0:
                    S[j] = num / den
                    bnd[j] = (dnum + abs(S[j]) * (den / V) * dV) / abs(den) + 4 * 2 * U * abs(S[j])
        return V, S1, ST, dV + 8 * U * abs(V), b1, bt

    for r in range(M):
        row = y[r, :n * (k + 2)]
        if not np.isfinite(row).all():
            continue
        yA, yB = row[:n], row[n:2 * n]
        ab = np.concatenate([yA, yB])
        mu = math.fsum(ab) / two_n
        dmu = (2 * n - 1) * U * math.fsum(np.abs(ab)) / two_n + U * abs(mu)
        uA, uB = yA - mu, yB - mu
        d = [row[(2 + j) * n:(3 + j) * n] - yA for j in range(k)]
        ad = [np.abs(x) for x in d]
        one = np.ones(n)
        V, S1, ST, bV, b1, bt = indices(uA, uB, d, ad, one, dmu)
        out['mu'][r], out['V'][r], out['bound_mu'][r], out['bound_V'][r] = mu, V, dmu, bV
        out['S1'][r], out['ST'][r], out['bound_S1'][r], out['bound_ST'][r] = S1, ST, b1, bt
        if not B or V == 0.0:
            continue
        rep = [indices(uA, uB, d, ad, counts[:, b].astype(np.float64), dmu) for b in range(B)]
        for name, col in (('S1', 1), ('ST', 2)):
            x = np.array([q[col] for q in rep])             # [B, k]
            worst = np.max(np.array([q[col + 3] for q in rep]), axis=0)
            for j in range(k):
                if B < 2:
                    continue
                mean = math.fsum(x[:, j]) / B
                std = math.sqrt(math.fsum((x[:, j] - mean) ** 2) / (B - 1))
                spread = math.fsum(np.abs(x[:, j] - x[0, j])) / B
                out[name + '_std'][r, j] = std
                out['bound_' + name + '_std'][r, j] = (math.sqrt(2.0) * worst[j] + math.sqrt(2.0) * (B - 1) * U * spread
                                                      + (B - 1) * U * std + 8 * U * std)
    return out if bounds else {key: v for key, v in out.items() if not key.startswith('bound_')}


def design_values(seed, n, k, R, inert=None):
    """A made-up model on a made-up Saltelli design -> y [R, n (k + 2)]: per row other weights of a quadratic with one
    interaction; the parameter `inert` enters nowhere, so yAB_inert equals yA bit for bit (elementwise arithmetic only)."""
    rng = np.random.default_rng(seed)
    A, Bm = rng.random((n, k)), rng.random((n, k))
    blocks = [A, Bm]
    for j in range(k):
        X = A.copy()
        X[:, j] = Bm[:, j]
        blocks.append(X)
    X = np.concatenate(blocks)
    y = np.empty((R, n * (k + 2)))
    for r in range(R):
        w = rng.normal(1.0, 0.7, k)
        v = np.full(n * (k + 2), 3.0 + 0.1 * r)
        for j in range(k):
            if j != inert:
                v = v + w[j] * X[:, j] + 0.3 * w[j] * X[:, j] ** 2
        if k > 1 and inert not in (0, k - 1):
            v = v + X[:, 0] * X[:, k - 1]
        y[r] = v
    return y


def ishigami(X, a=7.0, b=0.1):
    return np.sin(X[:, 0]) + a * np.sin(X[:, 1]) ** 2 + b * X[:, 2] ** 4 * np.sin(X[:, 0])
