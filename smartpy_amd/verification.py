"""Ensemble verification, host side: what is said about a whole run from the per-step scores engine.ensemble_scores
leaves ([5, R]: CRPS, SPREAD, PIT_LOW, PIT_HIGH, MEAN) and the observations.  numpy only, nothing hot: R numbers per
column.  The VALID steps are those with a finite CRPS (an observation, a total weight above zero, finite members).

    mean_crps, mean_spread   over the valid steps
    crps_climatology         the CRPS, at every valid step, of the forecast "all finite observations, equal weights"
    skill                    1 - mean_crps / mean(crps_climatology)
    pit_histogram            non-randomised (Czado, Gneiting & Held 2009): a step spreads a mass of 1 uniformly over
                             [PIT_LOW, PIT_HIGH], or puts it on the point where the two are equal
    reliability              alpha of Renard et al. 2010: 1 - (2 / n) sum |p_(i) - i / (n + 1)| over the sorted midpoints
                             of the two PITs
"""
import numpy as np

CRPS, SPREAD, PIT_LOW, PIT_HIGH, MEAN = range(5)


def crps_climatology(obs, at=None):
    """The CRPS of the climatological forecast -- the finite observations as an ensemble of equal weights -- against
    `at` (default: those observations themselves): the integral of (F - 1[x >= y])^2 as in the kernel, a sum of
    non-negative terms, from the sorted observations, prefix sums of the gap terms and one searchsorted.  -> array like
    `at`, NaN where `at` is not finite or there is no finite observation."""
    obs = np.asarray(obs, dtype=np.float64).reshape(-1)
    c = np.sort(obs[np.isfinite(obs)])
    y = c if at is None else np.asarray(at, dtype=np.float64)
    out = np.full(y.shape, np.nan)
    K = c.size
    ok = np.isfinite(y)
    if K == 0 or not ok.any():
        return out
    gap = np.diff(c)                                    # gap i lies between c[i] and c[i + 1]
    P = np.arange(1, K) / K
    Q = np.arange(K - 1, 0, -1) / K
    below = np.concatenate(([0.0], np.cumsum(gap * P * P)))             # below[k] = sum over gaps i < k
    above = np.concatenate((np.cumsum((gap * Q * Q)[::-1])[::-1], [0.0]))   # above[k] = sum over gaps i >= k
    v = y[ok]
    j = np.searchsorted(c, v, side='right')             # the number of observations <= v
    res = np.empty(v.shape)
    low, high = j == 0, j == K
    mid = ~(low | high)
    res[low] = (c[0] - v[low]) + above[0]
    res[high] = (v[high] - c[-1]) + below[K - 1]
    g = j[mid] - 1                                      # v lies in gap g
    res[mid] = below[g] + (v[mid] - c[g]) * P[g] ** 2 + (c[g + 1] - v[mid]) * Q[g] ** 2 + above[g + 1]
    out[ok] = res
    return out


def pit_histogram(pit_low, pit_high, bins=10):
    """The non-randomised PIT histogram over `bins` equal bins of [0, 1] -> float64 [bins]; the counts sum to the
    number of steps whose two PITs are finite.  p = 1 belongs to the last bin."""
    lo, hi = np.asarray(pit_low, dtype=np.float64), np.asarray(pit_high, dtype=np.float64)
    ok = np.isfinite(lo) & np.isfinite(hi)
    lo, hi = lo[ok], hi[ok]
    bins = int(bins)
    counts = np.zeros(bins)
    point = hi <= lo
    at = np.minimum((lo[point] * bins).astype(np.int64), bins - 1)
    np.add.at(counts, at, 1.0)
    lo, hi = lo[~point], hi[~point]
    edges = np.arange(bins + 1) / bins
    overlap = np.minimum(hi[:, None], edges[None, 1:]) - np.maximum(lo[:, None], edges[None, :-1])
    share = np.clip(overlap, 0.0, None)
    total = share.sum(axis=1, keepdims=True)            # = hi - lo up to rounding: every step weighs exactly 1
    counts += (share / total).sum(axis=0)
    return counts


def reliability(pit_low, pit_high):
    """alpha = 1 - (2 / n) sum |p_(i) - i / (n + 1)|, p the sorted midpoints of the two PITs; NaN without a step."""
    lo, hi = np.asarray(pit_low, dtype=np.float64), np.asarray(pit_high, dtype=np.float64)
    ok = np.isfinite(lo) & np.isfinite(hi)
    p = np.sort(0.5 * (lo[ok] + hi[ok]))
    n = p.size
    if n == 0:
        return float('nan')
    return float(1.0 - 2.0 / n * np.abs(p - np.arange(1, n + 1) / (n + 1.0)).sum())


class EnsembleVerification(object):
    """What GLUE.ensemble_verification returns.  Per report step, numpy [R] float64: `crps`, `spread`, `pit_low`,
    `pit_high`, `mean`; `datetime` (the R report stamps); over the valid steps (finite CRPS, `n_valid` of them):
    `mean_crps`, `mean_spread`, `crps_climatology` ([R], NaN where the step is not valid), `skill`, `pit_histogram`
    ([bins]), `reliability`; `file` (the path written, or None)."""

    def __init__(self, scores, obs, stamps=None, bins=10, file=None):
        scores = np.asarray(scores, dtype=np.float64)
        self.crps, self.spread, self.pit_low, self.pit_high, self.mean = (scores[c] for c in range(5))
        self.datetime, self.file = stamps, file
        valid = np.isfinite(self.crps)
        self.n_valid = int(valid.sum())
        self.crps_climatology = np.full(self.crps.shape, np.nan)
        nan = float('nan')
        self.mean_crps = self.mean_spread = self.skill = nan
        if self.n_valid and obs is not None:
            obs = np.asarray(obs, dtype=np.float64)
            self.crps_climatology[valid] = crps_climatology(obs, obs[valid])
            self.mean_crps = float(self.crps[valid].mean())
            self.mean_spread = float(self.spread[valid].mean())
            self.skill = float(1.0 - self.mean_crps / self.crps_climatology[valid].mean())
        self.pit_histogram = pit_histogram(self.pit_low[valid], self.pit_high[valid], bins)
        self.reliability = reliability(self.pit_low[valid], self.pit_high[valid])
