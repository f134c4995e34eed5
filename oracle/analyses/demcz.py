"""DE-MCz posterior sampling: the numpy statement of include/smart_amd.h (smart_demcz_step_hip), which the kernels are
held to BIT FOR BIT.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

from oracle.analyses.de_move import crossover, launch_rows, move, mulhi
from oracle.philox import philox4x32, u53

LOGP, RMSE, RMSE_SIGMA = 0, 1, 2


# ---- the statement ----------------------------------------------------------------------------------------------------
class Chains(object):
    """The state of the statement, in numpy: what demcz.DemczState keeps on the device."""

    def __init__(self, x, lo, hi, capacity, seed=0, cr=0.9, p_jump=0.1, b_star=1e-6, n_carry=0, columns=None, ld=None,
                 fill=np.nan, score_kind=LOGP, n_obs=0, n_eff=0.0, sigma=0.0):
        self.x = np.array(x, dtype=np.float64)
        N, d = self.x.shape
        self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        self.scale = float(b_star) * (self.hi - self.lo)
        self.gamma = 2.38 / np.sqrt(2.0 * np.arange(1, d + 1, dtype=np.float64))
        self.J, self.C = int(math.floor(float(p_jump) * 2.0 ** 32)), int(math.floor(float(cr) * 2.0 ** 32))
        self.key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        self.columns = np.arange(d) if columns is None else np.asarray(columns)
        self.score_kind, self.n_obs, self.n_eff, self.sigma = score_kind, n_obs, n_eff, sigma
        self.logp = np.full(N, -np.inf)
        self.carry = np.zeros((N, n_carry))
        self.accepted = np.zeros(N, dtype=np.int32)
        self.proposal = self.x.copy()
        self.out = np.zeros(N, dtype=np.uint8)
        self.archive = np.zeros((capacity, d))
        self.archive_logp = np.zeros(capacity)
        self.archive_carry = np.zeros((capacity, n_carry))
        self.rows = np.full((N, d if ld is None else ld), fill)
        self.rows[:, self.columns] = self.x
        self.M, self.g = 0, 1
        self.fallbacks = self.jumps = 0         # how often the fallback dimension was taken, gamma = 1 was drawn


def log_density(score, kind, n_obs, n_eff, sigma):
    score = np.asarray(score, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        if kind == RMSE:
            return -((n_eff * 0.5) * np.log(np.float64(n_obs) * (score * score)))
        if kind == RMSE_SIGMA:
            return -(n_eff * (score * score)) / ((2.0 * sigma) * sigma)
    return score.copy()


class Decisions(object):
    """What the accept phase of the statement decided: take [n] bool, log_u, delta (l* - l) and margin = |log u - delta|
    per chain (NaN where nothing was compared: an `out` proposal, a NaN l*, the initial population); `smallest` is the
    smallest margin among the finite comparisons, relative to max(1, |delta|, |log u|) (inf where there was none)."""

    def __init__(self, take, log_u, delta, compared):
        self.take, self.log_u, self.delta = take, log_u, delta
        with np.errstate(invalid='ignore'):
            self.margin = np.where(compared, np.abs(log_u - delta), np.nan)
            finite = compared & np.isfinite(log_u) & np.isfinite(delta)
            rel = self.margin / np.maximum(1.0, np.maximum(np.abs(delta), np.abs(log_u)))
        self.finite = finite
        self.smallest = float(rel[finite].min()) if finite.any() else np.inf
        self.absolute = float(self.margin[finite].min()) if finite.any() else np.inf


def demcz_statement(s, scores=None, carry_new=None, propose=True, append=False, chains=None):
    """One call of smart_demcz_step_hip, as include/smart_amd.h words it, on a Chains object -> Decisions of the accept
    phase (None without one).  chains=(first, count): that part of the chains only; s.M and s.g are then left alone."""
    N, d = s.x.shape
    first, count = (0, N) if chains is None else chains
    sl = slice(first, first + count)
    c = np.arange(first, first + count, dtype=np.uint64)
    decisions = None
    M = s.M
    if scores is not None:
        lstar = log_density(np.asarray(scores, dtype=np.float64)[sl], s.score_kind, s.n_obs, s.n_eff, s.sigma)
        if s.g - 1 == 0:
            take = np.ones(count, dtype=bool)
            decisions = Decisions(take, np.full(count, np.nan), np.full(count, np.nan), np.zeros(count, dtype=bool))
        else:
            w = philox4x32((c, s.g - 1, 1, 0), s.key)
            with np.errstate(divide='ignore', invalid='ignore'):
                log_u = np.log(u53(w[0], w[1]))
                delta = lstar - s.logp[sl]
                compared = (s.out[sl] == 0) & ~np.isnan(lstar)
                take = compared & (log_u < delta)
            decisions = Decisions(take, log_u, delta, compared)
            s.x[sl][take] = s.proposal[sl][take]
            s.accepted[sl][take] += 1
        s.logp[sl][take] = lstar[take]
        if s.carry.shape[1]:
            s.carry[sl][take] = np.asarray(carry_new)[sl][take]
        if append:
            assert M + first + count <= len(s.archive), 'the archive of %d rows is full' % len(s.archive)
            at = slice(M + first, M + first + count)
            s.archive[at], s.archive_logp[at], s.archive_carry[at] = s.x[sl], s.logp[sl], s.carry[sl]
            M = M + first + count
    if propose:
        assert M >= 2, 'a proposal draws two archive rows, the archive holds %d' % M
        r = philox4x32((c, s.g, 0, 0), s.key)
        a = mulhi(r[0], M)
        b = mulhi(r[1], M - 1)
        b = b + (b >= a).astype(np.uint64)
        jump = r[2] < np.uint64(s.J)
        W, moved, fallbacks = crossover(c, s.g, s.key, d, s.C, mulhi(r[3], d).astype(np.int64))
        s.fallbacks += fallbacks
        s.jumps += int(jump.sum())
        gamma = np.where(jump, 1.0, s.gamma[moved.sum(axis=1) - 1])
        x = s.x[sl]
        s.proposal[sl], out = move(W, moved, s.scale, s.lo, s.hi, x, s.archive[a.astype(np.int64)],
                                   s.archive[b.astype(np.int64)], gamma[:, None])
        s.out[sl] = out
        s.rows[sl, s.columns] = launch_rows(out, x, s.proposal[sl])
    if chains is None:
        s.M = M
        s.g += 1 if propose else 0
    return decisions


def run_statement(s, density, generations, thin, keep=None):
    """The loop of montecarlo.DEMCz on a Chains object and a density of the test's -> the smallest relative margin.
    keep: a list that takes a copy of the states after every generation."""
    smallest = np.inf
    demcz_statement(s, scores=density(s.rows[:, s.columns]), append=True, propose=True)
    for g in range(1, generations + 1):
        dec = demcz_statement(s, scores=density(s.rows[:, s.columns]), append=g % thin == 0, propose=g < generations)
        smallest = min(smallest, dec.smallest)
        if keep is not None:
            keep.append(s.x.copy())
    return smallest
