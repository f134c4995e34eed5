"""Residual error model (heteroscedastic AR(1)): the numpy statement of the likelihood kernel, its truth in fifty digits
with the bounds derived for it, and the statement of the error draws.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle.exact import U
from oracle.philox import philox4x32, u53

LN_TWO_PI = 1.8378770664093453
TWO_PI = 6.283185307179586


# ---- the statement of the likelihood -------------------------------------------------------------------------------------
def loglik_statement(sim, obs, theta):
    """smart_error_model_loglik_hip in numpy, every operation rounded once, the sums in the order of the report steps ->
    (LOGLIK, SSQ, LOGSIG), [N] each.  sim [R, N], obs [R], theta [N, 3]."""
    sim, obs = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    R, N = sim.shape
    s0, s1, phi = theta[:, 0], theta[:, 1], theta[:, 2]
    with np.errstate(all='ignore'):
        q = (1.0 - phi) * (1.0 + phi)
        bad = ~(np.isfinite(s0) & np.isfinite(s1) & np.isfinite(phi) & (np.abs(phi) < 1.0))
        ssq, logsig, before = np.zeros(N), np.zeros(N), np.zeros(N)
        n = starts = 0
        for t in range(R):
            if np.isnan(obs[t]):
                continue
            x = sim[t]
            sigma = s0 + s1 * x
            a = (obs[t] - x) / sigma
            if t > 0 and not np.isnan(obs[t - 1]):
                d = a - phi * before
                term = d * d
            else:
                term = q * (a * a)
                starts += 1
            ssq = ssq + term
            logsig = logsig + np.log(sigma)
            bad |= ~(np.isfinite(x) & (sigma > 0.0))
            before = a
            n += 1
        loglik = -0.5 * ssq - logsig
        loglik = loglik + (0.5 * starts) * np.log(q)
        loglik = loglik - (0.5 * n) * LN_TWO_PI
    if n == 0:
        loglik = np.zeros(N)
    return np.where(bad, -np.inf, loglik), np.where(bad, np.nan, ssq), np.where(bad, np.nan, logsig)


class Truth(object):
    """The definition in 50-digit arithmetic for valid columns, cumulative along the report steps: after(R') gives what a
    record cut after its first R' steps has -- LOGLIK, SSQ, LOGSIG as mpmath numbers per column, and the terms of the
    bounds (n, S, sum B_t, sum |ln sigma_t|, |ln(1 - phi^2)|) as floats."""

    def __init__(self, sim, obs, theta, cuts=None):
        import mpmath
        self.mp = mp = mpmath.mp.clone()
        mp.dps = 50
        sim, obs = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64)
        theta = np.asarray(theta, dtype=np.float64)
        R, N = sim.shape
        cuts = sorted(set([R] if cuts is None else cuts))
        self.at = {cut: [] for cut in cuts}
        half, ln2pi = mp.mpf(1) / 2, mp.log(2 * mp.pi)
        seen = ~np.isnan(obs)
        cont = seen & np.concatenate([[False], seen[:-1]])
        # the terms of the bounds, in floats: B_t and |ln sigma_t| summed up to every step
        with np.errstate(all='ignore'):
            sigma_f = theta[:, 0] + theta[:, 1] * sim
            a_f = np.where(seen[:, None], (obs[:, None] - sim) / sigma_f, 0.0)
            b_f = np.where(cont[:, None], theta[:, 2] * np.vstack([np.zeros((1, N)), a_f[:-1]]), 0.0)
            B_sum = np.cumsum(np.where(seen[:, None], (np.abs(a_f) + np.abs(b_f)) ** 2, 0.0), axis=0)
            L_sum = np.cumsum(np.where(seen[:, None], np.abs(np.log(sigma_f)), 0.0), axis=0)
        n_sum, S_sum = np.cumsum(seen), np.cumsum(seen & ~cont)
        for i in range(N):
            s0, s1, phi = (mp.mpf(float(v)) for v in theta[i])
            q = (1 - phi) * (1 + phi)
            lnq = mp.log(q)
            ssq, product = mp.mpf(0), mp.mpf(1)    # (LOGSIG is the logarithm of the product of the sigma_t: one log a cut)
            before = mp.mpf(0)
            for t in range(R):
                if seen[t]:
                    x = mp.mpf(float(sim[t, i]))
                    sigma = s0 + s1 * x
                    a = (mp.mpf(float(obs[t])) - x) / sigma
                    ssq += (a - phi * before) ** 2 if cont[t] else q * a * a
                    product *= sigma
                    before = a
                if t + 1 in self.at:
                    n, S = int(n_sum[t]), int(S_sum[t])
                    logsig = mp.log(product)
                    ll = -half * ssq - logsig + half * S * lnq - half * n * ln2pi if n else mp.mpf(0)
                    self.at[t + 1].append((ll, ssq, logsig, n, S, float(B_sum[t, i]), float(L_sum[t, i]), abs(float(lnq))))

    def after(self, cut):
        return self.at[cut]


def bounds(n, S, B, L, lnq):
    """the bounds of the issue -> (for SSQ and for LOGLIK, for LOGSIG)"""
    return U * ((n + 16) * (0.5 * B + L + 0.5 * S * lnq) + 4 * n), U * ((n + 4) * L + 4 * n)


def shares(got, truth_row, mp):
    """(LOGLIK, SSQ, LOGSIG) of one column against its truth -> the share of each bound that is used (0 where both the
    error and the bound are 0)"""
    ll, ssq, logsig, n, S, B, L, lnq = truth_row
    wide, narrow = bounds(n, S, B, L, lnq)
    out = []
    for value, exact, bound in ((got[0], ll, wide), (got[1], ssq, wide), (got[2], logsig, narrow)):
        err = float(abs(mp.mpf(float(value)) - exact))
        out.append(0.0 if err == 0.0 else (err / bound if bound > 0.0 else np.inf))
    return out


def flood_record(seed, R, N):
    """lognormal flows with a 1e6-fold flood in every column, observations with gaps of every kind: a leading one,
    isolated single observed steps, gaps of one step, a trailing one"""
    rng = np.random.default_rng(seed)
    sim = np.exp(rng.normal(0.0, 1.0, size=(R, N)))
    sim[R // 3] *= 1e6
    obs = sim[:, 0] * np.exp(rng.normal(0.0, 0.3, size=R))
    obs[R // 3] = sim[R // 3, 0] * 0.7
    obs[:3] = np.nan                        # leading
    obs[5:9] = np.nan
    obs[10:12] = np.nan                     # ... steps 9 and 12 stand alone between gaps
    obs[13] = np.nan
    obs[R // 2] = np.nan                    # a gap of one step
    obs[R - 4:] = np.nan                    # trailing
    return rng, sim, obs


# ---- the statement of the draws ------------------------------------------------------------------------------------------
class Draws(object):
    """smart_error_model_draw_hip in numpy: y [R, C], and what the bounds of the device test are carried with -- eps, r
    (of the step's Box-Muller pair) and a, [R, C] each; bad [C]."""

    def __init__(self, sim, theta, replicates=1, seed=0, truncate=True, column_offset=0):
        sim, theta = np.asarray(sim, dtype=np.float64), np.asarray(theta, dtype=np.float64)
        R, N = sim.shape
        K = int(replicates)
        C = N * K
        i = np.arange(C) // K
        s0, s1, phi = theta[i, 0], theta[i, 1], theta[i, 2]
        x = sim[:, i]
        key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        column = np.arange(C, dtype=np.uint64) + np.uint64(column_offset)
        self.eps, self.r = np.empty((R, C)), np.empty((R, C))
        with np.errstate(all='ignore'):
            q = (1.0 - phi) * (1.0 + phi)
            self.sigma = s0 + s1 * x
            self.bad = ~(np.isfinite(s0) & np.isfinite(s1) & np.isfinite(phi) & (np.abs(phi) < 1.0)) | \
                ~(np.isfinite(x) & (self.sigma > 0.0)).all(axis=0)
            for j in range((R + 1) // 2):
                w = philox4x32((column, j, 0, 0), key)
                u1, u2 = 1.0 - u53(w[0], w[1]), u53(w[2], w[3])
                r = np.sqrt(-2.0 * np.log(u1))
                ang = TWO_PI * u2
                self.eps[2 * j], self.r[2 * j] = r * np.cos(ang), r
                if 2 * j + 1 < R:
                    self.eps[2 * j + 1], self.r[2 * j + 1] = r * np.sin(ang), r
            self.a = np.empty((R, C))
            self.a[0] = self.eps[0] / np.sqrt(q)
            for t in range(1, R):
                self.a[t] = phi * self.a[t - 1] + self.eps[t]
            y = x + self.sigma * self.a
            if truncate:
                y = np.where(y > 0.0, y, 0.0)
        self.phi, self.x = phi, x
        self.y = np.where(self.bad[None, :], np.nan, y)
