"""The seven scores NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE in exact arithmetic, and what the one-pass moments of the
kernels may differ from them by.  TEST INFRASTRUCTURE ONLY.

Every path to the scores ends in finish_objectives (smart_device.h) on the moments A = sum(s - e), B = sum((s - e)^2),
C1 = sum(s - c), C2 = sum((s - c)^2), C3 = sum((e - a)(s - c)) over the rows that carry an observation, c a constant per
sample and a the observation reference (their mean, or the launch's g in the bootstrap).  var_s = C2 / n - (C1 / n)^2
loses digits as kappa = 1 + ((c - mean s) / std s)^2 grows: c among the summed values keeps kappa <= about n, a value
from outside them (a report before the first observation) does not.

`truth`    the scores in fractions.Fraction, rounded once; square roots in float on correctly rounded rationals.
`bounds`   per column and score what ANY order of the kernel's additions may differ from `truth` by (derived there).
`emulate`  the five sums in float64, in one of three orders, finished as finish_objectives finishes them.
`window_reference`, `bootstrap_reference`: truth and bounds of the windowed entry and of the bootstrap's replicates."""
import math
from fractions import Fraction

import numpy as np

from oracle import objfn_oracle
from oracle.exact import U, SLACK, gamma, mul, div, sqrt

LOG_EPS = 0.05
# ln as two libraries evaluate it (each within 1 ulp of the true value, and 1 ulp <= 2 u of the value): the kernel's
# ln(x + eps) against the one `truth` is given lies within 4 u of itself (x + eps is one IEEE addition on both sides)
LOG_REL = 4 * U
# sqrt, x + eps and 1 / y are one correctly rounded IEEE operation each, on the device as in numpy (the analysis units are
# built without fast-math): the kernel's transformed values ARE the ones `truth` is given.  ln alone is a library's.
INPUT_REL = {'none': 0.0, 'sqrt': 0.0, 'log': LOG_REL, 'inverse': 0.0}


def observed_rows(obs, rows=None):
    """The row indices the scores are taken over: `rows` (None: all; a boolean mask; or indices, repeats allowed -- a
    bootstrap replicate is a multiset) without those whose observation is missing."""
    obs = np.asarray(obs, dtype=np.float64)
    if rows is None:
        idx = np.arange(obs.size)
    else:
        rows = np.asarray(rows)
        idx = np.flatnonzero(rows) if rows.dtype == bool else rows.astype(np.int64)
    return idx[~np.isnan(obs[idx])]


def first_observed(obs, rows=None):
    return int(np.min(observed_rows(obs, rows)))


def _quot(num, den):
    """num / den of two rationals as IEEE division has it: x / 0 = +-inf, 0 / 0 = NaN; else the correctly rounded float."""
    if den == 0:
        return math.nan if num == 0 else math.copysign(math.inf, num)
    return float(num / den)


def _exact(s, e):
    """Centred sums of one column over its rows, as Fractions: n, Se, Ss, sum (s - e)^2, see = sum (e - mean e)^2,
    sss = sum (s - mean s)^2, sse = sum (e - mean e)(s - mean s)."""
    # every float is an integer over a power of two: the sums are taken on integers over ONE such power (no gcd per term)
    pairs = [float(x).as_integer_ratio() for x in list(s) + list(e)]
    shift = max(den.bit_length() for _, den in pairs) - 1
    ints = [num << (shift - den.bit_length() + 1) for num, den in pairs]
    n = len(s)
    fs, fe = ints[:n], ints[n:]
    one, two = 1 << shift, 1 << (2 * shift)
    Se, Ss = Fraction(sum(fe), one), Fraction(sum(fs), one)
    B = Fraction(sum((a - b) * (a - b) for a, b in zip(fs, fe)), two)
    see = Fraction(sum(b * b for b in fe), two) - Se * Se / n
    sss = Fraction(sum(a * a for a in fs), two) - Ss * Ss / n
    sse = Fraction(sum(a * b for a, b in zip(fs, fe)), two) - Ss * Se / n
    return n, Se, Ss, B, see, sss, sse


def _scores(n, Se, Ss, B, see, sss, sse):
    nse = 1.0 - _quot(B, see)
    if sss == 0 or see == 0:
        cc = math.nan                                                   # 0 / 0 in np.corrcoef and in the kernels alike
    else:
        cc = math.copysign(math.sqrt(float(sse * sse / (sss * see))), sse)
    a2 = _quot(sss, see)
    alpha = math.sqrt(a2) if a2 >= 0.0 else math.nan
    beta = _quot(Ss, Se)
    if math.isnan(cc) or math.isnan(alpha) or math.isinf(alpha) or not math.isfinite(beta):
        kge = 1.0 - math.sqrt(sum((x - 1.0) ** 2 for x in (cc, alpha, beta)))        # the pattern, by IEEE arithmetic
    else:
        q = sum(((Fraction(x) - 1) ** 2 for x in (cc, alpha)), Fraction(0)) + (Ss / Se - 1) ** 2
        kge = 1.0 - math.sqrt(float(q))
    pbias = _quot(100 * (Ss - Se), Se)
    rmse = math.sqrt(float(B / n))
    return [nse, kge, cc, alpha, beta, pbias, rmse]


def truth(sim, obs, rows=None):
    """sim [R, n], obs [R] (NaN = missing) -> [n, 7] float64: the scores of every column over the observed rows in
    fractions.Fraction, each rounded once at the end (KGEc, KGEa, RMSE and the distance inside KGE are square roots, taken
    in float on the correctly rounded rational under them).  No observed row: NaN.  A column with a value among its
    observed rows that is not finite has no rational statement: it gets what oracle.objfn_oracle gives, which is where its
    pattern of NaN and infinities is defined; zero denominators (constant observations, a constant column, one row)
    follow IEEE division, as they do there."""
    sim, obs = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    idx = observed_rows(obs, rows)
    out = np.full((sim.shape[1], 7), np.nan)
    if idx.size == 0:
        return out
    e = obs[idx]
    for j in range(sim.shape[1]):
        s = sim[idx, j]
        if np.isfinite(s).all() and np.isfinite(e).all():
            out[j] = _scores(*_exact(s, e))
        else:
            with np.errstate(all='ignore'):
                out[j] = objfn_oracle.objective_functions(s, e)[:7]
    return out


def bounds(sim, obs, shift_row, rows=None, obs_ref=None, input_rel=0.0):
    """-> [n, 7]: what a float64 computation of the kernels' form, with its additions in ANY order, may differ from
    `truth(sim, obs, rows)` by, when the moments are taken about c = sim[shift_row] (per column).  u = 2^-53,
    gamma(k) = k u / (1 - k u), m the number of observed rows.

    The sums.  A sum of m terms added in any order (any binary tree) is off by at most gamma(m - 1) sum|term|; a term
    that is a rounded difference adds u, a rounded product of two such 3 u in all (a fused multiply-add drops a rounding,
    never adds one):
        dA = gamma(m) sum|s - e|      dB = gamma(m + 2) sum (s - e)^2      dSe = gamma(m - 1) sum|e|
        dC1 = gamma(m) sum|s - c|     dC2 = gamma(m + 2) sum (s - c)^2     dC3 = gamma(m + 2) sum|(e - a)(s - c)|
        dQ = gamma(m) sum|e - a|      dP = gamma(m + 2) sum (e - a)^2
    kappa enters through sum (s - c)^2 = n var_s kappa, and through sum|s - c| and sum|(e - a)(s - c)| likewise.
    The observation side.  Without obs_ref, a is the kernel's own mean of the observations, off the exact mean by at most
    da = gamma(m - 1) sum|e| / m + u |mean|; see is taken as P, which is the exact see + m (a - mean)^2: dsee = dP + m da^2.
    With obs_ref = (g, dg) (the bootstrap: g the launch's reference, known to dg), see = P - Q^2 / m is formed:
    dsee = dP + (2 |Q| dQ + dQ^2) / m + 3 u Q^2 / m + u see, with |Q| <= |sum (e - g)| + m dg.
    The quotients, every "/ n" a multiplication by the rounded 1 / n (2 u):
        m1 = C1 / n              dm1 = dC1 / n + 2 u |m1|
        var_s = C2 / n - m1^2    dvar_s = dC2 / n + 2 u C2 / n + 2 |m1| dm1 + dm1^2 + u m1^2 + u var_s
        n cov = C3 - Q m1        (an identity for ANY a)    d = dC3 + |Q| dm1 + |m1| dQ + u |Q m1| + u |n cov|
        cov                      dcov = d / n + 2 u |cov|
    and then through finish_objectives with relative errors composed exactly ((1 + x)(1 + y) - 1, (x + y) / (1 - y),
    1 - sqrt(1 - x)) and one u for every rounded operation:
        KGEc = cov / D, D = sqrt(var_s var_e):  (dcov + |KGEc| dD) / (D - dD) + u |KGEc|   (clipping to [-1, 1] only nears)
        KGEa = sqrt(var_s / var_e);  x = A / Se: dx = (dA + |x| dSe) / (|Se| - dSe) + u |x|;  KGEb = 1 + x;  PBias = 100 x
        NSE = 1 - B / see;  RMSE = sqrt(B / n)
        KGE = 1 - sqrt q, q = sum (t - 1)^2 over t = KGEc, KGEa, KGEb: with dt' = dt + u |t - 1|,
              dq = sum (2 |t - 1| dt' + dt'^2) + 4 u q,   d sqrt q = min(sqrt dq, dq / sqrt q) + u sqrt q.
    input_rel = tau: every s and e the kernel sums may differ from the one `truth` sees by tau times itself (a transform
    evaluated by two libraries); to first order that moves A by tau sum(|s| + |e|), B by 2 tau sum|s - e|(|s| + |e|), Se by
    tau sum|e|, see by 2 tau sum|e - mean||e|, n var_s by 2 tau sum|s - mean s||s| and n cov by
    tau sum(|e - mean||s| + |s - mean s||e|), which are added to the above.
    Last, 4 ulp of the value itself (truth's own rounding, the final subtraction), and everything times 1 + 2^-20: the
    magnitudes above are float64 sums of non-negative terms, right to m 2^-53 of themselves.  No constant is fitted."""
    sim, obs = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    idx = observed_rows(obs, rows)
    n_cols = sim.shape[1]
    out = np.full((n_cols, 7), np.inf)
    m = idx.size
    if m < 2:
        return out
    e = obs[idx][:, None]
    s = sim[idx]
    c = sim[shift_row][None, :]
    want = truth(sim, obs, rows)
    with np.errstate(all='ignore'):
        n = float(m)
        mean_e, mean_s = np.mean(e), np.mean(s, axis=0)
        if obs_ref is None:
            a, da = mean_e, gamma(m - 1) * np.sum(np.abs(e)) / n + U * abs(mean_e)
        else:
            a, da = obs_ref
        d, us, w = s - e, s - c, e - a
        tau = input_rel
        mag = np.abs(s) + np.abs(e)
        Se = np.sum(e)
        dSe = gamma(m - 1) * np.sum(np.abs(e)) + tau * np.sum(np.abs(e))
        A, B = np.sum(d, axis=0), np.sum(d * d, axis=0)
        dA = gamma(m) * np.sum(np.abs(d), axis=0) + tau * np.sum(mag, axis=0)
        dB = gamma(m + 2) * B + 2 * tau * np.sum(np.abs(d) * mag, axis=0)
        C1, C2 = np.sum(us, axis=0), np.sum(us * us, axis=0)
        dC1, dC2 = gamma(m) * np.sum(np.abs(us), axis=0), gamma(m + 2) * C2
        dC3 = gamma(m + 2) * np.sum(np.abs(w * us), axis=0)
        P, Q, dQ = np.sum(w * w), abs(np.sum(w)) + n * da, gamma(m) * np.sum(np.abs(w))
        see = np.sum((e - mean_e) ** 2)
        dsee = gamma(m + 2) * P + 2 * tau * np.sum(np.abs(e - mean_e) * np.abs(e))
        dsee += n * da * da if obs_ref is None else (2 * Q * dQ + dQ * dQ) / n + 3 * U * Q * Q / n + U * see
        var_e, r_e = see / n, mul(dsee / see, 2 * U)
        m1 = C1 / n
        dm1 = dC1 / n + 2 * U * np.abs(m1)
        var_s = np.sum((s - mean_s) ** 2, axis=0) / n
        dvar_s = (dC2 / n + 2 * U * C2 / n + 2 * np.abs(m1) * dm1 + dm1 * dm1 + U * m1 * m1 + U * var_s
                  + 2 * tau * np.sum(np.abs(s - mean_s) * np.abs(s), axis=0) / n)
        r_s = dvar_s / var_s
        ncov = np.sum((e - mean_e) * (s - mean_s), axis=0)
        dncov = (dC3 + Q * dm1 + np.abs(m1) * dQ + U * Q * np.abs(m1) + U * np.abs(ncov)
                 + tau * np.sum(np.abs(e - mean_e) * np.abs(s) + np.abs(s - mean_s) * np.abs(e), axis=0))
        cov, dcov = ncov / n, dncov / n + 2 * U * np.abs(ncov / n)
        D = np.sqrt(var_s * var_e)
        r_D = mul(sqrt(mul(mul(r_s, r_e), U)), U)
        cc, alpha, beta = want[:, 2], want[:, 3], want[:, 4]
        b_cc = np.where(r_D < 1.0, (dcov + np.abs(cc) * D * r_D) / (D * (1.0 - r_D)), np.inf) + U * np.abs(cc)
        b_alpha = alpha * mul(sqrt(mul(div(r_s, r_e), U)), U)
        x = A / Se
        dx = np.where(dSe < abs(Se), (dA + np.abs(x) * dSe) / (abs(Se) - dSe), np.inf) + U * np.abs(x)
        b_beta, b_pbias = dx + U * np.abs(beta), 100.0 * dx + U * np.abs(want[:, 5])
        y = B / see
        b_nse = np.where(dsee < see, (dB + y * dsee) / (see - dsee), np.inf) + U * y + U * np.abs(want[:, 0])
        q, dq = 0.0, 0.0
        for t, dt in ((cc, b_cc), (alpha, b_alpha), (beta, b_beta)):
            dt = dt + U * np.abs(t - 1.0)
            q, dq = q + (t - 1.0) ** 2, dq + 2 * np.abs(t - 1.0) * dt + dt * dt
        dq = dq + 4 * U * q
        root = np.sqrt(q)
        b_kge = np.minimum(np.sqrt(dq), np.where(root > 0.0, dq / root, np.inf)) + U * root + U * np.abs(want[:, 1])
        b_rmse = np.where(B > 0.0, want[:, 6] * mul(sqrt(mul(dB / np.where(B > 0.0, B, 1.0), 2 * U)), U), np.sqrt(dB / n))
        raw = np.stack([b_nse, b_kge, b_cc, b_alpha, b_beta, b_pbias, b_rmse], axis=1)
        out = (raw + 4 * U * np.abs(want)) * SLACK
    out[~np.isfinite(out)] = np.inf
    return out


def kappa(sim, obs, shift_row, rows=None):
    """[n]: 1 + ((c - mean s) / std s)^2 of every column over the observed rows, c = sim[shift_row]."""
    s = np.asarray(sim, dtype=np.float64)[observed_rows(obs, rows)]
    with np.errstate(all='ignore'):
        return 1.0 + (np.asarray(sim, dtype=np.float64)[shift_row] - s.mean(axis=0)) ** 2 / s.var(axis=0)


# ---- the sums as a kernel forms them ---------------------------------------------------------------------------------
ORDERS = ('forward', 'reversed', 'strided')


def emulate(sim, obs, shift_row, order='forward', rows=None):
    """-> [n, 7]: the five sums about c = sim[shift_row] in float64, one addition at a time -- 'forward' as one lane walks
    its rows, 'reversed', or 'strided': eight partial sums take the rows round-robin and are added in order (the eight
    wavefronts of smart_objfn_matrix<1, 8, 4>) -- the observation statistics the same way, and the end as
    finish_objectives has it."""
    sim, obs = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    idx = observed_rows(obs, rows)
    if order == 'reversed':
        idx = idx[::-1]
    lanes = 8 if order == 'strided' else 1
    n_cols = sim.shape[1]
    c = sim[shift_row]
    with np.errstate(all='ignore'):
        cnt, se = np.zeros(lanes), np.zeros(lanes)
        for k, r in enumerate(idx):
            cnt[k % lanes] += 1.0
            se[k % lanes] += obs[r]
        n, se = _in_order(cnt), _in_order(se)
        ebar = se / n
        see, sd = np.zeros(lanes), np.zeros(lanes)
        mom = np.zeros((lanes, 5, n_cols))
        for k, r in enumerate(idx):
            w = obs[r] - ebar
            see[k % lanes] += w * w
            sd[k % lanes] += w
            d, u = sim[r] - obs[r], sim[r] - c
            acc = mom[k % lanes]
            acc[0] += d
            acc[1] += d * d
            acc[2] += u
            acc[3] += u * u
            acc[4] += w * u
        see, sd = _in_order(see), _in_order(sd)
        A, B, C1, C2, C3 = _in_order(mom)
        inv_n = 1.0 / n
        m1 = C1 * inv_n
        var_s, var_e = C2 * inv_n - m1 * m1, see * inv_n
        cov = (C3 - sd * m1) * inv_n
        cc = cov / np.sqrt(var_s * var_e)
        cc = np.where(np.isnan(cc), cc, np.minimum(np.maximum(cc, -1.0), 1.0))
        alpha = np.sqrt(var_s / var_e)
        beta = 1.0 + A / se
        kge = 1.0 - np.sqrt((cc - 1.0) * (cc - 1.0) + (alpha - 1.0) * (alpha - 1.0) + (beta - 1.0) * (beta - 1.0))
        return np.stack([1.0 - B / see, kge, cc, alpha, beta, 100.0 * (A / se), np.sqrt(B * inv_n)], axis=1)


def _in_order(parts):
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total


def transformed_pair(sim, obs, transform):
    with np.errstate(all='ignore'):
        if transform == 'none':
            return sim, obs
        if transform == 'sqrt':
            return np.sqrt(sim), np.sqrt(obs)
        if transform == 'inverse':
            return 1.0 / (sim + LOG_EPS), 1.0 / (obs + LOG_EPS)
        assert transform == 'log', 'transform %r unknown' % (transform,)
        return np.log(sim + LOG_EPS), np.log(obs + LOG_EPS)


def window_reference(sim, obs, win, W, transform='none', rule=True):
    """-> (want, bound) [W, n, 7] of smart_objfn_windows_hip: per window truth over its observed rows on the transformed
    values, with the entry's two rules (fewer than two rows, a transformed value that is not finite: NaN in all seven),
    and the bound about the window's own first observed row."""
    fs, fe = transformed_pair(sim, obs, transform)
    n = sim.shape[1]
    want, bnd = np.full((W, n, 7), np.nan), np.full((W, n, 7), np.inf)
    for w in range(W):
        idx = observed_rows(fe, win == w)
        if idx.size < 2 or not np.isfinite(fe[idx]).all():
            continue
        want[w] = truth(fs, fe, idx)
        want[w][~np.isfinite(fs[idx]).all(axis=0)] = np.nan
        bnd[w] = bounds(fs, fe, int(idx.min()), idx, input_rel=INPUT_REL[transform])
    return want, bnd


def bootstrap_reference(sim, obs, win, counts):
    """-> (want, bound) [B, n, 7] of the replicates of smart_objfn_bootstrap_hip: replicate b is the multiset of the
    observed rows of window w taken counts[b, w] times; every moment is about the value at the launch's first valid row
    (whether the replicate holds that row or not) and about g, the mean of all valid observations, which the kernel and
    this function know to twice the error of a sum of that length."""
    valid = observed_rows(obs, (win >= 0) & (win < counts.shape[1]))
    r0 = int(valid.min())
    g = float(np.mean(obs[valid]))
    dg = 2 * (gamma(valid.size - 1) * float(np.sum(np.abs(obs[valid]))) / valid.size + U * abs(g))
    want, bnd = [], []
    for row in np.asarray(counts, dtype=np.int64):
        idx = np.concatenate([np.repeat(observed_rows(obs, win == w), row[w]) for w in range(row.size)])
        want.append(truth(sim, obs, idx))
        bnd.append(bounds(sim, obs, r0, idx, obs_ref=(g, dg)))
    return np.array(want), np.array(bnd), r0
