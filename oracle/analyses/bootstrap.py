"""Score uncertainty (block bootstrap and jackknife of the objective functions).  TEST INFRASTRUCTURE ONLY.

`truth` is the yardstick of the host and the GPU tests: direct resampling in np.longdouble.  For every replicate
the valid rows of the windows it draws are taken with their multiplicities (a row drawn c times enters every sum c times:
the sums run over (row, multiplicity) pairs, so that a count of 65,535 costs what a count of 1 costs), two-pass means,
variances and covariance, the seven formulas, rounded to float64 at the end; MEAN and STD (ddof = 1) over the replicates in
longdouble; quantiles np.quantile(method='inverted_cdf') on the float64 replicate values with NaN last.  The transform
itself is applied in float64, as the kernel applies it, before anything is widened.

`pooled` is the kernel's formulation in plain float64 numpy: per-window one-pass moments about the launch-wide constants g
and c_n, a replicate as counts x moments, finish_objectives.  It is held to `truth` at the suite's usual gate -- relative
1e-9 with |want| floored at 1e-12, every compared |want| asserted to be 0 or above 1e-6 (a seed that fails this is changed,
not the gate) -- which tells a wrong formula from a rounding difference before a GPU is involved."""
import numpy as np

from oracle.analyses.windows import transformed

LD = np.longdouble
NAMES = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE']


def _seven(s, e, m):
    """s [rows, n], e [rows], m [rows] multiplicities, all longdouble -> [7, n] longdouble: two-pass moments of the
    multiset, the formulas of montecarlo.py:193-209"""
    with np.errstate(all='ignore'):
        cnt = m.sum()
        mc = m[:, None]
        me, ms = (m * e).sum() / cnt, (mc * s).sum(axis=0) / cnt
        de, ds = e - me, s - ms
        var_e, var_s = (m * de * de).sum() / cnt, (mc * ds * ds).sum(axis=0) / cnt
        cov = (mc * ds * de[:, None]).sum(axis=0) / cnt
        d = s - e[:, None]
        A, B, se = (mc * d).sum(axis=0), (mc * d * d).sum(axis=0), (m * e).sum()
        cc = cov / np.sqrt(var_s * var_e)
        cc = np.where(np.isnan(cc), cc, np.clip(cc, -1.0, 1.0))
        alpha = np.sqrt(var_s / var_e)
        beta = 1.0 + A / se
        kge = 1.0 - np.sqrt((cc - 1.0) ** 2 + (alpha - 1.0) ** 2 + (beta - 1.0) ** 2)
        return np.stack([1.0 - B / (var_e * cnt), kge, cc, alpha, beta, 100.0 * (A / se), np.sqrt(B / cnt)])


def inverted_cdf(reps, probs):
    """reps [B, ...] float64 -> [K, ...]: the max(1, ceil(q B))-th smallest along axis 0, NaN last (np.sort puts it there);
    np.quantile(method='inverted_cdf') wherever the column holds no NaN (asserted by the host tests)"""
    B = reps.shape[0]
    ordered = np.sort(reps, axis=0)
    return np.stack([ordered[max(1, int(np.ceil(q * B))) - 1] for q in probs])


def truth(sim, obs, win, W, counts, transform='none', eps=0.0, probs=(0.05, 0.5, 0.95)):
    """-> (point [n, 7], stats [7, 2 + K, n] or None for B == 0, replicates [B, 7, n]), float64"""
    sim, obs, win = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64), np.asarray(win)
    counts = np.asarray(counts).reshape(-1, W).astype(np.int64)
    R, n = sim.shape
    valid = (win >= 0) & (win < W) & ~np.isnan(obs)
    fe64, fs64 = transformed(transform, np.where(valid, obs, 1.0), eps), transformed(transform, sim, eps)
    fe, fs = fe64.astype(LD), fs64.astype(LD)

    def replicate(c):
        m = np.where(valid, c[np.clip(win, 0, W - 1)], 0)
        rows = m > 0
        out = np.full((7, n), np.nan)
        if m.sum() < 2 or not np.isfinite(fe64[rows]).all():
            return out
        clean = np.isfinite(fs64[rows]).all(axis=0)
        if clean.any():
            out[:, clean] = _seven(fs[rows][:, clean], fe[rows], m[rows].astype(LD)).astype(np.float64)
        return out

    point = replicate(np.ones(W, dtype=np.int64)).T.copy()
    B = counts.shape[0]
    reps = np.full((B, 7, n), np.nan)
    for b in range(B):
        reps[b] = replicate(counts[b])
    if B == 0:
        return point, None, reps
    with np.errstate(all='ignore'):
        wide = reps.astype(LD)
        mean = wide.sum(axis=0) / B
        std = np.sqrt(((wide - mean) ** 2).sum(axis=0) / (B - 1)) if B > 1 else np.full((7, n), np.nan)
    stats = np.concatenate([mean.astype(np.float64)[:, None], np.asarray(std, dtype=np.float64)[:, None],
                            np.transpose(inverted_cdf(reps, probs), (1, 0, 2))], axis=1)
    return point, stats, reps


def pooled(sim, obs, win, W, counts, transform='none', eps=0.0):
    """The kernel's formulation in float64 -> (point [n, 7], replicates [B, 7, n])"""
    sim, obs, win = np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64), np.asarray(win)
    counts = np.asarray(counts).reshape(-1, W).astype(np.int64)
    R, n = sim.shape
    valid = (win >= 0) & (win < W) & ~np.isnan(obs)
    with np.errstate(all='ignore'):
        fe, fs = transformed(transform, np.where(valid, obs, 1.0), eps), transformed(transform, sim, eps)
        fin = valid & np.isfinite(fe)
        g = fe[fin].sum() / fin.sum() if fin.any() else 0.0
        shift = np.zeros(n)
        if valid.any():
            shift = fs[np.flatnonzero(valid)[0]].copy()
            shift[~np.isfinite(shift)] = 0.0
        ow, mom = np.zeros((W, 4)), np.zeros((W, 5, n))
        for w in range(W):
            rows = valid & (win == w)
            e, s = fe[rows], fs[rows]
            d, u = s - e[:, None], s - shift
            ow[w] = [rows.sum(), e.sum(), (e - g).sum(), ((e - g) ** 2).sum()]
            mom[w] = [d.sum(axis=0), (d * d).sum(axis=0), u.sum(axis=0), (u * u).sum(axis=0),
                      ((e - g)[:, None] * u).sum(axis=0)]

        def replicate(c):
            rn = se = s1 = s2 = 0.0
            acc = np.zeros((5, n))
            for w in range(W):
                if c[w]:                            # a count of 0 does not touch the window's sums (0 x inf)
                    rn, se, s1, s2 = (x + c[w] * y for x, y in zip((rn, se, s1, s2), ow[w]))
                    acc = acc + float(c[w]) * mom[w]
            if rn < 2 or not (np.isfinite(se) and np.isfinite(s2)):
                return np.full((7, n), np.nan)
            A, B, C1, C2, C3 = acc
            see, m1 = s2 - s1 * s1 / rn, C1 / rn
            var_s, var_e, cov = C2 / rn - m1 * m1, see / rn, (C3 - s1 * m1) / rn
            cc = cov / np.sqrt(var_s * var_e)
            cc = np.where(np.isnan(cc), cc, np.clip(cc, -1.0, 1.0))
            alpha, beta = np.sqrt(var_s / var_e), 1.0 + A / se
            out = np.stack([1.0 - B / see, 1.0 - np.sqrt((cc - 1.0) ** 2 + (alpha - 1.0) ** 2 + (beta - 1.0) ** 2), cc,
                            alpha, beta, 100.0 * (A / se), np.sqrt(B / rn)])
            out[:, ~np.isfinite(acc).all(axis=0)] = np.nan
            return out
        point = replicate(np.ones(W, dtype=np.int64)).T.copy()
        reps = np.stack([replicate(c) for c in counts]) if len(counts) else np.empty((0, 7, n))
    return point, reps


def windows_of(rng, R, W):
    """arange(R) * W // R with 10 % of the rows in no window (every row in its window for R < 8)"""
    win = (np.arange(R) * W // R).astype(np.int32)
    if R >= 8:
        win[rng.random(R) < 0.10] = -1
    return win


def make_counts(rng, W, B):
    """[B, W] uint16: random draws (every row sums to W); row 0 all ones, row 1 all zeros, row 2 one window W times, row 3
    with 65,535 somewhere -- as many of the four as B has room for"""
    counts = np.zeros((B, W), dtype=np.int64)
    for b in range(B):
        counts[b] = np.bincount(rng.integers(W, size=W), minlength=W)
    special = [np.ones(W), np.zeros(W), np.where(np.arange(W) == W // 2, W, 0),
               np.where(np.arange(W) == W - 1, 65535, counts[min(3, B - 1)] if B else 0)]
    for b, row in enumerate(special[:B]):
        counts[b] = row
    return counts.astype(np.uint16)


def worst(got, want, floor=1e-12):
    """max |got - want| / max(|want|, floor) over the finite entries of want; the pattern of NaN and the infinities are
    required to be the same (else inf)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return float('inf')
    special = np.isinf(want) | np.isinf(got)
    if not np.array_equal(got[special], want[special]):
        return float('inf')
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), floor)))


def assert_comparable(want, what):
    """every compared |want| is 0 or above 1e-6 (a seed that fails this is changed, not the gate)"""
    x = np.asarray(want, dtype=np.float64)
    x = x[np.isfinite(x)]
    assert x.size == 0 or np.all((x == 0.0) | (np.abs(x) > 1e-6)), '%s: a compared |want| is neither 0 nor above 1e-6' % what
