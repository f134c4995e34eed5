"""Flow duration curves: smart_flow_duration_hip as a numpy statement, and its scores in exact arithmetic (the pairs of a
segment in the form oracle/analyses/objfn.py takes).  TEST INFRASTRUCTURE ONLY.

`statement`: per window sort the rows that belong to it (and carry an observation), take rank max(1, ceil(q * m)); for the
objective functions pair the sorted simulation with the sorted observations by rank, keep the ranks of the segment, apply f,
oracle.objfn_oracle.objective_functions(...)[:7], and the two rules (fewer than two pairs -> NaN; a transformed value of
the segment that is not finite -> NaN)."""
import numpy as np

from oracle import objfn_oracle
from oracle.analyses.objfn import INPUT_REL, bounds, truth
from oracle.analyses.windows import transformed


def rank_of(q, m):
    """1-based rank of the order statistic: max(1, ceil(q * m)), the product formed in double."""
    return max(1, int(np.ceil(float(q) * float(m))))


def statement(sim, probs, obs=None, win=None, n_windows=1, transform='none', eps=0.0, segment=(0.0, 1.0), objfn=False):
    """sim [R, n], probs [K], obs [R] or None (NaN = missing), win [R] or None -> (quant [W, K, n], objfn [W, n, 7] or
    None)."""
    R, n = sim.shape
    quant = np.full((n_windows, len(probs), n), np.nan)
    scores = np.full((n_windows, n, 7), np.nan) if objfn else None
    lo, hi = float(segment[0]), float(segment[1])
    for w in range(n_windows):
        rows = np.ones(R, dtype=bool) if win is None else (np.asarray(win) == w)
        if obs is not None:
            rows = rows & ~np.isnan(obs)
        m = int(rows.sum())
        if m == 0:
            continue
        x = np.sort(sim[rows], axis=0)                       # NaN sorts last, above +inf
        for k, q in enumerate(probs):
            quant[w, k] = x[rank_of(q, m) - 1]
        if not objfn:
            continue
        i = np.arange(m, dtype=np.float64)
        keep = (lo * float(m) <= i) & (i < hi * float(m))
        e = transformed(transform, np.sort(obs[rows])[keep], eps)
        if keep.sum() < 2 or not np.isfinite(e).all():
            continue
        for c in range(n):
            s = transformed(transform, x[keep, c], eps)
            if np.isfinite(s).all():
                with np.errstate(all='ignore'):
                    scores[w, c] = objfn_oracle.objective_functions(s, e)[:7]
    return quant, scores


def segment_ranks(m, segment):
    """i0, i1 as the kernel has them: ceil(lo * m), min(m, ceil(hi * m)), the products in double"""
    return int(np.ceil(float(segment[0]) * float(m))), min(m, int(np.ceil(float(segment[1]) * float(m))))


def window_rows(obs, win, w):
    rows = ~np.isnan(obs)
    return rows if win is None else rows & (np.asarray(win) == w)


# ---- truth and bounds --------------------------------------------------------------------------------------------------
def curve_pairs(sim, obs, win, w, transform, eps, segment):
    """-> (S [c, n], E [c], i0, m): f of the sorted simulation and of the sorted observations over the ranks i0 <= i < i1
    of window w's m rows (the window, and an observation present).  np.sort along time, NaN last; f after the sort, as the
    kernel applies it: the keys are of the raw flow, and 'inverse' is decreasing."""
    rows = window_rows(obs, win, w)
    m = int(rows.sum())
    i0, i1 = segment_ranks(m, segment)
    x, e = np.sort(sim[rows], axis=0), np.sort(obs[rows])
    return transformed(transform, x[i0:i1], eps), transformed(transform, e[i0:i1], eps), i0, m


def curve_reference(sim, obs, win, W, transform, eps, segment):
    """-> (want, bnd) [W, n, 7]: per window truth(S, E) and bounds(S, E, 0) -- the moments about rank i0 -- of its pairs.
    The entry's two rules: fewer than two ranks, or an f(obs) of the segment that is not finite: NaN for the window; an
    f(sim) of the segment that is not finite: NaN for that sample.  (A bound where truth is NaN is +inf.)"""
    n = sim.shape[1]
    want, bnd = np.full((W, n, 7), np.nan), np.full((W, n, 7), np.inf)
    for w in range(W):
        S, E, _, _ = curve_pairs(sim, obs, win, w, transform, eps, segment)
        if E.size < 2 or not np.isfinite(E).all():
            continue
        bad = ~np.isfinite(S).all(axis=0)
        want[w] = truth(S, E)
        want[w][bad] = np.nan
        with np.errstate(all='ignore'):
            bnd[w] = bounds(S, E, 0, input_rel=INPUT_REL[transform])
        bnd[w][bad] = np.inf
    return want, bnd


def with_window_rank_0(sim, obs, win, w, transform, eps, segment):
    """-> (S' [1 + c, n], E' [1 + c]): the pairs of the segment with f(x_(0)), rank 0 of the WINDOW, in front of them as an
    unobserved row -- `emulate` and `kappa` with shift_row = 0 then take the moments about that value"""
    S, E, _, _ = curve_pairs(sim, obs, win, w, transform, eps, segment)
    x0 = transformed(transform, np.sort(sim[window_rows(obs, win, w)], axis=0)[:1], eps)
    return np.concatenate([x0, S]), np.concatenate([[np.nan], E])
