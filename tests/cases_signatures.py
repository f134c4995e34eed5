"""The inputs of the signature tests: the benign generator and the pulse thresholds of tests/test_gpu_signatures.py, and a
family on which a badly chosen constant of AC1's one-pass moments shows (`stress`: KINDS, columns of one matrix, with the
three window arrays of the GPU test).  A plain module: pytest does not collect it."""
import numpy as np

from oracle.analyses.signatures import bounds, exact
from support import SMALL

FLOOR = 1e-12               # the relative gate of tests/test_gpu_signatures.py floors |truth| here


# ---- the benign generator and the thresholds (tests/test_gpu_signatures.py) --------------------------------------------
def data(seed, R, n):
    """-> (rng, obs [R] with 15 % missing, sim [R, n]): hydrographs, every column a recession fed by events, the
    observations the first column times noise.  (Not the `data` of tests/support.py, whose columns are independent noise.)"""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.80, 0.98, n)
    event = np.where(rng.random((R, n)) < 0.15, rng.exponential(2.0, (R, n)), 0.0)
    sim = np.empty((R, n))
    s = rng.exponential(1.0, n)
    for r in range(R):
        s = k * s + event[r]
        sim[r] = 0.05 + s
    obs = sim[:, 0] * rng.uniform(0.7, 1.3, R) + 0.01
    obs[rng.random(R) < 0.15] = np.nan
    return rng, obs, sim


def thresholds(sim, obs, win, W):
    """(lo, hi) per window: the 30th and the 80th percentile of the window's simulated values; window 0 takes two values
    of the matrix itself; the last of several windows a NaN pair"""
    pulse = np.full((W, 2), np.nan)
    for w in range(W):
        rows = np.ones(len(sim), dtype=bool) if win is None else (win == w)
        if obs is not None:
            rows = rows & ~np.isnan(obs)
        if rows.any() and not (W > 1 and w == W - 1):
            pulse[w] = np.quantile(sim[rows], [0.3, 0.8], method='inverted_cdf' if w == 0 else 'linear')
    return pulse


# ---- the family ------------------------------------------------------------------------------------------------------
FACTORS = (10.0, 100.0, 1e4)
SPREADS = (1.0, 1e-2)
KINDS = (['benign'] * 4 + ['barely'] * 4 +
         ['first_%s_%g_%g' % (place, f, s) for f in FACTORS for s in SPREADS for place in ('pair', 'gap')] +
         ['flood'] * 3 + ['zeros'] * 3 + ['const_first'] * 2 + ['const_last'] * 2)
FLOOD_KINDS = [k for k, name in enumerate(KINDS) if name.startswith('first_')]
CONSTANT_KINDS = [k for k, name in enumerate(KINDS) if name.startswith('const_')]
STRESS_R = (9, 501, 1025)
RESEEDED = {}                       # R -> another seed, where the first broke a condition (none did)


def stress(seed, R):
    """-> (sim [R, len(KINDS)], obs [R], [(W, window ids or None)] x 3, kinds).  Columns, by KINDS:
      benign        the generator of `data`: s <- k s + event, x = 0.05 + s;
      barely        level (1 + spread z), z the benign column scaled to [0, 1], level 10^U(-2, 4), spread 10^U(-3, -2);
      first_*       mu (1 + spread (z - 1/2)), mu 10^U(-1, 1), spread 1 or 1e-2, and the value 10, 100 or 1e4 mu at the
                    window's first valid row: 'pair' at row 0, with row 1 valid (the one window and the first half open on
                    it, and it is the first x_{r-1}); 'gap' at row h = R // 2, the first row of the second half, with rows
                    h - 1 and h + 1 unobserved (it is in no pair of any window);
      flood         benign, with 1e6 times the column's mean arriving at row R // 3 and receding at the column's own k;
      zeros         benign with stretches of exact zeros (one of them from row 0 on);
      const_first   one value but for row 0 (and row h, which is in no pair): the x_r list is constant;
      const_last    one value but for row R - 1 (row R - 2 is valid): the x_{r-1} list is constant.
    obs: 15 % missing; rows 0, 1, h, R - 3, R - 2, R - 1 observed, h - 1 and h + 1 not.  Windows: one; two halves; sixteen
    blocks with 10 % of the rows in no window."""
    assert R >= 9, 'the family needs R >= 9, not %d' % R
    n = len(KINDS)
    rng, obs, base = data(seed, R, n)
    h = R // 2
    obs[[0, 1, h, R - 3, R - 2, R - 1]] = 1.0
    obs[[h - 1, h + 1]] = np.nan
    z = (base - base.min(axis=0)) / (base.max(axis=0) - base.min(axis=0))
    sim = base.copy()
    k_rec = rng.uniform(0.80, 0.98, n)
    for c, kind in enumerate(KINDS):
        if kind == 'barely':
            sim[:, c] = 10.0 ** rng.uniform(-2.0, 4.0) * (1.0 + 10.0 ** rng.uniform(-3.0, -2.0) * z[:, c])
        elif kind.startswith('first_'):
            _, place, factor, spread = kind.split('_')
            mu = 10.0 ** rng.uniform(-1.0, 1.0)
            sim[:, c] = mu * (1.0 + float(spread) * (z[:, c] - 0.5))
            sim[0 if place == 'pair' else h, c] = float(factor) * mu
        elif kind == 'flood':
            at = R // 3
            sim[at:, c] += 1e6 * base[:, c].mean() * k_rec[c] ** np.arange(R - at)
        elif kind == 'zeros':
            for start in [0] + list(rng.integers(1, R, 3)):
                sim[start:start + int(rng.integers(2, R // 8 + 3)), c] = 0.0
        elif kind == 'const_first':
            level = 10.0 ** rng.uniform(-2.0, 4.0)
            sim[:, c] = level
            sim[[0, h], c] = level * (100.0 if c == CONSTANT_KINDS[0] else 1.01)
        elif kind == 'const_last':
            level = 10.0 ** rng.uniform(-2.0, 4.0)
            sim[:, c] = level
            sim[R - 1, c] = level * (100.0 if c == CONSTANT_KINDS[2] else 0.99)
    sixteen = (np.arange(R) * 16 // R).astype(np.int32)
    sixteen[rng.random(R) < 0.10] = -1
    windows = [(1, None), (2, (np.arange(R) >= h).astype(np.int32)), (16, sixteen)]
    return sim, obs, windows, list(KINDS)


def stress_case(R):
    """the family at one R of the GPU test, with the thresholds of every window array (from the benign columns, so that
    both kinds of run occur in them) -> (sim, obs, [(W, win, pulse)], kinds)"""
    sim, obs, windows, kinds = stress(RESEEDED.get(R, 7000 + R), R)
    return sim, obs, [(W, win, thresholds(sim[:, :4], obs, win, W)) for W, win in windows], kinds


_REFERENCES = {}


def stress_reference(R, alpha=0.925):
    """-> [(W, win, pulse, truth, bounds of the 'per_list' form)] of stress_case(R): computed once, shared, left unchanged"""
    if (R, alpha) not in _REFERENCES:
        sim, obs, windows, _ = stress_case(R)
        ref = []
        for W, win, pulse in windows:
            reference = exact(sim, obs, win, W, alpha, pulse)
            bnd = bounds(sim, obs, win, W, alpha, pulse, 'per_list', reference)
            for a in (reference[0], bnd):
                a.setflags(write=False)
            ref.append((W, win, pulse, reference[0], bnd))
        _REFERENCES[(R, alpha)] = ref
    return _REFERENCES[(R, alpha)]


# ---- the conditions --------------------------------------------------------------------------------------------------
def left_out(want):
    """the entries a relative gate leaves out: finite, not zero, below SMALL"""
    return np.isfinite(want) & (want != 0.0) & (np.abs(want) < SMALL)
