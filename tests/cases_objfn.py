"""The inputs of the objective-function truth tests: a family on which a badly chosen constant of the one-pass moments
shows, and the cases that tests/test_objfn_truth_host.py holds to its conditions and tests/test_gpu_objfn_conditioning.py
launches.  A plain module: pytest does not collect it."""
import numpy as np

from oracle.analyses.objfn import INPUT_REL, LOG_EPS, LOG_REL      # noqa: F401 (the cases' users take them from here)
from support import GATE, SMALL

# ---- the family ------------------------------------------------------------------------------------------------------
FACTORS = (1.0, 2.0, 10.0, 100.0)
SPECIALS = (('nan', np.nan), ('inf', np.inf), ('1e308', 1e308))
# 1 / (x + eps) of a column of mean 1e4 and relative spread 1e-4 has a standard deviation of 1e-8: KGEa, its ratio to that
# of the observations, falls below SMALL, and with means of 10^U(-2, 4) more than 2 % of the scores do -- condition (d).
# The cases under 'inverse' draw their means from 10^U(-1, 2) (the same stream of the generator, another range)
INVERSE_DECADES = (-1.0, 2.0)
EPS = {'none': 0.0, 'sqrt': 0.0, 'log': LOG_EPS, 'inverse': LOG_EPS}


def stress(seed, R, n, r1, special_row=None, lead=(), missing=0.15, decades=(-2.0, 4.0)):
    """-> (sim [R, n], obs [R], info).  obs: a flood and its recession under log-normal noise, positive, `missing` of the
    rows absent, every row before r1 absent, rows r1 and R - 1 present.  Columns, by (j + 2) % 3: 0 follows the observations
    with noise, 1 is a flood then a recession of its own, 2 barely moves (relative spread 10^U(-4, -3)); mean 10^U(-2, 4)
    (10^U(decades): the cases under 'inverse' narrow it, INVERSE_DECADES), relative spread 10^U(-4, 0), every value
    positive.  The rows before r1 -- and the rows `lead` names, which are made
    unobserved, with the row after each of them observed -- hold mean x FACTORS[(j + 1) % 4] (column 0 barely moves, after twice its mean).  special_row (made unobserved)
    takes NaN, +inf and 1e308 in the columns info['special'] names (n >= 8)."""
    rng = np.random.default_rng(seed)
    lead = np.asarray(lead, dtype=np.int64)
    t = np.arange(R, dtype=np.float64)
    obs = (0.5 + 3.0 * np.exp(-np.maximum(t - r1, 0.0) / max(R / 4.0, 2.0))) * np.exp(rng.normal(0.0, 0.3, R))
    gone = rng.random(R) < missing
    gone[lead + 1] = False
    gone[[r1, R - 1]] = False
    gone[:r1] = True
    gone[lead] = True
    if special_row is not None:
        assert n >= 8 and special_row not in (r1, R - 1) and special_row not in lead + 1, \
            'special_row %d needs n >= 8 and a row that stays unobserved' % special_row
        gone[special_row] = True
    z_obs = (obs - obs.mean()) / obs.std()
    obs[gone] = np.nan
    kind = (np.arange(n) + 2) % 3
    mean = 10.0 ** rng.uniform(decades[0], decades[1], n)
    spread = np.where(kind == 2, 10.0 ** rng.uniform(-4.0, -3.0, n), 10.0 ** rng.uniform(-4.0, 0.0, n))
    noise = rng.normal(0.0, 1.0, (R, n))
    tau = rng.uniform(2.0, max(R / 3.0, 3.0), n)
    z = np.where(kind[None, :] == 1, np.exp(-np.maximum(t - r1, 0.0)[:, None] / tau[None, :]) + 0.05 * noise,
                 0.7 * z_obs[:, None] + 0.7 * noise)
    z = z - z.mean(axis=0)
    sim = mean * (1.0 + 0.9 * spread * z / np.max(np.abs(z), axis=0))
    before = mean * np.asarray(FACTORS)[(np.arange(n) + 1) % 4]
    sim[:r1] = before
    sim[lead] = before
    special = {}
    if special_row is not None:
        for k, (name, value) in enumerate(SPECIALS):
            special[name] = 3 + k
            sim[special_row, 3 + k] = value
    return sim, obs, {'mean': mean, 'spread': spread, 'special': special, 'r1': r1}


def compared(want):
    """the entries a relative comparison takes: finite and not below SMALL"""
    return np.isfinite(want) & (np.abs(want) >= SMALL)


# ---- the cases of tests/test_gpu_objfn_conditioning.py, held to the conditions here ------------------------------------
# smart_objfn_hip: r1 across the 4 x 8-row unroll of the <1, 8, 4> instance (rows 0 .. 31 are its first trip), R with no
# full trip, N one lane, one block and a lane, two blocks and two lanes
MATRIX_CASES = [(R, N, r1) for R in (2, 9, 501) for N in (1, 65, 130)
                for r1 in sorted({0, 1, 31, 32, 33, R - 2}) if r1 <= R - 2]
# (R, N, r1, special row): NaN, +inf, 1e308 at an unobserved row 0 and at an unobserved row in the middle
SPECIAL_CASES = [(501, 65, 33, 0), (501, 65, 1, 250), (9, 65, 3, 0)]
BIG_CASE = (9, 262144 + 37, 3)        # one lane per sample: smart_objfn_matrix<4, 1, 8> from 4 x 65,536 samples on
# (R, N, r1) or (window case, transform) -> another seed, where the first broke a condition.  Seed 73 under 'sqrt': the NSE
# of one (window, column) is 2.6e-5, and its bound, 3e-14, is 1.2e-9 of THAT -- over the gate that condition (b) asserts
RESEEDED = {('second_chunk', 'sqrt'): 75}


def matrix_case(R, N, r1, special_row=None):
    return stress(RESEEDED.get((R, N, r1), 1000 * R + 10 * (N % 1000) + r1), R, N, r1, special_row)


def big_columns(N):
    """the columns of the one-lane-per-sample case that are held to truth: the ends of wavefronts and workgroups, the
    last full workgroup and the lanes past it, and a few from anywhere"""
    edge = [0, 1, 63, 64, 255, 256, 257, 65535, 65536, 131071, 131072, 262143, 262144, 262145, N - 2, N - 1]
    return np.unique(np.concatenate([edge, np.random.default_rng(N).integers(0, N, 16)]))


def blocks(R, W, stop=None):
    """W windows of consecutive rows over [0, stop), every 17th row in no window"""
    stop = R if stop is None else stop
    win = np.full(R, -1, dtype=np.int32)
    win[:stop] = np.arange(stop) * W // stop
    win[16::17] = -1
    return win


def window_case(name, transform='none'):
    """-> (sim, obs, win, W); under 'inverse' the columns' means come from INVERSE_DECADES, a (name, transform) in RESEEDED
    takes that seed.  'one': a single window, the first observation at row 33.  'seven': seven windows whose
    first two rows each are unobserved and hold the column's mean x 1, 2, 10, 100.  'second_chunk': R = 1,025 + 9, window
    6 is the last nine rows -- its first listed row lies in the second chunk of 1,024 -- the first of them unobserved."""
    decades = INVERSE_DECADES if transform == 'inverse' else (-2.0, 4.0)
    seed = RESEEDED.get((name, transform), {'one': 71, 'seven': 72, 'second_chunk': 73}[name])
    if name == 'one':
        sim, obs, _ = stress(seed, 501, 65, 33, special_row=0, decades=decades)     # (NaN, +inf, 1e308 at row 0, never read)
        return sim, obs, np.zeros(501, dtype=np.int32), 1
    if name == 'seven':
        win = blocks(501, 7)
        first = np.array([np.flatnonzero(win == w)[0] for w in range(7)])
        win[first + 1] = np.arange(7)
        sim, obs, _ = stress(seed, 501, 130, 2, lead=np.concatenate([first[1:], first[1:] + 1]), decades=decades)
        return sim, obs, win, 7
    assert name == 'second_chunk', 'window case %r unknown' % (name,)
    R = 1025 + 9
    win = blocks(R, 6, stop=1025)
    win[1025:] = 6
    sim, obs, _ = stress(seed, R, 65, 1, lead=[1025], decades=decades)
    return sim, obs, win, 7


WINDOW_CASES = [(name, transform) for name in ('one', 'seven', 'second_chunk')
                for transform in ('none', 'sqrt', 'log', 'inverse')]


def bootstrap_case():
    """R = 501, N = 65, W = 11 windows of consecutive rows; the launch's first valid row is 3, in window 0."""
    sim, obs, _ = stress(81, 501, 65, 3)
    return sim, obs, blocks(501, 11), 11


# ---- the conditions ---------------------------------------------------------------------------------------------------
def inside_and_below_the_gate(want, bnd, what, gate=True):
    """conditions (b) and (d) on one array of truth and its bounds; the finite entries -> their number"""
    keep = compared(want)
    held = np.isfinite(want)
    assert np.isfinite(bnd[held]).all() and np.all(bnd[held] > 0.0), '%s: a bound is not finite and positive' % (what,)
    assert (held & ~keep).sum() <= 0.02 * held.sum(), '%s: over 2 %% of the finite entries lie below SMALL' % (what,)    # (d)
    if gate:
        assert np.max(bnd[keep] / np.abs(want[keep])) < GATE, \
            '%s: a bound is %.3g of |truth|, the gate is %g' % (what, np.max(bnd[keep] / np.abs(want[keep])), GATE)
    return int(held.sum())
