"""The scores of the flow duration curve in exact arithmetic, host side: the truth, the bounds, the cases and the data of
tests/test_gpu_flow_duration_truth.py, held here to four conditions on the INPUTS (a seed that breaks one of them is
changed and recorded in RESEEDED, never a bound).

smart_flow_duration_hip pairs the sorted simulation with the sorted observations by rank, keeps the ranks i0 <= i < i1 of
the segment, applies f and ends in finish_objectives on one-pass moments about the column's value at rank i0, the first
of the summed values.  That choice is what keeps kappa of tests/test_objfn_truth_host.py small, and nothing but this
module enforces it: on the uniform noise of support.data the moments about rank 0 of the WINDOW, about the unsorted first
row or about a neighbour's value cost 1e-12, three orders below the suite's gate (1 / (x + eps) of the top 2 % alone lies
far enough from that of the smallest value to show at that gate, at 1e-7).

`curve_pairs`      the pairs (f(x_(i)), f(obs_(i))) of one window's segment as a [c, n] matrix and a [c] vector, rank i0
                   in row 0: the form `truth`, `bounds` and `emulate` of tests/test_objfn_truth_host.py take as they are.
`curve_reference`  per window truth(S, E) and bounds(S, E, 0), with the entry's two rules.
`curves`           the family `stress` of that module, sorted by the kernel into curves.
`plateau`          a family on which a constant from outside the segment shows: inside the segment of its window a column
                   holds scale (1 + rel U(0, 1)), scale = 10^U(-2, 4), rel = 10^U(-6, -3); the ranks below i0 lie at scale
                   10^U(-4, -1) and the ranks from i1 on at scale (2 + U(0, 1)); the rows are shuffled.  The moments about
                   rank 0 of the window have kappa of (1 / rel)^2 and more.  The observations are a plateau of their own,
                   1 + 3e-3 U(0, 1) inside the segment, 10^U(-3, -1) below and 2 + U(0, 1) above it: a spread of the
                   order of the columns' keeps KGEa = std f(s) / std f(e) above SMALL (against observations that span
                   decades a sixth of the columns would fall below it).  Built per window and per segment.
Under 'inverse' both families draw the columns' means (scales) from 10^U(-1, 2), INVERSE_DECADES of the truth module: the
standard deviation of 1 / (x + eps) is spread / mean, and with means up to 1e4 more than 2 % of the scores (KGEa) lie
below SMALL, which condition (d) forbids.  eps is 0.05 under 'log' and 'inverse', 0 otherwise.

The conditions:
 (a) on support.data and on `curves`, curve_reference has the NaN pattern of the float64 `statement` of
     tests/test_flow_duration_host.py and agrees with it within 1e-11 on the compared entries (the statement is two-pass).
 (b) every bound of a finite truth is finite and positive; for 'none', 'sqrt' and 'inverse' it is below the gate relative
     to |truth| (the largest here: 4.6e-11, 'inverse' with its narrowed means).  'log' is not held to the gate: its bound
     holds the ulp of ln (LOG_REL) times the series' |mean| / std, the score's own sensitivity to the transform and none
     of the sums', and a plateau of relative spread 1e-6 takes it to 1.3e-8 whatever the kernel does
     (test_the_window_cases_meet_the_conditions of the truth module has the same for the windows kernel).  The kernel is
     held to the bound under all four.
 (c) for every `plateau` case with i0 > 0, the float64 emulation of the sums about rank 0 of the window misses
     bounds(S, E, 0) at least a hundredfold in some compared entry of EVERY window that has a score (a NaN there -- the
     cancelled variance came out negative -- is a miss), and about rank i0 it is inside in all three orders.
 (d) at most 2 % of the finite truth entries of a case lie below SMALL."""
import functools
import zlib

import numpy as np
import pytest

from support import data
from test_flow_duration_host import statement
from test_objfn_truth_host import (EPS, GATE, INPUT_REL, INVERSE_DECADES, LOG_REL, ORDERS, SMALL, U, bounds,   # noqa: F401
                                   compared, emulate, kappa, stress, truth)     # (LOG_REL, SMALL, U: named in the docstrings)
from test_windows_host import transformed

TRANSFORMS = ('none', 'sqrt', 'log', 'inverse')
# (EPS, and INPUT_REL -- LOG_REL under 'log', 0 under the other three: sqrt, x + eps and 1 / y are one correctly rounded
# operation each on both sides -- are the truth module's)
SEGMENTS = ((0.0, 1.0), (0.98, 1.0), (0.0, 0.3), (0.3, 0.7))
# R -> (the instance of smart_fdc_sort it runs, N: the last workgroup of that instance's COLS is partial)
INSTANCES = {501: ('1024 x 16', 17), 1025: ('2048 x 8', 15), 2049: ('4096 x 4', 5), 4097: ('8192 x 2', 3),
             16384: ('16384 x 1', 3)}
BIG_TRANSFORMS = ('sqrt', 'inverse')    # R = 16,384 is held to truth under two transforms (its three columns all are)


# ---- the windows -------------------------------------------------------------------------------------------------------
UNEVEN = (0.0, 0.05, 0.15, 0.30, 0.50, 0.62, 0.87, 1.0)     # where the seven windows of 'uneven' begin, as shares of R
EMPTY = 4                                                   # the window of 'uneven' whose observations are all missing


def window_array(R, windows):
    """-> (W, win or None).  'none': no array, one window of every row.  'uneven': seven windows of consecutive rows of
    5, 10, 15, 20, 12, 25 and 13 % of R, every 17th row in no window."""
    if windows == 'none':
        return 1, None
    assert windows == 'uneven'
    win = np.searchsorted(np.asarray(UNEVEN[1:]) * R, np.arange(R), side='right').astype(np.int32)
    win[16::17] = -1
    return 7, win


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


# ---- the two families --------------------------------------------------------------------------------------------------
def curves(seed, R, n, transform):
    """-> (sim [R, n], obs [R]): stress(seed, R, n, 0) as it is (under 'inverse': its means from INVERSE_DECADES)"""
    sim, obs, _ = stress(seed, R, n, 0, decades=INVERSE_DECADES if transform == 'inverse' else (-2.0, 4.0))
    return sim, obs


def plateau(seed, R, n, win, W, transform, segment):
    """-> (sim [R, n], obs [R]) (module docstring); 15 % of the observations are missing, a row outside every window
    holds 1e3 times the column's scale."""
    rng = np.random.default_rng(seed)
    lo, hi = INVERSE_DECADES if transform == 'inverse' else (-2.0, 4.0)
    scale = 10.0 ** rng.uniform(lo, hi, n)
    rel = 10.0 ** rng.uniform(-6.0, -3.0, n)
    obs = np.full(R, np.nan)
    sim = np.tile(1e3 * scale, (R, 1))
    seen = rng.random(R) >= 0.15
    for w in range(W):
        rows = np.flatnonzero(seen if win is None else seen & (win == w))
        m = rows.size
        i0, i1 = segment_ranks(m, segment)
        rows = rng.permutation(rows)
        below, inside, above = rows[:i0], rows[i0:i1], rows[i1:]
        sim[below] = scale * 10.0 ** rng.uniform(-4.0, -1.0, (below.size, n))
        sim[inside] = scale * (1.0 + rel * rng.random((inside.size, n)))
        sim[above] = scale * (2.0 + rng.random((above.size, n)))
        obs[below] = 10.0 ** rng.uniform(-3.0, -1.0, below.size)
        obs[inside] = 1.0 + 3e-3 * rng.random(inside.size)
        obs[above] = 2.0 + rng.random(above.size)
    return sim, obs


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _cases():
    """(R, N, W, windows, transform, segment, family): every R under every transform (R = 16,384 under two) and family,
    once as one window without an array and once as the seven uneven ones.  `curves` walks the four segments so that every
    (R, W) and every (transform, W) meets each of them; `plateau` takes the two with i0 > 0."""
    out = []
    for ri, (R, (_, N)) in enumerate(sorted(INSTANCES.items())):
        for ti, transform in enumerate(TRANSFORMS):
            if R == 16384 and transform not in BIG_TRANSFORMS:
                continue
            for wi, (W, windows) in enumerate(((1, 'none'), (7, 'uneven'))):
                out.append((R, N, W, windows, transform, SEGMENTS[(ri + ti + 2 * wi) % 4], 'curves'))
                # (of seven windows of 501 rows none keeps two ranks of the top 2 %)
                top = (R, W) != (501, 7) and (ti + wi) % 2 == 0
                out.append((R, N, W, windows, transform, SEGMENTS[1 if top else 3], 'plateau'))
    return out


CASES = _cases()
RESEEDED = {}                           # case -> another seed, where the first broke a condition


def case_id(case):
    R, N, W, windows, transform, segment, family = case
    return '%d-%d-W%d-%s-%g_%g-%s' % (R, N, W, transform, segment[0], segment[1], family)


def case_seed(case):
    return RESEEDED.get(case, zlib.crc32(case_id(case).encode()))


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> (sim [R, N], obs [R], win [R] or None, eps); in 'uneven' window EMPTY has no observation"""
    R, N, W, windows, transform, segment, family = case
    _, win = window_array(R, windows)
    if family == 'curves':
        sim, obs = curves(case_seed(case), R, N, transform)
    else:
        sim, obs = plateau(case_seed(case), R, N, win, W, transform, segment)
    if win is not None:
        obs[win == EMPTY] = np.nan
    for a in (sim, obs):
        a.setflags(write=False)
    return sim, obs, win, EPS[transform]


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """-> (want, bnd) [W, N, 7] of the case, computed once and shared"""
    R, N, W, windows, transform, segment, family = case
    sim, obs, win, eps = case_data(case)
    want, bnd = curve_reference(sim, obs, win, W, transform, eps, segment)
    for a in (want, bnd):
        a.setflags(write=False)
    return want, bnd


# ---- the conditions ----------------------------------------------------------------------------------------------------
def test_the_cases_reach_what_they_must():
    assert sorted({c[0] for c in CASES}) == [501, 1025, 2049, 4097, 16384]
    assert {(c[0], c[1]) for c in CASES} == {(501, 17), (1025, 15), (2049, 5), (4097, 3), (16384, 3)}
    for R in INSTANCES:
        mine = [c for c in CASES if c[0] == R]
        assert {c[2] for c in mine} == {1, 7} and {c[6] for c in mine} == {'curves', 'plateau'}
        assert {c[4] for c in mine} == (set(BIG_TRANSFORMS) if R == 16384 else set(TRANSFORMS))
        assert any(c[6] == 'plateau' and c[5][0] > 0.0 for c in mine)
    assert {c[5] for c in CASES} == set(SEGMENTS) and {c[4] for c in CASES} == set(TRANSFORMS)
    for transform in TRANSFORMS:
        assert {c[5] for c in CASES if c[4] == transform} == set(SEGMENTS)
    assert len(set(CASES)) == len(CASES) and len({case_id(c) for c in CASES}) == len(CASES)
    W, win = window_array(501, 'uneven')
    m = [int((win == w).sum()) for w in range(W)]
    assert W == 7 and len(set(m)) == 7 and (win == -1).sum() >= 501 // 17 and min(m) > 20


@pytest.mark.parametrize('transform', TRANSFORMS)
def test_truth_is_the_statement_on_benign_data_and_on_curves(transform):
    """(a)"""
    worst = 0.0
    for R, n, windows, source in ((501, 5, 'uneven', 'data'), (501, 6, 'none', 'curves'), (2049, 4, 'uneven', 'curves')):
        W, win = window_array(R, windows)
        if source == 'data':
            _, obs, sim = data(7000 + R, R, n, obs_plus=0.05)
        else:
            sim, obs = curves(R + n, R, n, transform)
        if win is not None:
            obs[win == EMPTY] = np.nan
        for segment in SEGMENTS:
            want, _ = curve_reference(sim, obs, win, W, transform, EPS[transform], segment)
            _, oracle = statement(sim, [0.5], obs, win, W, transform, EPS[transform], segment, objfn=True)
            assert np.array_equal(np.isnan(want), np.isnan(oracle)), (R, source, segment)
            assert win is None or np.isnan(want[EMPTY]).all()
            keep = compared(want)
            assert keep.any()
            worst = max(worst, float(np.max(np.abs(want - oracle)[keep] / np.abs(want[keep]))))
    print('%s: truth against the two-pass float64 statement: %.3g' % (transform, worst))
    assert worst < 1e-11


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_the_cases_meet_the_conditions(case):
    """(b), (c) and (d)"""
    R, N, W, windows, transform, segment, family = case
    sim, obs, win, eps = case_data(case)
    want, bnd = case_reference(case)
    held, keep = np.isfinite(want), compared(want)
    assert held.any() and np.all(sim > 0.0)
    assert win is None or (np.isnan(want[EMPTY]).all() and not window_rows(obs, win, EMPTY).any())
    assert np.isfinite(bnd[held]).all() and np.all(bnd[held] > 0.0)                             # (b)
    tight = float(np.max(bnd[keep] / np.abs(want[keep])))
    small = float((held & ~keep).sum()) / float(held.sum())
    assert small <= 0.02, small                                                                 # (d)
    if transform != 'log':
        assert tight < GATE, tight                                                              # (b)
    used, miss, far, shifted = 0.0, np.inf, np.inf, 0
    for w in range(W):
        if not held[w].any():
            continue
        S, E, i0, m = curve_pairs(sim, obs, win, w, transform, eps, segment)
        for order in ORDERS:
            err = np.where(held[w], np.abs(emulate(S, E, 0, order) - want[w]) / bnd[w], 0.0)
            assert np.all(err <= 1.0), (w, order, float(np.max(err)))
            used = max(used, float(np.max(err)))
        if i0 > 0:
            shifted += 1
            S0, E0 = with_window_rank_0(sim, obs, win, w, transform, eps, segment)
            wrong = emulate(S0, E0, 0)
            far = min(far, float(np.max(kappa(S0, E0, 0))))
            off = np.abs(wrong - want[w]) / bnd[w]
            miss = min(miss, float(np.max(np.where(keep[w], np.where(np.isnan(off), np.inf, off), 0.0))))
    print('%s: bound over |truth| up to %.3g, %.2f %% below SMALL, the emulation about rank i0 uses %.3g of the bound, '
          'about rank 0 of the window it misses by %.3g and kappa reaches %.3g (the least over %d windows)'
          % (case_id(case), tight, 100.0 * small, used, miss, far, shifted))
    if family == 'plateau' and segment[0] > 0.0:
        assert shifted > 0 and miss >= 100.0 and far > 1e6, (miss, far)                         # (c), in every window
