"""The scores of the flow duration curve in exact arithmetic, host side: the truth, the bounds, the cases and the data of
tests/test_gpu_flow_duration_truth.py, held here to four conditions on the INPUTS (a seed that breaks one of them is
changed and recorded in RESEEDED, never a bound).

smart_flow_duration_hip pairs the sorted simulation with the sorted observations by rank, keeps the ranks i0 <= i < i1 of
the segment, applies f and ends in finish_objectives on one-pass moments about the column's value at rank i0, the first
of the summed values.  That choice is what keeps kappa of oracle/analyses/objfn.py small, and nothing but this
module enforces it: on the uniform noise of support.data the moments about rank 0 of the WINDOW, about the unsorted first
row or about a neighbour's value cost 1e-12, three orders below the suite's gate (1 / (x + eps) of the top 2 % alone lies
far enough from that of the smallest value to show at that gate, at 1e-7).

The pairs of a segment, their truth and bounds: oracle/analyses/flow_duration.py (`curve_pairs`, `curve_reference`); the
two families, `curves` and `plateau`, and the cases: tests/cases_flow_duration.py.

The conditions:
 (a) on support.data and on `curves`, curve_reference has the NaN pattern of the float64 `statement` of
     oracle/analyses/flow_duration.py and agrees with it within 1e-11 on the compared entries (the statement is two-pass).
 (b) every bound of a finite truth is finite and positive; for 'none', 'sqrt' and 'inverse' it is below the gate relative
     to |truth| (the largest here: 4.6e-11, 'inverse' with its narrowed means).  'log' is not held to the gate: its bound
     holds the ulp of ln (LOG_REL) times the series' |mean| / std, the score's own sensitivity to the transform and none
     of the sums', and a plateau of relative spread 1e-6 takes it to 1.3e-8 whatever the kernel does
     (test_the_window_cases_meet_the_conditions of tests/test_objfn_truth_host.py has the same for the windows kernel).  The kernel is
     held to the bound under all four.
 (c) for every `plateau` case with i0 > 0, the float64 emulation of the sums about rank 0 of the window misses
     bounds(S, E, 0) at least a hundredfold in some compared entry of EVERY window that has a score (a NaN there -- the
     cancelled variance came out negative -- is a miss), and about rank i0 it is inside in all three orders.
 (d) at most 2 % of the finite truth entries of a case lie below SMALL."""
import numpy as np
import pytest

from cases_flow_duration import (BIG_TRANSFORMS, CASES, EMPTY, INSTANCES, SEGMENTS, TRANSFORMS, case_data, case_id,
                                 case_reference, curves, window_array)
from cases_objfn import EPS, compared
from oracle.analyses.flow_duration import curve_pairs, curve_reference, statement, window_rows, with_window_rank_0
from oracle.analyses.objfn import ORDERS, emulate, kappa
from support import GATE, data


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
