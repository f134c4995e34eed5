"""The exact truth of the twelve signatures (oracle/analyses/signatures.py) against the series worked by hand, the
statement and mpmath, and the stress family of tests/test_gpu_signatures.py (tests/cases_signatures.py) held to four
conditions on the INPUTS (a seed or a spread that breaks one of them is changed, never a bound or a cap)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from cases_signatures import (CONSTANT_KINDS, FLOOD_KINDS, FLOOR, KINDS, STRESS_R, data, left_out, stress, stress_case,
                              stress_reference, thresholds)
from oracle.analyses.signatures import (INTEGER, ORDERS, RELATIVE, bounds, emulate, exact, margins, statement, truth, X8,
                                        NAMES, MEAN, BFI, FLASHINESS, AC1, RLD, RECESSION, PEAK, PEAK_ROW,
                                        HIGH_COUNT, HIGH_DURATION, LOW_COUNT, LOW_DURATION)
from oracle.exact import U
from support import GATE


# ---- truth against the hand-worked series and the statement ----------------------------------------------------------
def test_truth_on_the_series_worked_by_hand():
    """X8 of tests/test_signatures_host.py, the observation of row 4 missing; alpha = 0.5, lo = 3.5, hi = 2"""
    sim = np.array(X8).reshape(8, 1)
    obs = np.ones(8)
    obs[4] = np.nan
    got = truth(sim, obs, None, 1, 0.5, [(3.5, 2.0)])[0, :, 0]
    assert got[MEAN] == 19.0 / 7.0 and got[BFI] == (19.0 - 3.75) / 19.0
    assert got[FLASHINESS] == 8.0 / 14.0
    assert got[AC1] == -math.sqrt(float(Fraction(484, 100) / (Fraction(68, 10) * Fraction(28, 10))))
    assert abs(got[AC1] - (-2.2 / np.sqrt(6.8 * 2.8))) < 1e-15
    assert got[RLD] == 2.0 / 3.0 and got[RECESSION] == math.log(0.5)
    assert got[PEAK] == 4.0 and got[PEAK_ROW] == 2.0
    assert got[HIGH_COUNT] == 3.0 and got[HIGH_DURATION] == 4.0 / 3.0
    assert got[LOW_COUNT] == 3.0 and got[LOW_DURATION] == 5.0 / 3.0
    strict = truth(sim, obs, None, 1, 0.5, [(2.0, 4.0)])[0, :, 0]
    assert strict[HIGH_COUNT] == 0.0 and np.isnan(strict[HIGH_DURATION]) and strict[LOW_COUNT] == 1.0 and strict[LOW_DURATION] == 1.0
    free = truth(sim, None, None, 1, 0.5, None)[0, :, 0]
    assert free[PEAK] == 9.0 and free[PEAK_ROW] == 4.0 and free[MEAN] == 3.5 and np.isnan(free[HIGH_COUNT:]).all()
    assert free[RLD] == 3.0 / 4.0


def test_truth_has_the_statements_rules_and_its_values_on_benign_data():
    """m == 0, a value that is not finite, an overflowing sum, NaN thresholds, a window that never occurs: the pattern of
    `statement`; on benign data the two agree to 1e-12 (the two-pass float64 statement is itself right to about 1e-14),
    the integer columns bit for bit."""
    rng, obs, sim = data(31, 60, 9)
    win = (np.arange(60) * 3 // 60).astype(np.int32)
    win[rng.random(60) < 0.1] = -1
    sim[:, 1] = 2.5
    sim[:, 2] = 0.0
    valid = np.flatnonzero(~np.isnan(obs) & (win == 1))
    sim[valid[2], 3], sim[valid[3], 4] = np.nan, np.inf
    sim[valid[::2], 5] = 1e308
    sim[np.flatnonzero(np.isnan(obs)), 6] = np.nan                      # never seen
    pulse = thresholds(sim[:, 7:], obs, win, 4)
    pulse[1, 0] = np.nan
    want = statement(sim, obs, win, 4, 0.5, pulse)
    got = truth(sim, obs, win, 4, 0.5, pulse)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[3]).all() and np.isnan(got[1, :, 3:6]).all() and not np.isnan(got[0][[MEAN, BFI, AC1, PEAK]][:, 3:7]).any()
    assert np.isnan(got[:3, AC1, 1]).all() and np.all(got[:3, BFI, 1] == 1.0) and np.isnan(got[:3, BFI, 2]).all()
    assert np.array_equal(got[:, INTEGER], want[:, INTEGER], equal_nan=True)
    ok = ~np.isnan(want)
    assert np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), FLOOR)) < 1e-12


def test_truth_against_mpmath():
    """the float64 ends of truth (a square root, log1p and fsum) against 60 digits"""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 60
    sim, obs, windows, kinds = stress(5, 41)
    got = truth(sim, obs)
    rows = np.flatnonzero(~np.isnan(obs))
    pairs = [r for r in rows if r >= 1 and not np.isnan(obs[r - 1])]
    for c in range(sim.shape[1]):
        a = [mp.mpf(float(sim[r - 1, c])) for r in pairs]
        b = [mp.mpf(float(sim[r, c])) for r in pairs]
        ma, mb = mp.fsum(a) / len(a), mp.fsum(b) / len(b)
        va, vb = mp.fsum((v - ma) ** 2 for v in a), mp.fsum((v - mb) ** 2 for v in b)
        if va == 0 or vb == 0:
            assert np.isnan(got[0, AC1, c]), kinds[c]
        else:
            ac1 = mp.fsum((x - ma) * (y - mb) for x, y in zip(a, b)) / mp.sqrt(va * vb)
            assert abs(got[0, AC1, c] - ac1) <= 4 * U * abs(ac1), kinds[c]
        logs = [mp.log(y / x) for x, y in zip(a, b) if 0 < y < x]
        if logs:
            rec = mp.fsum(logs) / len(logs)
            steep = max(float((x - y) / y) for x, y in zip(a, b) if 0 < y < x)
            assert abs(got[0, RECESSION, c] - rec) <= (6 + steep) * U * mp.fsum(abs(v) for v in logs) / len(logs), kinds[c]
        mean = mp.fsum(mp.mpf(float(sim[r, c])) for r in rows) / len(rows)
        assert abs(got[0, MEAN, c] - mean) <= U * abs(mean)


@pytest.mark.parametrize('R', STRESS_R)
def test_the_stress_family_meets_the_conditions(R):
    """(1) every bound of the 'per_list' form is below the suite's gate; (2) `emulate('per_list')` is inside it in all three
    orders; (3) `emulate('shared')` misses the AC1 gate a hundredfold on a flood column, in every order; (4) at most 5 % of a
    relatively compared column is left out, none of AC1, and both constant-but-for-one-row kinds have AC1 = NaN by the
    exact rule."""
    sim, obs, windows, kinds = stress_case(R)
    assert kinds == KINDS and sim.shape == (R, len(KINDS)) and np.all(sim >= 0.0)
    worst_shared = {order: 0.0 for order in ORDERS}
    finite = np.zeros(12)
    small = np.zeros(12)
    for (W, win, pulse), (_, _, _, want, bnd) in zip(windows, stress_reference(R)):
        held = np.isfinite(want)
        assert np.isfinite(bnd[held]).all() and np.all(bnd[held] >= 0.0) and np.all(bnd[:, INTEGER][held[:, INTEGER]] == 0.0)
        # (1)
        keep = held & ~left_out(want)
        gate = GATE * np.maximum(np.abs(want), FLOOR)
        gate[:, AC1] = GATE
        assert np.all(bnd[keep] < gate[keep]), (W, np.nanmax(np.where(keep, bnd / gate, 0.0), axis=(0, 2)))
        # (4)
        finite += held.sum(axis=(0, 2))
        small += left_out(want).sum(axis=(0, 2))
        assert np.isnan(want[:, AC1][:, CONSTANT_KINDS]).all()
        # (2)
        for order in ORDERS:
            worst = margins(emulate(sim, obs, win, W, 0.925, pulse, 'per_list', order), want, bnd)
            assert np.all(worst <= 1.0), (W, order, np.max(worst, axis=(0, 2)))
        # (3)
        for order in ORDERS:
            bad = emulate(sim, obs, win, W, 0.925, pulse, 'shared', order)[:, AC1][:, FLOOD_KINDS]
            miss = np.abs(bad - want[:, AC1][:, FLOOD_KINDS]) / GATE
            miss = np.where(np.isnan(bad) & ~np.isnan(want[:, AC1][:, FLOOD_KINDS]), np.inf, miss)
            worst_shared[order] = max(worst_shared[order], float(np.nanmax(miss)))
    assert all(v >= 100.0 for v in worst_shared.values()), worst_shared
    for c in RELATIVE:
        assert small[c] <= 0.05 * finite[c], (NAMES[c], small[c], finite[c])


def test_the_bound_about_a_shared_shift_says_so():
    """kappa enters `bounds`: about the window's first valid value the AC1 bound of a flood column is beyond the gate, about
    the lists' own members it is a thousand times smaller"""
    sim, obs, windows, kinds = stress_case(501)
    W, win, pulse = windows[1]
    reference = exact(sim, obs, win, W, 0.925, pulse)
    shared = bounds(sim, obs, win, W, 0.925, pulse, 'shared', reference)[1, AC1][FLOOD_KINDS]
    own = bounds(sim, obs, win, W, 0.925, pulse, 'per_list', reference)[1, AC1][FLOOD_KINDS]
    assert np.max(shared) > GATE and np.max(own) < GATE and np.max(shared / own) > 1e3
