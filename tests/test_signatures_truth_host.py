"""The twelve hydrological signatures in exact arithmetic, what a float64 computation of the kernel's documented form may
differ from them by, and a family of inputs on which a badly chosen constant of AC1's one-pass moments shows.  Host side:
the truth, the bounds and the data of the stress test of tests/test_gpu_signatures.py, held here to four conditions on the
INPUTS (a seed or a spread that breaks one of them is changed, never a bound or a cap).

smart_signatures (csrc/smart_signatures.hip) forms, per (window, sample) and in row order, sum x, sum (x - f), over the
pairs sum |x_r - x_{r-1}| and sum x_r, the five moments Sa = sum ua, Sb = sum ub, Saa, Sbb, Sab of ua = x_{r-1} - sa,
ub = x_r - sb, and over the falling pairs sum (ln x_r - ln x_{r-1}).  var = S2 - S1^2 / p loses digits as
kappa = 1 + ((s - mean) / std)^2 grows: a constant that is a member of the list it centres keeps kappa <= about p, a value
from outside it (the window's first valid row is never an x_r; before a gap it is in neither list) does not.

`truth`    the columns in integers over one power of two (fractions.Fraction at the end), each rounded once.
`bounds`   per entry what the kernel's form, its additions in ANY order, may differ from `truth` by (derived below).
`emulate`  the kernel's sums in float64 in one of three orders, about the shifts of one of two forms: 'shared' (both lists
           about the window's first valid value) and 'per_list' (each list about its own member of the first pair).
`stress`   the family: KINDS, columns of one matrix, with the three window arrays of the GPU test.
`data`, `thresholds`: the benign generator and the pulse thresholds of tests/test_gpu_signatures.py (they live here so
that the family can start from them)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from test_signatures_host import (statement, X8, NAMES, MEAN, BFI, FLASHINESS, AC1, RLD, RECESSION, PEAK, PEAK_ROW,
                                  HIGH_COUNT, HIGH_DURATION, LOW_COUNT, LOW_DURATION)

U = 2.0 ** -53
GATE = 1e-9                 # the gate of tests/test_gpu_signatures.py: relative, |truth| floored at FLOOR; absolute for AC1
FLOOR = 1e-12
SMALL = 1e-6                # a finite, non-zero |truth| below this is left out of relative comparisons
SLACK = 1.0 + 2.0 ** -20    # the magnitudes inside `bounds` are themselves float64 sums (docstring of bounds)
ROUNDED = [MEAN, BFI, FLASHINESS, AC1, RECESSION]                  # sums of roundings: a bound that is not zero
INTEGER = [RLD, PEAK, PEAK_ROW, HIGH_COUNT, HIGH_DURATION, LOW_COUNT, LOW_DURATION]    # a value, or one IEEE quotient of counts
RELATIVE = [MEAN, BFI, FLASHINESS, RLD, RECESSION, HIGH_DURATION, LOW_DURATION]
FORMS = ('shared', 'per_list')
ORDERS = ('forward', 'reversed', 'pairwise')


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


def valid_rows(R, obs, win, w):
    """[R] bool: the rows of window w that carry an observation"""
    rows = np.ones(R, dtype=bool) if win is None else (np.asarray(win) == w)
    return rows if obs is None else rows & ~np.isnan(np.asarray(obs, dtype=np.float64))


# ---- truth -----------------------------------------------------------------------------------------------------------
def _dyadic(x):
    """a finite double -> (n, e): x = n / 2^e exactly, e >= 0"""
    n, d = float(x).as_integer_ratio()
    return n, d.bit_length() - 1


def _ints(values):
    """doubles -> (their integers over one power of two, its exponent S): no gcd per term"""
    pairs = [_dyadic(v) for v in values]
    S = max(e for _, e in pairs)
    return [n << (S - e) for n, e in pairs], S


def _column(x, rows, pair, alpha, lo, hi):
    """one (window, sample): x the values of the valid rows `rows`, pair[k] whether row rows[k] - 1 is valid too
    -> (the twelve columns, (va, vb, cov): the exact centred sums of the pair lists, rounded once)"""
    nan = math.nan
    out, centred = [nan] * 12, (nan, nan, nan)
    m = len(rows)
    if m == 0 or not all(math.isfinite(v) for v in x):
        return out, centred
    total = 0.0
    for v in x:
        total += v
    if not math.isfinite(total):        # the statement's rule: the sum of x, in row order, overflows
        return out, centred
    xi, S = _ints(x)
    (An, Ae), (Gn, Ge) = _dyadic(alpha), _dyadic((1.0 + alpha) / 2.0)
    sum_x = sum(xi)
    fn, fe = 0, 0                       # the filter: f = fn / 2^(S + fe)
    bn, be = 0, 0                       # sum f = bn / 2^(S + be)
    p = rises = limbs = falls = 0
    num = den = sa = sb = saa = sbb = sab = 0
    logs = []
    was_rising = False
    peak, peak_row = -math.inf, 0
    hi_runs = hi_rows = lo_runs = lo_rows = 0
    for k in range(m):
        v, vn = x[k], xi[k]
        if pair[k]:
            before, pn = x[k - 1], xi[k - 1]
            p += 1
            dn = vn - pn
            e = max(fe + Ae, Ge)        # alpha f + gain d over 2^(S + e)
            tn = ((An * fn) << (e - fe - Ae)) + ((Gn * dn) << (e - Ge))
            if tn <= 0:
                tn, e = 0, 0
            if tn > (vn << e):
                tn, e = vn, 0
            z = min(e, (tn & -tn).bit_length() - 1) if tn else e
            fn, fe = tn >> z, e - z
            num += abs(dn)
            den += vn
            sa, sb, saa, sbb, sab = sa + pn, sb + vn, saa + pn * pn, sbb + vn * vn, sab + pn * vn
            rising = vn > pn
            rises += rising
            limbs += rising and not was_rising
            was_rising = rising
            if 0 < vn < pn:
                falls += 1
                logs.append(math.log1p(float(Fraction(dn, pn))))
            hi_runs += v > hi and before <= hi
            lo_runs += v < lo and before >= lo
        else:
            fn, fe = 0, 0
            was_rising = False
            hi_runs += v > hi
            lo_runs += v < lo
        if fe > be:
            bn, be = bn << (fe - be), fe
        bn += fn << (be - fe)
        if v > peak:
            peak, peak_row = v, rows[k]
        hi_rows += v > hi
        lo_rows += v < lo
    out[MEAN] = float(Fraction(sum_x, m << S))
    if sum_x != 0:
        out[BFI] = ((sum_x << be) - bn) / (sum_x << be)         # (int / int is correctly rounded, whatever the lengths)
    if p > 0 and den != 0:
        out[FLASHINESS] = float(Fraction(num, den))
    if p >= 2:
        va, vb, cov = p * saa - sa * sa, p * sbb - sb * sb, p * sab - sa * sb
        unit = p << (2 * S)
        centred = (va / unit, vb / unit, cov / unit)
        if va != 0 and vb != 0:
            out[AC1] = math.copysign(math.sqrt(float(Fraction(cov * cov, va * vb))), cov)
    if rises:
        out[RLD] = float(Fraction(limbs, rises))
    if falls:
        out[RECESSION] = math.fsum(logs) / falls
    out[PEAK], out[PEAK_ROW] = peak, float(peak_row)
    if not math.isnan(hi):
        out[HIGH_COUNT] = float(hi_runs)
        out[HIGH_DURATION] = float(Fraction(hi_rows, hi_runs)) if hi_runs else nan
    if not math.isnan(lo):
        out[LOW_COUNT] = float(lo_runs)
        out[LOW_DURATION] = float(Fraction(lo_rows, lo_runs)) if lo_runs else nan
    return out, centred


def exact(sim, obs=None, win=None, W=1, alpha=0.925, pulse=None):
    """-> (truth [W, 12, n], the exact centred sums (va, vb, cov) of the pair lists [W, 3, n], which `bounds` divides by)"""
    sim = np.asarray(sim, dtype=np.float64)
    R, n = sim.shape
    out, centred = np.full((W, 12, n), np.nan), np.full((W, 3, n), np.nan)
    for w in range(W):
        valid = valid_rows(R, obs, win, w)
        rows = [int(r) for r in np.flatnonzero(valid)]
        pair = [r >= 1 and bool(valid[r - 1]) for r in rows]
        lo, hi = (math.nan, math.nan) if pulse is None else (float(pulse[w][0]), float(pulse[w][1]))
        for c in range(n):
            col, cen = _column([float(v) for v in sim[rows, c]], rows, pair, alpha, lo, hi)
            out[w, :, c], centred[w, :, c] = col, cen
    return out, centred


def truth(sim, obs=None, win=None, W=1, alpha=0.925, pulse=None):
    """sim [R, n], obs [R] or None (NaN = missing), win [R] or None, pulse [W, 2] (lo, hi) or None -> [W, 12, n] float64:
    the definition of tests/test_signatures_host.py on the exact values of the doubles.  MEAN, FLASHINESS, RLD, both
    durations, the counts, PEAK and PEAK_ROW are rationals (or values of the matrix), rounded once.  BFI runs
    min(max(alpha f + (1 + alpha) / 2 d, 0), x) exactly, alpha and the gain the exact values of their doubles (the gain
    the double the kernel forms), and rounds the quotient of the two exact sums once.  AC1 from the exact centred sums: NaN
    iff p < 2 or a variance is exactly 0, else copysign(sqrt(float(cov^2 / (va vb))), cov).  RECESSION is
    fsum(log1p(float((x_r - x_{r-1}) / x_{r-1}))) / count over the falling pairs: the argument is a correctly rounded
    rational, so a term is off its logarithm by u |y| / (1 + y) and the 1 ulp of log1p, however close the ratio is to 1
    (`bounds` holds that share as well).  m == 0, a valid value that is not finite, a sum of x that overflows in row order and
    NaN thresholds as in `statement`."""
    return exact(sim, obs, win, W, alpha, pulse)[0]


# ---- the kernel's terms in float64 -----------------------------------------------------------------------------------
def _terms(sim, valid, alpha, form):
    """One window: what the kernel adds, in row order, as float64 [rows or pairs, n] arrays, with the magnitudes `bounds`
    needs beside them.  The filter is walked forward (it is a recurrence); `e` carries its error bound (bounds, BFI)."""
    R, n = sim.shape
    gain = (1.0 + alpha) / 2.0
    rows = np.flatnonzero(valid)
    t = {k: [] for k in ('x', 'base', 'e', 'abs', 'pair', 'ua', 'ub', 'rec', 'falling', 'logmag', 'steep')}
    g2, g3 = 2 * U / (1 - 2 * U), 3 * U / (1 - 3 * U)
    f, e = np.zeros(n), np.zeros(n)
    shift_a = shift_b = None
    with np.errstate(all='ignore'):
        for r in rows:
            x = sim[r]
            if form == 'shared' and shift_a is None:
                shift_a = shift_b = x
            if r >= 1 and valid[r - 1]:
                before = sim[r - 1]
                if form == 'per_list' and shift_a is None:
                    shift_a, shift_b = before, x
                d = x - before
                e = alpha * (1 + g2) * e + g2 * alpha * (np.abs(f) + e) + g3 * gain * np.abs(d) * (1 + U)
                f = np.minimum(np.maximum(alpha * f + gain * d, 0.0), x)
                falling = (0.0 < x) & (x < before)
                lx, lb = np.log(np.where(falling, x, 1.0)), np.log(np.where(falling, before, 1.0))
                t['abs'].append(np.abs(d))
                t['pair'].append(x)
                t['ua'].append(before - shift_a)
                t['ub'].append(x - shift_b)
                t['rec'].append(np.where(falling, lx - lb, 0.0))
                t['falling'].append(falling)
                t['logmag'].append(np.where(falling, np.abs(lx) + np.abs(lb), 0.0))
                t['steep'].append(np.where(falling, (before - x) / np.where(falling, x, 1.0), 0.0))
            else:
                f, e = np.zeros(n), np.zeros(n)
            t['x'].append(x)
            t['base'].append(x - f)
            t['e'].append(e)
    return {k: np.array(v, dtype=bool if k == 'falling' else np.float64).reshape(len(v), n) for k, v in t.items()}


def _sum(terms, order):
    """[k, n] -> [n]: one addition at a time in row order, in reversed order, or pairwise (neighbours, then neighbours of
    the sums, an odd one carried)"""
    k, n = terms.shape
    if k == 0:
        return np.zeros(n)
    if order == 'pairwise':
        while len(terms) > 1:
            half = len(terms) // 2
            head = terms[0:2 * half:2] + terms[1:2 * half:2]
            terms = head if len(terms) % 2 == 0 else np.concatenate([head, terms[-1:]])
        return terms[0]
    total = np.zeros(n)
    for row in (terms[::-1] if order == 'reversed' else terms):
        total = total + row
    return total


def emulate(sim, obs=None, win=None, W=1, alpha=0.925, pulse=None, form='per_list', order='forward'):
    """-> [W, 12, n]: the kernel's sums in float64 -- 'forward' as a lane walks its rows, 'reversed', or 'pairwise' -- with
    AC1's moments about the shifts of `form`, finished as the kernel finishes them.  The columns that are counts, values of
    the matrix or one quotient of two counts are the statement's: no order of additions reaches them."""
    sim = np.asarray(sim, dtype=np.float64)
    R, n = sim.shape
    out = statement(sim, obs, win, W, alpha, pulse)
    with np.errstate(all='ignore'):
        for w in range(W):
            valid = valid_rows(R, obs, win, w)
            t = _terms(sim, valid, alpha, form)
            m, p = len(t['x']), len(t['pair'])
            if m == 0:
                continue
            sum_x = _sum(t['x'], order)
            o = np.full((12, n), np.nan)
            o[MEAN] = sum_x / m
            o[BFI] = np.where(sum_x == 0.0, np.nan, _sum(t['base'], order) / sum_x)
            sum_pair = _sum(t['pair'], order)
            if p > 0:
                o[FLASHINESS] = np.where(sum_pair == 0.0, np.nan, _sum(t['abs'], order) / sum_pair)
            if p >= 2:
                ua, ub, q = t['ua'], t['ub'], float(p)
                Sa, Sb = _sum(ua, order), _sum(ub, order)
                Saa, Sbb, Sab = _sum(ua * ua, order), _sum(ub * ub, order), _sum(ua * ub, order)
                va, vb = Saa - Sa * Sa / q, Sbb - Sb * Sb / q
                o[AC1] = np.where((va > 0.0) & (vb > 0.0), (Sab - Sa * Sb / q) / np.sqrt(va * vb), np.nan)
            n_rec = t['falling'].sum(axis=0) if p else np.zeros(n)
            if p > 0:
                o[RECESSION] = np.where(n_rec > 0, _sum(t['rec'], order) / np.maximum(n_rec, 1), np.nan)
            o[:, ~np.isfinite(sum_x)] = np.nan
            out[w, ROUNDED] = o[ROUNDED]
    return out


# ---- what the kernel may differ by -----------------------------------------------------------------------------------
def _gamma(k):
    return k * U / (1.0 - k * U)


def _mul(a, b):
    """relative errors of two factors -> of their product"""
    return a + b + a * b


def _sqrt(a):
    """relative error a of x -> of sqrt x (the lower side is the larger one)"""
    return np.where(a < 1.0, 1.0 - np.sqrt(np.maximum(1.0 - a, 0.0)), np.inf)


def bounds(sim, obs=None, win=None, W=1, alpha=0.925, pulse=None, form='per_list', reference=None):
    """-> [W, 12, n]: what a float64 computation of the kernel's form, with its additions in ANY order, may differ from
    `truth` by; NaN where truth is NaN.  `reference` = exact(...) of the same arguments, where the caller has it.
    u = 2^-53, gamma(k) = k u / (1 - k u); m valid rows, p pairs, k falling pairs; a hat marks the float64 value.

    A sum of k terms added in any order is off by at most gamma(k - 1) sum|term|; a term that is a rounded difference adds
    u, a rounded product of two such 3 u in all (a fused multiply-add drops a rounding, never adds one).
    MEAN        dSx = gamma(m - 1) sum|x|;  dSx / m + u |MEAN| (the division).
    FLASHINESS  dnum = gamma(p + 1) sum|d^|, dden = gamma(p - 1) sum x_r:  (dnum + |F| dden) / (den - dden) + u |F|.
    BFI         t = alpha f + gain d in float64 is (alpha f^ (1 + d3) + gain d (1 + d1)(1 + d2))(1 + d4), and the clamp
                min(max(., 0), x) moves nothing apart, so the filter's error obeys
                    e_r <= alpha (1 + gamma(2)) e_{r-1} + gamma(2) alpha (|f^_{r-1}| + e_{r-1}) + gamma(3) gain |d^_r| (1 + u),
                e = 0 at a row without a pair: carried with factor alpha per step.  A term x - f^ is off x - f by e_r and
                its own rounding: dSb = sum e_r + gamma(m + 1) sum|x - f^|;  (dSb + |BFI| dSx) / (Sx - dSx) + u |BFI|.
    AC1         about the shifts of `form`, with ua, ub rounded differences:
                    dSa = gamma(p + 1) sum|ua|,  dSaa = gamma(p + 3) sum ua^2,  dSab = gamma(p + 3) sum|ua ub|  (b alike);
                va = Saa - Sa Sa / p is two roundings under the quotient and one above it, with |Sa| <= |Sa^| + dSa = A:
                    dva = dSaa + (2 A dSa + dSa^2) / p + gamma(2) (A + dSa)^2 / p, then + u (va + dva);
                    dcov = dSab + (A dSb + B dSa + dSa dSb) / p + gamma(2) (A + dSa)(B + dSb) / p, then + u (|cov| + dcov);
                D = sqrt(va vb) with relative errors composed exactly ((1 + x)(1 + y) - 1, 1 - sqrt(1 - x)) and one u per
                rounded operation (the product, the root):  (dcov + |AC1| D rD) / (D (1 - rD)) + u |AC1|.  Absolute.
                kappa enters through sum ua^2 = p var kappa, sum|ua| and sum|ua ub| likewise.
    RECESSION   the device's double log is within 1 ulp (HIP math API, double precision: log, 1 ULP), 1 ulp <= 2 u of the
                value: a term ln x_r - ln x_{r-1} is off by 2 u (|ln x_r| + |ln x_{r-1}|) and its own rounding, 2 u |t^|;
                the sum adds gamma(k - 1) sum|t^|; the division u.  Truth's own share: per term u (x_{r-1} - x_r) / x_r (the
                rounded argument of log1p) + 2 u |t^| (log1p), and u for fsum and the division.
    RLD, PEAK, PEAK_ROW, the counts and the durations: 0 -- integers, values of the matrix, and one IEEE quotient of two
    integers, which is the correctly rounded rational that `truth` holds.
    Last, 4 ulp of the value itself (truth's own rounding, the final operation), and everything times 1 + 2^-20: the
    magnitudes above are float64 sums of non-negative terms, right to m 2^-53 of themselves.  No constant is fitted."""
    sim = np.asarray(sim, dtype=np.float64)
    R, n = sim.shape
    want, centred = exact(sim, obs, win, W, alpha, pulse) if reference is None else reference
    out = np.zeros((W, 12, n))
    with np.errstate(all='ignore'):
        for w in range(W):
            t = _terms(sim, valid_rows(R, obs, win, w), alpha, form)
            m, p = len(t['x']), len(t['pair'])
            if m == 0:
                continue
            raw = np.zeros((12, n))
            Sx, dSx = t['x'].sum(axis=0), _gamma(m - 1) * np.abs(t['x']).sum(axis=0)
            raw[MEAN] = dSx / m + U * np.abs(want[w, MEAN])
            dSb = t['e'].sum(axis=0) + _gamma(m + 1) * np.abs(t['base']).sum(axis=0)
            b = np.abs(want[w, BFI])
            raw[BFI] = np.where(dSx < np.abs(Sx), (dSb + b * dSx) / (np.abs(Sx) - dSx), np.inf) + U * b
            if p > 0:
                den, F = t['pair'].sum(axis=0), np.abs(want[w, FLASHINESS])
                dnum, dden = _gamma(p + 1) * t['abs'].sum(axis=0), _gamma(p - 1) * np.abs(t['pair']).sum(axis=0)
                raw[FLASHINESS] = np.where(dden < np.abs(den), (dnum + F * dden) / (np.abs(den) - dden), np.inf) + U * F
                k = np.maximum(t['falling'].sum(axis=0), 1)
                mag = np.abs(t['rec']).sum(axis=0)
                dsum = 2 * U * t['logmag'].sum(axis=0) + 2 * U * mag + _gamma(k - 1) * mag
                own = U * t['steep'].sum(axis=0) + 2 * U * mag
                raw[RECESSION] = (dsum + own) / k + 2 * U * np.abs(want[w, RECESSION])
            if p >= 2:
                ua, ub, q = t['ua'], t['ub'], float(p)
                dSa, dSb_ = _gamma(p + 1) * np.abs(ua).sum(axis=0), _gamma(p + 1) * np.abs(ub).sum(axis=0)
                A, B = np.abs(ua.sum(axis=0)) + dSa, np.abs(ub.sum(axis=0)) + dSb_
                dSaa, dSbb = _gamma(p + 3) * (ua * ua).sum(axis=0), _gamma(p + 3) * (ub * ub).sum(axis=0)
                dSab = _gamma(p + 3) * np.abs(ua * ub).sum(axis=0)
                va, vb, cov = centred[w]
                dva = dSaa + (2 * A * dSa + dSa * dSa) / q + _gamma(2) * (A + dSa) ** 2 / q
                dvb = dSbb + (2 * B * dSb_ + dSb_ * dSb_) / q + _gamma(2) * (B + dSb_) ** 2 / q
                dcov = dSab + (A * dSb_ + B * dSa + dSa * dSb_) / q + _gamma(2) * (A + dSa) * (B + dSb_) / q
                dva, dvb, dcov = dva + U * (va + dva), dvb + U * (vb + dvb), dcov + U * (np.abs(cov) + dcov)
                D = np.sqrt(va * vb)
                rD = _mul(_sqrt(_mul(_mul(dva / va, dvb / vb), U)), U)
                ac1 = np.abs(want[w, AC1])
                raw[AC1] = np.where(rD < 1.0, (dcov + ac1 * D * rD) / (D * (1.0 - rD)), np.inf) + U * ac1
            out[w] = raw
            out[w, ROUNDED] = (raw[ROUNDED] + 4 * U * np.abs(want[w, ROUNDED])) * SLACK
    out[np.isnan(want)] = np.nan
    return out


def margins(got, want, bnd):
    """|got - want| / bound per entry, over the entries where truth is finite: 0 where both are equal (a bound of 0 is met
    only so), inf where a NaN stands on one side alone"""
    got, want, bnd = np.asarray(got), np.asarray(want), np.asarray(bnd)
    with np.errstate(all='ignore'):
        err = np.abs(got - want)
        ratio = np.where(err == 0.0, 0.0, np.where(bnd > 0.0, err / bnd, np.inf))
    ratio = np.where(np.isnan(got) != np.isnan(want), np.inf, ratio)
    return np.where(np.isnan(got) & np.isnan(want), 0.0, ratio)


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
    assert R >= 9
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


# ---- the conditions --------------------------------------------------------------------------------------------------
def left_out(want):
    """the entries a relative gate leaves out: finite, not zero, below SMALL"""
    return np.isfinite(want) & (want != 0.0) & (np.abs(want) < SMALL)


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
