"""Hydrological signatures: the statement of smart_signatures_hip in plain Python loops over the rows, the twelve columns
in exact arithmetic, what a float64 computation of the kernel's documented form may differ from them by, and an emulation
of the kernel's sums.  TEST INFRASTRUCTURE ONLY.

`statement` restates the definition of include/smart_amd.h.  For window w a row r is VALID iff win[r] == w and, where obs
is given, obs[r] is not NaN (m valid rows); there is a PAIR at r iff r >= 1 and rows r-1 and r are both valid (p pairs);
rows are walked in ascending r.  The twelve columns, x_r = sim[r][c]:
   MEAN sum x / m;  BFI sum (x_r - f_r) / sum x_r with f_r = 0 at a valid row without a pair, else
   min(max(alpha f_{r-1} + (1 + alpha) / 2 (x_r - x_{r-1}), 0), x_r), NaN if sum x is 0;  FLASHINESS sum over the pairs
   |x_r - x_{r-1}| / sum over the pairs x_r, NaN if p is 0 or the denominator is 0;  AC1 the Pearson correlation of
   (x_{r-1}, x_r) over the pairs (two-pass here: the mean-centred sums of the pair lists), NaN if p < 2 or either variance
   is <= 0;  RLD limbs / rising pairs (rising: x_r > x_{r-1}; a limb starts at a rising pair at r when there is no rising
   pair at r-1), NaN without a rising pair;  RECESSION the mean of log(x_r / x_{r-1}) over the pairs with 0 < x_r <
   x_{r-1}, NaN if there is none;  PEAK the maximum of x;  PEAK_ROW the smallest r attaining it;  HIGH_COUNT the runs above
   hi (a run starts at a valid row with x_r > hi that has no pair, or whose x_{r-1} <= hi);  HIGH_DURATION rows with x_r
   > hi / runs, NaN with no run;  LOW_COUNT, LOW_DURATION the same with x_r < lo.
Rules: m == 0 -> twelve NaN; a valid row with a value that is not finite (or a sum of x that overflows) -> twelve NaN for
that (window, column); no thresholds, or a NaN threshold -> NaN in the two columns it feeds.

smart_signatures (csrc/smart_signatures.hip) forms, per (window, sample) and in row order, sum x, sum (x - f), over the
pairs sum |x_r - x_{r-1}| and sum x_r, the five moments Sa = sum ua, Sb = sum ub, Saa, Sbb, Sab of ua = x_{r-1} - sa,
ub = x_r - sb, and over the falling pairs sum (ln x_r - ln x_{r-1}).  var = S2 - S1^2 / p loses digits as
kappa = 1 + ((s - mean) / std)^2 grows: a constant that is a member of the list it centres keeps kappa <= about p, a value
from outside it (the window's first valid row is never an x_r; before a gap it is in neither list) does not.

`truth`    the columns in integers over one power of two (fractions.Fraction at the end), each rounded once.
`bounds`   per entry what the kernel's form, its additions in ANY order, may differ from `truth` by (derived below).
`emulate`  the kernel's sums in float64 in one of three orders, about the shifts of one of two forms: 'shared' (both lists
           about the window's first valid value) and 'per_list' (each list about its own member of the first pair)."""
import math
from fractions import Fraction

import numpy as np

from oracle.exact import U, SLACK, gamma, mul, sqrt

NAMES = ['MEAN', 'BFI', 'FLASHINESS', 'AC1', 'RLD', 'RECESSION', 'PEAK', 'PEAK_ROW', 'HIGH_COUNT', 'HIGH_DURATION',
         'LOW_COUNT', 'LOW_DURATION']
(MEAN, BFI, FLASHINESS, AC1, RLD, RECESSION, PEAK, PEAK_ROW, HIGH_COUNT, HIGH_DURATION, LOW_COUNT,
 LOW_DURATION) = range(12)
PAIR_COLUMNS = [FLASHINESS, AC1, RLD, RECESSION]         # NaN wherever there is no pair


def statement(sim, obs=None, win=None, n_windows=1, alpha=0.925, pulse=None):
    """sim [R, n], obs [R] or None (NaN = missing), win [R] or None, pulse [W, 2] (lo, hi) or None -> [W, 12, n].  One
    Python loop over the rows; the n columns of a row are carried side by side as numpy vectors."""
    sim = np.asarray(sim, dtype=np.float64)
    R, n = sim.shape
    out = np.full((n_windows, 12, n), np.nan)
    nan = np.full(n, np.nan)
    for w in range(n_windows):
        valid = [(win is None or win[r] == w) and (obs is None or not np.isnan(obs[r])) for r in range(R)]
        lo, hi = (np.nan, np.nan) if pulse is None else (float(pulse[w][0]), float(pulse[w][1]))
        m = p = 0
        sum_x, sum_base, f = np.zeros(n), np.zeros(n), np.zeros(n)
        num, den = np.zeros(n), np.zeros(n)
        first, second = [], []                                  # the pair lists of AC1
        rises, limbs, was_rising = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
        rec_sum, rec_n = np.zeros(n), np.zeros(n)
        peak, peak_row = np.full(n, -np.inf), np.zeros(n)
        hi_runs, hi_rows, lo_runs, lo_rows = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        with np.errstate(all='ignore'):
            for r in range(R):
                if not valid[r]:
                    continue
                x = sim[r]
                m += 1
                sum_x = sum_x + x
                if r >= 1 and valid[r - 1]:
                    before = sim[r - 1]
                    p += 1
                    f = np.minimum(np.maximum(alpha * f + (1.0 + alpha) / 2.0 * (x - before), 0.0), x)
                    num = num + np.abs(x - before)
                    den = den + x
                    first.append(before)
                    second.append(x)
                    rising = x > before
                    rises = rises + rising
                    limbs = limbs + (rising & ~was_rising)
                    was_rising = rising
                    falling = (0.0 < x) & (x < before)
                    rec_sum = rec_sum + np.where(falling, np.log(np.where(falling, x / before, 1.0)), 0.0)
                    rec_n = rec_n + falling
                    hi_runs = hi_runs + ((x > hi) & (before <= hi))
                    lo_runs = lo_runs + ((x < lo) & (before >= lo))
                else:
                    f = np.zeros(n)
                    was_rising = np.zeros(n, dtype=bool)
                    hi_runs = hi_runs + (x > hi)
                    lo_runs = lo_runs + (x < lo)
                sum_base = sum_base + (x - f)
                top = x > peak
                peak_row = np.where(top, float(r), peak_row)
                peak = np.where(top, x, peak)
                hi_rows = hi_rows + (x > hi)
                lo_rows = lo_rows + (x < lo)
            if m == 0:
                continue
            o = out[w]
            o[MEAN] = sum_x / m
            o[BFI] = np.where(sum_x == 0.0, np.nan, sum_base / sum_x)
            o[FLASHINESS] = nan if p == 0 else np.where(den == 0.0, np.nan, num / den)
            if p >= 2:
                a, b = np.array(first), np.array(second)
                a, b = a - a.mean(axis=0), b - b.mean(axis=0)
                va, vb, cov = (a * a).sum(axis=0), (b * b).sum(axis=0), (a * b).sum(axis=0)
                o[AC1] = np.where((va > 0.0) & (vb > 0.0), cov / np.sqrt(va * vb), np.nan)
            o[RLD] = np.where(rises > 0, limbs / rises, np.nan)
            o[RECESSION] = np.where(rec_n > 0, rec_sum / rec_n, np.nan)
            o[PEAK], o[PEAK_ROW] = peak, peak_row
            if not np.isnan(hi):
                o[HIGH_COUNT], o[HIGH_DURATION] = hi_runs, np.where(hi_runs > 0, hi_rows / hi_runs, np.nan)
            if not np.isnan(lo):
                o[LOW_COUNT], o[LOW_DURATION] = lo_runs, np.where(lo_runs > 0, lo_rows / lo_runs, np.nan)
            o[:, ~np.isfinite(sum_x)] = np.nan
    return out


X8 = [1.0, 3.0, 4.0, 2.0, 9.0, 4.0, 2.0, 3.0]       # the series the host tests work by hand
ROUNDED = [MEAN, BFI, FLASHINESS, AC1, RECESSION]                  # sums of roundings: a bound that is not zero
INTEGER = [RLD, PEAK, PEAK_ROW, HIGH_COUNT, HIGH_DURATION, LOW_COUNT, LOW_DURATION]    # a value, or one IEEE quotient of counts
RELATIVE = [MEAN, BFI, FLASHINESS, RLD, RECESSION, HIGH_DURATION, LOW_DURATION]
FORMS = ('shared', 'per_list')
ORDERS = ('forward', 'reversed', 'pairwise')


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
    the definition of `statement` on the exact values of the doubles.  MEAN, FLASHINESS, RLD, both
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
            Sx, dSx = t['x'].sum(axis=0), gamma(m - 1) * np.abs(t['x']).sum(axis=0)
            raw[MEAN] = dSx / m + U * np.abs(want[w, MEAN])
            dSb = t['e'].sum(axis=0) + gamma(m + 1) * np.abs(t['base']).sum(axis=0)
            b = np.abs(want[w, BFI])
            raw[BFI] = np.where(dSx < np.abs(Sx), (dSb + b * dSx) / (np.abs(Sx) - dSx), np.inf) + U * b
            if p > 0:
                den, F = t['pair'].sum(axis=0), np.abs(want[w, FLASHINESS])
                dnum, dden = gamma(p + 1) * t['abs'].sum(axis=0), gamma(p - 1) * np.abs(t['pair']).sum(axis=0)
                raw[FLASHINESS] = np.where(dden < np.abs(den), (dnum + F * dden) / (np.abs(den) - dden), np.inf) + U * F
                k = np.maximum(t['falling'].sum(axis=0), 1)
                mag = np.abs(t['rec']).sum(axis=0)
                dsum = 2 * U * t['logmag'].sum(axis=0) + 2 * U * mag + gamma(k - 1) * mag
                own = U * t['steep'].sum(axis=0) + 2 * U * mag
                raw[RECESSION] = (dsum + own) / k + 2 * U * np.abs(want[w, RECESSION])
            if p >= 2:
                ua, ub, q = t['ua'], t['ub'], float(p)
                dSa, dSb_ = gamma(p + 1) * np.abs(ua).sum(axis=0), gamma(p + 1) * np.abs(ub).sum(axis=0)
                A, B = np.abs(ua.sum(axis=0)) + dSa, np.abs(ub.sum(axis=0)) + dSb_
                dSaa, dSbb = gamma(p + 3) * (ua * ua).sum(axis=0), gamma(p + 3) * (ub * ub).sum(axis=0)
                dSab = gamma(p + 3) * np.abs(ua * ub).sum(axis=0)
                va, vb, cov = centred[w]
                dva = dSaa + (2 * A * dSa + dSa * dSa) / q + gamma(2) * (A + dSa) ** 2 / q
                dvb = dSbb + (2 * B * dSb_ + dSb_ * dSb_) / q + gamma(2) * (B + dSb_) ** 2 / q
                dcov = dSab + (A * dSb_ + B * dSa + dSa * dSb_) / q + gamma(2) * (A + dSa) * (B + dSb_) / q
                dva, dvb, dcov = dva + U * (va + dva), dvb + U * (vb + dvb), dcov + U * (np.abs(cov) + dcov)
                D = np.sqrt(va * vb)
                rD = mul(sqrt(mul(mul(dva / va, dvb / vb), U)), U)
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
