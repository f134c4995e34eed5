"""Evaluation windows over the report stamps: which report step belongs to which hydrological year, season, month or
period of a split-sample test.  Pure host code; the ids go to engine.objective_functions_windows
(MonteCarlo.window_objective_functions), which scores every sample per window on the GPU, and to engine.flow_duration
(MonteCarlo.flow_duration_curves), which sorts every sample's flows per window there, and to engine.signatures
(MonteCarlo.hydrological_signatures), which walks every sample's flows of a window in time order there.
"""
from bisect import bisect_right
from datetime import datetime

import numpy as np

OBJ_FN_NAMES = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE']      # the seven columns of a window
SEASONS = ['DJF', 'MAM', 'JJA', 'SON']
_SEASON_OF_MONTH = [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 0]                      # January .. December
_BY = ('all', 'year', 'hydro_year', 'season', 'month', 'split')
_STAMP = '%Y-%m-%d %H:%M:%S'


def evaluation_windows(stamps, by='hydro_year', start_month=10, split=None):
    """-> (ids: int32 ndarray [R], labels: list of str) for the R report stamps (datetimes).

    by='all'         one window, 'all'
    by='year'        the calendar year of the stamp; labelled with the year
    by='hydro_year'  the twelve months from `start_month`; labelled with the calendar year in which it ENDS
    by='season'      DJF, MAM, JJA, SON, in that order (the ids interleave along the run)
    by='month'       '01' .. '12'
    by='split'       `split` is one datetime or an ascending list of them: window k holds the stamps in
                     [split[k-1], split[k]), open at both ends of the run; labelled '<first stamp>..<last stamp>'

    Only windows that occur are numbered, in ascending label order (seasons in the order above, periods in time).  A
    stamp decides its window as it is written in the flow files: nothing is shifted."""
    if by not in _BY:
        raise Exception("The kind of evaluation windows '{}' is not recognised. Please choose one of: {}."
                        .format(by, ', '.join(_BY)))
    stamps = list(stamps)
    if len(stamps) == 0:
        raise Exception("Evaluation windows need at least one report stamp.")
    if not (isinstance(start_month, (int, np.integer)) and 1 <= start_month <= 12):
        raise Exception("The first month of the hydrological year must be between 1 and 12, not {}.".format(start_month))
    if by == 'all':
        keys, label = [0] * len(stamps), lambda k: 'all'
    elif by == 'year':
        keys, label = [s.year for s in stamps], str
    elif by == 'hydro_year':
        keys = [s.year + (1 if start_month > 1 and s.month >= start_month else 0) for s in stamps]
        label = str
    elif by == 'season':
        keys, label = [_SEASON_OF_MONTH[s.month - 1] for s in stamps], lambda k: SEASONS[k]
    elif by == 'month':
        keys, label = [s.month for s in stamps], lambda k: '%02d' % k
    else:
        if split is None:
            raise Exception("Evaluation windows by 'split' need the date(s) to split at (split=...).")
        bounds = [split] if isinstance(split, datetime) else list(split)
        if len(bounds) == 0:
            raise Exception("Evaluation windows by 'split' need the date(s) to split at (split=...).")
        if any(b <= a for a, b in zip(bounds, bounds[1:])):
            raise Exception("The dates to split the evaluation windows at must be in ascending order.")
        keys = [bisect_right(bounds, s) for s in stamps]
        ends = {}
        for k, s in zip(keys, stamps):
            lo, hi = ends.get(k, (s, s))
            ends[k] = (min(lo, s), max(hi, s))

        def label(k):
            return '{}..{}'.format(ends[k][0].strftime(_STAMP), ends[k][1].strftime(_STAMP))
    present = sorted(set(keys))
    number = {k: i for i, k in enumerate(present)}
    return np.array([number[k] for k in keys], dtype=np.int32), [label(k) for k in present]


def header_columns(labels, transform='none', names=OBJ_FN_NAMES):
    """The column names of a `.windows` file: NSE@<label>, KGE@<label>, ... window by window, with ':<transform>' behind
    the function's name when the flows were transformed (NSE:log@1994)."""
    tag = '' if transform == 'none' else ':' + transform
    return ['{}{}@{}'.format(name, tag, label) for label in labels for name in names]


def header_line(labels, transform='none', names=OBJ_FN_NAMES):
    return ','.join(header_columns(labels, transform, names)) + '\n'


def default_eps(transform, obs):
    """0 for 'none' and 'sqrt'; for 'log' and 'inverse' one hundredth of the mean of the non-missing observations
    (Pushpalatha et al. 2012, J. Hydrol. 420-421)."""
    if transform in ('none', 'sqrt'):
        return 0.0
    obs = np.asarray(obs, dtype=np.float64)
    return float(np.mean(obs[~np.isnan(obs)])) / 100.0


class WindowObjectives(object):
    """What MonteCarlo.window_objective_functions returns: `names` (the seven objective functions), `labels` (one per
    window), `transform`, `eps` (the value used), `values` (numpy [W, N, 7] float64, in the order of the sample's
    rows), `device_values` (the same as a device tensor, or None for an empty sample: device_values[w][:, [0]] goes to
    selection.condition_mask as it is) and `file` (the path written, or None)."""

    def __init__(self, labels, transform, eps, values, device_values, file=None):
        self.names = list(OBJ_FN_NAMES)
        self.labels, self.transform, self.eps = list(labels), transform, eps
        self.values, self.device_values, self.file = values, device_values, file


# ---- flow duration curves -------------------------------------------------------------------------------------------
def non_exceedance(exceedance):
    """Exceedance probabilities p (the hydrologist's axis of a flow duration curve: Q1 is a high flow) -> the
    non-exceedance probabilities q = 1 - p the engine takes, as a float64 array.  Each p must lie in [0, 1]."""
    p = np.atleast_1d(np.asarray(exceedance, dtype=np.float64))
    if p.ndim != 1 or p.size == 0 or not np.all((p >= 0.0) & (p <= 1.0)):
        raise Exception("The exceedance probabilities of a flow duration curve must lie between 0 and 1.")
    return 1.0 - p


def observed_duration(obs, ids, n_windows, q):
    """The rule of engine.flow_duration applied to the observations with numpy -> [W, K]: per window the
    max(1, ceil(q * m))-th smallest of its m non-missing observations, NaN for a window without any."""
    obs, ids = np.asarray(obs, dtype=np.float64), np.asarray(ids)
    out = np.full((n_windows, len(q)), np.nan)
    for w in range(n_windows):
        x = np.sort(obs[(ids == w) & ~np.isnan(obs)])
        if x.size:
            out[w] = [x[max(1, int(np.ceil(qk * x.size))) - 1] for qk in q]
    return out


def fdc_header_line(exceedance, labels, transform='none'):
    """The header of a `.fdc` file: Q<p>@<label> for every probability, window by window, then the columns of a
    `.windows` file (NSE@<label>, ... with ':<transform>' behind the function's name when the flows were transformed)."""
    quant = ['Q{:g}@{}'.format(p, label) for label in labels for p in exceedance]
    return ','.join(quant + header_columns(labels, transform)) + '\n'


class FlowDuration(object):
    """What MonteCarlo.flow_duration_curves returns: `exceedance` (the K probabilities asked for), `labels` (one per
    window), `curves` (numpy [W, K, N]: the flow of every sample exceeded with that probability), `observed` ([W, K], the
    same rule on the observations), `names` / `values` (numpy [W, N, 7]: the objective functions of the sorted simulation
    against the sorted observations over `segment`, on `transform`ed flows with `eps`), `device_values` (the same as a
    device tensor, or None for an empty sample: device_values[w][:, [0]] goes to selection.condition_mask as it is) and
    `file` (the path written, or None)."""

    def __init__(self, exceedance, labels, curves, observed, transform, eps, segment, values, device_values, file=None):
        self.names = list(OBJ_FN_NAMES)
        self.exceedance, self.labels = [float(p) for p in exceedance], list(labels)
        self.curves, self.observed = curves, observed
        self.transform, self.eps, self.segment = transform, eps, (float(segment[0]), float(segment[1]))
        self.values, self.device_values, self.file = values, device_values, file


# ---- score uncertainty ----------------------------------------------------------------------------------------------
def eligible_windows(obs, ids, n_windows, min_steps=None):
    """Which windows take part in MonteCarlo.score_uncertainty -> (bool mask [W], the threshold used): those with at least
    `min_steps` observed (non-missing) report steps.  min_steps=None: 1 if there are fewer than 3 windows, otherwise 90 %
    of the longest window's observed count -- the "complete years" rule of Clark et al. 2021 (Water Resour. Res. 57)."""
    obs, ids = np.asarray(obs, dtype=np.float64), np.asarray(ids)
    observed = np.array([int(np.sum((ids == w) & ~np.isnan(obs))) for w in range(n_windows)], dtype=np.int64)
    if min_steps is None:
        min_steps = 1 if n_windows < 3 else 0.9 * float(observed.max())
    return observed >= min_steps, float(min_steps)


def jackknife_factor(n_eligible):
    """se_jack = jackknife_factor(E) x std(ddof=1) of the E leave-one-out values = sqrt((E - 1) / E x sum (t_i - mean)^2)"""
    E = float(n_eligible)
    return np.sqrt((E - 1.0) ** 2 / E)


def uncertainty_header_columns(quantiles, names=OBJ_FN_NAMES):
    """The column names of a `.uncertainty` file, score by score: NSE, NSE_se, NSE_jse, NSE_q0.05, ..."""
    return [col for name in names for col in
            [name, name + '_se', name + '_jse'] + ['{}_q{:g}'.format(name, q) for q in quantiles]]


def uncertainty_header_line(quantiles, names=OBJ_FN_NAMES):
    return ','.join(uncertainty_header_columns(quantiles, names)) + '\n'


class ScoreUncertainty(object):
    """What MonteCarlo.score_uncertainty returns: `names` (the seven objective functions), `labels` (one per window),
    `eligible` (bool [W]: the windows that were resampled), `min_steps`, `transform`, `eps`, `probs` (the K quantile
    probabilities), `point` (numpy [N, 7], every eligible window once), `mean` and `se_boot` ([7, N]: mean and standard
    deviation, ddof = 1, over the bootstrap replicates), `quantiles` ([7, K, N]), `se_jack` ([7, N]: the jackknife
    standard error sqrt((E - 1) / E x sum (t_i - mean)^2) over the E leave-one-window-out values), `device_stats` (the
    bootstrap call's [7, 2 + K, N] device tensor, or None for an empty sample: device_stats[s, c] is a contiguous [N]
    vector that goes to selection.condition_mask / pareto_rows / Pareto(extra=) as it is), `path` (the file written, or
    None), `seed` and `resamples`."""

    def __init__(self, labels, eligible, min_steps, transform, eps, probs, point, mean, se_boot, quantiles, se_jack,
                 device_stats, path, seed, resamples):
        self.names = list(OBJ_FN_NAMES)
        self.labels, self.eligible, self.min_steps = list(labels), np.asarray(eligible, dtype=bool), min_steps
        self.transform, self.eps, self.probs = transform, eps, [float(q) for q in probs]
        self.point, self.mean, self.se_boot, self.quantiles, self.se_jack = point, mean, se_boot, quantiles, se_jack
        self.device_stats, self.path, self.seed, self.resamples = device_stats, path, seed, resamples


# ---- hydrological signatures ----------------------------------------------------------------------------------------
from ._lib import SIGNATURE_NAMES      # noqa: E402 -- the twelve columns of a window, SMART_SIG_* (names only: no library is loaded)


def default_alpha(report_days):
    """The Lyne-Hollick filter parameter of a report step of `report_days` days: 0.925 for daily means (Nathan and
    McMahon 1990, Water Resour. Res. 26), the same decay per day for any other step."""
    return 0.925 ** float(report_days)


def pulse_thresholds(obs, ids, n_windows, high=3.0, low=0.2):
    """The default pulse thresholds of MonteCarlo.hydrological_signatures -> [W, 2] float64, (lo, hi) per window from the
    window's non-missing observations: hi = high x their median, lo = low x their mean; NaN for a window without any."""
    obs, ids = np.asarray(obs, dtype=np.float64), np.asarray(ids)
    out = np.full((n_windows, 2), np.nan)
    for w in range(n_windows):
        x = obs[(ids == w) & ~np.isnan(obs)]
        if x.size:
            out[w] = (float(low) * float(np.mean(x)), float(high) * float(np.median(x)))
    return out


def signatures_header_line(labels):
    """The header of a `.signatures` file: MEAN@<label>, BFI@<label>, ... window by window."""
    return header_line(labels, names=SIGNATURE_NAMES)


class Signatures(object):
    """What MonteCarlo.hydrological_signatures returns: `names` (the twelve signatures), `labels` (one per window),
    `alpha` (the filter parameter used), `thresholds` ([W, 2]: the (lo, hi) of the pulse columns), `values` (numpy
    [W, 12, N] float64, in the order of the sample's rows), `device_values` (the same as a device tensor, or None for an
    empty sample: device_values[w, c] is a contiguous [N] vector that goes to selection.pareto_rows / Pareto(extra=) as
    it is), `observed` ([W, 12]: the same signatures of the observations, by the same kernel; NaN for an empty sample,
    which launches nothing) and `path` (the file written, or None)."""

    def __init__(self, labels, alpha, thresholds, values, device_values, observed, path=None):
        self.names = list(SIGNATURE_NAMES)
        self.labels, self.alpha = list(labels), float(alpha)
        self.thresholds = np.asarray(thresholds, dtype=np.float64)
        self.values, self.device_values, self.observed, self.path = values, device_values, observed, path

    def relative_error(self):
        """(values - observed) / |observed| -> [W, 12, N]: the signed relative error of every signature of every sample
        (PEAK_ROW included: its difference is the timing error in report steps, which a caller reads from
        values - observed instead)."""
        with np.errstate(all='ignore'):
            ref = self.observed[:, :, None]
            return (self.values - ref) / np.abs(ref)
