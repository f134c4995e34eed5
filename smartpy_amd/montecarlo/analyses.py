"""The analyses of the stored discharge matrix that every Monte-Carlo workflow offers (no counterpart in the reference).

`Analyses` is a plain class of methods; montecarlo.MonteCarlo inherits it, and LHS, GLUE, Sobol, DEMCz, Best, Total and
Pareto with it.  Each method makes one launch of its own over the sample at hand with the [R, N] matrix kept on the device
(_launch_stored), hands the matrix to one entry of smartpy_amd.engine where it lies, and brings back the small result --
and with write=True a side file beside the sampling database.  What the methods share is written once, here: the preamble
of a windowed analysis (_windowed), the side-file block (_write_side), the likelihood-to-weights rule (likelihood_weights:
GLUE's prediction bounds go through it as well) and the containment of the observations in a band (containment).  The
object they are mixed into brings the sample (_sample, _launch_rows), the model, the objective functions of a finished
run() and db_file.
"""
import numpy as np
import torch

from .. import _lib, engine, errormodel, identifiability as ident, pawn, windows as swin
from .. import distributed as sdist
from ..engine import SmartEngineError
from ..verification import EnsembleVerification
from .selection import write_float32_table

#: the refusals of likelihood_weights as the analyses of this class word them (GLUE has its own: glue.py)
ROW_WEIGHT_TEXTS = {
    'name': "{who}: the likelihood '{name}' is not one of the objective functions of a finished run() of this object "
            "({names}).",
    'shape': "{who}: the likelihood array has shape {shape} where one value per row of the sample ({n}) is expected.",
    'values': "{who}: {bad} of the {n} likelihood values are negative or not finite: they cannot be used as weights.",
}


def likelihood_weights(likelihood, n, names, table, texts, **said):
    """None (equal weights) | the name of an objective function (its column of `table` [n, len(names)]; a table that is
    None or of another length has no column for any name) | an array [n] -> float64 [n] or None; negative or non-finite
    weights raise, nothing is clipped.  texts: the caller's wording of the three refusals ('name', 'shape', 'values'),
    formatted with name / names / shape / n / bad and whatever else the caller says (`who`)."""
    if likelihood is None:
        return None
    if isinstance(likelihood, str):
        if likelihood not in names or table is None or table.shape[0] != n:
            raise Exception(texts['name'].format(name=likelihood, names=', '.join(names), **said))
        weights = np.asarray(table[:, names.index(likelihood)], dtype=np.float64)
    else:
        weights = np.asarray(likelihood, dtype=np.float64)
        if weights.shape != (n,):
            raise Exception(texts['shape'].format(shape=weights.shape, n=n, **said))
    bad = int(np.count_nonzero(~(np.isfinite(weights) & (weights >= 0.0))))
    if bad:
        raise Exception(texts['values'].format(bad=bad, n=n, **said))
    return weights


def containment(band, obs):
    """The share of the non-missing observations o_r (device tensor [R], or None) with band[0, r] <= o_r <= band[-1, r]
    (band: device tensor [K, R]); NaN without observations."""
    if obs is None:
        return float('nan')
    there = ~torch.isnan(obs)
    hit = there & (band[0] <= obs) & (obs <= band[-1])
    return float(hit.sum()) / float(there.sum()) if int(there.sum()) > 0 else float('nan')


class Analyses(object):
    # ---- what the analyses of the stored discharge matrix share (this class, GLUE, Sobol, DEMCz) --------------
    @staticmethod
    def _check_transform(transform):
        if transform not in list(_lib.TRANSFORMS):
            raise Exception("The flow transform '{}' is not recognised. Please choose one of: {}."
                            .format(transform, ', '.join(_lib.TRANSFORMS)))

    def _resolve_windows(self, windows, start_month, split):
        """a `by` word of windows.evaluation_windows over the report stamps, or a ready (ids, labels) pair -> (ids, labels)"""
        if isinstance(windows, str):
            return swin.evaluation_windows(self.model.timeseries_report[1:], by=windows, start_month=start_month,
                                           split=split)
        ids, labels = windows
        return np.asarray(ids), list(labels)

    def _check_observations(self):
        if self.model.nd_flow is None:
            raise Exception("The observation array does not exist. Please make sure that a value is assigned "
                            "to the gauged_area_m2 attribute of your SMART class instance.")

    def _windowed(self, windows, start_month, split, transform=None, eps=None):
        """The preamble of a windowed analysis, its refusals in this order: the transform (None: the analysis has none),
        the windows, the observations -> (ids, labels, W, eps), eps=None resolved to the default of the transform"""
        if transform is not None:
            self._check_transform(transform)
        ids, labels = self._resolve_windows(windows, start_month, split)
        self._check_observations()
        if eps is None and transform is not None:
            eps = swin.default_eps(transform, self.model.nd_flow)
        return ids, labels, len(labels), eps

    def _launch_stored(self):
        """One launch over the sample with the [R, N] discharge matrix kept on the device -> (the launch's result, the
        observations it has left on the device, or None)"""
        out = self.model.simulate_ensemble(self._launch_rows(), save_discharge=True, math_mode=self.math_mode)
        return out, self.model._device_cache[2]

    @staticmethod
    def _writes(write):
        """Whether this process writes the side file of a call: write=True, and under torch.distributed rank 0 alone."""
        return write and sdist.rank_world()[0] == 0

    def _side_file(self, suffix):
        """`<out>/<catchment>.SMART.<func><suffix>`: beside the sampling database, whatever its format."""
        return (self.db_file[:-3] if self.db_file.endswith('.nc') else self.db_file) + suffix

    def _write_side(self, write, suffix, writer):
        """The side file of a call: where this process writes (_writes), writer(path) with path = _side_file(suffix) ->
        the path written, or None"""
        if not self._writes(write):
            return None
        path = self._side_file(suffix)
        writer(path)
        return path

    # ---- split-sample and low-flow scores -----------------------------------------------------------------
    def window_objective_functions(self, windows='hydro_year', transform='none', eps=None, start_month=10, split=None,
                                   write=False):
        """NSE, KGE, KGEc, KGEa, KGEb, PBias and RMSE of every row of the sample PER WINDOW of report steps (per
        hydrological year, season, period of a split-sample test ...) and on transformed flows ('sqrt', 'log' = ln(Q +
        eps), 'inverse' = 1 / (Q + eps): low-flow scores).  windows: a `by` word of windows.evaluation_windows (with
        start_month / split) over the report stamps, or a ready (ids, labels) pair.  eps=None: 0 for 'none' and 'sqrt',
        one hundredth of the mean observation for 'log' and 'inverse'; the value used is on the result.  One launch of
        its own over the sample; the [R, N] matrix stays on the device and only [W, N, 7] comes back.  write=True also
        writes `<out>/<catchment>.SMART.<func>.windows` (one line per sample in the sample's order, the float32 '%.6e'
        of the sampling database; header NSE@<label>,KGE@<label>,... window by window).  Under torch.distributed every
        rank that calls this computes all rows itself (no collective); rank 0 alone writes.  -> WindowObjectives"""
        ids, labels, W, eps = self._windowed(windows, start_month, split, transform, eps)
        if self._sample.shape[0] == 0:      # e.g. GLUE with no behavioural set: nothing to launch
            on_device, values = None, np.empty((W, 0, len(swin.OBJ_FN_NAMES)))
        else:
            out, obs = self._launch_stored()
            on_device = engine.objective_functions_windows(out.discharge_report_major, obs, ids, n_windows=W,
                                                           transform=transform, eps=eps)
            values = on_device.cpu().numpy()
        path = self._write_side(write, '.windows', lambda path: _write_windows_file(path, labels, transform, values))
        return swin.WindowObjectives(labels, transform, float(eps), values, on_device, path)

    @property
    def windows_file(self):
        """`<out>/<catchment>.SMART.<func>.windows`: beside the sampling database, whatever its format."""
        return self._side_file('.windows')

    # ---- flow duration curves -----------------------------------------------------------------------------
    def flow_duration_curves(self, exceedance=(0.01, 0.05, 0.1, 0.2, 0.5, 0.8, 0.9, 0.95, 0.99), windows='all',
                             transform='none', eps=None, segment=(0.0, 1.0), start_month=10, split=None, write=False):
        """The flow duration curve of every row of the sample PER WINDOW of report steps: the flow exceeded with
        probability p, for each p of `exceedance` (at most 16), and the objective functions of the curve -- NSE, KGE,
        KGEc, KGEa, KGEb, PBias, RMSE of the sorted simulation against the sorted observations, paired by rank, over the
        `segment` (lo, hi) of the ascending ranks ((0, 1): the whole curve; (0.98, 1): the top 2 %, whose PBias is a
        high-flow-volume bias; (0, 0.3) with transform='log': a low-flow bias).  An EXCEEDANCE probability p is turned
        into the non-exceedance probability q = 1 - p here, on the host; the engine returns the max(1, ceil(q * m))-th
        smallest of the window's m flows (numpy's 'inverted_cdf': a simulated value, nothing interpolated).  Report steps
        without an observation are left out of both series.  windows / start_month / split / transform / eps as for
        window_objective_functions.  One launch of its own over the sample; the [R, N] matrix stays on the device and
        only [W, K, N] and [W, N, 7] come back.  write=True also writes `<out>/<catchment>.SMART.<func>.fdc` (one line
        per sample in the sample's order, the float32 '%.6e' of the sampling database; header Q<p>@<label>,... window by
        window, then NSE@<label>,KGE@<label>,...).  Under torch.distributed every rank that calls this computes all rows
        itself (no collective); rank 0 alone writes.  -> FlowDuration"""
        self._check_transform(transform)        # (ahead of _windowed: a transform is refused before a probability is)
        exceedance = [float(p) for p in np.atleast_1d(np.asarray(exceedance, dtype=np.float64))]
        q = swin.non_exceedance(exceedance)
        ids, labels, W, eps = self._windowed(windows, start_month, split, transform, eps)
        if self._sample.shape[0] == 0:      # e.g. GLUE with no behavioural set: nothing to launch
            on_device, curves = None, np.empty((W, len(q), 0))
            values = np.empty((W, 0, len(swin.OBJ_FN_NAMES)))
        else:
            out, obs = self._launch_stored()
            quant, on_device = engine.flow_duration(out.discharge_report_major, q, obs=obs, windows=ids, n_windows=W,
                                                    transform=transform, eps=eps, segment=segment, objfn=True)
            curves, values = quant.cpu().numpy(), on_device.cpu().numpy()
        observed = swin.observed_duration(self.model.nd_flow, ids, W, q)
        path = self._write_side(write, '.fdc',
                                lambda path: _write_fdc_file(path, exceedance, labels, transform, curves, values))
        return swin.FlowDuration(exceedance, labels, curves, observed, transform, float(eps), segment, values, on_device,
                                 path)

    @property
    def fdc_file(self):
        """`<out>/<catchment>.SMART.<func>.fdc`: beside the sampling database, whatever its format."""
        return self._side_file('.fdc')

    # ---- hydrological signatures -------------------------------------------------------------------------
    def hydrological_signatures(self, windows='all', alpha=None, high=3.0, low=0.2, thresholds=None, start_month=10,
                                split=None, write=False):
        """The hydrological signatures of every row of the sample PER WINDOW of report steps -- the scores that depend on
        the ORDER of the report steps: MEAN, BFI (baseflow index, one forward pass of the Lyne-Hollick filter),
        FLASHINESS (Richards-Baker), AC1 (lag-1 autocorrelation), RLD (rising limb density), RECESSION (mean ln(Q_r /
        Q_r-1) of the falling steps), PEAK and PEAK_ROW (the report step of the peak), HIGH_COUNT / HIGH_DURATION and
        LOW_COUNT / LOW_DURATION (number and mean length of the runs above `hi` and below `lo`) -- and the same twelve
        of the observations, by the same kernel.  Report steps without an observation are left out and break the
        series there.  alpha=None: 0.925 ** (report step in days), 0.925 for daily means; the value used is on the
        result.  The thresholds of a window default to hi = high x the median and lo = low x the mean of its non-missing
        observations; a ready [W, 2] array of (lo, hi) passed as thresholds= overrides them.  windows / start_month /
        split as for window_objective_functions.  One launch of its own over the sample; the [R, N] matrix stays on
        the device and only [W, 12, N] comes back.  write=True also writes `<out>/<catchment>.SMART.<func>.signatures`
        (one line per sample in the sample's order, the float32 '%.6e' of the sampling database; header MEAN@<label>,
        BFI@<label>,... window by window).  Under torch.distributed every rank that calls this computes all rows itself
        (no collective); rank 0 alone writes.  -> windows.Signatures"""
        ids, labels, W, _ = self._windowed(windows, start_month, split)
        if alpha is None:
            alpha = swin.default_alpha(self.model.delta_save.total_seconds() / 86400.0)
        obs = np.asarray(self.model.nd_flow, dtype=np.float64)
        if thresholds is None:
            thresholds = swin.pulse_thresholds(obs, ids, W, high=high, low=low)
        thresholds = np.ascontiguousarray(thresholds, dtype=np.float64)
        if thresholds.shape != (W, 2):
            raise Exception("The pulse thresholds must be (lo, hi) per window, shape ({}, 2), not {}."
                            .format(W, thresholds.shape))
        if self._sample.shape[0] == 0:      # e.g. GLUE with no behavioural set: nothing to launch
            on_device, values = None, np.empty((W, len(swin.SIGNATURE_NAMES), 0))
            observed = np.full((W, len(swin.SIGNATURE_NAMES)), np.nan)
        else:
            out, on_obs = self._launch_stored()
            on_device = engine.signatures(out.discharge_report_major, obs=on_obs, windows=ids, n_windows=W, alpha=alpha,
                                          thresholds=thresholds)
            values = on_device.cpu().numpy()
            # the observations as an [R, 1] matrix under the same mask: one definition serves both
            observed = engine.signatures(obs.reshape(-1, 1), obs=obs, windows=ids, n_windows=W, alpha=alpha,
                                         thresholds=thresholds).cpu().numpy()[:, :, 0]
        path = self._write_side(write, '.signatures', lambda path: _write_signatures_file(path, labels, values))
        return swin.Signatures(labels, alpha, thresholds, values, on_device, observed, path)

    @property
    def signatures_file(self):
        """`<out>/<catchment>.SMART.<func>.signatures`: beside the sampling database, whatever its format."""
        return self._side_file('.signatures')

    # ---- score uncertainty ---------------------------------------------------------------------------------
    def score_uncertainty(self, windows='hydro_year', resamples=1000, seed=None, quantiles=(0.05, 0.5, 0.95),
                          transform='none', eps=None, min_steps=None, start_month=10, split=None, write=False):
        """How much of NSE, KGE, KGEc, KGEa, KGEb, PBias and RMSE of every row of the sample is sampling noise of the
        windows that happen to lie in the evaluation period: a block bootstrap over the windows (hydrological years)
        with a leave-one-window-out jackknife, after Clark et al. 2021 (Water Resour. Res. 57).  The eligible windows
        are those with at least `min_steps` observed report steps (None: 1 with fewer than 3 windows, else 90 % of the
        longest window's observed count); report steps of the other windows take no part, in the point value either;
        fewer than three eligible windows is an error.  Each of `resamples` replicates draws as many windows as are
        eligible, with replacement (engine.bootstrap_counts with `seed`); the scores of a replicate are those of its
        report steps pooled.  -> windows.ScoreUncertainty: point value, mean, standard error (se_boot) and `quantiles`
        (numpy 'inverted_cdf', at most 16) of the replicates, and the jackknife standard error (se_jack).  windows /
        start_month / split / transform / eps as for window_objective_functions.  One launch of its own over the sample,
        then two calls on the [R, N] matrix where it lies, which read it once each.  write=True also writes
        `<out>/<catchment>.SMART.<func>.uncertainty` (one line per sample in the sample's order, the float32 '%.6e' of
        the sampling database; header NSE,NSE_se,NSE_jse,NSE_q0.05,... score by score).  Under torch.distributed every
        rank that calls this computes all rows itself (no collective); rank 0 alone writes."""
        ids, labels, W, eps = self._windowed(windows, start_month, split, transform, eps)
        n = self._sample.shape[0]
        probs = [float(q) for q in np.atleast_1d(np.asarray(quantiles, dtype=np.float64))]
        eligible, min_steps = swin.eligible_windows(self.model.nd_flow, ids, W, min_steps)
        E = int(eligible.sum())
        if E < 3:
            raise Exception("The uncertainty of the scores needs at least three windows with {:g} or more observed report "
                            "steps to resample; {} of the {} windows have that many.".format(min_steps, E, W))
        boot = engine.bootstrap_counts(W, resamples, seed=seed, eligible=eligible)
        jack = engine.jackknife_counts(W, eligible=eligible)
        used = np.where(eligible[np.maximum(ids, 0)] & (ids >= 0), ids, -1).astype(np.int32)
        k, K = len(swin.OBJ_FN_NAMES), len(probs)
        if n == 0:      # e.g. GLUE with no behavioural set: nothing to launch
            on_device, point = None, np.empty((0, k))
            mean = se_boot = se_jack = np.empty((k, 0))
            quant = np.empty((k, K, 0))
        else:
            out, obs = self._launch_stored()
            b = engine.objective_functions_bootstrap(out.discharge_report_major, obs, used, boot, probs=probs, n_windows=W,
                                                     transform=transform, eps=eps)
            j = engine.objective_functions_bootstrap(out.discharge_report_major, obs, used, jack, probs=probs, n_windows=W,
                                                     transform=transform, eps=eps)
            on_device, point = b.stats, b.point.cpu().numpy()
            stats = on_device.cpu().numpy() if on_device is not None else np.full((k, 2 + K, n), np.nan)
            mean, se_boot, quant = stats[:, 0], stats[:, 1], stats[:, 2:]
            se_jack = swin.jackknife_factor(E) * j.stats[:, 1].cpu().numpy()
        path = self._write_side(write, '.uncertainty',
                                lambda path: _write_uncertainty_file(path, probs, point, se_boot, se_jack, quant))
        return swin.ScoreUncertainty(labels, eligible, min_steps, transform, float(eps), probs, point, mean, se_boot, quant,
                                     se_jack, on_device, path, seed, int(resamples))

    @property
    def uncertainty_file(self):
        """`<out>/<catchment>.SMART.<func>.uncertainty`: beside the sampling database, whatever its format."""
        return self._side_file('.uncertainty')

    # ---- dynamic identifiability --------------------------------------------------------------------------
    def dynamic_identifiability(self, half_width=None, fraction=0.1, bins=20, support='linear', min_valid=None, level=0.9,
                                ranges=None, write=False):
        """WHEN in the record each parameter is identifiable (DYNIA, Wagener et al. 2003, Hydrol. Process. 17), from the
        sample as it is: per report step every row is scored by its absolute error over the observed steps of the moving
        window of `half_width` report steps to either side (None: the report steps of 15 days), the best `fraction` of
        the rows is retained, and their support ('linear': the distance to the cut; 'equal': 1 each) is shared out over
        `bins` equal bins of every parameter's range.  From the shares: the `level` confidence limits of every parameter
        and its information content 1 - width / range (smartpy_amd.identifiability) -- near 1 where the data of that
        period pin the parameter down.  ranges=None: the ranges the sample was drawn from (model.parameters.ranges: for a
        GLUE object the prior ranges, not the extent of the behavioural rows); a dict name -> (lo, hi) or [P, 2] overrides
        them.  A window with fewer than `min_valid` observed steps (None: half of it) is NaN.  One launch of its own over
        the sample; the [R, N] matrix stays on the device and only [R, P, bins] comes back.  write=True also writes
        `<out>/<catchment>.SMART.<func>.dynia` (header DateTime,IC@<name>,LO@<name>,HI@<name>,...; one line per report
        step, '%.6e').  Under torch.distributed every rank that calls this computes all rows itself (no collective);
        rank 0 alone writes.  -> identifiability.DynamicIdentifiability"""
        stamps = self.model.timeseries_report[1:]
        names = list(self.param_names)
        if half_width is None:
            half_width = int(15 * 86400 // self.model.delta_save.total_seconds())
        half_width, bins = int(half_width), int(bins)
        if min_valid is None:
            min_valid = half_width + 1
        if ranges is None:
            ranges = self.model.parameters.ranges
        self._check_observations()
        n, R, P = self._sample.shape[0], len(stamps), len(names)
        on_device = None
        if n == 0:      # e.g. GLUE with no behavioural set: nothing to launch
            shares = np.full((R, P, bins), np.nan)
            cut, retained, count = np.full(R, np.nan), np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
        else:
            cat = ident.bin_table(self._launch_rows(), ident._ranges(ranges, names), bins)
            out, obs = self._launch_stored()
            res = engine.dynamic_identifiability(out.discharge_report_major, obs, cat, bins, half_width, fraction=fraction,
                                                 min_valid=min_valid, support=support)
            on_device = res.shares
            shares, cut = on_device.cpu().numpy(), res.cut.cpu().numpy()
            retained, count = res.retained.cpu().numpy(), res.count.cpu().numpy()
        result = ident.DynamicIdentifiability(stamps, names, ranges, shares, cut, retained, count, level=level,
                                              half_width=half_width, fraction=float(fraction), support=support,
                                              min_valid=int(min_valid), device_shares=on_device)
        result.file = self._write_side(write, '.dynia', lambda path: ident.write_file(path, stamps, names, result.information,
                                                                                      result.limits))
        return result

    @property
    def dynia_file(self):
        """`<out>/<catchment>.SMART.<func>.dynia`: beside the sampling database, whatever its format."""
        return self._side_file('.dynia')

    # ---- PAWN sensitivity ---------------------------------------------------------------------------------
    def pawn_sensitivity(self, of='discharge', bins=10, statistic='median', dummies=3, seed=0, min_count=None, ranges=None,
                         method='auto', write=False):
        """HOW MUCH every parameter moves the distribution of an output (PAWN, Pianosi & Wagener 2015; the given-data
        form, 2018), from the sample as it is -- no design of its own.  Per output the Kolmogorov-Smirnov distance between
        the CDF over all rows and the CDF over the rows whose parameter lies in one of `bins` equal bins of its range;
        the index of a parameter is the `statistic` ('median', 'mean', 'max') of those distances over the bins that hold
        at least `min_count` rows (None: max(10, N // (4 bins))).  of='discharge': every report step, from the [R, N]
        matrix where a launch of its own leaves it (time-varying sensitivity); of='objective_functions': NSE, KGE, KGEc,
        KGEa, KGEb, PBias, RMSE and the groundwater ratio of every row ([8, N]; those of the last run() where there was
        one); an array or tensor [M, N]: any per-row values of the caller's.  `dummies` factors that influence nothing by
        construction (random partitions of the rows into `bins` groups, numpy.random.default_rng(seed)) travel through
        the same launch: the largest index among them is the noise floor `dummy`, and `influential` = index > dummy.
        ranges=None: the ranges the sample was drawn from, as dynamic_identifiability takes them.  The distances are
        ratios of integers: the same bits as the definition in numpy, whatever `method` ('auto', 'lds', 'global').
        write=True also writes `<out>/<catchment>.SMART.<func>.pawn` (header DateTime,<name>,...,dummy; one line per
        output, '%.6e').  Under torch.distributed every rank that calls this computes all rows itself (no collective);
        rank 0 alone writes.  -> pawn.PawnSensitivity"""
        names = list(self.param_names)
        bins, dummies = int(bins), int(dummies)
        n, P = self._sample.shape[0], len(names)
        if not 0 <= dummies <= _lib.PAWN_MAX_FACTORS - P:
            raise SmartEngineError(-2, "pawn_sensitivity: dummies {} must be in 0 .. {} ({} factors a launch, {} of them "
                                       "parameters).".format(dummies, _lib.PAWN_MAX_FACTORS - P,
                                                             _lib.PAWN_MAX_FACTORS, P))
        if statistic not in pawn.STATISTICS:
            raise SmartEngineError(-7, "pawn_sensitivity: statistic '{}' unknown.".format(statistic))
        if ranges is None:
            ranges = self.model.parameters.ranges
        if min_count is None:
            min_count = pawn.default_min_count(n, bins)
        values = None
        if isinstance(of, str):
            if of not in ('discharge', 'objective_functions'):
                raise SmartEngineError(-7, "pawn_sensitivity: of '{}' unknown.".format(of))
            stamps = self.model.timeseries_report[1:] if of == 'discharge' else swin.OBJ_FN_NAMES + ['GW_RATIO']
        else:
            values = of
            if len(values.shape) != 2 or values.shape[1] != n:
                raise SmartEngineError(-2, "pawn_sensitivity: the values must be [M, {}] (a column per row of the sample), "
                                           "not {}.".format(n, tuple(values.shape)))
            stamps = list(range(values.shape[0]))
        on_device = None
        if n == 0:      # e.g. GLUE with no behavioural set: nothing to launch
            ks = np.full((len(stamps), P + dummies, bins), np.nan)
            counts = np.zeros((P + dummies, bins), dtype=np.int32)
            table = np.empty((P + dummies, 0), dtype=np.uint8)
        else:
            cat = ident.bin_table(self._launch_rows(), ident._ranges(ranges, names), bins)
            extra = pawn.dummy_table(n, bins, dummies, seed)
            if ident._is_tensor(cat):
                cat = torch.cat([cat, torch.from_numpy(extra).to(cat.device)], dim=0)
            else:
                cat = np.concatenate([cat, extra], axis=0)
            if values is None and of == 'discharge':
                values = self._launch_stored()[0].discharge_report_major
            elif values is None:
                values = self._score_table()
            res = engine.pawn_ks(values, cat, bins, method=method)
            on_device = res.ks
            ks, counts = res.numpy()
            table = cat.cpu().numpy() if ident._is_tensor(cat) else cat
        result = pawn.PawnSensitivity(stamps, names, ks, counts, statistic=statistic, min_count=min_count,
                                      categories=table, device_ks=on_device)
        result.file = self._write_side(write, '.pawn',
                                       lambda path: pawn.write_file(path, stamps, names, result.index, result.dummy))
        return result

    def _score_table(self):
        """[8, N] on the device: the seven objective functions and the groundwater ratio of every row of the sample --
        those of the last run(), or of a launch of its own where there was none"""
        n = self._sample.shape[0]
        if self.device_obj_fns is not None and self.device_obj_fns.shape[0] == n:
            scores, gw = self.device_obj_fns, self.device_gw
        else:
            self._check_observations()
            out = self.model.simulate_ensemble(self._launch_rows(), objective_functions=True,
                                               gw_constraint=self.constraints['gw'], math_mode=self.math_mode)
            scores, gw = out.objfn[:n], out.gw[:n]
        return torch.cat([scores[:, :len(swin.OBJ_FN_NAMES)], gw.unsqueeze(1)], dim=1).t().contiguous()

    @property
    def pawn_file(self):
        """`<out>/<catchment>.SMART.<func>.pawn`: beside the sampling database, whatever its format."""
        return self._side_file('.pawn')

    # ---- the residual error model: likelihood and total predictive bounds -----------------------------------
    def _default_error_parameters(self):
        """[N, 3] where the object has inferred error parameters of its own (DEMCz with likelihood='ar1'), else None"""
        return None

    def _error_parameters(self, who, error_parameters):
        """error_parameters of a call -> numpy [N, 3]: one (sigma0, sigma1, phi) per row of the sample, or one triple for
        all of them; None takes the object's own"""
        if error_parameters is None:
            error_parameters = self._default_error_parameters()
            if error_parameters is None:
                raise SmartEngineError(-1, "{}: error_parameters are needed ([N, 3] or one triple of sigma0, sigma1, phi; "
                                           "a DEMCz run with likelihood='ar1' brings its own).".format(who))
        if type(error_parameters).__module__.startswith('torch'):
            error_parameters = error_parameters.cpu().numpy()
        return errormodel.parameter_table(error_parameters, self._sample.shape[0])

    def _row_weights(self, who, likelihood):
        """likelihood_weights for the rows of the sample; a name stands for its values in the last run()"""
        return likelihood_weights(likelihood, self._sample.shape[0], self.obj_fn_names, self.obj_fns, ROW_WEIGHT_TEXTS,
                                  who=who)

    def residual_likelihood(self, error_parameters=None, write=False):
        """The log-likelihood of the observed flow under the residual error model of smartpy_amd.errormodel, for every
        row of the sample: sigma_t = sigma0 + sigma1 sim_t, an AR(1) with coefficient phi on the standardised residuals
        that restarts after every gap of the observations.  error_parameters: [N, 3] (sigma0, sigma1, phi per row) or one
        triple for all rows; None: those a DEMCz run with likelihood='ar1' archived.  One launch of its own over the
        sample; the [R, N] matrix stays on the device and only [3, N] comes back (engine.residual_log_likelihood).
        write=True also writes `<out>/<catchment>.SMART.<func>.errormodel` (header sigma0,sigma1,phi,LOGLIK,SSQ,LOGSIG;
        one line per row of the sample, '%.6e').  Under torch.distributed every rank that calls this computes all rows
        itself (no collective); rank 0 alone writes.  -> errormodel.ResidualLikelihood"""
        self._check_observations()
        theta = self._error_parameters('residual_likelihood', error_parameters)
        on_device = None
        if self._sample.shape[0] == 0:      # e.g. GLUE with no behavioural set: nothing to launch
            values = np.empty((len(errormodel.LIKELIHOOD_NAMES), 0))
        else:
            out, obs = self._launch_stored()
            on_device = engine.residual_log_likelihood(out.discharge_report_major, obs, theta)
            values = on_device.cpu().numpy()
        path = self._write_side(write, '.errormodel', lambda path: errormodel.write_likelihood_file(path, theta, values))
        return errormodel.ResidualLikelihood(theta, values, on_device, path)

    def predictive_bounds(self, error_parameters=None, quantiles=(0.05, 0.5, 0.95), replicates=1, likelihood=None, seed=0,
                          truncate=True, verify=False, write=False):
        """The TOTAL prediction bounds of the sample: at every report step the weighted quantiles of `replicates` error
        realisations on top of every row's simulation (engine.predictive_draws: the residual error model with the row's
        sigma0, sigma1, phi), each row's weight repeated over its replicates -- where GLUE.prediction_bounds describes
        the spread of the parameter ensemble alone.  error_parameters: as for residual_likelihood.  likelihood: None =
        equal weights (a posterior sample), the name of an objective function of this object's finished run(), or an
        array [N]; negative or non-finite weights raise.  seed: of the draws (the same seed, the same bits); truncate:
        negative flows become 0.  One launch of its own over the sample; the [R, N] matrix and the [R, N replicates]
        draws stay on the device, and the draws matrix goes into engine.weighted_quantiles as any stored matrix does --
        with verify=True into engine.ensemble_scores too (verification.EnsembleVerification of the total predictive
        distribution: CRPS, PIT histogram, reliability).  The result also carries the parametric-only bounds of the same
        rows and the containment of both.  write=True also writes `<out>/<catchment>.SMART.<func>.predictive` (CSV:
        DateTime,q<p>,...,param_q<p>,...).  Under torch.distributed every rank that calls this computes all rows itself
        (no collective); rank 0 alone writes.  -> errormodel.PredictiveBounds"""
        who = 'predictive_bounds'
        q = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
        K = int(replicates)
        if K < 1:
            raise SmartEngineError(-2, "{}: replicates must be at least 1 (got {}).".format(who, replicates))
        stamps = self.model.timeseries_report[1:]
        theta = self._error_parameters(who, error_parameters)
        weights = self._row_weights(who, likelihood)
        nan = float('nan')
        verification = None
        if self._sample.shape[0] == 0:      # e.g. GLUE with no behavioural set: nothing to launch
            bounds = parametric = np.full((q.size, len(stamps)), nan)
            inside = alone = nan
        else:
            out, obs = self._launch_stored()
            sim = out.discharge_report_major
            draws = engine.predictive_draws(sim, theta, replicates=K, seed=seed, truncate=truncate)
            repeated = None if weights is None else np.repeat(weights, K)
            total = engine.weighted_quantiles(draws, q, repeated)
            spread = engine.weighted_quantiles(sim, q, weights)
            inside, alone = containment(total, obs), containment(spread, obs)
            bounds, parametric = total.cpu().numpy(), spread.cpu().numpy()
            if verify:
                flow = self.model.nd_flow
                scores = engine.ensemble_scores(draws, obs, repeated).cpu().numpy()
                verification = EnsembleVerification(scores, None if flow is None else np.asarray(flow, dtype=np.float64),
                                                    stamps)
        path = self._write_side(write, '.predictive',
                                lambda path: errormodel.write_predictive_file(path, stamps, q, bounds, parametric))
        return errormodel.PredictiveBounds(q, bounds, parametric, inside, alone, stamps, K, seed, truncate,
                                           verification, path)


def _write_windows_file(path, labels, transform, values):
    """values [W, N, 7] -> header line + one line per sample, window by window (the sampling database's float32
    '%.6e', formatted by the library)."""
    W, n, k = values.shape
    write_float32_table(path, swin.header_line(labels, transform), np.transpose(values, (1, 0, 2)).reshape(n, W * k))


def _write_signatures_file(path, labels, values):
    """values [W, 12, N] -> header line + one line per sample, window by window (the sampling database's float32
    '%.6e', formatted by the library)."""
    W, k, n = values.shape
    write_float32_table(path, swin.signatures_header_line(labels), np.transpose(values, (2, 0, 1)).reshape(n, W * k))


def _write_uncertainty_file(path, probs, point, se_boot, se_jack, quant):
    """point [N, 7], se_boot and se_jack [7, N], quant [7, K, N] -> header line + one line per sample, score by score:
    the point value, its bootstrap and jackknife standard errors, the K quantiles (the sampling database's float32
    '%.6e', formatted by the library)."""
    n, k = point.shape
    table = np.concatenate([point[:, :, None], se_boot.T[:, :, None], se_jack.T[:, :, None],
                            np.transpose(quant, (2, 0, 1))], axis=2).reshape(n, k * (3 + quant.shape[1]))
    write_float32_table(path, swin.uncertainty_header_line(probs), table)


def _write_fdc_file(path, exceedance, labels, transform, curves, values):
    """curves [W, K, N] and values [W, N, 7] -> header line + one line per sample: the K flows of every window, then
    the seven objective functions of every window (the sampling database's float32 '%.6e', formatted by the library)."""
    W, K, n = curves.shape
    table = np.concatenate([np.transpose(curves, (2, 0, 1)).reshape(n, W * K),
                            np.transpose(values, (1, 0, 2)).reshape(n, W * values.shape[2])], axis=1)
    write_float32_table(path, swin.fdc_header_line(exceedance, labels, transform), table)
