"""GLUE conditioning run (counterpart of smartpy/montecarlo/glue.py): keep the behavioural sets of a previous
LHS sampling, re-simulate them (typically on another period) -- and, beyond the reference, hand out what a GLUE
analysis is run for: the likelihood-weighted prediction bounds of the behavioural ensemble (prediction_bounds), and
how good that predictive distribution is against the observations (ensemble_verification)."""
import numpy as np

from .analyses import containment, likelihood_weights
from .montecarlo import MonteCarlo
from .selection import condition_mask, check_shapes, write_text_table, SecondStage
from ..verification import EnsembleVerification

#: the refusals of analyses.likelihood_weights as GLUE words them
LIKELIHOOD_TEXTS = {
    'name': "The likelihood '{name}' is not one of the objective functions of the sampling run ({names}).",
    'shape': "The likelihood array has shape {shape} where one value per behavioural set ({n}) is expected.",
    'values': "{bad} of the {n} likelihood values are negative or not finite: they cannot be used as weights (shift or "
              "select them first, nothing is clipped here).",
}


class PredictionBounds(object):
    """What GLUE.prediction_bounds returns: `quantiles` (the K probabilities), `bounds` (numpy [K, R] float64, row k
    the weighted quantile quantiles[k] of the behavioural ensemble's discharge at every report step), `datetime`
    (the R report stamps, model.timeseries_report[1:]), `containment` (the share of the non-missing observations o_r
    with bounds[0, r] <= o_r <= bounds[-1, r]; NaN without observations) and `file` (the path written, or None)."""

    def __init__(self, quantiles, bounds, stamps, containment, file=None):
        self.quantiles, self.bounds, self.datetime = quantiles, bounds, stamps
        self.containment, self.file = containment, file


class GLUE(SecondStage, MonteCarlo):
    """Constructor of the reference (glue.py:34-37) plus `sampling=`: a finished sampling run of this process (an LHS
    object after run()) whose objective functions are still on the GPU -- the behavioural mask is then evaluated
    there and only the selected parameter rows travel, instead of re-reading and parsing the database file."""

    def __init__(self, catchment, root_f, in_format, out_format,
                 conditioning,
                 parallel='seq', save_sim=False, settings_filename=None,
                 decompression_csv=False, sampling=None):
        MonteCarlo.__init__(self, catchment, root_f, in_format, out_format,
                            parallel=parallel, save_sim=save_sim, func='glue', settings_filename=settings_filename)
        self.objective_fn_indices = self._columns_of(
            conditioning, "One of the names of objective functions for conditioning in GLUE is not recognised."
                          "Please check for typos and case sensitive issues.")
        self.conditions_types = [conditioning[fn][0] for fn in conditioning]
        self.conditions_values = [conditioning[fn][1] for fn in conditioning]
        self._load_sampling(catchment, decompression_csv, sampling)
        if sampling is not None:
            keep = condition_mask(self._device_obj_fns[:, self.objective_fn_indices], self.conditions_values,
                                  self.conditions_types)
            self.behavioural_params = self._rows_as_stored(keep)
            keep = keep.cpu().numpy()
        else:
            self.behavioural_params = self._get_behavioural_sets(
                self.sampled_params, self.sampled_obj_fns[:, self.objective_fn_indices],
                self.conditions_values, self.conditions_types)
            keep = condition_mask(self.sampled_obj_fns[:, self.objective_fn_indices], self.conditions_values,
                                  self.conditions_types)
        #: the sampling run's objective functions of the behavioural rows (float32 [N_behavioural, 7|8], as the
        #: database keeps them): the numbers the sets were selected on, and the likelihoods prediction_bounds weighs with
        self.behavioural_obj_fns = self.sampled_obj_fns[keep, :]
        self._set_sample(self.behavioural_params)

    @staticmethod
    def _get_behavioural_sets(params, obj_fns, conditions_val, conditions_typ):
        """glue.py:222-289 -> the rows of params (float32, possibly none) that meet every condition."""
        check_shapes(params, obj_fns, conditions_val, conditions_typ, 'objective')
        return params[condition_mask(obj_fns, conditions_val, conditions_typ), :]

    # ---- prediction bounds ------------------------------------------------------------------------------
    def _likelihood_weights(self, likelihood):
        """None (equal weights) | the name of an objective function (its values in the sampling run, for the
        behavioural rows) | an array [N_behavioural] -> float64 [N_behavioural] or None.  Nothing is clipped."""
        return likelihood_weights(likelihood, self._sample.shape[0], self.obj_fn_names, self.behavioural_obj_fns,
                                  LIKELIHOOD_TEXTS)

    def prediction_bounds(self, quantiles=(0.05, 0.5, 0.95), likelihood=None, write=False):
        """The GLUE prediction bounds: at every report step the likelihood-weighted quantiles of the behavioural
        ensemble's discharge -- Q(q) = the smallest simulated value v with sum(w[x <= v]) >= q * sum(w), no
        interpolation (engine.weighted_quantiles).  One launch of its own over the behavioural rows; the [R, N] matrix
        stays on the device and only the [K, R] bounds come back.  likelihood: None = equal weights, the name of an
        objective function = its values in the sampling run (behavioural_obj_fns), or an array [N_behavioural];
        negative or non-finite weights raise.  write=True also writes `<out>/<catchment>.SMART.glue.bounds` (CSV:
        DateTime,q<p>,... with the dates and the '%e' of the modelled flow file).  Under torch.distributed every rank
        that calls this computes all rows itself (no collective); rank 0 alone writes.  -> PredictionBounds"""
        from .. import engine
        q = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
        stamps = self.model.timeseries_report[1:]
        weights = self._likelihood_weights(likelihood)
        if self._sample.shape[0] == 0:      # no behavioural set: nothing to launch
            bounds, inside = np.full((q.size, len(stamps)), np.nan), float('nan')
        else:
            out, obs = self._launch_stored()
            on_device = engine.weighted_quantiles(out.discharge_report_major, q, weights)
            inside = containment(on_device, obs)
            bounds = on_device.cpu().numpy()
        header = ','.join(['DateTime'] + ['q%g' % p for p in q])
        path = self._write_side(write, '.bounds',
                                lambda path: write_text_table(path, header, bounds.T, '%e', '\r\n', labels=stamps))
        return PredictionBounds(q, bounds, stamps, inside, path)

    # ---- ensemble verification --------------------------------------------------------------------------
    def ensemble_verification(self, likelihood=None, bins=10, write=False):
        """How good the predictive distribution of the behavioural ensemble is: at every report step the CRPS of the
        likelihood-weighted ensemble against the observation, the ensemble's spread, the PIT of the observation from
        below and from above and the weighted mean (engine.ensemble_scores), and over the steps that have all of them
        the mean CRPS and spread, the skill against climatology, the non-randomised PIT histogram over `bins` bins and
        the reliability index (smartpy_amd.verification).  One launch of its own over the behavioural rows; the [R, N]
        matrix stays on the device and only the [5, R] scores come back.  likelihood: as for prediction_bounds.
        write=True also writes `<out>/<catchment>.SMART.glue.verification` (CSV: DateTime,crps,spread,pit_low,pit_high,
        mean with the dates and the '%e' of the modelled flow file).  Under torch.distributed every rank that calls this
        computes all rows itself (no collective); rank 0 alone writes.  -> EnsembleVerification"""
        from .. import engine
        stamps = self.model.timeseries_report[1:]
        weights = self._likelihood_weights(likelihood)
        flow = self.model.nd_flow
        if self._sample.shape[0] == 0:      # no behavioural set: nothing to launch
            scores = np.full((5, len(stamps)), np.nan)
        else:
            out, obs = self._launch_stored()
            scores = engine.ensemble_scores(out.discharge_report_major, obs, weights).cpu().numpy()
        path = self._write_side(write, '.verification',
                                lambda path: write_text_table(path, 'DateTime,crps,spread,pit_low,pit_high,mean', scores.T,
                                                              '%e', '\r\n', labels=stamps))
        return EnsembleVerification(scores, None if flow is None else np.asarray(flow, dtype=np.float64), stamps, bins,
                                    path)
