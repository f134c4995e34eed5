"""Sobol sensitivity analysis on a Saltelli design (no counterpart in the reference, whose sampling tool ships
sensitivity samplers beside its Latin hypercube).

Which of the ten SMART parameters does an answer depend on, and when during the run?  A Saltelli design of base size n
over k parameters is n (k + 2) rows: the engine simulates them in one launch like any other sample, and
engine.sobol_indices turns the values of the rows -- objective functions, the groundwater ratio, the discharge of every
report step, anything the caller computed per row -- into first-order (Saltelli 2010) and total (Jansen) indices with
bootstrap confidence intervals, on the GPU.
"""
from statistics import NormalDist

import numpy as np

from .montecarlo import MonteCarlo
from .selection import write_float32_table
from ..sampling import saltelli_design

INDICES_HEADER = 'target,parameter,S1,S1_conf,ST,ST_conf\n'


class SobolIndices(object):
    """What Sobol.sensitivity returns: `parameters` (the k names that vary), `targets` (M names), S1, ST, S1_conf, ST_conf
    [M, k] (the half-widths of the confidence intervals; None without resamples), mean and variance [M] of the target
    over the A and B blocks, conf_level, resamples, `device` (the engine.SobolResult with the device tensors) and `file`
    (the `.indices` file, or None)."""

    def __init__(self, parameters, targets, S1, ST, S1_conf, ST_conf, mean, variance, conf_level, resamples, device, file):
        self.parameters, self.targets = list(parameters), list(targets)
        self.S1, self.ST, self.S1_conf, self.ST_conf = S1, ST, S1_conf, ST_conf
        self.mean, self.variance = mean, variance
        self.conf_level, self.resamples, self.device, self.file = conf_level, resamples, device, file


class SobolSeries(object):
    """What Sobol.sensitivity_series returns: S1, ST [R, k] per report step, variance and mean [R], `datetime` (the report
    stamps), S1_conf, ST_conf [R, k] or None, `parameters`, conf_level, resamples, `device` and `file`."""

    def __init__(self, parameters, datetime, S1, ST, S1_conf, ST_conf, mean, variance, conf_level, resamples, device, file):
        self.parameters, self.datetime = list(parameters), datetime
        self.S1, self.ST, self.S1_conf, self.ST_conf = S1, ST, S1_conf, ST_conf
        self.mean, self.variance = mean, variance
        self.conf_level, self.resamples, self.device, self.file = conf_level, resamples, device, file


def normal_quantile(conf_level):
    """The two-sided standard normal quantile of a confidence level in (0, 1): 1.96 for 0.95."""
    level = float(conf_level)
    if not 0.0 < level < 1.0:
        raise Exception("The confidence level must lie between 0 and 1 (got {}).".format(conf_level))
    return NormalDist().inv_cdf(0.5 + level / 2.0)


class Sobol(MonteCarlo):
    """Simulate a Saltelli design and analyse the sensitivity of its results.

    base_size: n; the sample has n (k + 2) rows, k = len(vary) (default: all ten parameters).  vary / fixed / seed as for
    sampling.saltelli_design; the ranges are model.parameters.ranges.  `run()` is the inherited one and writes
    `<catchment>.SMART.sobol` in the database format; `sensitivity()` then works on what it left on the device,
    `sensitivity_series()` makes a launch of its own with the discharge stored."""

    def __init__(self, catchment, root_f, in_format, out_format,
                 base_size,
                 parallel='seq', save_sim=False, settings_filename=None,
                 vary=None, fixed=None, seed=None):
        MonteCarlo.__init__(self, catchment, root_f, in_format, out_format,
                            parallel=parallel, save_sim=save_sim, func='sobol', settings_filename=settings_filename)
        self.base_size, self.seed = int(base_size), seed
        design, self.vary = saltelli_design(base_size, self.model.parameters.ranges, self.param_names, vary=vary,
                                            fixed=fixed, seed=seed)
        self._set_sample(design)

    # ---- scalar targets ------------------------------------------------------------------------------------
    def _target_rows(self, targets):
        """-> (names, [M, N] device tensor or host array)"""
        import torch
        if targets is None:
            targets = [name for name in self.obj_fn_names if name != 'GW']
        if isinstance(targets, str):
            targets = [targets]
        if isinstance(targets, (list, tuple)) and all(isinstance(t, str) for t in targets):
            if self.device_obj_fns is None:
                raise Exception("Sobol.sensitivity: run() has to come first (there are no results to analyse).")
            rows = []
            for name in targets:
                if name == 'GW':
                    rows.append(self.device_gw)
                elif name in self.obj_fn_names:
                    rows.append(self.device_obj_fns[:, self.obj_fn_names.index(name)])
                else:
                    raise Exception("Sobol.sensitivity: the target '{}' is not one of: {}."
                                    .format(name, ', '.join(self.obj_fn_names + ['GW'])))
            return list(targets), torch.stack(rows).contiguous()
        if self.obj_fns is None:
            raise Exception("Sobol.sensitivity: run() has to come first (there are no results to analyse).")
        values = targets if isinstance(targets, torch.Tensor) else np.asarray(targets, dtype=np.float64)
        if len(values.shape) == 1:
            values = values.reshape(1, -1)
        if len(values.shape) != 2 or values.shape[1] != self._sample.shape[0]:
            raise Exception("Sobol.sensitivity: targets of shape {} do not hold one value per row of the design ({})."
                            .format(tuple(values.shape), self._sample.shape[0]))
        return ['target%d' % m for m in range(values.shape[0])], values

    def _analyse(self, values, resamples, conf_level, seed):
        """-> (engine.SobolResult, S1, ST, S1_conf, ST_conf, mean, variance) with the host copies"""
        from .. import engine
        z = normal_quantile(conf_level)
        resamples = int(resamples)
        counts = engine.sobol_counts(self.base_size, resamples, seed) if resamples > 0 else None
        res = engine.sobol_indices(values, self.base_size, len(self.vary), counts=counts)
        S1, ST, moments = res.S1.cpu().numpy(), res.ST.cpu().numpy(), res.moments.cpu().numpy()
        S1_conf = ST_conf = None
        if resamples > 0:
            S1_conf, ST_conf = z * res.S1_std.cpu().numpy(), z * res.ST_std.cpu().numpy()
        return res, S1, ST, S1_conf, ST_conf, moments[:, 0], moments[:, 1]

    def sensitivity(self, targets=None, resamples=128, conf_level=0.95, seed=None, write=False):
        """First-order and total Sobol indices of scalar results of the design's rows.  targets: names among obj_fn_names
        (default: all objective functions), 'GW' (the groundwater ratio), or an [N] / [M, N] array of the caller's own
        with one value per row (a flow_duration_curves quantile, one window's KGE from window_objective_functions ...;
        named target0, target1 ...).  resamples: bootstrap replicates behind S1_conf / ST_conf (0: none; at most
        engine.sobol_max_resamples()), the half-width z * std with z the normal quantile of conf_level; seed: of the
        bootstrap draws.  After run(), on device_obj_fns / device_gw; no launch of the model.  write=True also writes
        `<catchment>.SMART.sobol.indices` (header, then target,parameter,S1,S1_conf,ST,ST_conf per line, the float32
        '%.6e' of the sampling database; rank 0 alone writes).  -> SobolIndices"""
        names, values = self._target_rows(targets)
        res, S1, ST, S1_conf, ST_conf, mean, variance = self._analyse(values, resamples, conf_level, seed)
        path = self._write_side(write, '.indices',
                                lambda path: _write_indices_file(path, names, self.vary, S1, S1_conf, ST, ST_conf))
        return SobolIndices(self.vary, names, S1, ST, S1_conf, ST_conf, mean, variance, float(conf_level), int(resamples),
                            res, path)

    # ---- time-varying sensitivity --------------------------------------------------------------------------
    def sensitivity_series(self, resamples=0, conf_level=0.95, seed=None, write=False):
        """The indices of the DISCHARGE of every report step: one launch of its own over the design with the [R, N]
        matrix stored, every report step one row of engine.sobol_indices (its blocks are contiguous: block-major
        design).  resamples > 0 adds the confidence half-widths per step.  write=True also writes
        `<catchment>.SMART.sobol.series` (DateTime,S1_<p>...,ST_<p>..., the float32 '%.6e' of the sampling database;
        rank 0 alone writes).  Under torch.distributed every rank computes everything itself.  -> SobolSeries"""
        out, _ = self._launch_stored()
        res, S1, ST, S1_conf, ST_conf, mean, variance = self._analyse(out.discharge_report_major, resamples, conf_level,
                                                                      seed)
        stamps = self.model.timeseries_report[1:]
        path = self._write_side(write, '.series', lambda path: _write_series_file(path, stamps, self.vary, S1, ST))
        return SobolSeries(self.vary, stamps, S1, ST, S1_conf, ST_conf, mean, variance, float(conf_level), int(resamples),
                           res, path)

    @property
    def indices_file(self):
        """`<out>/<catchment>.SMART.sobol.indices`: beside the sampling database, whatever its format."""
        return self._side_file('.indices')

    @property
    def series_file(self):
        """`<out>/<catchment>.SMART.sobol.series`"""
        return self._side_file('.series')


def series_header_line(parameters):
    return ','.join(['DateTime'] + ['S1_%s' % p for p in parameters] + ['ST_%s' % p for p in parameters]) + '\n'


def _write_indices_file(path, targets, parameters, S1, S1_conf, ST, ST_conf):
    """[M, k] arrays -> one line per (target, parameter); confidence half-widths that were not asked for are NaN."""
    M, k = S1.shape
    nan = np.full((M, k), np.nan)
    table = np.stack([S1, nan if S1_conf is None else S1_conf, ST, nan if ST_conf is None else ST_conf], axis=2)
    labels = ['%s,%s' % (t, p) for t in targets for p in parameters]
    write_float32_table(path, INDICES_HEADER, table.reshape(M * k, 4), labels)


def _write_series_file(path, stamps, parameters, S1, ST):
    """S1, ST [R, k] -> one line per report step: its stamp, the k first-order and the k total indices."""
    labels = [t.strftime('%Y-%m-%d %H:%M:%S') for t in stamps]
    write_float32_table(path, series_header_line(parameters), np.concatenate([S1, ST], axis=1), labels)
