"""Pareto conditioning run (no counterpart in the reference, which selects by one threshold per function -- GLUE -- or by
the largest value of one function -- Best): keep the sets of a previous sampling that no other set beats on every chosen
objective function at once, and re-simulate them (typically on another period).

The fronts are peeled on the GPU (engine.pareto_ranks, selection.pareto_rows) over the sampling run's objective
functions as its database keeps them, and over any further per-row scores the caller brings (`extra`: the scores of a
validation period, of a season, of a flow duration curve's segment ...)."""
import numpy as np

from .montecarlo import MonteCarlo
from .selection import condition_mask, pareto_rows, SecondStage, _is_torch


class Pareto(SecondStage, MonteCarlo):
    """objectives: a dict {name of an objective function: direction} or a list of names taking DEFAULT_DIRECTIONS; a
    direction is 'max', 'min' or ('target', value).  conditioning: as GLUE's, applied first -- only the rows that meet it
    take part.  max_rank: how many fronts to keep (1: the Pareto set; None: every row, ranked).  extra: {label: (values
    [N], direction)}, per-row scores that are not in the database, in the sampling run's row order (a device tensor such
    as window_objective_functions(...).device_values[w, :, c], or a host array).  sampling: as GLUE's -- a finished
    sampling run of this process instead of its database file; both ways select the same rows.

    Sets `pareto_index` (rows of the sampling run, ordered by rank and then by row), `pareto_rank` (their ranks),
    `pareto_params` (float32 [n, 10], as the database keeps them) and `pareto_obj_fns`; `run()` is the inherited one and
    writes `<catchment>.SMART.pareto`.  A row with a NaN among its selected scores takes part in nothing.  Under
    torch.distributed every rank selects for itself (no collective)."""

    DEFAULT_DIRECTIONS = {'NSE': 'max', 'KGE': 'max', 'KGEc': 'max', 'KGEa': ('target', 1.0), 'KGEb': ('target', 1.0),
                          'PBias': ('target', 0.0), 'RMSE': 'min', 'GW': 'max'}

    def __init__(self, catchment, root_f, in_format, out_format,
                 objectives, conditioning=None, max_rank=1,
                 parallel='seq', save_sim=False, settings_filename=None,
                 decompression_csv=False, sampling=None, extra=None):
        MonteCarlo.__init__(self, catchment, root_f, in_format, out_format,
                            parallel=parallel, save_sim=save_sim, func='pareto', settings_filename=settings_filename)
        if not isinstance(objectives, dict):
            objectives = {name: self.DEFAULT_DIRECTIONS.get(name, 'max') for name in objectives}
        extra = dict(extra or {})
        if not objectives:
            raise Exception("Pareto needs at least one objective function.")
        self.objective_fn_indices = self._columns_of(
            objectives, "One of the names of objective functions in Pareto is not recognised."
                        "Please check for typos and case sensitive issues.")
        self.objective_names = list(objectives) + list(extra)
        self.directions = [objectives[name] for name in objectives] + [extra[label][1] for label in extra]
        conditioning = conditioning or {}
        self.conditioning_indices = self._columns_of(
            conditioning, "One of the names of objective functions for conditioning in Pareto is not recognised."
                          "Please check for typos and case sensitive issues.")
        self.conditions_types = [conditioning[fn][0] for fn in conditioning]
        self.conditions_values = [conditioning[fn][1] for fn in conditioning]
        self.max_rank = max_rank
        self._load_sampling(catchment, decompression_csv, sampling)
        n = self.sampled_obj_fns.shape[0]
        for label in extra:
            shape = tuple(extra[label][0].shape)
            if shape != (n,):
                raise Exception("The extra objective '{}' has shape {} where one value per sampled set ({},) is "
                                "expected.".format(label, shape, n))
        fns = self._device_obj_fns if sampling is not None else self.sampled_obj_fns
        allowed = condition_mask(fns[:, self.conditioning_indices], self.conditions_values, self.conditions_types) \
            if conditioning else None
        rows, ranks = pareto_rows(self._scores(fns, [extra[label][0] for label in extra]), self.directions, allowed,
                                  max_rank)
        if sampling is not None:
            self.pareto_params = self._rows_as_stored(rows)
            rows, ranks = rows.cpu().numpy(), ranks.cpu().numpy()
        else:
            self.pareto_params = self.sampled_params[rows, :]
        self.pareto_index, self.pareto_rank = rows, ranks
        #: the sampling run's objective functions of the selected rows (float32, as the database keeps them)
        self.pareto_obj_fns = self.sampled_obj_fns[rows, :]
        self._set_sample(self.pareto_params)

    def _scores(self, fns, columns):
        """the selected columns of the stored objective functions and the extra columns, side by side, float64 -- where
        the objective functions are (a device tensor with sampling=, else a host array)"""
        if _is_torch(fns):
            import torch
            parts = [fns[:, self.objective_fn_indices].to(torch.float64)]
            parts += [(c if _is_torch(c) else torch.from_numpy(np.ascontiguousarray(c))).to(fns.device, torch.float64)
                      .reshape(-1, 1) for c in columns]
            return torch.cat(parts, dim=1)
        parts = [fns[:, self.objective_fn_indices].astype(np.float64)]
        parts += [np.asarray(c.cpu().numpy() if _is_torch(c) else c, dtype=np.float64).reshape(-1, 1) for c in columns]
        return np.concatenate(parts, axis=1)
