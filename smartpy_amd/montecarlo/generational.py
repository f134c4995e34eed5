"""What the generational samplers of the workflows share (demcz.py: DEMCz, nsga2.py: NSGA2): N rows that move in lockstep,
one ensemble launch per generation, one step call around it (smartpy_amd/generational.py), and at the end a MonteCarlo
object like any other.  The base class holds the parameters that vary and the box they move in, the starting population,
the launch of a generation, the adoption of the rows the sampler carried as the object's sample and tables, and the files.
A sampler supplies its own size rules, its state, what a launch's table becomes for its step, and its diagnostics.
"""
import numpy as np

from .montecarlo import MonteCarlo, OBJ_FN_NAMES
from .. import distributed as sdist
from ..engine import SmartEngineError
from ..sampling import latin_hypercube

GW_FLAG_COLUMN = len(OBJ_FN_NAMES)
N_CARRY = len(OBJ_FN_NAMES) + 2      # the seven objective functions, the GW flag and the groundwater ratio


class Generational(MonteCarlo):
    """A refusal carries the name of the sampler's class."""

    def _resolve_box(self, vary, fixed, max_dims=None):
        """vary / fixed as for Sobol -> the dict `fixed`; sets vary, columns (of the varying parameters in a row), lo, hi"""
        who = type(self).__name__
        names, ranges = list(self.param_names), self.model.parameters.ranges
        self.vary = list(names if vary is None else vary)
        if max_dims is not None and len(self.vary) > max_dims:
            raise SmartEngineError(-2, "{}: {} dimensions, at most {}.".format(who, len(self.vary), max_dims))
        unknown = [p for p in self.vary if p not in names]
        if unknown or len(set(self.vary)) != len(self.vary) or not self.vary:
            raise Exception("{}: `vary` must name at least one of {}, each once (got {}).".format(who, names, self.vary))
        fixed = dict(fixed or {})
        unknown = [p for p in fixed if p not in names or p in self.vary]
        if unknown:
            raise Exception("{}: the fixed parameter(s) {} are unknown or also vary.".format(who, unknown))
        self.columns = [names.index(p) for p in self.vary]
        self.lo = np.asarray([ranges[p][0] for p in self.vary], dtype=np.float64)
        self.hi = np.asarray([ranges[p][1] for p in self.vary], dtype=np.float64)
        return fixed

    def _start_from(self, n_rows, fixed, population=None):
        """population: [n_rows, >= 10], a Latin hypercube over the ranges (None: drawn here, sampling.latin_hypercube with
        the object's seed).  A parameter that does not vary is set to fixed[name], or to the middle of its range; the result is
        `initial_population`, and its ten model columns the sample."""
        names, ranges = list(self.param_names), self.model.parameters.ranges
        if population is None:
            population = latin_hypercube(n_rows, ranges, names, seed=self.seed)
        for j, p in enumerate(names):
            if p not in self.vary:
                population[:, j] = fixed.get(p, 0.5 * (float(ranges[p][0]) + float(ranges[p][1])))
        self.initial_population = population
        self._set_sample(population[:, :len(names)])

    def _population_of_all_ranks(self):
        population = self.initial_population
        if sdist.rank_world()[1] > 1:       # (seed=None draws from NumPy's global stream: rank 0's population is THE population)
            population = sdist.broadcast_matrix(population, src=0)
        return population

    def _device_rows(self, population, device):
        """-> the launch matrix: the population at full width on the device, the state's own to rewrite"""
        from ..engine import as_device
        return as_device(population, device).clone()

    def _launch(self, rows, save_discharge=False):
        """One launch over [N, 10] rows on the device -> (the engine's result, the [N, 8] objective table, the payload
        [N, 9] a row carries: the table and the groundwater ratio)"""
        import torch
        n = rows.shape[0]
        out = self.model.simulate_ensemble(rows, objective_functions=True, gw_constraint=self.constraints['gw'],
                                           save_discharge=save_discharge, math_mode=self.math_mode)
        table = out.objfn[:n]
        return out, table, torch.cat([table, out.gw[:n].unsqueeze(1)], dim=1)

    def _full_rows(self, population, moved):
        """moved: [n, d] device tensor of the varying dimensions -> [n, width of the population]: the other columns as the
        population's first row has them"""
        from ..engine import as_device
        full = as_device(population[:1], moved.device).repeat(moved.shape[0], 1)
        full[:, self.columns] = moved
        return full

    def _adopt(self, sample, carry):
        """The MonteCarlo object every second stage and analysis takes: sample [n, 10] and the payload [n, 9] its rows
        carried, both on the device"""
        n_obj = len(self.obj_fn_names)
        self._set_sample(sample)
        self.device_obj_fns, self.device_gw = carry[:, :n_obj].contiguous(), carry[:, N_CARRY - 1].contiguous()
        host = carry.cpu().numpy()
        self.obj_fns, self.gw_contributions = np.ascontiguousarray(host[:, :n_obj]), np.ascontiguousarray(host[:, -1])

    def _write_files(self, compression, write, writer):
        """On rank 0: the database, and with write=True the diagnostics file through writer(path) -> its path, or None"""
        written = []

        def write_files():
            self._write_database(None, compression)
            written.append(self._write_side(write, '.diagnostics', writer))
        sdist.on_rank_zero(write_files)
        return written[0] if written else None

    @property
    def diagnostics_file(self):
        """`<out>/<catchment>.SMART.<func>.diagnostics`: beside the sampling database, whatever its format."""
        return self._side_file('.diagnostics')
