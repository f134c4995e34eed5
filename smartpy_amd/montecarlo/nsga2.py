"""Multi-objective calibration of the SMART parameters by NSGA-II (no counterpart in the reference, whose sampling tool
ships NSGA-II beside the plain Monte-Carlo loop the reference wraps).

Pareto picks the non-dominated rows of a sample that was drawn once; this workflow MOVES its rows towards the Pareto front:
a population of N rows in lockstep, one ensemble launch per generation, and around it one call of smart_nsga2_step_hip
(smartpy_amd/nsga2.py) that ranks parents and offspring together from the objective table the launch has just left on the
device, keeps the N best by non-dominated rank and crowding distance, and makes the next offspring by differential
evolution on that selection (NSDE / GDE3).  What is left is a MonteCarlo object like any other: the final population as the
sample, device_obj_fns, device_gw and the database, for GLUE / Best / Pareto with `sampling=` and every analysis of the
stored matrix.
"""
import numpy as np

from .generational import GW_FLAG_COLUMN, N_CARRY, Generational
from .montecarlo import MonteCarlo
from .pareto import Pareto
from .. import nsga2 as core
from ..engine import SmartEngineError


class NSGA2(Generational):
    """Move a population towards the Pareto front of several objective functions.

    objectives: as for Pareto -- a dict {name of an objective function: direction} or a list of names taking
    Pareto.DEFAULT_DIRECTIONS; a direction is 'max', 'min' or ('target', value); between two and four of them.
    population: N, the rows of every launch (4 .. 8192); generations: launches after the initial one; f: the weight of the
    difference of two rows; cr: the crossover probability of a dimension; b_star: the width of the uniform jitter, as a
    share of each range.  There is no simulated binary crossover and no polynomial mutation: both need pow, which is not
    correctly rounded, and the step is defined to the bit (smartpy_amd/nsga2.py).  vary / fixed: as for DEMCz (default: all
    ten vary; a parameter that does not stays at fixed[name], or at the middle of its range).  gw_constraint=True: only
    the rows that meet the groundwater constraint of the settings file take part in the ranking.  seed: of the initial
    Latin hypercube (sampling.latin_hypercube over model.parameters.ranges) and of the counter-based draws of the
    variation: the same seed gives the same bits.

    run() leaves the final population as the sample, IN TOURNAMENT ORDER (rank ascending, crowding distance descending),
    obj_fns / device_obj_fns / device_gw of those rows as they were carried, `rank` and `crowding` (numpy, per row),
    `front_index` (the rows of rank 1), `keys` (device tensor [N, M]: larger is better), `diagnostics` ([rows, 2 + M]:
    generation, size of front 1, best key per objective -- one row every `thin` generations and the last one) and the
    database `<catchment>.SMART.nsga2`."""

    def __init__(self, catchment, root_f, in_format, out_format, objectives,
                 population=1024, generations=100, f=0.5, cr=0.9, b_star=1e-6, vary=None, fixed=None,
                 gw_constraint=False, seed=0, settings_filename=None, thin=10):
        MonteCarlo.__init__(self, catchment, root_f, in_format, out_format,
                            parallel='seq', save_sim=False, func='nsga2', settings_filename=settings_filename)
        if not isinstance(objectives, dict):
            objectives = {name: Pareto.DEFAULT_DIRECTIONS.get(name, 'max') for name in objectives}
        self.population, self.generations, self.thin = int(population), int(generations), int(thin)
        self.f, self.cr, self.b_star, self.seed = float(f), float(cr), float(b_star), seed
        self.gw_constraint = bool(gw_constraint)
        if not 2 <= len(objectives) <= core._lib.NSGA2_MAX_OBJECTIVES:
            raise SmartEngineError(-2, "NSGA2: {} objectives, between 2 and {}.".format(
                len(objectives), core._lib.NSGA2_MAX_OBJECTIVES))
        unknown = [name for name in objectives if name not in self.obj_fn_names]
        if unknown:
            raise SmartEngineError(-7, "NSGA2: the objective function(s) {} are not among {}.".format(
                unknown, self.obj_fn_names))
        if not 4 <= self.population <= core._lib.NSGA2_MAX_ROWS:
            raise SmartEngineError(-2, "NSGA2: a population of {} rows, between 4 and {}.".format(
                population, core._lib.NSGA2_MAX_ROWS))
        if self.generations < 1 or self.thin < 1:
            raise SmartEngineError(-2, "NSGA2: need generations >= 1 and thin >= 1 (got {}, {}).".format(generations, thin))
        if gw_constraint and not self.constraints['gw']:
            raise SmartEngineError(-2, "NSGA2: gw_constraint needs the groundwater constraint of the settings file.")
        core.cr_threshold(self.cr)
        self._check_observations()
        self.objective_names = list(objectives)
        self.directions = [objectives[name] for name in objectives]
        self.objectives = [(self.obj_fn_names.index(name), objectives[name]) for name in objectives]
        core.directions_of(self.objectives)
        fixed = self._resolve_box(vary, fixed, max_dims=core._lib.NSGA2_MAX_DIMS)
        self._start_from(self.population, fixed)
        self.rank = self.crowding = self.front_index = self.keys = self.diagnostics = self.state = None

    def _new_state(self, population, device):
        """The population on the device: the launch matrix is the population at full width"""
        rows = self._device_rows(population, device)
        return core.Nsga2State(rows[:, self.columns], self.lo, self.hi, self.objectives,
                               seed=0 if self.seed is None else self.seed, f=self.f, cr=self.cr, b_star=self.b_star,
                               n_carry=N_CARRY, columns=self.columns, rows=rows, device=device)

    def _launch_population(self, state):
        """One launch over the launch matrix -> (the [N, 8] objective table, read in place by the step; the payload
        [N, 9]; the eligible flags or None)"""
        import torch
        n = self.population
        # (a view of its own per launch: what the engine remembers about a tensor object is not asked about rows that the
        # step kernel rewrites behind torch's back)
        _, table, payload = self._launch(state.rows.view(n, len(self.param_names)))
        eligible = (table[:, GW_FLAG_COLUMN] > 0.0).to(torch.uint8).contiguous() if self.gw_constraint else None
        return table, payload, eligible

    def _diagnostics_row(self, g, state):
        import torch
        keys = torch.where(torch.isnan(state.keys), torch.full_like(state.keys, float('-inf')), state.keys)
        return torch.cat([torch.tensor([float(g)], dtype=torch.float64, device=state.device),
                          state.counts[1:2].to(torch.float64), keys.max(dim=0)[0]])

    # ---- run -----------------------------------------------------------------------------------------------------
    def run(self, compression=None, write=False):
        """The generations, then the database.  One launch and one step call per generation; the caller reads nothing in
        between (the diagnostics are gathered on the device and read once at the end).  write=True also writes
        `<catchment>.SMART.nsga2.diagnostics` (generation, front_size, best_<objective> ...).  Under torch.distributed
        every rank computes everything itself and rank 0 alone writes."""
        import torch
        from ..engine import default_device
        population = self._population_of_all_ranks()
        G = self.generations
        device = default_device()
        state = self._new_state(population, device)
        rows = []
        for g in range(0, G + 1):
            table, payload, eligible = self._launch_population(state)
            core.nsga2_step(state, scores=table, carry_new=payload, eligible=eligible, vary=g < G)
            if g % self.thin == 0 or g == G:
                rows.append(self._diagnostics_row(g, state))
        self.state = state
        self.diagnostics = torch.stack(rows).cpu().numpy()
        # ---- the MonteCarlo object every second stage and analysis takes: the final population, in tournament order
        self._adopt(self._full_rows(population, state.x), state.carry)
        self.keys = state.keys
        self.rank, self.crowding = state.rank.cpu().numpy(), state.crowding.cpu().numpy()
        self.front_index = np.nonzero(self.rank == 1)[0]
        self.diagnostics_written = self._write_files(compression, write, lambda path: core.write_diagnostics(
            path, self.objective_names, self.diagnostics))
