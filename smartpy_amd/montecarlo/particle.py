"""Sequential data assimilation of the SMART states by a particle filter (no counterpart in the reference).

Every other workflow here conditions the PARAMETERS on the whole record at once; this one conditions the STATES: N
particles -- parameter rows with their twelve model states -- run the record window by window, one ensemble launch per
window of `assimilate_every` report steps started from the particles' own states, and after each window one call of
smart_particle_step_hip (smartpy_amd/particle.py) that weighs the particles by the window's observed flows and, where the
effective sample size has fallen below tau N, resamples them and perturbs their states (and, with jitter > 0, their
parameters).  What is left are the states and parameters consistent with the flows up to the end of the record -- the
starting point of a forecast -- with the one-window-ahead forecast and the analysis quantiles per report step.
"""
import numpy as np

from .generational import Generational
from .montecarlo import MonteCarlo
from .selection import write_text_table
from .. import particle as core
from .. import structure
from ..engine import SmartEngineError

STATES_FROM = 7      # the twelve states are columns 7 .. 18 of final_vars


class ParticleFilter(Generational):
    """Filter the states (and, with jitter, the parameters) given the observed flow.

    particles: N, the rows of every launch (None: as many as `sampling` holds); assimilate_every: the report steps of a
    window; sigma = (sigma0, sigma1): the standard deviation sigma0 + sigma1 |obs| of the observation error; tau: the
    particles are resampled where the effective sample size falls below tau N; state_noise: the relative width of the
    uniform perturbation of every state after an update (a number, or twelve; without any the filter degenerates);
    jitter: the width of the uniform jitter of the varying parameters, as a share of each range (0: the parameters of a
    particle never change; a child whose jittered row leaves the box even after one reflection takes its parent's WHOLE
    row, the rule of the generational samplers, so with a jitter of the order of the ranges many children lose all of
    theirs); vary / fixed: as for DEMCz -- a parameter that does not vary has ONE value for every particle, fixed[name] or
    the middle of its range, whatever the rows came from: the step writes the varying columns of a child only, so a
    column that differed from row to row would pair a parent's parameters and states with another row's; sampling: a
    finished MonteCarlo object (LHS, a DE-MCz posterior) whose sample gives the varying columns of the initial rows --
    with particles=n below its size, n rows at equal strides through it (a posterior's archive is ordered by generation)
    -- otherwise a Latin hypercube over the ranges; seed: of that hypercube and of the counter-based draws of the filter:
    the same seed gives the same bits.

    run() leaves forecast_bounds and analysis_bounds ([K, R]: the quantiles `probs` of the window's discharge under the
    weights before and after the update), analysis_mean [R], ess and resampled (per window), log_evidence (the sum of
    the windows' increments), diagnostics ([windows, 6]: window, resampled, distinct parents, flags, ess, evidence
    increment), states ([N, 12], device: valid as engine.run_ensemble(initial=)), parameters ([N, 10], device), weights
    ([N], device, summing to 1) and, with verify=True, verification ([5, R]: engine.ensemble_scores of the forecast)."""

    def __init__(self, catchment, root_f, in_format, out_format, particles=None, assimilate_every=1, sigma=(0.1, 0.1),
                 tau=0.5, state_noise=0.05, jitter=0.0, vary=None, fixed=None, sampling=None, seed=None,
                 settings_filename=None, probs=(0.05, 0.5, 0.95)):
        MonteCarlo.__init__(self, catchment, root_f, in_format, out_format,
                            parallel='seq', save_sim=False, func='pf', settings_filename=settings_filename)
        population = None
        if sampling is not None:
            population = np.array(sampling._sample, dtype=np.float64)
            if particles is not None and int(particles) > population.shape[0]:
                raise SmartEngineError(-2, "ParticleFilter: {} particles from a sample of {} rows."
                                       .format(particles, population.shape[0]))
            if particles is not None:          # equal strides through the sample, not its first rows
                population = population[(np.arange(int(particles)) * population.shape[0]) // int(particles)]
        self.particles = int(population.shape[0] if particles is None and population is not None else particles or 0)
        self.assimilate_every, self.tau, self.jitter, self.seed = int(assimilate_every), float(tau), float(jitter), seed
        if not 1 <= self.particles <= core._lib.PARTICLE_MAX_PARTICLES:
            raise SmartEngineError(-2, "ParticleFilter: {} particles, between 1 and {}."
                                   .format(self.particles, core._lib.PARTICLE_MAX_PARTICLES))
        if self.assimilate_every < 1:
            raise SmartEngineError(-2, "ParticleFilter: assimilate_every {} must be >= 1.".format(assimilate_every))
        self.sigma = (float(sigma[0]), float(sigma[1]))
        if not (self.sigma[0] > 0.0 and self.sigma[1] >= 0.0 and np.isfinite(self.sigma).all()):
            raise SmartEngineError(-2, "ParticleFilter: sigma {} must be (> 0, >= 0).".format(sigma))
        if not (self.tau >= 0.0 and self.jitter >= 0.0):
            raise SmartEngineError(-2, "ParticleFilter: tau {} and jitter {} must be >= 0.".format(tau, jitter))
        self.state_noise = core.noise_of(state_noise)
        self.probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        self._check_observations()
        fixed = self._resolve_box(vary, fixed, max_dims=core._lib.PARTICLE_MAX_DIMS)
        # (the rows of a sampling run go the same way as a hypercube: their columns that do not vary are set to one value)
        self._start_from(self.particles, fixed, population)
        self.forecast_bounds = self.analysis_bounds = self.analysis_mean = self.ess = self.resampled = None
        self.log_evidence = self.diagnostics = self.states = self.parameters = self.weights = self.verification = None
        self.state = self.stored = self.file = self.diagnostics_written = None

    # ---- the time axis ---------------------------------------------------------------------------------------------
    def _axis(self):
        """-> (delta_sec, T simulation steps, gap = steps per report, n_warm, R report steps)"""
        model = self.model
        delta_sec = model.delta_simu.total_seconds()
        T = len(model.timeseries) - 1
        R = len(model.timeseries_report) - 1
        gap = T // R
        n_warm = structure.warm_up_length(model.warm_up, delta_sec, T) if model.warm_up != 0 else 0
        if T % gap or n_warm % gap:
            raise ValueError("cannot reshape array of size {} into shape ({})".format(T if T % gap else n_warm, gap))
        return delta_sec, T, gap, n_warm, R

    def _launch_window(self, state, forcing, t0, t1, axis, states, want_discharge=True):
        """One launch of the particles over the steps [t0, t1) from `states` (None: the model's own start) -> its result"""
        from .. import engine
        delta_sec, _, gap, _, _ = axis
        n, model = self.particles, self.model
        # (views of their own per launch: what the engine remembers about a tensor object is not asked about rows and
        # states that the step kernel rewrites behind torch's back)
        return engine.run_ensemble(state.rows.view(n, len(self.param_names)), forcing[t0:t1], float(model.area), delta_sec,
                                   0, gap, extra=model.extra if states is None and model.extra else None,
                                   initial=None if states is None else states.view(n, core._lib.PARTICLE_STATES),
                                   math_mode=self.math_mode, want_discharge=want_discharge, want_final=True)

    # ---- run -----------------------------------------------------------------------------------------------------
    def run(self, write=False, verify=False, store=False):
        """The windows.  One launch and one step call per window, and the two quantile calls on the window's matrix;
        nothing is read back in between (what the engine's own preparation of a launch reads apart): the header of every
        step is gathered on the device and read once at the end.  write=True writes `<catchment>.SMART.pf` (DateTime,
        observed, the forecast and the analysis quantiles per report step) and `<catchment>.SMART.pf.diagnostics`.
        store=True keeps, as device tensors in `stored`, the discharge of every particle as it was forecast ([R, N]) and
        the integer weights and the parents of every window ([windows, N] each)."""
        import torch
        from .. import engine
        from ..engine import as_device, default_device
        device = default_device()
        axis = self._axis()
        delta_sec, T, gap, n_warm, R = axis
        model, N, A = self.model, self.particles, self.assimilate_every
        forcing = model._device_forcing(device)
        obs = model._device_cache[2]
        # (seed=None draws from NumPy's global stream: under torch.distributed rank 0's rows are THE rows)
        self.initial_population = self._population_of_all_ranks()
        rows = as_device(self.initial_population[:, :len(self.param_names)], device).clone().contiguous()
        state = core.ParticleState(rows, torch.zeros((N, core._lib.PARTICLE_STATES), dtype=torch.float64, device=device),
                                   self.lo, self.hi, self.columns, float(model.area), sigma=self.sigma, tau=self.tau,
                                   state_noise=self.state_noise, jitter=self.jitter,
                                   seed=0 if self.seed is None else self.seed, device=device)
        started = False
        if n_warm:      # the spin-up: the reference's states after the warm-up
            spin = self._launch_window(state, forcing, 0, n_warm, axis, None, want_discharge=False)
            state.states.copy_(spin.final_vars[:, STATES_FROM:])
            started = True
        unit = torch.full((N,), core.UNIT, dtype=torch.int64, device=device)
        prior = unit.clone()
        forecast, analysis, mean, stats, counts, scores = [], [], [], [], [], []
        kept = dict(discharge=[], q=[], parents=[])
        for r0 in range(0, R, A):
            r1 = min(r0 + A, R)
            out = self._launch_window(state, forcing, r0 * gap, r1 * gap, axis, state.states if started else None)
            started = True
            matrix = out.discharge_report_major
            state.states.copy_(out.final_vars[:, STATES_FROM:])
            weights = prior.double()
            forecast.append(engine.weighted_quantiles(matrix, self.probs, weights))
            if verify:
                scores.append(engine.ensemble_scores(matrix, obs[r0:r1], weights))
            core.particle_step(state, matrix, obs[r0:r1].contiguous())
            weights = state.q.double()
            analysis.append(engine.weighted_quantiles(matrix, self.probs, weights))
            # (a particle of weight 0 takes no part, whatever its value)
            mean.append(torch.where(weights > 0.0, matrix * weights, torch.zeros_like(matrix)).sum(dim=1) / weights.sum())
            stats.append(state.stats.clone())
            counts.append(state.counts.clone())
            if store:
                kept['discharge'].append(matrix.clone())
                kept['q'].append(state.q.clone())
                kept['parents'].append(state.parents.clone())
            prior = torch.where(state.counts[0] != 0, unit, state.q)
        # ---- what the filter leaves
        self.state = state
        self.forecast_bounds = torch.cat(forecast, dim=1).cpu().numpy()
        self.analysis_bounds = torch.cat(analysis, dim=1).cpu().numpy()
        self.analysis_mean = torch.cat(mean).cpu().numpy()
        stats, counts = torch.stack(stats).cpu().numpy(), torch.stack(counts).cpu().numpy()
        self.ess, self.resampled = stats[:, 0], counts[:, 0].astype(bool)
        self.log_evidence = float(stats[:, 1].sum())
        self.diagnostics = np.column_stack([np.arange(len(stats)), counts[:, 0], counts[:, 2], counts[:, 3], stats[:, 0],
                                            stats[:, 1]]).astype(np.float64)
        self.states, self.parameters = state.states, state.rows
        self.weights = prior.double() / prior.double().sum()
        self.verification = torch.cat(scores, dim=1).cpu().numpy() if verify else None
        self.stored = dict(discharge=torch.cat(kept['discharge']), q=torch.stack(kept['q']),
                           parents=torch.stack(kept['parents'])) if store else None
        self._set_sample(state.rows)
        stamps = model.timeseries_report[1:]
        header = ','.join(['DateTime', 'observed'] + ['forecast_q%g' % p for p in self.probs] +
                          ['analysis_q%g' % p for p in self.probs] + ['analysis_mean'])
        table = np.column_stack([np.asarray(model.nd_flow, dtype=np.float64)[:R], self.forecast_bounds.T,
                                 self.analysis_bounds.T, self.analysis_mean])
        self.file = self._write_side(write, '', lambda path: write_text_table(path, header, table, '%e', '\r\n',
                                                                              labels=stamps))
        self.diagnostics_written = self._write_side(write, '.diagnostics',
                                                    lambda path: core.write_diagnostics(path, self.diagnostics))
        return self
