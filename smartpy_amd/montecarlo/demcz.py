"""DE-MCz posterior sampling of the SMART parameters (no counterpart in the reference, whose sampling tool ships DE-MCz
and DREAM beside the plain Monte-Carlo loop the reference wraps).

Every other workflow here works on a sample drawn once; this one MOVES its rows towards the posterior: N chains in
lockstep, one ensemble launch per generation, and around it one call of smart_demcz_step_hip (smartpy_amd/demcz.py) that
decides on the proposals the launch has just scored, appends to the archive every `thin`-th generation and proposes the
next rows -- differential evolution with sampling from the past (ter Braak & Vrugt 2008), subspace crossover as in DREAM
(Vrugt 2016), a uniform prior on the parameter ranges.  What is left is a MonteCarlo object like any other: the sample,
device_obj_fns, device_gw and the database, for GLUE / Best / Pareto with `sampling=` and every analysis of the stored
matrix.
"""
import math

import numpy as np

from .generational import GW_FLAG_COLUMN, N_CARRY, Generational
from .montecarlo import MonteCarlo, OBJ_FN_NAMES
from .. import demcz as core
from .. import errormodel
from ..engine import SmartEngineError
from ..sampling import latin_hypercube

RMSE_COLUMN = OBJ_FN_NAMES.index('RMSE')


class DEMCz(Generational):
    """Sample the posterior of the parameters given the observed flow.

    chains: N, the rows of every launch; generations: launches after the initial one; thin: every thin-th generation is
    archived (the archive is what proposals are drawn from AND what the posterior sample is taken from); burn_in: the
    share of the archived snapshots that is dropped from the sample; cr: the crossover probability of a dimension;
    p_jump: the share of proposals with gamma = 1 (mode jumping); b_star: the width of the uniform jitter, as a share
    of each range.  likelihood='gaussian': independent Gaussian errors on the report steps that carry an observation --
    sigma=None integrates the error variance out (log-density -(n_eff / 2) ln(n RMSE^2)), a number fixes it
    (-n_eff RMSE^2 / (2 sigma^2)); n_eff (default: n, the observed report steps) is the number of observations the
    errors are worth, for autocorrelated residuals.  likelihood='ar1': the residual error model of smartpy_amd.errormodel
    -- a standard deviation sigma0 + sigma1 sim_t and an AR(1) with coefficient phi on the standardised residuals -- whose
    parameters are inferred with the model's: error_model maps 'sigma0' / 'sigma1' / 'phi' to a (lo, hi) range (the
    parameter is a further dimension of the chains, initialised by the same Latin hypercube call over the widened ranges)
    or to a number (it is fixed); a name that is missing takes errormodel.default_ranges.  The launch matrix is then 13
    columns wide: the step kernel writes the error parameters like any other, the model launch sees a copy of the ten
    model columns, and a generation is the launch with the discharge matrix kept, engine.residual_log_likelihood on the
    matrix where it lies (the error parameters read in place from the launch matrix) and the step with a ready
    log-density.  sigma= and n_eff= do not go with 'ar1'.  vary / fixed: as for Sobol (default: all ten vary; a parameter
    that does not stays at fixed[name], or at the middle of its range).  gw_prior=True gives a row that fails the
    groundwater constraint of the settings file the log-density -inf.  seed: of the initial Latin hypercube
    (sampling.latin_hypercube over model.parameters.ranges) and of the counter-based draws of the chains: the same seed
    gives the same bits.

    run() leaves `posterior` (demcz.PosteriorSample; with 'ar1' its `error_parameters` [n, 3] hold sigma0, sigma1, phi of
    every archived row, fixed ones filled in, and `names`, `rhat` and `diagnostics` cover the sampled error parameters
    after the model's), `log_density`, `acceptance_rate`, `rhat`, `diagnostics`, the sample
    (the archived rows after the burn-in, full parameter width), obj_fns / device_obj_fns / device_gw of those rows as the
    chains carried them, and the database `<catchment>.SMART.demcz`."""

    def __init__(self, catchment, root_f, in_format, out_format,
                 chains=1024, generations=500, thin=10, burn_in=0.5, cr=0.9, p_jump=0.1, b_star=1e-6,
                 likelihood='gaussian', sigma=None, n_eff=None, vary=None, fixed=None, gw_prior=False, seed=0,
                 settings_filename=None, error_model=None):
        MonteCarlo.__init__(self, catchment, root_f, in_format, out_format,
                            parallel='seq', save_sim=False, func='demcz', settings_filename=settings_filename)
        self.chains, self.generations, self.thin = int(chains), int(generations), int(thin)
        self.burn_in, self.cr, self.p_jump, self.b_star = float(burn_in), float(cr), float(p_jump), float(b_star)
        self.likelihood, self.sigma, self.gw_prior, self.seed = likelihood, sigma, bool(gw_prior), seed
        if self.chains < 2 or self.generations < 1 or self.thin < 1:
            raise SmartEngineError(-2, "DEMCz: need chains >= 2, generations >= 1 and thin >= 1 (got {}, {}, {})."
                                   .format(chains, generations, thin))
        if not 0.0 <= self.burn_in < 1.0:
            raise SmartEngineError(-2, "DEMCz: burn_in {} must be in [0, 1).".format(burn_in))
        if likelihood not in ('gaussian', 'ar1'):
            raise SmartEngineError(-7, "DEMCz: likelihood '{}' unknown.".format(likelihood))
        if likelihood == 'ar1' and (sigma is not None or n_eff is not None):
            raise SmartEngineError(-2, "DEMCz: sigma= and n_eff= belong to likelihood='gaussian'; 'ar1' infers its error "
                                       "parameters (error_model=).")
        if likelihood != 'ar1' and error_model is not None:
            raise SmartEngineError(-2, "DEMCz: error_model= belongs to likelihood='ar1'.")
        if gw_prior and not self.constraints['gw']:
            raise SmartEngineError(-2, "DEMCz: gw_prior needs the groundwater constraint of the settings file.")
        core.thresholds(self.p_jump, self.cr)
        self._check_observations()
        self.n_obs = int(np.count_nonzero(~np.isnan(np.asarray(self.model.nd_flow, dtype=np.float64))))
        self.n_eff = float(self.n_obs if n_eff is None else n_eff)
        fixed = self._resolve_box(vary, fixed)
        names, ranges = list(self.param_names), self.model.parameters.ranges
        population = None
        self.error_sampled, self.error_fixed = [], {}
        if likelihood == 'ar1':
            # the sampled error parameters: further dimensions of the chains, further columns of the launch matrix
            self.error_sampled, error_ranges, self.error_fixed = errormodel.resolve(error_model, self.model.nd_flow)
            if len(self.vary) + len(self.error_sampled) > core._lib.DEMCZ_MAX_DIMS:
                raise SmartEngineError(-2, "DEMCz: {} dimensions, at most {}.".format(
                    len(self.vary) + len(self.error_sampled), core._lib.DEMCZ_MAX_DIMS))
            widened = dict((p, ranges[p]) for p in names)
            widened.update(error_ranges)
            drawn = latin_hypercube(self.chains, widened, names + self.error_sampled, seed=seed)
            population = np.empty((self.chains, len(names) + len(errormodel.PARAMETER_NAMES)), dtype=np.float64)
            population[:, :len(names)] = drawn[:, :len(names)]
            for k, p in enumerate(errormodel.PARAMETER_NAMES):
                population[:, len(names) + k] = drawn[:, len(names) + self.error_sampled.index(p)] \
                    if p in self.error_sampled else self.error_fixed[p]
            self.columns += [len(names) + errormodel.PARAMETER_NAMES.index(p) for p in self.error_sampled]
            self.lo = np.concatenate([self.lo, [error_ranges[p][0] for p in self.error_sampled]])
            self.hi = np.concatenate([self.hi, [error_ranges[p][1] for p in self.error_sampled]])
        self._start_from(self.chains, fixed, population)
        self.posterior = self.log_density = self.acceptance_rate = self.rhat = self.diagnostics = None

    # ---- the log-density of a score ---------------------------------------------------------------------------
    @property
    def score_kind(self):
        if self.likelihood == 'ar1':
            return 'logp'
        return 'rmse' if self.sigma is None else 'rmse_sigma'

    @property
    def dimension_names(self):
        """The dimensions of the chains: the model parameters that vary, then the error parameters that are sampled"""
        return self.vary + self.error_sampled

    def log_density_of(self, rmse):
        """The log-density the chains are moved by, from the RMSE of a row (array or tensor; answered in kind)"""
        log = np.log if isinstance(rmse, np.ndarray) else __import__('torch').log
        if self.sigma is None:
            return -((self.n_eff * 0.5) * log(self.n_obs * (rmse * rmse)))
        return -(self.n_eff * (rmse * rmse)) / ((2.0 * float(self.sigma)) * float(self.sigma))

    def _new_state(self, population, snapshots, device):
        """The chains on the device: the launch matrix is the population at full width, the archive holds `snapshots` of
        the chains"""
        rows = self._device_rows(population, device)
        return core.DemczState(rows[:, self.columns], self.lo, self.hi, capacity=int(snapshots) * self.chains,
                               seed=0 if self.seed is None else self.seed, cr=self.cr, p_jump=self.p_jump,
                               b_star=self.b_star, n_carry=N_CARRY, columns=self.columns, rows=rows,
                               score_kind=self.score_kind, n_obs=self.n_obs, n_eff=self.n_eff,
                               sigma=0.0 if self.sigma is None else float(self.sigma), device=device)

    def _launch_chains(self, state):
        """One launch over the launch matrix of the chains -> (scores [N] at a stride, payload [N, 9])"""
        import torch
        if self.likelihood == 'ar1':
            return self._launch_chains_ar1(state)
        # (a view of its own per launch: what the engine remembers about a tensor object is not asked about rows that the
        # step kernel rewrites behind torch's back)
        _, table, payload = self._launch(state.rows.view(self.chains, len(self.param_names)))
        scores = table[:, RMSE_COLUMN]                      # read in place: stride 8
        if self.gw_prior:
            scores = torch.where(table[:, GW_FLAG_COLUMN] > 0.0, scores, torch.full_like(scores, float('inf')))
        return scores, payload

    def _launch_chains_ar1(self, state):
        """The launch of a generation with likelihood='ar1' -> (log-likelihoods [N], payload [N, 9]): the model runs on a
        contiguous copy of the ten model columns of the launch matrix (the engine takes a dense [N, 10]), keeps the [R, N]
        matrix, and the likelihood kernel reads it where it lies, with the three error columns of the launch matrix at
        the stride of its rows"""
        import torch
        from .. import engine
        w = len(self.param_names)
        out, table, payload = self._launch(state.rows[:, :w].contiguous(), save_discharge=True)
        theta = state.rows[:, w:w + len(errormodel.PARAMETER_NAMES)]
        scores = engine.residual_log_likelihood(out.discharge_report_major, self.model._device_cache[2], theta)[0]
        if self.gw_prior:
            scores = torch.where(table[:, GW_FLAG_COLUMN] > 0.0, scores, torch.full_like(scores, float('-inf')))
        return scores, payload

    def _check_memory(self, device):
        """likelihood='ar1' keeps the [R, N] discharge matrix of a launch on the device: a chain count whose matrix does
        not fit what is free there is refused before the first launch"""
        import torch
        R = len(self.model.timeseries_report) - 1
        need = 8 * R * self.chains
        free = torch.cuda.mem_get_info(device)[0]
        if need > free:
            raise SmartEngineError(-2, "DEMCz: likelihood='ar1' stores the [{}, {}] discharge matrix of a launch, {} bytes, "
                                       "and the device has {} free: fewer chains, or a shorter period."
                                   .format(R, self.chains, need, free))

    # ---- run -----------------------------------------------------------------------------------------------------
    def run(self, compression=None, write=False):
        """The chains, then the database.  One step call and one launch per generation, nothing copied to the host in
        between beyond what the engine's own preparation reads.  write=True also writes
        `<catchment>.SMART.demcz.diagnostics` (generation, acceptance_rate, Rhat_<p> per archived generation).  Under
        torch.distributed every rank computes everything itself and rank 0 alone writes."""
        import torch
        from ..engine import default_device
        population = self._population_of_all_ranks()
        N, G, thin, d = self.chains, self.generations, self.thin, len(self.dimension_names)
        S = 1 + G // thin
        device = default_device()
        if self.likelihood == 'ar1':
            self._check_memory(device)
        state = self._new_state(population, S, device)
        accepted_at = [torch.zeros((), dtype=torch.int64, device=device)]
        scores, payload = self._launch_chains(state)
        core.demcz_step(state, scores=scores, carry_new=payload, append=True, propose=True)     # the initial population
        for g in range(1, G + 1):
            scores, payload = self._launch_chains(state)
            core.demcz_step(state, scores=scores, carry_new=payload, append=g % thin == 0, propose=g < G)
            if g % thin == 0:
                accepted_at.append(state.accepted.sum())
        assert state.M == S * N
        # ---- what the archive holds
        history = state.archive.view(S, N, d)
        history_logp = state.archive_logp.view(S, N)
        first = min(S - 1, int(math.floor(self.burn_in * S)))
        sample_d = state.archive[first * N:]
        carry = state.archive_carry[first * N:]
        full = self._full_rows(population, sample_d)
        # (with 'ar1' the rows are 13 wide: the ten model columns are the sample, the last three the error parameters)
        width = len(self.param_names)
        error_parameters = full[:, width:].contiguous() if self.likelihood == 'ar1' else None
        full = full[:, :width].contiguous()
        accepted = state.accepted.cpu().numpy()
        gens = np.arange(S) * thin
        counts = torch.stack(accepted_at).cpu().numpy().astype(np.float64)
        rates = np.where(gens > 0, counts / np.maximum(gens * N, 1), np.nan)
        rhats = np.stack([core.gelman_rubin(history[:s + 1]).cpu().numpy() for s in range(S)])
        self.diagnostics = np.concatenate([gens[:, None].astype(np.float64), rates[:, None], rhats], axis=1)
        self.rhat = rhats[-1]
        self.acceptance_rate = float(accepted.sum()) / float(N * G)
        self.log_density = history_logp.reshape(-1)[first * N:]
        self.state = state
        self._adopt(full, carry)
        self.posterior = core.PosteriorSample(self.dimension_names, sample_d, self.log_density, carry, history,
                                              history_logp, accepted, self.rhat, self.acceptance_rate, self.diagnostics,
                                              first, error_parameters=error_parameters)
        self.posterior.file = self._write_files(compression, write, lambda path: core.write_diagnostics(
            path, self.dimension_names, self.diagnostics))

    def _default_error_parameters(self):
        """what residual_likelihood and predictive_bounds take where none are given: the archived ones of an 'ar1' run"""
        if self.posterior is None or self.posterior.error_parameters is None:
            return None
        return self.posterior.error_parameters.cpu().numpy()
