"""Sequential data assimilation by a bootstrap particle filter (Gordon et al. 1993; systematic resampling: Kitagawa 1996),
the part around the model: the particles on the device (ParticleState: launch rows, the twelve model states and the
log-weights, each in two halves, the header of the last step and the workspace) and the thin binding of the one C entry that
assimilates a window (particle_step -> smart_particle_step_hip, include/smart_amd.h: weigh the particles by the window's
observations, turn the weights into integers, resample where the effective sample size has fallen below tau N, jitter the
parameters and perturb the states).  montecarlo.ParticleFilter puts the SMART ensemble launch of a window between two
steps; any other model can stand there (tests/test_gpu_particle_filter.py plays one).

From the integers on nothing is floating point, so the resampling has one answer: the numpy statement of the tests
(tests/cases_particle_filter.py) holds the kernels to it bit for bit.
"""
import ctypes

import numpy as np

from . import _lib, generational
from ._lib import SmartEngineError

ALL_PHASES = _lib.PARTICLE_WEIGH | _lib.PARTICLE_RESAMPLE | _lib.PARTICLE_MOVE
UNIT = 1 << 22      # the integer a particle of the largest weight gets
Z_COLUMN = 5        # of a row of the ten model parameters (parameters.py)


def noise_of(state_noise):
    """a number (every state alike) or twelve -> the twelve relative widths the entry takes"""
    noise = np.ascontiguousarray(np.broadcast_to(np.asarray(state_noise, dtype=np.float64), (_lib.PARTICLE_STATES,)))
    if not np.all((noise >= 0.0) & (noise < 1.0)):
        raise SmartEngineError(-2, "particle: state_noise {} must be in [0, 1).".format(state_noise))
    return noise


class ParticleState(generational.BoxState):
    """N particles on the device, and what the host keeps of them.

    Device tensors, each with a second half that the next step writes (`*_next`; a step that moves swaps the halves): rows
    [N, ld] (the launch matrix: the step writes the d columns `columns`, the others are the caller's in both halves),
    states [N, 12] (what the engine takes as `initial`) and logw [N].  Of the last step: q [N] int64 (the integer weights
    after the update), parents [N] int32, stats [4] (ess, evidence increment, the two maxima) and counts [8] int64
    (resampled, Q, distinct parents, flags, offset, S2, Q of the prior) -- _lib.PARTICLE_STATS / PARTICLE_COUNTS name them --
    and the workspace of the entry.  Host: k (the window the next step assimilates, 0 at first), seed, lo, hi, scale =
    jitter (hi - lo), noise [12], sigma0, sigma1, tau, z_column, area_m2.

    rows: [N, ld], the launch matrix (host or device); states: [N, 12]."""

    def __init__(self, rows, states, lo, hi, columns, area_m2, sigma=(1.0, 0.0), tau=0.5, state_noise=0.0, jitter=0.0,
                 seed=0, z_column=Z_COLUMN, device=None):
        import torch
        from .engine import as_device
        matrix = self._place('particle', 'particles', rows, device)
        device = self.device
        N = matrix.shape[0]
        columns = np.ascontiguousarray(columns, dtype=np.int32).reshape(-1)
        d = len(columns)
        if not 1 <= N <= _lib.PARTICLE_MAX_PARTICLES:
            raise SmartEngineError(-2, "particle: {} particles, between 1 and {}.".format(N, _lib.PARTICLE_MAX_PARTICLES))
        if not 1 <= d <= _lib.PARTICLE_MAX_DIMS:
            raise SmartEngineError(-2, "particle: {} dimensions, between 1 and {}.".format(d, _lib.PARTICLE_MAX_DIMS))
        if not float(jitter) >= 0.0:
            raise SmartEngineError(-2, "particle: jitter {} must be >= 0.".format(jitter))
        self.n_particles, self.n_dims = N, d
        self._set_box('particle', matrix[:, torch.from_numpy(columns.astype(np.int64)).to(device)], lo, hi, jitter, seed,
                      columns, None, matrix, 0.0)
        self.rows_next = self.rows.clone()
        self.states = as_device(states, device).clone().contiguous()
        if tuple(self.states.shape) != (N, _lib.PARTICLE_STATES):
            raise SmartEngineError(-2, "particle: the states must be [{}, {}], not {}."
                                   .format(N, _lib.PARTICLE_STATES, tuple(self.states.shape)))
        self.states_next = self.states.clone()
        self.logw = torch.zeros((N,), dtype=torch.float64, device=device)
        self.logw_next = torch.zeros_like(self.logw)
        self.sigma0, self.sigma1, self.tau = float(sigma[0]), float(sigma[1]), float(tau)
        self.noise = noise_of(state_noise)
        self.z_column, self.area_m2 = int(z_column), float(area_m2)
        self.q = torch.full((N,), UNIT, dtype=torch.int64, device=device)
        self.parents = torch.arange(N, dtype=torch.int32, device=device)
        self.stats = torch.zeros((4,), dtype=torch.float64, device=device)
        self.counts = torch.zeros((8,), dtype=torch.int64, device=device)
        need = int(_lib.lib().smart_particle_workspace_bytes(N))
        if need < 0:
            raise SmartEngineError(need, "particle: no workspace for {} particles.".format(N))
        self.workspace = torch.empty((need,), dtype=torch.uint8, device=device)
        self.k = 0


def _dbl(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def particle_step(state, sim=None, obs=None, q_in=None, offset=-1, phases=ALL_PHASES):
    """One call of smart_particle_step_hip on torch's current stream (include/smart_amd.h has the definition).

    sim: the window's discharge as the launch left it, a float64 device tensor [Rw, >= N] whose rows lie at a constant
    stride (read in place); obs: a float64 device tensor [Rw], NaN where nothing was observed.  q_in: None, or an int64
    device tensor [N] of integer weights in 0 .. 2^22 that stand in for the weighing (sim and obs are not read then).
    offset: < 0 for the drawn offset of the comb, else the offset itself.  phases: a mask of _lib.PARTICLE_WEIGH,
    PARTICLE_RESAMPLE and PARTICLE_MOVE; a call that moves swaps the halves of the state and moves state.k on, so that
    state.rows, state.states and state.logw are what the next window is launched from."""
    import torch
    s = state
    L = _lib.lib()
    N = s.n_particles
    sim_ptr = obs_ptr = None
    Rw = ld_sim = 0
    if sim is not None or obs is not None:
        if not (isinstance(sim, torch.Tensor) and sim.is_cuda and sim.dtype == torch.float64 and sim.dim() == 2
                and sim.shape[1] >= N and sim.stride(1) == 1):
            raise SmartEngineError(-2, "particle_step: sim must be a float64 device tensor [reports, >= {}].".format(N))
        Rw = sim.shape[0]
        ld_sim = sim.stride(0) if Rw > 1 else sim.shape[1]
        if not (isinstance(obs, torch.Tensor) and obs.is_cuda and obs.dtype == torch.float64
                and tuple(obs.shape) == (Rw,) and obs.is_contiguous()):
            raise SmartEngineError(-2, "particle_step: obs must be a contiguous float64 device tensor [{}].".format(Rw))
        sim_ptr, obs_ptr = sim.data_ptr(), obs.data_ptr()
    if q_in is not None and not (isinstance(q_in, torch.Tensor) and q_in.is_cuda and q_in.dtype == torch.int64
                                 and tuple(q_in.shape) == (N,) and q_in.is_contiguous()):
        raise SmartEngineError(-2, "particle_step: q_in must be a contiguous int64 device tensor [{}].".format(N))
    with torch.cuda.device(s.device):
        _lib.check(L.smart_particle_step_hip(
            N, s.n_dims, s.seed, s.k, int(phases), Rw, sim_ptr, ld_sim, obs_ptr, s.sigma0, s.sigma1, s.tau,
            None if q_in is None else q_in.data_ptr(), int(offset),
            s.rows.data_ptr(), s.rows_next.data_ptr(), s.ld, s.columns.ctypes.data_as(ctypes.c_void_p), s.z_column,
            s.area_m2, _dbl(s.lo), _dbl(s.hi), _dbl(s.scale), _dbl(s.noise),
            s.states.data_ptr(), s.states_next.data_ptr(), s.logw.data_ptr(), s.logw_next.data_ptr(),
            s.q.data_ptr(), s.parents.data_ptr(), s.stats.data_ptr(), s.counts.data_ptr(),
            s.workspace.data_ptr(), s.workspace.numel(), torch.cuda.current_stream(s.device).cuda_stream))
    if int(phases) & _lib.PARTICLE_MOVE:
        s.rows, s.rows_next = s.rows_next, s.rows
        s.states, s.states_next = s.states_next, s.states
        s.logw, s.logw_next = s.logw_next, s.logw
        s.k += 1
    return s


DIAGNOSTICS_COLUMNS = ['window', 'resampled', 'distinct_parents', 'flags', 'ess', 'log_evidence']


def diagnostics_header():
    """The header of `<catchment>.SMART.pf.diagnostics`"""
    return ','.join(DIAGNOSTICS_COLUMNS) + '\n'


def write_diagnostics(path, diagnostics):
    """diagnostics: rows of (window, resampled, distinct parents, flags, ess, evidence increment) -- one per window; the
    first four as integers, the others '%.6e'."""
    generational.write_diagnostics(path, diagnostics_header(), 4, diagnostics)
