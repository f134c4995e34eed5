"""DE-MCz posterior sampling (ter Braak & Vrugt 2008, Stat. Comput. 18: differential evolution Markov chain with sampling
from the past; the subspace crossover of DREAM, Vrugt 2016; a uniform prior on the parameter box), the part around the
model: the state of N chains on the device (DemczState), the thin binding of the one C entry that moves them
(demcz_step -> smart_demcz_step_hip, include/smart_amd.h: accept the outstanding proposals from their scores, append to the
archive, propose the next generation -- two small kernels, no synchronisation), the Gelman-Rubin statistic over archived
snapshots (gelman_rubin) and the result object (PosteriorSample) with its diagnostics file.  montecarlo.DEMCz puts the
SMART ensemble launch between two steps; any other density can stand there (tests/test_gpu_demcz.py plays one).
"""
import ctypes

import numpy as np

from . import _lib, generational
from ._lib import SmartEngineError


def thresholds(p_jump, cr):
    """-> (J, C) = (floor(p_jump 2^32), floor(CR 2^32)): what a 32-bit word is compared with"""
    return generational.threshold('demcz', 'p_jump', p_jump), generational.threshold('demcz', 'cr', cr)


def gamma_table(d):
    """gamma[d' - 1] = 2.38 / sqrt(2 d') for d' = 1 .. d (ter Braak & Vrugt 2008)"""
    return 2.38 / np.sqrt(2.0 * np.arange(1, int(d) + 1, dtype=np.float64))


def _dbl(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class DemczState(generational.BoxState):
    """N chains of d varying parameters on the device, and what the host keeps of them.

    Device tensors: x [N, d] (the chains), logp [N], carry [N, n_carry] (a payload that travels with a chain: the
    objective functions of its row), accepted [N] int32, proposal [N, d] and out [N] uint8 (the outstanding proposals),
    archive [capacity, d] / archive_logp [capacity] / archive_carry [capacity, n_carry], rows [N, ld] (the launch matrix:
    the step writes the d columns `columns`, the others are the caller's).  Host: M (archive rows in use), g (the
    generation the next propose phase makes, 1 at first), seed, lo, hi, scale = b_star (hi - lo), gamma, J, C, and how a
    score becomes a log-density: score_kind 'logp', 'rmse' (n_obs, n_eff) or 'rmse_sigma' (n_eff, sigma).

    x: [N, d], the initial population (host or device); rows: a launch matrix of the caller's, or None for one of ld
    columns filled with `fill` (NaN: columns that nobody reads)."""

    def __init__(self, x, lo, hi, capacity, seed=0, cr=0.9, p_jump=0.1, b_star=1e-6, n_carry=0, columns=None, ld=None,
                 rows=None, fill=float('nan'), score_kind='logp', n_obs=0, n_eff=0.0, sigma=0.0, device=None):
        import torch
        self.x = self._place('demcz', 'chains', x, device)
        device = self.device
        N, d = self.x.shape
        self.n_chains, self.n_dims, self.n_carry, self.capacity = N, d, int(n_carry), int(capacity)
        self._set_box('demcz', self.x, lo, hi, b_star, seed, columns, ld, rows, fill)
        self.gamma = np.ascontiguousarray(gamma_table(d))
        self.J, self.C = thresholds(p_jump, cr)
        self.score_kind = score_kind
        self.n_obs, self.n_eff, self.sigma = int(n_obs), float(n_eff), float(sigma)
        f64 = dict(dtype=torch.float64, device=device)
        self.logp = torch.full((N,), float('-inf'), **f64)
        self.carry = torch.zeros((N, self.n_carry), **f64)
        self.accepted = torch.zeros((N,), dtype=torch.int32, device=device)
        self.proposal = self.x.clone()
        self.out = torch.zeros((N,), dtype=torch.uint8, device=device)
        self.archive = torch.zeros((self.capacity, d), **f64)
        self.archive_logp = torch.zeros((self.capacity,), **f64)
        self.archive_carry = torch.zeros((self.capacity, self.n_carry), **f64)
        self.M, self.g = 0, 1


def demcz_step(state, scores=None, carry_new=None, propose=True, append=False, chains=None):
    """One call of smart_demcz_step_hip on torch's current stream (include/smart_amd.h has the definition).

    scores: None (no accept phase), or a float64 device tensor with one score per chain at a constant stride -- a column
    of the engine's [N, 8] objective table is read in place.  The accept phase of the call decides on the proposals of
    generation state.g - 1 (state.g == 1: the initial population takes its scores), and with append=True writes every
    chain as archive row M + chain.  propose=True then makes the proposals of generation state.g into state.proposal,
    state.out and state.rows, and state.g moves on.  carry_new: [N, n_carry], the payload of the proposals.
    chains=(first, count): the call works on that part of the chains only (the same bits as the call over all of them;
    a part that appends proposes in a call of its own, once every part has appended -- state.M and state.g are then the
    caller's to move: this function leaves both alone for a partial call)."""
    import torch
    s = state
    L = _lib.lib()
    kind = s.score_kind if isinstance(s.score_kind, int) else _lib.DEMCZ_SCORES.get(s.score_kind, -1)
    if not isinstance(s.score_kind, int) and kind < 0:
        raise SmartEngineError(-7, "demcz_step: score_kind '{}' unknown.".format(s.score_kind))
    first, count = (0, s.n_chains) if chains is None else (int(chains[0]), int(chains[1]))
    if not (0 <= first and count >= 0 and first + count <= s.n_chains):
        raise SmartEngineError(-2, "demcz_step: chains {} .. {} are not among the {} of the state."
                               .format(first, first + count - 1, s.n_chains))
    score_ptr, stride = None, 0
    if scores is not None:
        if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float64
                and scores.dim() == 1 and scores.shape[0] == s.n_chains):
            raise SmartEngineError(-2, "demcz_step: scores must be a float64 device tensor [{}].".format(s.n_chains))
        stride = scores.stride(0) if s.n_chains > 1 else 1
        score_ptr = scores.data_ptr() + 8 * stride * first
    generational.check_carry_new('demcz_step', carry_new, s.n_chains, s.n_carry)
    d, nc = s.n_dims, s.n_carry

    def at(t, width, size=8):       # the address of row `first` of a per-chain array
        return None if t is None else t.data_ptr() + size * width * first

    ld = s.ld
    with torch.cuda.device(s.device):
        _lib.check(L.smart_demcz_step_hip(
            count, first, d, s.seed, s.g, s.M, s.capacity,
            at(s.x, d), at(s.logp, 1), at(s.carry, nc), at(s.accepted, 1, 4), at(s.proposal, d), at(s.out, 1, 1),
            score_ptr, stride, kind, s.n_obs, s.n_eff, s.sigma, at(carry_new, nc), nc, int(bool(append)),
            s.archive.data_ptr(), s.archive_logp.data_ptr(), s.archive_carry.data_ptr(),
            int(bool(propose)), _dbl(s.lo), _dbl(s.hi), _dbl(s.scale), _dbl(s.gamma), s.J, s.C,
            s.rows.data_ptr() + 8 * ld * first, ld, s.columns.ctypes.data_as(ctypes.c_void_p),
            torch.cuda.current_stream(s.device).cuda_stream))
    if chains is None:
        if scores is not None and append:
            s.M += s.n_chains
        if propose:
            s.g += 1
    return s


def gelman_rubin(history):
    """The potential scale reduction factor R-hat (Gelman & Rubin 1992) per parameter, over the SECOND HALF of the
    archived snapshots.  history: [S, N, d] -- S snapshots of N chains (tensor of any device, or array; answered in
    kind).  With the n = S - S // 2 last snapshots, W the mean over the chains of their variances (n - 1 in the
    denominator) and B / n the variance of the chain means (N - 1): R-hat = sqrt(((n - 1) / n W + B / n) / W).  NaN where
    fewer than two snapshots or two chains are left."""
    import torch
    tensor = isinstance(history, torch.Tensor)
    h = history if tensor else torch.from_numpy(np.ascontiguousarray(np.asarray(history, dtype=np.float64)))
    if h.dim() != 3:
        raise ValueError("history must be [snapshots, chains, dimensions], not {}.".format(tuple(h.shape)))
    h = h.to(torch.float64)[h.shape[0] // 2:]
    n, N, d = h.shape
    if n < 2 or N < 2:
        r = torch.full((d,), float('nan'), dtype=torch.float64, device=h.device)
    else:
        means = h.mean(dim=0)                                                # [N, d]
        W = ((h - means.unsqueeze(0)) ** 2).sum(dim=0).div(n - 1).mean(dim=0)
        B_n = ((means - means.mean(dim=0, keepdim=True)) ** 2).sum(dim=0) / (N - 1)
        r = torch.sqrt(((n - 1) / n * W + B_n) / W)
    return r if tensor else r.numpy()


DIAGNOSTICS_PREFIX = ['generation', 'acceptance_rate']


def diagnostics_header(names):
    """The header of `<catchment>.SMART.demcz.diagnostics`: generation, acceptance_rate, one Rhat column per parameter."""
    return ','.join(DIAGNOSTICS_PREFIX + ['Rhat_%s' % p for p in names]) + '\n'


def write_diagnostics(path, names, diagnostics):
    """diagnostics: rows of (generation, acceptance rate so far, R-hat per parameter) -- one per archived generation; the
    generation as an integer, the others '%.6e'."""
    generational.write_diagnostics(path, diagnostics_header(names), 1, diagnostics)


class PosteriorSample(object):
    """What a DE-MCz run leaves.  `names` (the d parameters that varied); device tensors `sample` [n, d] (the archive
    rows after the burn-in, snapshot by snapshot), `log_density` [n] and `carry` [n, n_carry]; `history` [S, N, d] and
    `history_log_density` [S, N] (every archived snapshot, the burn-in included -- what rhat was computed from); numpy:
    `accepted` [N] (int32, per chain), `rhat` [d], `acceptance_rate` (a float: accepted proposals over proposals made),
    `diagnostics` [S, 2 + d] (generation, acceptance rate up to it, R-hat over the second half of the snapshots up to
    it); `burn_in` (snapshots dropped) and `file` (the diagnostics file, or None); `error_parameters` (device tensor [n, 3]:
    sigma0, sigma1, phi of every row of the sample, where the run inferred a residual error model; else None)."""

    def __init__(self, names, sample, log_density, carry, history, history_log_density, accepted, rhat, acceptance_rate,
                 diagnostics, burn_in, file=None, error_parameters=None):
        self.names = list(names)
        self.sample, self.log_density, self.carry, self.history = sample, log_density, carry, history
        self.history_log_density, self.accepted = history_log_density, np.asarray(accepted)
        self.rhat, self.acceptance_rate = np.asarray(rhat, dtype=np.float64), float(acceptance_rate)
        self.diagnostics = np.asarray(diagnostics, dtype=np.float64)
        self.burn_in, self.file, self.error_parameters = int(burn_in), file, error_parameters
