"""The analyses of a stored [R, N] discharge matrix (row r = every sample's discharge of report step r), each one launch
through the C ABI (csrc/smart_analysis_capi.hip): objective functions, weighted quantiles over the samples, objective
functions per window of report steps, flow duration curves, hydrological signatures, Sobol indices, ensemble
verification scores, the dynamic identifiability analysis, the PAWN sensitivity, the log-likelihood and the realisations
of the residual error model -- and the Pareto selection over the scores they leave, [N, C] with a row per sample.  torch tensors
in, torch tensors out, as in engine.py -- which imports this module and re-exports every public name of it
(engine.flow_duration and the others are these functions); what they share on the way to the launch are the private
helpers at the top.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import SmartEngineError


def _as_device(x, device, shape=None):
    from .engine import as_device      # (engine imports this module: looked up when called)
    return as_device(x, device, shape)


def _matrix(sim):
    """A matrix where a kernel can read it -> (tensor, rows, columns, ld): on a device (the default one, if it has to be
    moved), float64, unit stride along a row (copied if not), ld the stride from row to row -- and the length of a row
    where there is one row only, whose stride says nothing."""
    if not (isinstance(sim, torch.Tensor) and sim.is_cuda):
        from .engine import default_device
        sim = _as_device(sim, default_device())
    if sim.dtype != torch.float64:
        sim = sim.to(torch.float64)
    if sim.stride(-1) != 1:
        sim = sim.contiguous()
    rows, cols = sim.shape
    return sim, rows, cols, (sim.stride(0) if rows > 1 else cols)


def _window_ids(win, device):
    """checked window ids (_windows) -> contiguous int32 tensor on the device; None (one window) stays None"""
    if win is None:
        return None
    if not isinstance(win, torch.Tensor):
        win = torch.from_numpy(np.ascontiguousarray(win.astype(np.int32)))
    return win.to(device=device, dtype=torch.int32).contiguous()


def _code(who, what, table, name):
    """table[name], or the refusal of a name the table does not hold"""
    try:
        return table[name]
    except (KeyError, TypeError):
        raise SmartEngineError(-7, "{}: {} '{}' unknown.".format(who, what, name))


def _workspace(need, device):
    """What a *_workspace_bytes entry answered -> (scratch tensor or None, bytes).  Sizes the query refuses (a negative
    answer; smart_pareto_workspace_bytes answers 0) get no workspace: the entry refuses them too, with its own text."""
    need = max(0, int(need))
    return (torch.empty(need, dtype=torch.uint8, device=device) if need else None), need


def _launch(device, entry, *args):
    """Call a *_hip entry on `device` and on torch's current stream there -- the stream is the entry's last argument,
    after `args` -- and raise what it refuses."""
    with torch.cuda.device(device):
        _lib.check(entry(*args, torch.cuda.current_stream(device).cuda_stream))


def _weights(who, weights, device, n):
    """The weights= argument of a call: [n], finite and >= 0 -> float64 tensor on the device; None (equal weights) stays"""
    if weights is None:
        return None
    weights = _as_device(weights, device, (n,))
    bad = int((~(torch.isfinite(weights) & (weights >= 0))).sum())
    if bad:
        raise SmartEngineError(-2, "{}: {} of the {} weights are negative or not finite.".format(who, bad, n))
    return weights


def _categories(who, categories, n_cols):
    """The categories= argument of a call: uint8 [factors, n_cols], host or device, checked before anything is moved
    -> a tensor where they lie (its first dimension is the number of factors)"""
    shape = tuple(getattr(categories, 'shape', ()))
    if len(shape) != 2 or shape[1] != n_cols or str(getattr(categories, 'dtype', '')).split('.')[-1] != 'uint8':
        raise SmartEngineError(-2, "{}: categories must be uint8 [factors, {}] (identifiability.bin_table), not {} {}."
                               .format(who, n_cols, getattr(categories, 'dtype', type(categories).__name__), shape))
    if not isinstance(categories, torch.Tensor):
        categories = torch.from_numpy(np.ascontiguousarray(categories))
    return categories


def _ptr(t):
    return None if t is None else t.data_ptr()


def _probs(probs):
    """-> (contiguous float64 array, its double* for the C ABI)"""
    q = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
    return q, q.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def objective_functions(discharge_report_major, obs, gw_sim=None, gw_obs=None):
    """montecarlo.py:193-209 for every column of a stored [R, N] discharge matrix (one pass over it, HBM-bound)."""
    L = _lib.lib()
    sim, R, N, ld = _matrix(discharge_report_major)
    obs = _as_device(obs, sim.device, (R,))
    gw_sim = _as_device(gw_sim, sim.device, (N,)) if gw_sim is not None else None
    out = torch.empty((N, 8), dtype=torch.float64, device=sim.device)
    _launch(sim.device, L.smart_objfn_hip, N, R, sim.data_ptr(), ld, obs.data_ptr(), _ptr(gw_sim),
            float('nan') if gw_obs is None else float(gw_obs), out.data_ptr())
    return out


_QUANTILE_METHODS = {'auto': _lib.QUANTILES_AUTO, 'sort': _lib.QUANTILES_SORT, 'select': _lib.QUANTILES_SELECT}


def quantiles_sort_capacity():
    """The largest number of samples the sort form of weighted_quantiles takes (no device needed)."""
    return int(_lib.lib().smart_quantiles_sort_capacity())


def weighted_quantiles(discharge_report_major, probs, weights=None, method='auto'):
    """Weighted quantiles over the samples of a stored [R, N] discharge matrix, per report step -> device tensor
    [K, R] float64 (the GLUE prediction bounds).  Q(q) is the smallest value v of the step with
    sum(w[x <= v]) >= q * sum(w): numpy's method='inverted_cdf' with weights=, no interpolation; NaN sorts last; a step
    whose weights sum to zero gives NaN.  probs: K <= 16 probabilities in (0, 1]; weights: [N], finite and >= 0, or
    None for equal weights; method: 'auto' (by size), 'sort' (N <= quantiles_sort_capacity()) or 'select'."""
    L = _lib.lib()
    code = _code('weighted_quantiles', 'method', _QUANTILE_METHODS, method)
    sim, R, N, ld = _matrix(discharge_report_major)
    q, q_ptr = _probs(probs)
    weights = _weights('weighted_quantiles', weights, sim.device, N)
    out = torch.empty((q.size, R), dtype=torch.float64, device=sim.device)
    _launch(sim.device, L.smart_weighted_quantiles_hip, N, R, sim.data_ptr(), ld, _ptr(weights), q_ptr, q.size,
            out.data_ptr(), code)
    return out


def _windows(who, sim, windows, n_windows, optional=False):
    """The windows= argument of a call on the matrix `sim`, checked where the ids lie (host array or device tensor),
    before anything is moved or launched -> (flat ids, W).  Where it is `optional`, None is one window holding every
    row -> (None, 1)."""
    shape = tuple(sim.shape)
    if windows is None and optional:
        if n_windows is not None and int(n_windows) != 1:
            raise SmartEngineError(-2, "{}: n_windows = {} without windows.".format(who, n_windows))
        if len(shape) != 2:
            raise SmartEngineError(-2, "{}: a matrix [R, N] is needed, not shape {}.".format(who, shape))
        return None, 1
    if isinstance(windows, torch.Tensor):
        win = windows.reshape(-1)
        integers = not (win.dtype.is_floating_point or win.dtype == torch.bool)
    else:
        win = np.asarray(windows).reshape(-1)
        integers = win.dtype.kind in 'iu'
    if not integers:
        raise SmartEngineError(-2, "{}: windows must be integers.".format(who))
    W = (int(win.max()) + 1 if len(win) else 0) if n_windows is None else int(n_windows)
    if W < 1:
        raise SmartEngineError(-2, "{}: no window (n_windows = {}).".format(who, W))
    bad = int(((win < -1) | (win >= W)).sum())
    if bad:
        raise SmartEngineError(-2, "{}: {} of the {} window ids are outside -1 .. {}."
                               .format(who, bad, len(win), W - 1))
    if len(shape) != 2 or shape[0] != len(win):
        raise SmartEngineError(-2, "{}: {} window ids for a matrix of shape {}.".format(who, len(win), shape))
    return win, W


def _counts16(who, counts, axis, size, layout):
    """The counts= argument of a call: 16-bit counts [., .] with `size` entries along `axis` -- uint16 on the host, uint16
    or int16 (the same 16 bits) on a device -> a tensor where they lie, a host array as its int16 view."""
    shape = tuple(getattr(counts, 'shape', ()))
    kinds = ('uint16', 'int16') if isinstance(counts, torch.Tensor) else ('uint16',)
    if len(shape) != 2 or shape[axis] != size or str(getattr(counts, 'dtype', '')).split('.')[-1] not in kinds:
        raise SmartEngineError(-2, "{}: counts must be uint16 {}, not {} {}."
                               .format(who, layout, getattr(counts, 'dtype', type(counts).__name__), shape))
    if not isinstance(counts, torch.Tensor):
        counts = torch.from_numpy(np.ascontiguousarray(counts).view(np.int16))
    return counts


def objfn_max_windows():
    """The largest number of windows objective_functions_windows takes in one call (no device needed)."""
    return int(_lib.lib().smart_objfn_max_windows())


def objective_functions_windows(discharge_report_major, obs, windows, n_windows=None, transform='none', eps=0.0):
    """The seven objective functions NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE of every column of a stored [R, N]
    discharge matrix, PER WINDOW of report steps and on transformed flows -> device tensor [W, N, 7] float64.
    windows: [R] integers, -1 = the report step belongs to no window, else 0 .. n_windows-1 (n_windows defaults to
    max + 1); transform: 'none', 'sqrt', 'log' (ln(x + eps)) or 'inverse' (1 / (x + eps)), applied to the observed and
    to the simulated flows.  A window with fewer than two observed steps is NaN for every sample; a (window, sample)
    that meets a transformed value that is not finite is NaN (include/smart_amd.h: smart_objfn_windows_hip)."""
    L = _lib.lib()
    code = _code('objective_functions_windows', 'transform', _lib.TRANSFORMS, transform)
    win, W = _windows('objective_functions_windows', discharge_report_major, windows, n_windows)
    sim, R, N, ld = _matrix(discharge_report_major)
    obs = _as_device(obs, sim.device, (R,))
    win = _window_ids(win, sim.device)
    out = torch.empty((W, N, _lib.OBJFN_WINDOW_COLS), dtype=torch.float64, device=sim.device)
    if N == 0:
        return out
    _launch(sim.device, L.smart_objfn_windows_hip, N, R, sim.data_ptr(), ld, obs.data_ptr(), win.data_ptr(), W, code,
            float(eps), out.data_ptr())
    return out


def flow_duration_sort_capacity():
    """The largest number of report steps the sort form of flow_duration takes (no device needed)."""
    return int(_lib.lib().smart_flow_duration_sort_capacity())


def flow_duration(discharge_report_major, probs, obs=None, windows=None, n_windows=None, transform='none', eps=0.0,
                  segment=(0.0, 1.0), objfn=False, method='auto'):
    """Flow duration curves of every column of a stored [R, N] discharge matrix: order statistics ALONG TIME, per sample
    and per window of report steps -> (quant [W, K, N], objfn [W, N, 7] or None), device tensors, float64.
    probs: K <= 16 NON-exceedance probabilities q in [0, 1]; Q(q) is the max(1, ceil(q * m))-th smallest of the window's
    m values of the column (numpy's method='inverted_cdf': an element of the column, NaN sorts last, m == 0 gives NaN).
    obs: [R] or None -- report steps without an observation (NaN) are left out; windows: [R] integers as for
    objective_functions_windows, or None for one window holding every step.  objfn=True (needs obs) adds NSE, KGE, KGEc,
    KGEa, KGEb, PBias, RMSE of f(sorted simulation) against f(sorted observations), paired by rank, over the ranks i with
    segment[0] * m <= i < segment[1] * m; transform / eps as for objective_functions_windows, and its two rules.
    method: 'auto', 'sort' (R <= flow_duration_sort_capacity(); the only one that gives objfn) or 'select'.  The
    workspace of the call is sized and owned here (include/smart_amd.h: smart_flow_duration_hip)."""
    L = _lib.lib()
    code = _code('flow_duration', 'transform', _lib.TRANSFORMS, transform)
    how = _code('flow_duration', 'method', _lib.FDC_METHODS, method)
    if objfn and obs is None:
        raise SmartEngineError(-1, "flow_duration: the objective functions of the curve need obs.")
    win, W = _windows('flow_duration', discharge_report_major, windows, n_windows, optional=True)
    sim, R, N, ld = _matrix(discharge_report_major)
    q, q_ptr = _probs(probs)
    lo, hi = (float(x) for x in segment)
    if obs is not None:
        obs = _as_device(obs, sim.device, (R,))
    win = _window_ids(win, sim.device)
    quant = torch.empty((W, q.size, N), dtype=torch.float64, device=sim.device)
    scores = torch.empty((W, N, _lib.OBJFN_WINDOW_COLS), dtype=torch.float64, device=sim.device) if objfn else None
    if N == 0:
        return quant, scores
    work, need = _workspace(L.smart_flow_duration_workspace_bytes(R, W, 1 if objfn else 0), sim.device)
    # (torch gives a matrix without a report step no address, and NULL would be the entry's first refusal: such a matrix
    # gets an address that is never followed, so that the entry refuses what its workspace query refused -- the size)
    _launch(sim.device, L.smart_flow_duration_hip, N, R, sim.data_ptr() or 0x1000, ld, _ptr(obs), _ptr(win), W, q_ptr,
            q.size, quant.data_ptr(), code, float(eps), lo, hi, _ptr(scores), _ptr(work), need, how)
    return quant, scores


SIGNATURE_NAMES = list(_lib.SIGNATURE_NAMES)


def signatures(discharge_report_major, obs=None, windows=None, n_windows=None, alpha=0.925, thresholds=None):
    """Hydrological signatures of every column of a stored [R, N] discharge matrix, per window of report steps -> device
    tensor [W, 12, N] float64, the columns in the order of SIGNATURE_NAMES: the mean, and the scores that depend on the
    ORDER of the report steps -- baseflow index (one forward pass of the Lyne-Hollick filter with `alpha`), Richards-Baker
    flashiness, lag-1 autocorrelation, rising limb density, mean log recession rate, the peak and its row, and the number
    and mean length of the runs above thresholds[w][1] and below thresholds[w][0].  out[w, c] is a contiguous [N] vector.
    obs: [R] or None -- a report step without an observation (NaN) is left out and breaks the series there; windows: [R]
    integers as for objective_functions_windows, or None for one window holding every step; thresholds: [W, 2] (lo, hi),
    host or device, or None (the four pulse columns are then NaN, as they are for a NaN threshold).  A (window, sample)
    without a row, or with a value that is not finite, is NaN (include/smart_amd.h: smart_signatures_hip)."""
    alpha = float(alpha)
    if not (0.0 < alpha < 1.0):
        raise SmartEngineError(-2, "signatures: alpha {} must lie inside (0, 1).".format(alpha))
    win, W = _windows('signatures', discharge_report_major, windows, n_windows, optional=True)
    if thresholds is not None and tuple(thresholds.shape if hasattr(thresholds, 'shape')
                                        else np.shape(thresholds)) != (W, 2):
        raise SmartEngineError(-2, "signatures: thresholds must be (lo, hi) per window, shape ({}, 2), not {}."
                               .format(W, tuple(np.shape(thresholds))))
    L = _lib.lib()
    sim, R, N, ld = _matrix(discharge_report_major)
    if obs is not None:
        obs = _as_device(obs, sim.device, (R,))
    win = _window_ids(win, sim.device)
    pulse = None if thresholds is None else _as_device(thresholds, sim.device, (W, 2))
    out = torch.empty((W, _lib.SIGNATURE_COLS, N), dtype=torch.float64, device=sim.device)
    if N == 0:
        return out
    _launch(sim.device, L.smart_signatures_hip, N, R, sim.data_ptr(), ld, _ptr(obs), _ptr(win), W, alpha, _ptr(pulse),
            out.data_ptr())
    return out


def sobol_max_resamples():
    """The largest number of bootstrap replicates of one sobol_indices call (no device needed)."""
    return int(_lib.lib().smart_sobol_max_resamples())


def sobol_lds_capacity():
    """The largest base size whose A and B blocks sobol_indices keeps in LDS (no device needed)."""
    return int(_lib.lib().smart_sobol_lds_capacity())


def sobol_counts(n_base, resamples, seed=None):
    """The bootstrap counts of sobol_indices -> [n_base, resamples] uint16 on the host: replicate b draws n_base base rows
    with replacement, numpy.random.Generator(PCG64(seed)).integers(n_base, size=(resamples, n_base)), and counts[i, b] is
    how often it drew row i (every column sums to n_base)."""
    n, B = int(n_base), int(resamples)
    if n < 1:
        raise SmartEngineError(-2, "sobol_counts: n_base must be at least 1 (got {}).".format(n_base))
    if B < 0 or B > sobol_max_resamples():
        raise SmartEngineError(-2, "sobol_counts: {} resamples, between 0 and {} per call.".format(resamples, sobol_max_resamples()))
    draws = np.random.Generator(np.random.PCG64(seed)).integers(n, size=(B, n))
    counts = np.zeros((n, B), dtype=np.int64)
    for b in range(B):
        counts[:, b] = np.bincount(draws[b], minlength=n)
    if counts.size and counts.max() > 65535:
        raise SmartEngineError(-2, "sobol_counts: a count of {} does not fit the uint16 of the kernel.".format(counts.max()))
    return np.ascontiguousarray(counts.astype(np.uint16))


class SobolResult(object):
    """Device tensors of one sobol_indices call: S1, ST [M, k], moments [M, 2] (mean and variance of A u B), S1_std and
    ST_std [M, k] or None without counts."""

    def __init__(self, S1, ST, moments, S1_std, ST_std):
        self.S1, self.ST, self.moments, self.S1_std, self.ST_std = S1, ST, moments, S1_std, ST_std


def sobol_indices(values, n_base, n_params, counts=None):
    """First-order (Saltelli 2010) and total (Jansen) Sobol indices of every row of `values` -> SobolResult.
    values: [M, N] or [N], host or device, N >= n_base * (n_params + 2) columns in the block-major order of
    sampling.saltelli_design ([A ; B ; AB_0 ; ...]; a row is a report step of a stored discharge matrix, or one scalar
    target); the leading dimension of a device matrix is honoured.  counts: [n_base, B] uint16 from sobol_counts (or a
    device tensor of those 16-bit patterns, uint16 or int16) adds the standard deviation of both indices over the B bootstrap replicates; None leaves it out.  A row with a
    value that is not finite, or without variance, is NaN (include/smart_amd.h: smart_sobol_indices_hip)."""
    L = _lib.lib()
    n, k = int(n_base), int(n_params)
    y = values
    if len(y.shape) == 1:
        y = y.reshape(1, -1)
    if len(y.shape) != 2:
        raise SmartEngineError(-2, "sobol_indices: values [M, N] or [N] are needed, not shape {}.".format(tuple(values.shape)))
    if n < 1 or k < 1 or k > _lib.SOBOL_MAX_PARAMS or y.shape[1] != n * (k + 2):
        raise SmartEngineError(-2, "sobol_indices: {} columns are not n_base * (n_params + 2) with n_base = {} >= 1 and "
                                   "n_params = {} in 1 .. {}.".format(y.shape[1], n_base, n_params, _lib.SOBOL_MAX_PARAMS))
    B = 0
    if counts is not None:
        counts = _counts16('sobol_indices', counts, 0, n, '[n_base, resamples] (engine.sobol_counts)')
        B = int(counts.shape[1])
        if B > sobol_max_resamples():
            raise SmartEngineError(-2, "sobol_indices: {} resamples, at most {} per call.".format(B, sobol_max_resamples()))
    y, M, N, ld = _matrix(y)
    dev = y.device
    S1 = torch.empty((M, k), dtype=torch.float64, device=dev)
    ST = torch.empty((M, k), dtype=torch.float64, device=dev)
    moments = torch.empty((M, 2), dtype=torch.float64, device=dev)
    S1_std = ST_std = None
    if M == 0:
        return SobolResult(S1, ST, moments, None, None)
    if B > 0:
        counts = counts.to(dev).contiguous()
        S1_std, ST_std = torch.empty_like(S1), torch.empty_like(ST)
    work, need = _workspace(L.smart_sobol_workspace_bytes(n, k, M, B), dev)
    _launch(dev, L.smart_sobol_indices_hip, n, k, M, y.data_ptr(), ld, S1.data_ptr(), ST.data_ptr(), moments.data_ptr(),
            counts.data_ptr() if B else None, B, _ptr(S1_std), _ptr(ST_std), _ptr(work), need)
    return SobolResult(S1, ST, moments, S1_std, ST_std)


def bootstrap_max_windows():
    """The largest number of windows objective_functions_bootstrap takes in one call (no device needed)."""
    return int(_lib.lib().smart_bootstrap_max_windows())


def bootstrap_max_resamples():
    """The largest number of replicates of one objective_functions_bootstrap call (no device needed)."""
    return int(_lib.lib().smart_bootstrap_max_resamples())


def _eligible_windows(who, n_windows, eligible):
    """-> the indices of the eligible windows among 0 .. n_windows-1 (every window for None), ascending"""
    W = int(n_windows)
    if W < 1:
        raise SmartEngineError(-2, "{}: n_windows must be at least 1 (got {}).".format(who, n_windows))
    if eligible is None:
        return W, np.arange(W)
    mask = np.asarray(eligible)
    if mask.shape != (W,):
        raise SmartEngineError(-2, "{}: eligible has shape {} where one entry per window ({},) is expected."
                               .format(who, mask.shape, W))
    return W, np.flatnonzero(mask != 0)


def bootstrap_counts(n_windows, resamples, seed=None, eligible=None):
    """The block-bootstrap counts of objective_functions_bootstrap -> [resamples, n_windows] uint16 on the host.  With E
    eligible windows (all of them for eligible=None, else the nonzero entries of the [n_windows] mask, ascending) replicate
    b draws E of them with replacement: numpy.random.Generator(PCG64(seed)).integers(E, size=(resamples, E)), draw j of
    row b naming the j-th eligible window, and counts[b, w] is how often replicate b drew window w.  Every row sums to E;
    the column of a window that is not eligible is 0."""
    W, idx = _eligible_windows('bootstrap_counts', n_windows, eligible)
    B, E = int(resamples), len(idx)
    if B < 0 or B > bootstrap_max_resamples():
        raise SmartEngineError(-2, "bootstrap_counts: {} resamples, between 0 and {} per call."
                               .format(resamples, bootstrap_max_resamples()))
    if E < 1:
        raise SmartEngineError(-2, "bootstrap_counts: no window is eligible.")
    if E > 65535:
        raise SmartEngineError(-2, "bootstrap_counts: a count of {} does not fit the uint16 of the kernel.".format(E))
    draws = np.random.Generator(np.random.PCG64(seed)).integers(E, size=(B, E))
    counts = np.zeros((B, W), dtype=np.int64)
    for b in range(B):
        counts[b, idx] = np.bincount(draws[b], minlength=E)
    return np.ascontiguousarray(counts.astype(np.uint16))


def jackknife_counts(n_windows, eligible=None):
    """The leave-one-window-out counts of objective_functions_bootstrap -> [E, n_windows] uint16 on the host: row i holds
    1 for every eligible window but the i-th of them, which it leaves out, and 0 for the windows that are not eligible."""
    W, idx = _eligible_windows('jackknife_counts', n_windows, eligible)
    counts = np.zeros((len(idx), W), dtype=np.uint16)
    counts[:, idx] = 1
    counts[np.arange(len(idx)), idx] = 0
    return counts


class BootstrapResult(object):
    """Device tensors of one objective_functions_bootstrap call: point [N, 7]; stats [7, 2 + K, N] -- per score the mean
    and the standard deviation (ddof = 1) over the replicates, then the K quantiles, stats[s, c] a contiguous [N] vector --
    or None without replicates (counts with no row); replicates [B, 7, N] or None; probs, the K probabilities."""

    def __init__(self, point, stats, replicates, probs):
        self.point, self.stats, self.replicates, self.probs = point, stats, replicates, probs


def objective_functions_bootstrap(discharge_report_major, obs, windows, counts, probs=(0.05, 0.5, 0.95), n_windows=None,
                                  transform='none', eps=0.0, replicates=False):
    """The seven objective functions NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE of every column of a stored [R, N] discharge
    matrix under resampling of WINDOWS of report steps -> BootstrapResult.  windows: [R] integers as for
    objective_functions_windows; counts: [B, W] uint16 from bootstrap_counts or jackknife_counts (or a device tensor of
    those 16-bit patterns, uint16 or int16) -- replicate b takes the observed report steps of window w counts[b, w] times;
    the point value takes every window once.  probs: K <= 16 probabilities in (0, 1]: numpy's 'inverted_cdf' quantiles of
    the B replicate values, an element of the set.  transform / eps as for objective_functions_windows.  replicates=True
    also returns every replicate, [B, 7, N].  A replicate with fewer than two report steps is NaN; a (window, sample) that
    meets a transformed value that is not finite makes NaN the replicates that draw that window, and no other; mean and
    standard deviation are NaN where a replicate is.  The matrix is read once; the workspace of the call is sized and
    owned here (include/smart_amd.h: smart_objfn_bootstrap_hip)."""
    who = 'objective_functions_bootstrap'
    L = _lib.lib()
    code = _code(who, 'transform', _lib.TRANSFORMS, transform)
    win, W = _windows(who, discharge_report_major, windows, n_windows)
    if W > bootstrap_max_windows():
        raise SmartEngineError(-2, "{}: {} windows, at most {} per call.".format(who, W, bootstrap_max_windows()))
    counts = _counts16(who, counts, 1, W,
                       '[resamples, {}] (engine.bootstrap_counts, engine.jackknife_counts)'.format(W))
    B = int(counts.shape[0])
    if B > bootstrap_max_resamples():
        raise SmartEngineError(-2, "{}: {} resamples, at most {} per call.".format(who, B, bootstrap_max_resamples()))
    q, q_ptr = _probs(probs)
    K = q.size
    if K < 1 or K > _lib.QUANTILES_MAX_PROBS or not np.all((q > 0.0) & (q <= 1.0)):
        raise SmartEngineError(-2, "{}: the probabilities must be 1 .. {} values in (0, 1], not {}."
                               .format(who, _lib.QUANTILES_MAX_PROBS, q.tolist()))
    eps = float(eps)
    if not (eps >= 0.0) or np.isinf(eps):
        raise SmartEngineError(-2, "{}: eps {} must be finite and >= 0.".format(who, eps))
    # ---- from here on the device
    sim, R, N, ld = _matrix(discharge_report_major)
    dev = sim.device
    obs = _as_device(obs, dev, (R,))
    win = _window_ids(win, dev)
    point = torch.empty((N, _lib.OBJFN_WINDOW_COLS), dtype=torch.float64, device=dev)
    stats = torch.empty((_lib.OBJFN_WINDOW_COLS, 2 + K, N), dtype=torch.float64, device=dev) if B else None
    reps = torch.empty((B, _lib.OBJFN_WINDOW_COLS, N), dtype=torch.float64, device=dev) if replicates and B else None
    if N == 0:
        return BootstrapResult(point, stats, reps, q)
    if B:
        counts = counts.to(dev).contiguous()
    work, need = _workspace(L.smart_bootstrap_workspace_bytes(N, W, B, 1 if reps is not None else 0), dev)
    _launch(dev, L.smart_objfn_bootstrap_hip, N, R, sim.data_ptr(), ld, obs.data_ptr(), win.data_ptr(), W, code, eps,
            counts.data_ptr() if B else None, B, q_ptr, K, point.data_ptr(), _ptr(stats), _ptr(reps), _ptr(work), need)
    return BootstrapResult(point, stats, reps, q)


def pareto_max_objectives():
    """The largest number of objectives of one pareto_counts call (no device needed)."""
    return int(_lib.lib().smart_pareto_max_objectives())


class _ParetoCall(object):
    """The checked arguments of pareto_counts / pareto_ranks.  Everything that can be refused from the words and the
    shapes alone is refused in the constructor, before anything is moved to a device; `counts` then launches the C
    entry, as often as a ranking has fronts."""

    def __init__(self, who, scores, directions, targets, columns, eligible):
        self.who = who
        if isinstance(directions, (str, bytes)) or (isinstance(directions, tuple) and len(directions) == 2
                                                    and directions[0] == 'target'):
            directions = [directions]
        directions = list(directions)
        M = len(directions)
        if M < 1 or M > _lib.PARETO_MAX_OBJECTIVES:
            raise SmartEngineError(-2, "{}: {} objectives, between 1 and {} per call."
                                   .format(who, M, _lib.PARETO_MAX_OBJECTIVES))
        if targets is not None and len(targets) != M:
            raise SmartEngineError(-2, "{}: {} targets for {} objectives.".format(who, len(targets), M))
        code, target = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.float64)
        for m, word in enumerate(directions):
            value = None
            if isinstance(word, (tuple, list)):
                if len(word) != 2:
                    raise SmartEngineError(-7, "{}: direction '{}' unknown.".format(who, word))
                word, value = word
            code[m] = _code(who, 'direction', _lib.PARETO_DIRECTIONS, word)
            if word == 'target':
                if value is None and targets is not None:
                    value = targets[m]
                if value is None:
                    raise SmartEngineError(-1, "{}: objective {} is a 'target' without a value.".format(who, m))
                target[m] = float(value)
                if not np.isfinite(target[m]):
                    raise SmartEngineError(-2, "{}: target {} of objective {} must be finite.".format(who, value, m))
            elif value is not None:
                raise SmartEngineError(-7, "{}: direction '{}' takes no value.".format(who, word))
        shape = tuple(scores.shape)
        if len(shape) == 1:
            shape = (shape[0], 1)
        if len(shape) != 2:
            raise SmartEngineError(-2, "{}: scores [N, C] or [N] are needed, not shape {}.".format(who, tuple(scores.shape)))
        N, C = shape
        cols = np.arange(M, dtype=np.int32) if columns is None else np.asarray(columns).reshape(-1)
        if cols.dtype.kind not in 'iu' or len(cols) != M:
            raise SmartEngineError(-2, "{}: columns must be {} integers, one per objective.".format(who, M))
        if len(set(cols.tolist())) != M or cols.min() < 0 or cols.max() >= C:
            raise SmartEngineError(-2, "{}: the columns {} are not {} different ones of the {} of the scores."
                                   .format(who, cols.tolist(), M, C))
        if eligible is not None and tuple(eligible.shape) != (N,):
            raise SmartEngineError(-2, "{}: eligible has shape {} where one entry per row ({},) is expected."
                                   .format(who, tuple(eligible.shape), N))
        self.N, self.M = N, M
        self.code, self.target = code, target
        self.cols = np.ascontiguousarray(cols.astype(np.int32))
        # ---- from here on the device
        self.L = _lib.lib()
        if len(scores.shape) == 1:
            scores = scores.reshape(-1, 1)
        self.scores, _, _, self.ld = _matrix(scores)
        self.device = self.scores.device
        self.eligible = None if eligible is None else self.mask(eligible)
        self.work, self.need = (None, 0) if N == 0 else \
            _workspace(self.L.smart_pareto_workspace_bytes(N, M), self.device)

    def mask(self, flags):
        """flags [N] (bool or numbers, host or device) -> contiguous uint8 device tensor, 1 where not zero"""
        if not isinstance(flags, torch.Tensor):
            flags = torch.from_numpy(np.ascontiguousarray(np.asarray(flags) != 0))
        return (flags.to(self.device) != 0).to(torch.uint8).contiguous()

    def counts(self, eligible):
        """eligible: uint8 device tensor [N] or None -> int32 device tensor [N]"""
        out = torch.empty((self.N,), dtype=torch.int32, device=self.device)
        if self.N == 0:
            return out
        i32, f64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        _launch(self.device, self.L.smart_pareto_counts_hip, self.N, self.scores.data_ptr(), self.ld,
                self.cols.ctypes.data_as(i32), self.code.ctypes.data_as(i32), self.target.ctypes.data_as(f64), self.M,
                _ptr(eligible), out.data_ptr(), _ptr(self.work), self.need)
        return out


def pareto_counts(scores, directions, targets=None, columns=None, eligible=None):
    """For every row of a score matrix, the number of rows that dominate it over the selected columns -> int32 device
    tensor [N]: 0 = the row is on the Pareto front, -1 = the row does not take part.
    scores: [N, C] or [N], host array or device tensor, float64 or float32 (widened exactly); the leading dimension of a
    device matrix is honoured.  directions: one word per objective, at most pareto_max_objectives(): 'max', 'min' or
    ('target', value) -- or 'target' with its value in targets[m].  columns: the column of every objective (default
    0 .. M-1), no column twice; columns that are not selected are never read.  eligible: [N] flags, or None for every row.
    The key of a score x is x, -x or -|x - value|; a row takes part iff it is eligible and none of its selected scores is
    a NaN; row j dominates row i iff both take part, every key of j is >= that of i and one is > (rows with equal keys do
    not dominate each other: a front keeps its duplicates).  include/smart_amd.h: smart_pareto_counts_hip."""
    call = _ParetoCall('pareto_counts', scores, directions, targets, columns, eligible)
    return call.counts(call.eligible)


def pareto_ranks(scores, directions, targets=None, columns=None, eligible=None, max_rank=1):
    """The non-dominated ranks of the rows of a score matrix, by peeling -> int32 device tensor [N]: rank 1 is the rows
    that pareto_counts gives 0, rank r the rows it gives 0 once the ranks below r are left out; 0 = not ranked within
    max_rank, -1 = the row does not take part.  max_rank=None ranks every row.  One launch and one read of the number of
    rows that are left per front; arguments as for pareto_counts."""
    if max_rank is not None and int(max_rank) < 1:
        raise SmartEngineError(-2, "pareto_ranks: max_rank must be at least 1 or None (got {}).".format(max_rank))
    call = _ParetoCall('pareto_ranks', scores, directions, targets, columns, eligible)
    ranks = torch.zeros((call.N,), dtype=torch.int32, device=call.device)
    left, rank = call.eligible, 0
    while call.N and (max_rank is None or rank < int(max_rank)):
        counts = call.counts(left)
        rank += 1
        if rank == 1:
            ranks[counts < 0] = -1
        ranks[counts == 0] = rank
        left = (counts > 0).to(torch.uint8)
        if int(left.sum()) == 0:        # the one read of this front
            break
    return ranks


ENSEMBLE_SCORE_NAMES = list(_lib.ENSEMBLE_SCORE_NAMES)


def ensemble_scores_lds_capacity():
    """The largest number of samples the LDS form of ensemble_scores takes (no device needed)."""
    return int(_lib.lib().smart_ensemble_scores_lds_capacity())


def ensemble_scores(discharge_report_major, obs=None, weights=None, method='auto'):
    """Verification scores of the ensemble of a stored [R, N] discharge matrix, per report step -> device tensor [5, R]
    float64, the rows in the order of ENSEMBLE_SCORE_NAMES: the continuous ranked probability score of the weighted
    ensemble against obs[r] (as the integral of (F - 1[x >= y])^2: a sum of non-negative terms), the ensemble's spread
    (the integral of F (1 - F) = E|X - X'| / 2), the probability integral transform of the observation from below
    (sum of w over x < y, / W) and from above (x <= y), and the weighted mean.  obs: [R] or None -- a step without a
    finite observation has NaN for CRPS and both PITs; weights: [N], finite and >= 0, or None for equal weights -- a
    member of weight zero takes no part, whatever its value; a step whose weights sum to zero, or with a live member that
    is not finite, is NaN in all five.  method: 'auto' (by size), 'lds' (N <= ensemble_scores_lds_capacity()) or
    'global' (N <= 2**24).  The workspace of the call is sized and owned here (include/smart_amd.h:
    smart_ensemble_scores_hip)."""
    L = _lib.lib()
    code = _code('ensemble_scores', 'method', _lib.ENSEMBLE_METHODS, method)
    sim, R, N, ld = _matrix(discharge_report_major)
    if obs is not None:
        obs = _as_device(obs, sim.device, (R,))
    weights = _weights('ensemble_scores', weights, sim.device, N)
    out = torch.empty((_lib.ENSEMBLE_SCORE_COLS, R), dtype=torch.float64, device=sim.device)
    if R == 0:
        return out
    work, need = _workspace(L.smart_ensemble_scores_workspace_bytes(N, R, 1 if weights is not None else 0, code),
                            sim.device)
    _launch(sim.device, L.smart_ensemble_scores_hip, N, R, sim.data_ptr(), ld, _ptr(weights), _ptr(obs), out.data_ptr(),
            code, _ptr(work), need)
    return out


def dynia_max_half_width():
    """The largest half width dynamic_identifiability takes, in report steps (no device needed)."""
    return int(_lib.lib().smart_dynia_max_half_width())


def dynia_lds_capacity():
    """The largest number of samples whose step dynamic_identifiability keeps in LDS for the selection (no device
    needed)."""
    return int(_lib.lib().smart_dynia_lds_capacity())


class DyniaResult(object):
    """Device tensors of one dynamic_identifiability call: shares [R, P, B] float64, cut [R] float64 (the window's SUM of
    absolute errors at the cut), retained [R] and count [R] int32, errors [R, N] float64 (the sums) or None."""

    def __init__(self, shares, cut, retained, count, errors):
        self.shares, self.cut, self.retained, self.count, self.errors = shares, cut, retained, count, errors


def dynamic_identifiability(discharge_report_major, obs, categories, n_bins, half_width, fraction=0.1, min_valid=None,
                            support='linear', keep_errors=False):
    """Dynamic identifiability analysis (DYNIA, Wagener et al. 2003) of a stored [R, N] discharge matrix -> DyniaResult.
    Per report step r the samples are scored by the sum of |sim - obs| over the observed steps of the moving window
    |s - r| <= half_width (cut at both ends of the record), the best `fraction` of the rows with a finite sum is retained
    -- k = max(1, ceil(fraction * M)), every tie at the cut stays in -- and shares[r, p, b] is the retained rows' support
    that falls into bin b of factor p, over the support of them all.  categories: [P, N] uint8, host or device, the bin
    of row n on factor p (identifiability.bin_table makes one), 255 = the row takes no part in the factor; P <= 16,
    n_bins <= 64.  support: 'equal' (every retained row 1) or 'linear' (cut - sum; 1 where every retained row ties).
    min_valid: the observed steps a window needs, None = (w + 1) // 2 with w = 2 * half_width + 1; a step with fewer
    is NaN in cut and shares, 0 in retained.  keep_errors=True also returns the sums, [R, N].  The workspace of the call
    is sized and owned here (include/smart_amd.h: smart_dynia_hip)."""
    who = 'dynamic_identifiability'
    L = _lib.lib()
    code = _code(who, 'support', _lib.DYNIA_SUPPORTS, support)
    h, B = int(half_width), int(n_bins)
    w = 2 * h + 1
    min_valid = (w + 1) // 2 if min_valid is None else int(min_valid)
    categories = _categories(who, categories, tuple(discharge_report_major.shape)[-1])
    P = categories.shape[0]
    # ---- from here on the device
    sim, R, N, ld = _matrix(discharge_report_major)
    dev = sim.device
    obs = _as_device(obs, dev, (R,))
    cat = categories.to(dev).contiguous()
    shares = torch.empty((R, P, B), dtype=torch.float64, device=dev)
    cut = torch.empty((R,), dtype=torch.float64, device=dev)
    retained = torch.empty((R,), dtype=torch.int32, device=dev)
    count = torch.empty((R,), dtype=torch.int32, device=dev)
    errors = torch.empty((R, N), dtype=torch.float64, device=dev) if keep_errors else None
    if R == 0 or N == 0:
        return DyniaResult(shares, cut, retained, count, errors)
    work, need = _workspace(L.smart_dynia_workspace_bytes(N, R, h, P, B), dev)
    _launch(dev, L.smart_dynia_hip, N, R, sim.data_ptr(), ld, obs.data_ptr(), h, min_valid, float(fraction),
            cat.data_ptr(), P, B, code, shares.data_ptr(), cut.data_ptr(), retained.data_ptr(), count.data_ptr(),
            _ptr(errors), N, _ptr(work), need)
    return DyniaResult(shares, cut, retained, count, errors)


def pawn_lds_capacity():
    """The largest number of samples the LDS form of pawn_ks takes (no device needed)."""
    return int(_lib.lib().smart_pawn_lds_capacity())


class PawnResult(object):
    """Device tensors of one pawn_ks call: ks [R, P, B] float64 and counts [P, B] int32; numpy() gives both on the host."""

    def __init__(self, ks, counts):
        self.ks, self.counts = ks, counts

    def numpy(self):
        return self.ks.cpu().numpy(), self.counts.cpu().numpy()


def pawn_ks(values_row_major, categories, n_bins, method='auto'):
    """The Kolmogorov-Smirnov distances of PAWN (Pianosi & Wagener 2015, 2018) on the sample at hand -> PawnResult.
    values_row_major: [R, N], a row per output -- the stored discharge matrix, or any table of per-sample values; per row
    its N values are sorted (-0.0 and +0.0 one value) and ks[r, p, b] is the largest distance between the empirical CDF
    of them all and that of the rows in bin b of factor p, taken at the end of every run of ties: a ratio of integers,
    the same bits as the numpy statement of the definition, whatever the form.  categories: [P, N] uint8, host or device
    (identifiability.bin_table, pawn.dummy_table), 255 = in no bin of the factor; P <= 16, n_bins <= 64.  counts[p, b]
    is the number of rows in the bin; an empty bin is NaN, and so is every ks of a row that holds a value that is not
    finite.  method: 'auto' (by size), 'lds' (N <= pawn_lds_capacity()) or 'global' (N <= 2**24).  The workspace of the
    call is sized and owned here (include/smart_amd.h: smart_pawn_ks_hip)."""
    who = 'pawn_ks'
    L = _lib.lib()
    code = _code(who, 'method', _lib.PAWN_METHODS, method)
    B = int(n_bins)
    categories = _categories(who, categories, tuple(values_row_major.shape)[-1])
    P = categories.shape[0]
    # ---- from here on the device
    y, R, N, ld = _matrix(values_row_major)
    dev = y.device
    cat = categories.to(dev).contiguous()
    ks = torch.empty((R, P, B), dtype=torch.float64, device=dev)
    counts = torch.empty((P, B), dtype=torch.int32, device=dev)
    if R == 0 or N == 0:
        return PawnResult(ks, counts)
    work, need = _workspace(L.smart_pawn_workspace_bytes(N, R, code), dev)
    _launch(dev, L.smart_pawn_ks_hip, N, R, y.data_ptr(), ld, cat.data_ptr(), P, B, ks.data_ptr(), counts.data_ptr(), code,
            _ptr(work), need)
    return PawnResult(ks, counts)


ERROR_MODEL_ROWS = list(_lib.ERROR_MODEL_ROWS)


def _error_parameters(who, error_parameters, device, n):
    """The error_parameters= argument of a call: [n, 3] (sigma0, sigma1, phi per column of the matrix) or one triple for
    all of them -> (float64 device tensor, its row stride).  Three columns of a wider device matrix -- rows[:, 10:13] of
    the launch matrix of DE-MCz -- are read where they lie; anything else becomes a contiguous [n, 3]."""
    t = error_parameters
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (n, 3) \
            and t.device == device and t.stride(1) == 1 and (n == 1 or t.stride(0) >= 3):
        return t, (t.stride(0) if n > 1 else 3)
    shape = tuple(getattr(t, 'shape', np.shape(t)))
    if shape == (3,):
        t = _as_device(t, device, (1, 3)).repeat(n, 1)
    elif shape == (n, 3):
        t = _as_device(t, device, (n, 3))
    else:
        raise SmartEngineError(-2, "{}: error_parameters must be [{}, 3] (sigma0, sigma1, phi) or one triple, not shape {}."
                               .format(who, n, shape))
    return t, 3


def residual_log_likelihood(discharge_report_major, obs, error_parameters):
    """The log-likelihood of the observations under the residual error model, for every column of a stored [R, N]
    discharge matrix -> device tensor [3, N] float64, the rows in the order of ERROR_MODEL_ROWS: LOGLIK, SSQ, LOGSIG.
    With (sigma0, sigma1, phi) = error_parameters[i]: sigma_t = sigma0 + sigma1 sim[t, i], a_t = (obs[t] - sim[t, i]) /
    sigma_t, and over the observed steps (obs not NaN) an AR(1) with coefficient phi on a_t that restarts, with its
    stationary density, after every gap.  error_parameters: [N, 3], or one triple for all columns; a device tensor that
    is three columns of a wider matrix is read in place.  A column with |phi| >= 1, a parameter that is not finite, or at
    an observed step a flow that is not finite or sigma_t <= 0 is invalid: -inf, NaN, NaN.  No observed step: +0.0 in all
    three.  Two calls give the same bits (include/smart_amd.h: smart_error_model_loglik_hip)."""
    L = _lib.lib()
    sim, R, N, ld = _matrix(discharge_report_major)
    obs = _as_device(obs, sim.device, (R,))
    out = torch.empty((len(ERROR_MODEL_ROWS), N), dtype=torch.float64, device=sim.device)
    if N == 0:
        return out
    err, err_ld = _error_parameters('residual_log_likelihood', error_parameters, sim.device, N)
    _launch(sim.device, L.smart_error_model_loglik_hip, N, R, sim.data_ptr(), ld, obs.data_ptr(), err.data_ptr(), err_ld,
            out.data_ptr())
    return out


def predictive_draws(discharge_report_major, error_parameters, replicates=1, seed=0, truncate=True, out=None):
    """Realisations of the residual error model on top of a stored [R, N] discharge matrix -> device tensor [R, N K]
    float64 with K = replicates: column i K + k is replicate k of column i, sim[t, i] + sigma_t a_t with a_0 = eps_0 /
    sqrt(1 - phi^2), a_t = phi a_{t-1} + eps_t over EVERY report step, eps standard normal (Philox4x32-10 counters
    (column, t // 2) under `seed`, Box-Muller: the same bits from the same seed, whatever the launch).  truncate=True
    replaces a negative flow by 0.  An invalid column (see residual_log_likelihood; judged over every step here) is NaN.
    out: a float64 device matrix [R, N K] of the caller's to write into (its row stride is honoured), or None for a new
    one.  The matrix goes into weighted_quantiles or ensemble_scores as any stored matrix does, with each column's
    weight repeated over its replicates (include/smart_amd.h: smart_error_model_draw_hip)."""
    who = 'predictive_draws'
    L = _lib.lib()
    K = int(replicates)
    if K < 1:
        raise SmartEngineError(-2, "{}: replicates must be at least 1 (got {}).".format(who, replicates))
    sim, R, N, ld = _matrix(discharge_report_major)
    C = N * K
    if out is None:
        out = torch.empty((R, C), dtype=torch.float64, device=sim.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == sim.device and out.dtype == torch.float64
              and tuple(out.shape) == (R, C) and (C == 0 or out.stride(1) == 1)):
        raise SmartEngineError(-2, "{}: out must be a float64 matrix [{}, {}] on {} with unit stride along a row."
                               .format(who, R, C, sim.device))
    if N == 0 or R == 0:
        return out
    err, err_ld = _error_parameters(who, error_parameters, sim.device, N)
    _launch(sim.device, L.smart_error_model_draw_hip, N, R, K, sim.data_ptr(), ld, err.data_ptr(), err_ld,
            int(seed) & (2 ** 64 - 1), 0, 1 if truncate else 0, out.data_ptr(), out.stride(0) if R > 1 else C)
    return out
