"""Multi-objective calibration by NSGA-II (Deb et al. 2002, IEEE Trans. Evol. Comput. 6: non-dominated sorting, crowding
distance, truncation over parents and offspring), the part around the model: the population of N rows on the device
(Nsga2State), the thin binding of the one C entry that moves it (nsga2_step -> smart_nsga2_step_hip, include/smart_amd.h:
rank parents and offspring together from the scores of the offspring, keep the N best in tournament order, make the next
offspring) and a diagnostic (hypervolume_2d).  montecarlo.NSGA2 puts the SMART ensemble launch between two steps; any other
score function can stand there (tests/test_gpu_nsga2.py plays one).

The variation is differential evolution on NSGA-II's selection, as in NSDE and GDE3 (Kukkonen & Lampinen 2005): the base
row is the winner of a binary tournament by rank and crowding, the difference of two rows of the population is added to
it, dimension by dimension with the crossover probability CR.  Simulated binary crossover and polynomial mutation are NOT
built: both need pow, which no library rounds correctly, and every output of the step is defined to the bit -- the numpy
statement of the tests holds the kernels to it bit for bit.
"""
import ctypes

import numpy as np

from . import _lib, generational
from ._lib import SmartEngineError


def cr_threshold(cr):
    """-> C = floor(CR 2^32): what a 32-bit word is compared with"""
    return generational.threshold('nsga2', 'cr', cr)


def directions_of(objectives):
    """[(column, direction)] with a direction 'max', 'min' or ('target', value) -> (columns, codes int32, targets
    float64), as smart_nsga2_step_hip takes them"""
    M = len(objectives)
    if not 2 <= M <= _lib.NSGA2_MAX_OBJECTIVES:
        raise SmartEngineError(-2, "nsga2: {} objectives, between 2 and {}.".format(M, _lib.NSGA2_MAX_OBJECTIVES))
    cols, code, target = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.float64)
    for m, (col, word) in enumerate(objectives):
        value = None
        if isinstance(word, (tuple, list)):
            if len(word) != 2:
                raise SmartEngineError(-7, "nsga2: direction '{}' unknown.".format(word))
            word, value = word
        if word not in _lib.PARETO_DIRECTIONS:
            raise SmartEngineError(-7, "nsga2: direction '{}' unknown.".format(word))
        if (word == 'target') != (value is not None):
            raise SmartEngineError(-7, "nsga2: a 'target' takes a value, '{}' takes none.".format(word))
        cols[m], code[m], target[m] = int(col), _lib.PARETO_DIRECTIONS[word], 0.0 if value is None else float(value)
    if len(set(cols.tolist())) != M:
        raise SmartEngineError(-2, "nsga2: the score columns {} are not {} different ones.".format(cols.tolist(), M))
    return cols, code, target


class _Population(object):
    """One of the two population buffers of a state: x [N, d], keys [N, M], carry [N, n_carry], part [N] uint8"""

    def __init__(self, N, d, M, n_carry, device):
        import torch
        f64 = dict(dtype=torch.float64, device=device)
        self.x = torch.zeros((N, d), **f64)
        self.keys = torch.full((N, M), float('nan'), **f64)
        self.carry = torch.zeros((N, n_carry), **f64)
        self.part = torch.zeros((N,), dtype=torch.uint8, device=device)


class Nsga2State(generational.BoxState):
    """N rows of d varying parameters on the device, and what the host keeps of them.

    Device tensors: two population buffers (`buffers`; `current` is the index of the one that holds the population: x [N, d],
    keys [N, M], carry [N, n_carry] -- a payload that travels with a row: its objective functions --, part [N] uint8: the
    properties x, keys, carry and part read the current one), rank [N] int32, crowding [N], origin [N] int32 (the candidate
    number a row had in the last survive phase) and counts [2] int32 (fronts peeled, candidates of rank 1) of the current
    population; offspring [N, d] and out [N] uint8 (the outstanding offspring), rows [N, ld] (the launch matrix: the step
    writes the d columns `columns`, the others are the caller's), and the workspace of the entry.  Host: g (the generation
    the next vary phase makes, 1 at first), parents (False until the first survive phase), seed, lo, hi, scale =
    b_star (hi - lo), f, C.

    x: [N, d], the initial population (host or device): it is launched as it is, as the offspring of a state without
    parents.  objectives: [(column of the score matrix, direction)], a direction 'max', 'min' or ('target', value).
    rows: a launch matrix of the caller's, or None for one of ld columns filled with `fill`."""

    def __init__(self, x, lo, hi, objectives, seed=0, f=0.5, cr=0.9, b_star=1e-6, n_carry=0, columns=None, ld=None,
                 rows=None, fill=float('nan'), device=None):
        import torch
        self.offspring = self._place('nsga2', 'rows', x, device)
        device = self.device
        N, d = self.offspring.shape
        self.score_columns, self.direction, self.target = directions_of(list(objectives))
        M = len(self.score_columns)
        if not 4 <= N <= _lib.NSGA2_MAX_ROWS:
            raise SmartEngineError(-2, "nsga2: a population of {} rows, between 4 and {}.".format(N, _lib.NSGA2_MAX_ROWS))
        if not 1 <= d <= _lib.NSGA2_MAX_DIMS:
            raise SmartEngineError(-2, "nsga2: {} dimensions, between 1 and {}.".format(d, _lib.NSGA2_MAX_DIMS))
        self.n_rows, self.n_dims, self.n_objectives, self.n_carry = N, d, M, int(n_carry)
        self._set_box('nsga2', self.offspring, lo, hi, b_star, seed, columns, ld, rows, fill)
        self.f, self.C = float(f), cr_threshold(cr)
        self.buffers = [_Population(N, d, M, self.n_carry, device) for _ in range(2)]
        self.current = 0
        self.rank = torch.full((N,), _lib.NSGA2_RANK_OUT, dtype=torch.int32, device=device)
        self.crowding = torch.zeros((N,), dtype=torch.float64, device=device)
        self.origin = torch.arange(N, dtype=torch.int32, device=device)
        self.counts = torch.zeros((2,), dtype=torch.int32, device=device)
        self.out = torch.zeros((N,), dtype=torch.uint8, device=device)
        need = int(_lib.lib().smart_nsga2_workspace_bytes(N, M))
        if need < 0:
            raise SmartEngineError(need, "nsga2: no workspace for {} rows and {} objectives.".format(N, M))
        self.workspace = torch.empty((need,), dtype=torch.uint8, device=device)
        self.parents, self.g = False, 1

    x = property(lambda self: self.buffers[self.current].x)
    keys = property(lambda self: self.buffers[self.current].keys)
    carry = property(lambda self: self.buffers[self.current].carry)
    part = property(lambda self: self.buffers[self.current].part)


def _host(a, kind):
    return a.ctypes.data_as(ctypes.POINTER(kind))


def nsga2_step(state, scores=None, carry_new=None, eligible=None, vary=True):
    """One call of smart_nsga2_step_hip on torch's current stream (include/smart_amd.h has the definition).

    scores: None (no survive phase), or a float64 device tensor [N, C] whose rows lie at a constant stride -- the engine's
    [N, 8] objective table is read in place, the state's score columns select from it.  The survive phase ranks the
    population and the outstanding offspring together (the first call: the N launched rows alone), keeps the N best in
    tournament order in the OTHER population buffer and makes that one current.  carry_new: [N, n_carry], the payload of
    the offspring; eligible: [N] uint8 flags or None.  vary=True then makes the offspring of generation state.g into
    state.offspring, state.out and state.rows, and state.g moves on."""
    import torch
    s = state
    L = _lib.lib()
    N, d, M, nc = s.n_rows, s.n_dims, s.n_objectives, s.n_carry
    score_ptr, ld_scores = None, 0
    if scores is not None:
        if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float64
                and scores.dim() == 2 and scores.shape[0] == N and scores.stride(1) == 1):
            raise SmartEngineError(-2, "nsga2_step: scores must be a float64 device tensor [{}, C] with contiguous rows."
                                   .format(N))
        if int(s.score_columns.max()) >= scores.shape[1]:
            raise SmartEngineError(-2, "nsga2_step: the score columns {} are not among the {} of the scores."
                                   .format(s.score_columns.tolist(), scores.shape[1]))
        score_ptr, ld_scores = scores.data_ptr(), scores.stride(0)
        if carry_new is None and nc > 0:
            raise SmartEngineError(-1, "nsga2_step: the state carries {} values per row: carry_new is needed.".format(nc))
    generational.check_carry_new('nsga2_step', carry_new, N, nc)
    if eligible is not None:
        if not (isinstance(eligible, torch.Tensor) and eligible.is_cuda and eligible.dtype == torch.uint8
                and tuple(eligible.shape) == (N,) and eligible.is_contiguous()):
            raise SmartEngineError(-2, "nsga2_step: eligible must be a contiguous uint8 device tensor [{}].".format(N))
    old, new = s.buffers[s.current], s.buffers[1 - s.current]
    ld = s.ld

    def ptr(t):
        return None if t is None else t.data_ptr()

    with torch.cuda.device(s.device):
        _lib.check(L.smart_nsga2_step_hip(
            N, d, M, nc, s.seed, s.g, int(s.parents),
            ptr(old.x), ptr(old.keys), ptr(old.carry), ptr(old.part),
            ptr(new.x), ptr(new.keys), ptr(new.carry), ptr(new.part),
            ptr(s.rank), ptr(s.crowding), ptr(s.origin), ptr(s.counts), ptr(s.offspring), ptr(s.out),
            score_ptr, ld_scores, _host(s.score_columns, ctypes.c_int32), _host(s.direction, ctypes.c_int32),
            _host(s.target, ctypes.c_double), ptr(eligible), ptr(carry_new), ptr(s.workspace), s.workspace.numel(),
            int(bool(vary)), _host(s.lo, ctypes.c_double), _host(s.hi, ctypes.c_double), _host(s.scale, ctypes.c_double),
            s.f, s.C, s.rows.data_ptr(), ld, _host(s.columns, ctypes.c_int32),
            torch.cuda.current_stream(s.device).cuda_stream))
    if scores is not None:
        s.current, s.parents = 1 - s.current, True
    if vary:
        s.g += 1
    return s


def hypervolume_2d(keys, reference):
    """The area that the rows of keys [n, 2] (larger is better; array or tensor of any device) dominate above the point
    `reference` (two numbers): the hypervolume indicator of two objectives, a diagnostic of how far a front has come.
    Rows with a NaN, and rows that are not better than the reference in both keys, add nothing."""
    import torch
    k = keys if isinstance(keys, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(keys, dtype=np.float64)))
    k = k.to(torch.float64).reshape(-1, 2)
    r0, r1 = float(reference[0]), float(reference[1])
    k = k[(k[:, 0] > r0) & (k[:, 1] > r1)]
    if k.shape[0] == 0:
        return 0.0
    order = torch.argsort(k[:, 0], descending=True, stable=True)
    a, b = k[order, 0], k[order, 1]
    best = torch.cummax(b, dim=0)[0]                        # the best second key among the rows with a first key >= a
    below = torch.cat([torch.full((1,), r1, dtype=torch.float64, device=k.device), best[:-1]])
    return float(((a - r0) * torch.clamp(best - below, min=0.0)).sum())


DIAGNOSTICS_PREFIX = ['generation', 'front_size']


def diagnostics_header(names):
    """The header of `<catchment>.SMART.nsga2.diagnostics`: generation, front_size, the best key per objective."""
    return ','.join(DIAGNOSTICS_PREFIX + ['best_%s' % p for p in names]) + '\n'


def write_diagnostics(path, names, diagnostics):
    """diagnostics: rows of (generation, size of front 1, best key per objective); the first two as integers, the keys
    '%.6e'."""
    generational.write_diagnostics(path, diagnostics_header(names), 2, diagnostics)
