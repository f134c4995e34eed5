"""Latin hypercube sampling of the SMART parameter space -- host side (montecarlo/lhs.py:133-167).

Same algorithm and the same random stream as the reference: one rand(n, 10) draw and ten permutation(n)
draws from NumPy's legacy global RNG, (permutation + rand) / n, then the inverse CDF of the uniform
distribution on [lo, hi], lo + u * (hi - lo) (what scipy.stats.uniform.ppf evaluates).  With the same
np.random.seed the matrix is bit-identical to the reference's (tests/test_host_logic.py, KAT-7).
"""
import numpy as np

PARAMETER_NAMES = ['T', 'C', 'H', 'D', 'S', 'Z', 'SK', 'FK', 'GK', 'RK']     # parameters.py:25


def latin_hypercube(sample_size, ranges, names=None, seed=None):
    """[sample_size, len(names)] float64.  seed=None draws from the current global stream like the reference;
    an integer seeds NumPy's legacy generator first (the reference leaves seeding to the caller)."""
    names = names or PARAMETER_NAMES
    if seed is not None:
        np.random.seed(seed)
    bounds = np.asarray([[ranges[p][0], ranges[p][1]] for p in names], dtype=np.float64)
    nb = len(names)
    random_matrix = np.random.rand(sample_size, nb)
    plan = np.empty((sample_size, nb), dtype=np.float64)
    for p in range(nb):
        plan[:, p] = np.random.permutation(sample_size)
    plan += random_matrix
    plan /= sample_size
    return bounds[:, 0] + plan * (bounds[:, 1] - bounds[:, 0])


def latin_hypercube_device(sample_size, ranges, names=None, seed=None, device=None):
    """The same sampling plan built on the GPU with torch (for N >= 1e6, where the host sampler's 1.5 s would be
    comparable to the whole ensemble launch): one rand(n, k) draw, one random permutation of the n strata per
    parameter, (stratum + rand) / n, inverse CDF of the uniform distribution.  Same algorithm as
    montecarlo/lhs.py:133-167 but NOT the same random stream as NumPy's legacy generator: use
    `latin_hypercube` when the sample has to be reproduced bit for bit."""
    import torch
    names = names or PARAMETER_NAMES
    device = torch.device(device) if device is not None else torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    gen = torch.Generator(device=device)
    if seed is not None:
        gen.manual_seed(int(seed))
    else:
        gen.seed()
    nb = len(names)
    lo = torch.tensor([ranges[p][0] for p in names], dtype=torch.float64, device=device)
    hi = torch.tensor([ranges[p][1] for p in names], dtype=torch.float64, device=device)
    rnd = torch.rand((sample_size, nb), dtype=torch.float64, device=device, generator=gen)
    # a random permutation per column: argsort of iid uniforms
    strata = torch.argsort(torch.rand((sample_size, nb), dtype=torch.float64, device=device, generator=gen), dim=0)
    plan = (strata.to(torch.float64) + rnd) / sample_size
    return lo + plan * (hi - lo)


def saltelli_design(base_size, ranges, names=None, vary=None, fixed=None, seed=None):
    """The Saltelli design of a Sobol sensitivity analysis -> ([base_size * (k + 2), len(names)] float64, the k names that
    vary).  vary: the parameters that move (default: all of `names`, in their order); the others stay at fixed[name], or
    at the midpoint of their range.  One Latin hypercube of base_size rows x 2k columns on [0, 1), built like
    latin_hypercube -- (permutation + uniform) / n -- but drawn from numpy.random.Generator(PCG64(seed)): the legacy
    global stream is neither read nor advanced.  Columns 0 .. k-1 scaled to the ranges are A, columns k .. 2k-1 are B,
    AB_j is A with column j taken from B, and the rows are BLOCK-MAJOR, [A ; B ; AB_0 ; ... ; AB_{k-1}]: in a report-major
    discharge matrix every block of a report step is base_size contiguous values (engine.sobol_indices)."""
    names = list(names or PARAMETER_NAMES)
    vary = list(names if vary is None else vary)
    unknown = [p for p in vary if p not in names]
    if unknown:
        raise Exception("saltelli_design: the parameter(s) {} to vary are not among {}."
                        .format(', '.join("'{}'".format(p) for p in unknown), ', '.join(names)))
    if len(set(vary)) != len(vary) or not vary:
        raise Exception("saltelli_design: `vary` must name at least one parameter, each once.")
    fixed = dict(fixed or {})
    unknown = [p for p in fixed if p not in names or p in vary]
    if unknown:
        raise Exception("saltelli_design: the fixed parameter(s) {} are unknown or also vary."
                        .format(', '.join("'{}'".format(p) for p in unknown)))
    n, k = int(base_size), len(vary)
    if n < 1:
        raise Exception("saltelli_design: base_size must be at least 1 (got {}).".format(base_size))
    rng = np.random.Generator(np.random.PCG64(seed))
    plan = rng.random((n, 2 * k))
    for c in range(2 * k):
        plan[:, c] += rng.permutation(n)
    plan /= n
    lo = np.asarray([ranges[p][0] for p in vary], dtype=np.float64)
    hi = np.asarray([ranges[p][1] for p in vary], dtype=np.float64)
    a = lo + plan[:, :k] * (hi - lo)
    b = lo + plan[:, k:] * (hi - lo)
    base = np.asarray([fixed.get(p, 0.5 * (float(ranges[p][0]) + float(ranges[p][1]))) for p in names], dtype=np.float64)
    cols = [names.index(p) for p in vary]
    design = np.tile(base, (n * (k + 2), 1))
    design[:n, cols] = a
    design[n:2 * n, cols] = b
    for j in range(k):
        block = design[(2 + j) * n:(3 + j) * n]
        block[:, cols] = a
        block[:, cols[j]] = b[:, j]
    return design, vary
