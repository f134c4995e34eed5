"""The way a stored matrix reaches the five analyses of smartpy_amd.analysis (one helper: on the device, unit stride along
a row, ld = the row stride): every function gives the same bits for a contiguous matrix, for a row-strided view of a
wider device tensor (ld = N + 6, NaN in the padding: a kernel that read it would show) and for a column-strided view
(every second column of a [R, 2N] tensor: copied before the launch).  Bits are compared as int64, so a NaN counts.

Shapes: N = 70 samples (a full wavefront and a partial one), R = 5 report steps, two windows and one step in neither, two
probabilities; for the Sobol indices n_base = 8, n_params = 2 (32 columns), three rows, four bootstrap replicates.  And
every function once more on the first row alone, where the row stride of a view says nothing and ld is the row length.
The C entries' own handling of ld is the business of the tests of each analysis; this one is about the Python side."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = 6
WINDOWS = np.array([0, 0, 1, 1, -1], dtype=np.int32)
PROBS = (0.25, 0.75)
N_BASE, N_PARAMS, RESAMPLES = 8, 2, 4


def flows(rows, cols, seed):
    return np.random.default_rng(seed).gamma(2.0, 1.5, size=(rows, cols)) + 0.05


def layouts(base):
    """host [R, N] -> {name: device tensor of the same values}: contiguous, a row-strided view, a column-strided view"""
    import torch
    R, N = base.shape
    dev = torch.from_numpy(base).cuda()
    wide = torch.full((R, N + PAD), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :N] = dev
    double = torch.full((R, 2 * N), float('nan'), dtype=torch.float64, device='cuda')
    double[:, ::2] = dev
    out = {'contiguous': dev, 'rows': wide[:, :N], 'columns': double[:, ::2]}
    assert out['rows'].stride() == (N + PAD, 1) and out['columns'].stride() == (2 * N, 2)
    assert all(torch.equal(t, dev) for t in out.values())
    return out


def call(name, sim):
    """-> the outputs of engine.<name> on the device matrix, as a tuple of tensors"""
    from smartpy_amd import engine
    R = sim.shape[0]
    obs = flows(1, R, 7)[0]
    if name == 'objective_functions':
        return (engine.objective_functions(sim, obs, gw_sim=flows(1, sim.shape[1], 8)[0] / 10.0, gw_obs=0.12667),)
    if name == 'weighted_quantiles':
        return (engine.weighted_quantiles(sim, PROBS, weights=flows(1, sim.shape[1], 9)[0]),)
    if name == 'objective_functions_windows':
        return (engine.objective_functions_windows(sim, obs, WINDOWS[:R], n_windows=2, transform='log', eps=0.01),)
    if name == 'flow_duration':
        return engine.flow_duration(sim, PROBS, obs=obs, windows=WINDOWS[:R], n_windows=2, transform='sqrt', objfn=True)
    res = engine.sobol_indices(sim, N_BASE, N_PARAMS, counts=engine.sobol_counts(N_BASE, RESAMPLES, seed=3))
    return res.S1, res.ST, res.moments, res.S1_std, res.ST_std


def bits(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.contiguous().cpu().numpy().view(np.int64) for t in tensors]


@pytest.mark.parametrize('name', ['objective_functions', 'weighted_quantiles', 'objective_functions_windows',
                                  'flow_duration', 'sobol_indices'])
def test_every_layout_of_the_matrix_gives_the_same_bits(name):
    base = flows(3, N_BASE * (N_PARAMS + 2), 1) if name == 'sobol_indices' else flows(5, 70, 2)
    for rows in (base, base[:1]):
        got = {how: bits(call(name, sim)) for how, sim in layouts(rows).items()}
        want = got['contiguous']
        if len(rows) > 1:       # (one report step alone is no window of two: NaN there is the answer)
            assert any(np.isfinite(a.view(np.float64)).any() for a in want), 'nothing but NaN: the comparison says nothing'
        for how in ('rows', 'columns'):
            assert len(got[how]) == len(want)
            for a, b in zip(got[how], want):
                assert a.shape == b.shape and np.array_equal(a, b), (name, how, len(rows))
