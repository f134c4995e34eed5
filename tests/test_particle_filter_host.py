"""The particle filter without a device: the numpy statement of the assimilation step (tests/cases_particle_filter.py)
against a brute-force reading of its resampling in Python integers, against a grid Bayes filter on a one-dimensional model
of this file's own, and on a synthetic twin of the example catchment run by the oracle; the refusals of the C entry."""
import ctypes
import os
import re

import numpy as np
import pytest

import cases_particle_filter as pf
from conftest import ROOT
from support import E_MODE, E_NO_DEVICE, E_NULL, E_SIZE, FAKE, Margins, margins_dir, refusal

from smartpy_amd import _lib

MARGINS = Margins()
LINES = {}


@pytest.fixture(scope='module', autouse=True)
def _publish():
    yield
    if LINES:
        Margins.publish(STATEMENT_HEAD + ''.join(LINES[k] for k in sorted(LINES)), margins_dir(),
                        'particle_filter_statement.txt')


STATEMENT_HEAD = """# tests/test_particle_filter_host.py: the numpy statement of the particle filter's step against its yardsticks
#
# grid: a one-dimensional storage x <- 0.9 x + rain, observed with Gaussian noise, filtered by the statement (N = 512, tau =
#   0.5, state noise 0.2) and by a Bayes filter on a grid of 4,000 cells of 0.01 (the model step splits a cell's mass
#   linearly between the two cells it lands in, which keeps its mean).  Per step, z = (the statement's weighted mean - the
#   grid's posterior mean) / (the grid's posterior standard deviation / sqrt(ess)): the error of the mean in units of its
#   Monte-Carlo standard error, taken after the update and before the resampling, where ess describes the weights.  The
#   central limit theorem puts the root mean square of z at 1 for independent draws; resampled particles share ancestors,
#   which raises it.  THE BOUND IS 2, from that reasoning and not from these figures; the worst single step is recorded.
# twin: the example catchment, daily steps, truth = the example row, 512 particles with parameters +-30 % around it,
#   observations with sigma = 0.02 mean + 0.1 Q, 120 daily windows, tau = 0.5, state noise 0.05, no jitter.  ratio = the RMSE
#   of the weighted analysis mean against the truth over the RMSE of the open-loop ensemble mean.  THE BOUND IS 1.
"""


# ---- the resampling against a brute-force reading -----------------------------------------------------------------------
def brute_parents(q, rho):
    """a_j = #{i : N C_i <= j Q + rho}, counted one by one in Python integers"""
    q = [int(v) for v in q]
    N, C, run = len(q), [], 0
    for v in q:
        run += v
        C.append(run)
    return [sum(1 for i in range(N) if N * C[i] <= j * C[-1] + rho) for j in range(N)]


@pytest.mark.parametrize('N', pf.RESAMPLING_SIZES)
def test_resampling_equals_the_brute_force_reading(N):
    for name, q in pf.weight_patterns(N, seed=N).items():
        Q = int(q.astype(object).sum())
        for rho in sorted({0, Q - 1, Q // 2, pf.comb_offset(7, 3, Q)}):
            got = pf.parents_of(q, rho)
            assert got.tolist() == brute_parents(q, rho), (name, rho)
            # every child has a parent of positive weight; particle i has floor(N q_i / Q) children or one more
            assert (q[got] > 0).all(), (name, rho)
            children = np.bincount(got, minlength=N)
            floor = np.array([N * int(v) // Q for v in q])
            assert ((children == floor) | (children == floor + 1)).all() and children.sum() == N, (name, rho)
            assert (children[q == 0] == 0).all()
            assert (np.diff(got) >= 0).all()


def test_a_threshold_exactly_on_a_boundary_belongs_to_the_next_particle():
    q = np.array([3, 1, 0, 4], dtype=np.uint64)         # N = 4, Q = 8, N C = 12, 16, 16, 32: j Q + rho = 16 at j = 2, rho = 0
    assert pf.parents_of(q, 0).tolist() == [0, 0, 3, 3] == brute_parents(q, 0)
    assert pf.parents_of(q, 4).tolist() == [0, 1, 3, 3] == brute_parents(q, 4)      # ... and 12 at j = 1


def test_the_drawn_offset_lies_below_Q_and_the_clamp_holds_it_there():
    for Q in (1, 2, 4194304, 3 * 4194304 + 17, 1 << 41):
        for k in range(50):
            rho = pf.comb_offset(seed=0xDEADBEEF12345678, k=k, Q=Q)
            assert 0 <= rho < Q
        assert pf.comb_offset(1, 0, Q, offset=Q) == Q - 1 == pf.comb_offset(1, 0, Q, offset=Q + 5)
        assert pf.comb_offset(1, 0, Q, offset=0) == 0
    # the draws differ from window to window and from seed to seed, and spread over [0, Q)
    draws = [pf.comb_offset(5, k, 1 << 30) for k in range(200)]
    assert len(set(draws)) == 200 and min(draws) < (1 << 30) // 20 and max(draws) > (1 << 30) * 19 // 20
    assert pf.comb_offset(6, 0, 1 << 30) != pf.comb_offset(5, 0, 1 << 30)


def test_quantise_and_decide():
    q, m = pf.quantise(np.array([0.0, -np.inf, np.log(0.5), np.nan, -1e6, -800.0]))
    assert q.tolist() == [pf.UNIT, 0, pf.UNIT // 2, 0, 0, 0] and m == 0.0
    assert pf.quantise(np.array([-np.inf, np.nan]))[0].tolist() == [0, 0]
    ess, Q, S2 = pf.effective_size(np.full(1 << 19, pf.UNIT, dtype=np.uint64))
    assert (ess, Q, S2) == (float(1 << 19), 1 << 41, 1 << 63)      # the largest sums: S2 needs all 64 bits
    ess = pf.effective_size(np.array([pf.UNIT, 0, 0, 0], dtype=np.uint64))[0]
    assert ess == 1.0


def test_the_statement_step_by_step():
    N = 65
    rows, states, columns, lo, hi = pf.particles(N, seed=3)
    rng = np.random.default_rng(4)
    sim = rng.uniform(1.0, 3.0, (3, N))
    obs = np.array([2.0, np.nan, 2.5])
    args = dict(k=5, seed=9, columns=columns, lo=lo, hi=hi, scale=0.01 * (hi - lo), noise=pf.NOISE, z_column=5, area=pf.AREA)
    o = pf.step(rows, states, np.zeros(N), tau=1.0, sim=sim, obs=obs, sigma=(0.1, 0.05), **args)
    assert o.resampled and o.flags == 0 and (o.logw == 0).all() and o.distinct < N
    assert o.Q == int(o.q.astype(object).sum()) and o.q.max() == pf.UNIT
    want = -0.5 * (((sim[0] - 2.0) / (0.1 + 0.05 * 2.0)) ** 2 + ((sim[2] - 2.5) / (0.1 + 0.05 * 2.5)) ** 2)
    assert np.allclose(o.logw_post, want, rtol=1e-14)
    # the evidence increment is the logarithm of the mean likelihood under equal prior weights
    assert abs(o.evidence - np.log(np.mean(np.exp(want)))) < 1e-5
    # a window without an observation changes no weight and resamples nothing, whatever tau says
    o = pf.step(rows, states, o.logw_post, tau=1.0, sim=sim, obs=np.full(3, np.nan), sigma=(0.1, 0.05), **args)
    assert o.flags == pf.NO_OBS and not o.resampled and o.evidence == 0.0 and o.parents.tolist() == list(range(N))
    # every particle lost: the particles are kept, the weights start again
    o = pf.step(rows, states, np.zeros(N), tau=1.0, sim=np.full((3, N), np.nan), obs=obs, sigma=(0.1, 0.05), **args)
    assert o.flags == pf.DEGENERATE and not o.resampled and (o.logw == 0).all() and (o.q == pf.UNIT).all()
    assert o.evidence == -np.inf
    # without jitter and noise the children are copies of their parents
    o = pf.step(rows, states, np.zeros(N), tau=1.0, sim=sim, obs=obs, sigma=(0.1, 0.05),
                **dict(args, scale=0.0 * lo, noise=np.zeros(12)))
    assert np.array_equal(o.rows[:, columns], rows[o.parents][:, columns]) and np.array_equal(o.states, states[o.parents])
    others = [c for c in range(rows.shape[1]) if c not in columns]
    assert np.array_equal(o.rows[:, others], rows[:, others])           # the columns that do not vary are the caller's
    # a soil layer above the capacity of the child's own Z is cut back to it
    high = states.copy()
    high[:, 7] = 1e9
    o = pf.step(rows, high, np.zeros(N), tau=0.0, q_in=np.full(N, pf.UNIT), **args)
    assert not o.resampled and np.array_equal(o.states[:, 7], ((o.rows[:, 5] / 6.0) / 1e3) * pf.AREA)
    assert (o.states[:, 11] != states[:, 11]).any() and (o.states[:, 1] == states[:, 1]).all()        # noise 0.9 and 0


# ---- the refusals of the C entry ----------------------------------------------------------------------------------------
K_ = 'smart_particle_step_hip'
TWO32 = 2 ** 32
_LO = (ctypes.c_double * 16)(*([0.0] * 16))
_HI = (ctypes.c_double * 16)(*([1.0] * 16))
_COLS = (ctypes.c_int32 * 16)(*range(16))
_TWICE = (ctypes.c_int32 * 16)(*([4, 2, 4] + list(range(3, 16))))
_BAD_LO = (ctypes.c_double * 16)(*([0.0, 2.0] + [0.0] * 14))
_NEG_SCALE = (ctypes.c_double * 16)(*([0.0, 0.0, -0.5] + [0.0] * 13))
_NOISE = (ctypes.c_double * 12)(*([0.05] * 12))
_NOISE_ONE = (ctypes.c_double * 12)(*([0.05] * 11 + [1.0]))
_NOISE_NAN = (ctypes.c_double * 12)(*([float('nan')] + [0.05] * 11))


def _addr(a):
    return ctypes.addressof(a)


VALID = dict(n_particles=8, n_dims=3, seed=1, step=0, phases=7, n_reports=2, sim=FAKE, ld_sim=8, obs=FAKE, sigma0=0.1,
             sigma1=0.1, tau=0.5, q_in=None, offset=-1, rows_in=FAKE, rows_out=FAKE, ld=10, columns=_addr(_COLS), z_column=5,
             area_m2=1e6, lo=_addr(_LO), hi=_addr(_HI), scale=_addr(_LO), noise=_addr(_NOISE), states_in=FAKE,
             states_out=FAKE, logw_in=FAKE, logw_out=FAKE, q=FAKE, parents=FAKE, stats=FAKE, counts=FAKE, workspace=FAKE,
             workspace_bytes=1 << 20, stream=None)
REQUIRED = K_ + ': logw_in, logw_out, q, parents, stats, counts and workspace are required (%s is NULL)'
WEIGH = K_ + ': the weigh phase without q_in needs sim and obs (%s is NULL)'
MOVE = K_ + ': the move phase needs rows_in, rows_out, states_in, states_out, lo, hi, scale, noise and columns (%s is NULL)'

CASES = [
    (dict(logw_in=None), E_NULL, REQUIRED % 'logw_in'),
    (dict(q=None, counts=None), E_NULL, REQUIRED % 'q'),
    (dict(workspace=None, n_particles=0), E_NULL, REQUIRED % 'workspace'),
    (dict(n_particles=0), E_SIZE, K_ + ': n_particles 0 must be in 1 .. 524288'),
    (dict(n_particles=(1 << 19) + 1, ld_sim=1 << 20), E_SIZE, K_ + ': n_particles 524289 must be in 1 .. 524288'),
    (dict(n_dims=0), E_SIZE, K_ + ': n_dims 0 must be in 1 .. 16'),
    (dict(n_dims=17), E_SIZE, K_ + ': n_dims 17 must be in 1 .. 16'),
    (dict(step=-1), E_SIZE, K_ + ': step -1 must be in 0 .. 4294967295'),
    (dict(step=TWO32), E_SIZE, K_ + ': step 4294967296 must be in 0 .. 4294967295'),
    (dict(phases=0), E_MODE, K_ + ": phases '0' unknown."),
    (dict(phases=8), E_MODE, K_ + ": phases '8' unknown."),
    (dict(tau=float('nan')), E_SIZE, K_ + ': tau nan must be finite and >= 0'),
    (dict(tau=-0.5), E_SIZE, K_ + ': tau -0.5 must be finite and >= 0'),
    (dict(offset=1 << 41), E_SIZE, K_ + ': offset 2199023255552 must be below 2^41 (negative: drawn)'),
    (dict(sim=None), E_NULL, WEIGH % 'sim'),
    (dict(obs=None), E_NULL, WEIGH % 'obs'),
    (dict(n_reports=0), E_SIZE, K_ + ': n_reports 0 must be in 1 .. 2^31 - 1'),
    (dict(ld_sim=7), E_SIZE, K_ + ': ld_sim 7 is less than n_samples 8'),
    (dict(sigma0=0.0), E_SIZE, K_ + ': sigma0 0 must be finite and > 0'),
    (dict(sigma0=-1.0), E_SIZE, K_ + ': sigma0 -1 must be finite and > 0'),
    (dict(sigma0=float('inf')), E_SIZE, K_ + ': sigma0 inf must be finite and > 0'),
    (dict(sigma1=-0.1), E_SIZE, K_ + ': sigma1 -0.1 must be finite and >= 0'),
    (dict(sigma1=float('nan')), E_SIZE, K_ + ': sigma1 nan must be finite and >= 0'),
    (dict(rows_in=None), E_NULL, MOVE % 'rows_in'),
    (dict(states_out=None), E_NULL, MOVE % 'states_out'),
    (dict(noise=None), E_NULL, MOVE % 'noise'),
    (dict(columns=None), E_NULL, MOVE % 'columns'),
    (dict(ld=2), E_SIZE, K_ + ': ld 2 is less than n_dims 3'),
    (dict(columns=_addr(_TWICE)), E_SIZE, K_ + ': columns[0] and columns[2] name the same column 4'),
    (dict(lo=_addr(_BAD_LO)), E_SIZE, K_ + ': lo[1] 2 and hi[1] 1: need finite lo <= hi'),
    (dict(z_column=10), E_SIZE, K_ + ': z_column 10 must be in 0 .. 9'),
    (dict(z_column=-1), E_SIZE, K_ + ': z_column -1 must be in 0 .. 9'),
    (dict(scale=_addr(_NEG_SCALE)), E_SIZE, K_ + ': scale[2] -0.5 must be finite and >= 0'),
    (dict(noise=_addr(_NOISE_ONE)), E_SIZE, K_ + ': noise[11] 1 must be in [0, 1)'),
    (dict(noise=_addr(_NOISE_NAN)), E_SIZE, K_ + ': noise[0] nan must be in [0, 1)'),
    (dict(area_m2=0.0), E_SIZE, K_ + ': area_m2 0 must be finite and > 0'),
    (dict(workspace_bytes=1000), E_SIZE, K_ + ': workspace_bytes 1000, need 99328'),
]


@pytest.mark.parametrize('changes,code,text', CASES, ids=['%02d-%s' % (i, '-'.join(c[0])) for i, c in enumerate(CASES)])
def test_refusals(changes, code, text):
    assert refusal({K_: VALID}, K_, changes) == (code, text)


def test_a_well_formed_call_gets_as_far_as_the_device():
    if _lib.lib().smart_device_count() == 0:
        for changes in (dict(), dict(phases=1), dict(phases=2, rows_in=None, sim=None), dict(phases=4, sim=None, obs=None),
                        dict(q_in=FAKE, sim=None, obs=None, sigma0=0.0, n_reports=0), dict(offset=(1 << 41) - 1),
                        dict(n_particles=1 << 19, ld_sim=1 << 19, workspace_bytes=98304 + (4 << 19)),
                        dict(step=TWO32 - 1, tau=0.0), dict(n_dims=16, ld=16)):
            rc, text = refusal({K_: VALID}, K_, changes)
            assert rc == E_NO_DEVICE and 'device' in text, changes
    else:
        assert refusal({K_: VALID}, K_, dict(q=None))[0] == E_NULL


def test_the_workspace_query_and_the_binding():
    L = _lib.lib()
    assert L.smart_particle_workspace_bytes(1) == 98304 + 1024 and L.smart_particle_workspace_bytes(257) == 98304 + 2048
    assert L.smart_particle_workspace_bytes(1 << 19) == 98304 + (4 << 19)
    assert L.smart_particle_workspace_bytes(0) == E_SIZE == L.smart_particle_workspace_bytes((1 << 19) + 1)
    header = open(os.path.join(ROOT, 'include', 'smart_amd.h')).read()
    declared = re.search(r'^int %s\(([^;]*)\);' % K_, header, re.M)
    names = re.findall(r'(\w+)\s*(?:,|$)', declared.group(1).replace('\n', ' '))
    assert names == list(VALID) and len(_lib.SYMBOLS[K_][1]) == len(VALID)
    for macro, value in (('SMART_PARTICLE_MAX_PARTICLES', 1 << 19), ('SMART_PARTICLE_STATES', pf.STATES),
                         ('SMART_PARTICLE_FIRST_LAYER', pf.FIRST_LAYER), ('SMART_PARTICLE_FLAG_DEGENERATE', pf.DEGENERATE),
                         ('SMART_PARTICLE_FLAG_NO_OBS', pf.NO_OBS), ('SMART_PARTICLE_WEIGH', _lib.PARTICLE_WEIGH),
                         ('SMART_PARTICLE_RESAMPLE', _lib.PARTICLE_RESAMPLE), ('SMART_PARTICLE_MOVE', _lib.PARTICLE_MOVE)):
        assert re.search(r'^#define %s %d$' % (macro, value), header, re.M), macro
    for table, prefix in ((_lib.PARTICLE_STATS, ''), (_lib.PARTICLE_COUNTS, '')):
        for index, name in enumerate(table):
            assert re.search(r'^#define SMART_PARTICLE_%s %d$' % (name, index), header, re.M), name
    from smartpy_amd import build, particle
    assert build.UNITS['smart_particle.hip'] == ['-ffp-contract=off']
    assert particle.UNIT == pf.UNIT and L.smart_abi_version() == 7
    with pytest.raises(_lib.SmartEngineError, match=r'state_noise 1.0 must be in \[0, 1\)'):
        particle.noise_of(1.0)


# ---- the statement against a grid Bayes filter --------------------------------------------------------------------------
GRID = dict(N=512, T=60, tau=0.5, noise=0.2, sigma=0.5, cells=4000, top=40.0)


def grid_run(seed):
    """-> (z per step, ess per step): the statement on x <- 0.9 x + rain against the Bayes filter on a grid"""
    g = GRID
    rng = np.random.default_rng(seed)
    rain = rng.exponential(1.0, g['T'])
    truth, x = [], 5.0
    for t in range(g['T']):
        x = (0.9 * x + rain[t]) * (1.0 + g['noise'] * rng.uniform(-1.0, 1.0))
        truth.append(x)
    # (the truth is perturbed after the model step, the filter's particles after the update: the same chain of densities,
    # read from the other side of the observation)
    obs = np.array(truth) + rng.normal(0.0, g['sigma'], g['T'])
    # ---- the grid: cell centres, the density as mass per cell
    n, top = g['cells'], g['top']
    h = top / n
    c = (np.arange(n) + 0.5) * h
    mass = np.where((c >= 2.0) & (c <= 8.0), 1.0, 0.0)
    mass /= mass.sum()
    # the multiplicative noise as a matrix: a cell's mass spreads uniformly over [c (1 - noise), c (1 + noise)]
    lo_e, hi_e = c * (1.0 - g['noise']), c * (1.0 + g['noise'])
    edges = np.arange(n + 1) * h
    overlap = np.clip(np.minimum(hi_e[None, :], edges[1:, None]) - np.maximum(lo_e[None, :], edges[:-1, None]), 0.0, None)
    spread = overlap / (hi_e - lo_e)[None, :]
    # ---- the particles: the statement's own arrays, state 0 is x, one varying parameter that is never jittered
    N = g['N']
    rows = np.full((N, 6), 100.0)
    states = np.zeros((N, pf.STATES))
    states[:, 0] = rng.uniform(2.0, 8.0, N)
    noise = np.zeros(pf.STATES)
    noise[0] = g['noise']
    logw = np.zeros(N)
    z, sizes = [], []
    for t in range(g['T']):
        # the model
        states[:, 0] = 0.9 * states[:, 0] + rain[t]
        moved = np.zeros(n)
        at = 0.9 * c + rain[t]
        place = np.clip(at / h - 0.5, 0.0, n - 1.000001)
        cell, share = place.astype(int), place - place.astype(int)
        np.add.at(moved, cell, mass * (1.0 - share))
        np.add.at(moved, cell + 1, mass * share)
        # the update
        like = np.exp(-0.5 * ((c - obs[t]) / g['sigma']) ** 2)
        post = moved * like
        post /= post.sum()
        mean = (post * c).sum()
        sd = np.sqrt((post * (c - mean) ** 2).sum())
        o = pf.step(rows, states, logw, k=t, seed=seed, columns=[0], lo=np.array([0.0]), hi=np.array([200.0]),
                    scale=np.array([0.0]), noise=noise, z_column=5, area=pf.AREA, tau=g['tau'],
                    sim=states[None, :, 0], obs=obs[t:t + 1], sigma=(g['sigma'], 0.0))
        w = o.q.astype(np.float64)
        z.append(((w * states[:, 0]).sum() / w.sum() - mean) / (sd / np.sqrt(o.ess)))
        sizes.append(o.ess)
        states, logw = o.states, o.logw
        mass = spread @ post
    return np.array(z), np.array(sizes)


@pytest.mark.parametrize('seed', range(1, 7))
def test_statement_follows_the_grid_bayes_filter(seed):
    z, sizes = grid_run(seed)
    rms = float(np.sqrt(np.mean(z ** 2)))
    LINES['grid %d' % seed] = 'grid  seed %d  rms z %.3f  worst |z| %.3f  smallest ess %.1f of %d\n' % (
        seed, rms, np.abs(z).max(), sizes.min(), GRID['N'])
    print(LINES['grid %d' % seed])
    assert rms <= 2.0


# ---- the synthetic twin on the oracle ------------------------------------------------------------------------------------
TWIN = dict(N=512, windows=120, tau=0.5, noise=0.05, spread=0.30)


def twin_run(example, seed):
    """-> (RMSE of the analysis mean, RMSE of the open-loop mean) against the truth's discharge"""
    from oracle import smart_oracle as so
    t = TWIN
    N, K = t['N'], t['windows']
    area, truth_row = example['area'], np.asarray(example['params'], dtype=np.float64)
    rain, peva = example['rain_daily'][:K], example['peva_daily'][:K]
    rng = np.random.default_rng(seed)

    def advance(rows, states, k):
        """one daily step of every particle -> (discharge [N], states [N, 12])"""
        dis, new = np.empty(len(rows)), np.empty_like(states)
        start = np.zeros(19)
        for i in range(len(rows)):
            start[7:] = states[i]
            d, _, fin = so.all_steps(area, 86400.0, 1, rain[k:k + 1], peva[k:k + 1], rows[i], start, so.REPORT_SUMMARY, 1)
            dis[i], new[i] = d[0], fin[7:]
        return dis, new

    x = so.initial(area, truth_row, example['extra'])[None, 7:]
    truth = np.empty(K)
    for k in range(K):
        d, x = advance(truth_row[None, :], x, k)
        truth[k] = d[0]
    sigma0, sigma1 = 0.02 * truth.mean(), 0.1
    obs = truth + rng.normal(0.0, 1.0, K) * (sigma0 + sigma1 * truth)
    rows = truth_row[None, :] * rng.uniform(1.0 - t['spread'], 1.0 + t['spread'], (N, 10))
    lo, hi = (1.0 - t['spread']) * truth_row, (1.0 + t['spread']) * truth_row
    start = np.stack([so.initial(area, r, example['extra'])[7:] for r in rows])
    # the open loop
    states, open_mean = start.copy(), np.empty(K)
    for k in range(K):
        d, states = advance(rows, states, k)
        open_mean[k] = d.mean()
    # the filter
    states, logw, analysis = start.copy(), np.zeros(N), np.empty(K)
    resampled = 0
    for k in range(K):
        d, states = advance(rows, states, k)
        o = pf.step(rows, states, logw, k=k, seed=seed, columns=list(range(10)), lo=lo, hi=hi, scale=np.zeros(10),
                    noise=np.full(pf.STATES, t['noise']), z_column=5, area=area, tau=t['tau'], sim=d[None, :],
                    obs=obs[k:k + 1], sigma=(sigma0, sigma1))
        w = o.q.astype(np.float64)
        analysis[k] = (w * d).sum() / w.sum()
        rows, states, logw = o.rows, o.states, o.logw
        resampled += o.resampled
    rmse = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))       # noqa: E731
    return rmse(analysis), rmse(open_mean), resampled


@pytest.mark.parametrize('seed', range(1, 7))
def test_synthetic_twin_beats_the_open_loop(example, seed):
    filtered, open_loop, resampled = twin_run(example, seed)
    LINES['twin %d' % seed] = 'twin  seed %d  analysis RMSE %.4f  open loop %.4f  ratio %.3f  resampled %d of %d windows\n' % (
        seed, filtered, open_loop, filtered / open_loop, resampled, TWIN['windows'])
    print(LINES['twin %d' % seed])
    assert filtered < open_loop
