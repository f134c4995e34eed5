"""The particle filter's step on the device: smart_particle_step_hip against the numpy statement of
tests/cases_particle_filter.py BIT FOR BIT -- parents, launch rows, states, log-weights, the effective sample size, the
decision, the sums and the count of distinct parents -- with the integer weights given (q_in) and with the window weighed on
the device, every array of the state inside a buffer with guards, the window's matrix with padding behind its columns.

The one device operation of the weights that is not correctly rounded by definition is exp: the device's integers may
differ from the statement's by one unit, never by more, and everything downstream is compared with the statement fed the
DEVICE's integers.  The evidence increment takes two logarithms and is held to 16 ulp of its largest term."""
import numpy as np
import pytest

import cases_particle_filter as pf
from support import Guarded, Margins, eng, margins_dir, padded, same_bits      # noqa: F401 (eng: a fixture)

pytestmark = pytest.mark.gpu

GUARD = 32
SENTINEL = {'float64': -7.0, 'int64': -7, 'int32': -7}
ARRAYS = ('rows', 'rows_next', 'states', 'states_next', 'logw', 'logw_next', 'q', 'parents', 'stats', 'counts')
RESAMPLED, Q_, DISTINCT, FLAGS, OFFSET, S2, Q_PRIOR = range(7)
ESS, EVIDENCE, MAX, MAX_PRIOR = range(4)
MARGINS = Margins()


@pytest.fixture(scope='module', autouse=True)
def _publish():
    yield
    lines = ['# tests/test_gpu_particle_filter.py: the share of its tolerance the evidence increment used (16 ulp of the',
             '# largest of its four terms), and the integers of the device that differ from the statement\'s (by one unit)']
    lines += ['%-44s %.3f  %s' % (key, value, where) for key, (value, where) in sorted(MARGINS.items())]
    Margins.publish('\n'.join(lines), margins_dir(), 'particle_filter_margins.txt')


class Host(object):
    """the host's copy of a state: rows, states, logw, and what every step takes"""

    def __init__(self, N, seed, jitter, noise, tau, z_varies=True, ld=12):
        self.rows, self.states, self.columns, self.lo, self.hi = pf.particles(N, seed, ld=ld, z_varies=z_varies)
        self.logw = np.zeros(N)
        self.N, self.seed, self.tau, self.k = N, seed, tau, 0
        self.scale, self.noise = jitter * (self.hi - self.lo), np.asarray(noise, dtype=np.float64)

    def step(self, **kw):
        o = pf.step(self.rows, self.states, self.logw, self.k, self.seed, self.columns, self.lo, self.hi, self.scale,
                    self.noise, 5, pf.AREA, self.tau, **kw)
        self.rows, self.states, self.logw = o.rows, o.states, o.logw
        self.k += 1
        return o


def device_state(h, jitter, sigma=(1.0, 0.0)):
    """-> (the ParticleState of the host's copy, its arrays moved into guarded buffers)"""
    from smartpy_amd import particle
    t = particle.ParticleState(h.rows, h.states, h.lo, h.hi, h.columns, pf.AREA, sigma=sigma, tau=h.tau,
                               state_noise=h.noise, jitter=jitter, seed=h.seed)
    t.logw.copy_(cuda(h.logw))
    buffers = {}
    for name in ARRAYS:
        a = getattr(t, name)
        dtype = str(a.dtype).split('.')[-1]
        buffers[name] = Guarded(a.numel(), dtype=dtype, guard=GUARD, sentinel=SENTINEL[dtype])
        inner = buffers[name].inner().view(a.shape)
        inner.copy_(a)
        setattr(t, name, inner)
    assert same_bits(t.scale, h.scale)
    return t, buffers


def cuda(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def compare(t, buffers, h, o, what=''):
    """the state after a step against the statement's, and the guards"""
    counts, stats = t.counts.cpu().numpy(), t.stats.cpu().numpy()
    assert counts[RESAMPLED] == int(o.resampled) and counts[FLAGS] == o.flags, what
    assert counts[Q_] == o.Q and np.uint64(counts[S2]) == np.uint64(o.S2 % (1 << 64)) and counts[OFFSET] == o.rho, what
    assert same_bits(stats[ESS], np.float64(o.ess)), what
    assert same_bits(t.parents.cpu().numpy(), o.parents.astype(np.int32)), what
    assert counts[DISTINCT] == o.distinct, what
    assert same_bits(t.q.cpu().numpy(), o.q.astype(np.int64)), what
    assert same_bits(t.rows.cpu().numpy(), h.rows), what
    assert same_bits(t.states.cpu().numpy(), h.states), what
    assert same_bits(t.logw.cpu().numpy(), h.logw), what
    assert t.k == h.k
    for name, b in buffers.items():
        assert b.intact(), (what, name)


# ---- the integers given ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', pf.STEP_SIZES)
def test_step_with_given_integers_equals_the_statement(N):
    from smartpy_amd import particle
    seen = set()
    for number, (name, q) in enumerate(pf.weight_patterns(N, seed=N).items()):
        for tau in (1.0, 0.0):
            jitter = (0.0, 0.02)[number % 2]
            h = Host(N, seed=N + number, jitter=jitter, noise=pf.NOISE, tau=tau, z_varies=number % 2 == 0)
            h.logw = -np.arange(N, dtype=np.float64)
            t, buffers = device_state(h, jitter)
            for k in range(2):          # two windows: the halves of the state swap
                o = h.step(q_in=q)
                particle.particle_step(t, q_in=cuda(q, np.int64))
                compare(t, buffers, h, o, (name, tau, k))
                assert np.isnan(t.stats.cpu().numpy()[EVIDENCE])
                seen.add(o.resampled)
                if o.resampled:
                    assert (h.logw == 0).all()
    assert seen == ({True, False} if N > 1 else {False})


def test_both_sides_of_tau_and_a_threshold_on_a_boundary():
    from smartpy_amd import particle
    N = 1000
    q = pf.weight_patterns(N, seed=5)['spread']
    ess = pf.effective_size(q)[0]
    assert 2.0 < ess < N - 2.0
    for tau, resampled in (((ess + 0.5) / N, True), ((ess - 0.5) / N, False), (ess / N, None)):
        h = Host(N, seed=11, jitter=0.0, noise=pf.NOISE, tau=tau)
        t, buffers = device_state(h, 0.0)
        o = h.step(q_in=q)
        particle.particle_step(t, q_in=cuda(q, np.int64))
        compare(t, buffers, h, o, tau)
        assert resampled is None or o.resampled == resampled
    # equal weights and offset 0: j Q + rho = N C_{j-1} for every j, and the particle ON the threshold is passed over
    for N in (4, 257, 1000):
        equal = np.full(N, pf.UNIT, dtype=np.uint64)
        h = Host(N, seed=12, jitter=0.0, noise=np.zeros(12), tau=2.0)       # ess = N < 2 N: resampled
        t, buffers = device_state(h, 0.0)
        o = h.step(q_in=equal, offset=0)
        assert o.resampled and o.parents.tolist() == list(range(N))
        particle.particle_step(t, q_in=cuda(equal, np.int64), offset=0)
        compare(t, buffers, h, o, N)
    q = np.array([3, 1, 0, 4], dtype=np.uint64)         # N C = 12, 16, 16, 32: the thresholds 16 (rho 0) and 12 (rho 4)
    for rho, want in ((0, [0, 0, 3, 3]), (4, [0, 1, 3, 3]), (7, [0, 1, 3, 3]), (1 << 40, [0, 1, 3, 3])):
        h = Host(4, seed=13, jitter=0.0, noise=np.zeros(12), tau=1.0)
        t, buffers = device_state(h, 0.0)
        o = h.step(q_in=q, offset=rho)
        assert o.parents.tolist() == want and o.rho == min(rho, 7)          # (the clamp: rho <= Q - 1)
        particle.particle_step(t, q_in=cuda(q, np.int64), offset=rho)
        compare(t, buffers, h, o, rho)


def test_reflected_and_kept_dimensions_and_a_clamped_layer():
    from smartpy_amd import particle
    N = 257
    q = pf.weight_patterns(N, seed=8)['spread']
    for jitter, kept in ((0.6, False), (1.5, True)):
        h = Host(N, seed=21, jitter=jitter, noise=pf.NOISE, tau=1.0)
        h.rows[::2, 0] = h.lo[1]                        # (column 0 is dimension 1) on the lower bound: half the draws reflect
        h.rows[1::4, 7] = h.hi[2]
        h.states[::3, 7] = 1e9                          # a soil layer far above any capacity
        h.states[::5, 2] = 1e9                          # ... and a reservoir that has none
        before = h.rows.copy()
        t, buffers = device_state(h, jitter)
        o = h.step(q_in=q)
        particle.particle_step(t, q_in=cuda(q, np.int64))
        compare(t, buffers, h, o, jitter)
        child, parent = o.rows[:, h.columns], before[o.parents][:, h.columns]
        assert ((child >= h.lo) & (child <= h.hi)).all()
        same = (child == parent).all(axis=1)
        assert same.any() == kept and not same.all()
        cap = ((o.rows[:, 5] / 6.0) / 1e3) * pf.AREA
        assert (o.states[:, 5:11] <= cap[:, None]).all() and (o.states[:, 7] == cap).any() and (o.states[:, 2] > 1e8).any()


def test_the_largest_ensemble():
    from smartpy_amd import particle
    N = pf.LARGEST
    q = pf.weight_patterns(N, seed=1)['zeros']
    h = Host(N, seed=31, jitter=0.01, noise=pf.NOISE, tau=1.0)
    t, buffers = device_state(h, 0.01)
    o = h.step(q_in=q)
    particle.particle_step(t, q_in=cuda(q, np.int64))
    compare(t, buffers, h, o)
    assert o.resampled and o.parents[-1] > N - 4096
    # all of them at the largest weight: Q = 2^41, S2 = 2^63
    h.tau = t.tau = 2.0
    equal = np.full(N, pf.UNIT, dtype=np.uint64)
    o = h.step(q_in=equal)
    particle.particle_step(t, q_in=cuda(equal, np.int64))
    compare(t, buffers, h, o)
    assert o.Q == 1 << 41 and o.S2 == 1 << 63 and o.resampled


# ---- the window weighed on the device ---------------------------------------------------------------------------------------
def window(N, Rw, seed, missing):
    rng = np.random.default_rng(seed)
    sim = rng.uniform(1.0, 3.0, (Rw, N))
    obs = rng.uniform(1.5, 2.5, Rw)
    obs[list(missing)] = np.nan
    if N > 8:
        sim[0, 3] = np.nan              # a particle that is lost
        sim[Rw - 1, 5] = np.inf
        sim[:, 6] = 1e4                 # differences beyond the range of exp: exp(-1e9) is 0
        sim[:, 7] = 1e200               # ... and beyond the range of the squares: the sum is +inf
    return sim, obs


@pytest.mark.parametrize('N', (1, 65, 1000, 4099))
@pytest.mark.parametrize('Rw,missing', ((1, ()), (3, (1,)), (3, (0, 1, 2))))
def test_weigh_on_the_device(N, Rw, missing):
    from smartpy_amd import _lib, particle
    sigma = (0.05, 0.1)
    sim, obs = window(N, Rw, seed=N + Rw, missing=missing)
    h = Host(N, seed=41, jitter=0.02, noise=pf.NOISE, tau=0.9)
    h.logw = -0.001 * np.arange(N, dtype=np.float64)
    if N > 8:
        h.logw[2] = -np.inf
    t, buffers = device_state(h, 0.02, sigma=sigma)
    sim_d, ld = padded(sim, 7)
    assert ld > N
    obs_d = cuda(obs)
    # the weigh phase alone: logw' bit for bit, the integers within one unit
    particle.particle_step(t, sim_d, obs_d, phases=_lib.PARTICLE_WEIGH)
    want = pf.step(h.rows, h.states, h.logw, 0, h.seed, h.columns, h.lo, h.hi, h.scale, h.noise, 5, pf.AREA, h.tau,
                   sim=sim, obs=obs, sigma=sigma)
    assert same_bits(t.logw_next.cpu().numpy(), want.logw_post)
    if N > 8 and len(missing) < Rw:
        assert np.isneginf(want.logw_post[[2, 3, 5, 7]]).all() and want.q[6] == 0 and np.isfinite(want.logw_post[6])
    q_device = t.q.cpu().numpy()
    differ = int((q_device != want.q.astype(np.int64)).sum())
    print('N %d, Rw %d, missing %s: %d of the integers differ from the statement\'s' % (N, Rw, missing, differ))
    MARGINS.note('q differ N=%d Rw=%d missing=%s' % (N, Rw, list(missing)), float(differ), 'integers')
    assert np.abs(q_device - want.q.astype(np.int64)).max() <= 1
    # the whole step, against the statement fed the device's integers
    o = h.step(sim=sim, obs=obs, sigma=sigma, q_device=q_device)
    particle.particle_step(t, sim_d, obs_d)
    compare(t, buffers, h, o, (N, Rw, missing))
    counts, stats = t.counts.cpu().numpy(), t.stats.cpu().numpy()
    assert same_bits(stats[MAX], np.float64(o.m)) and same_bits(stats[MAX_PRIOR], np.float64(o.m_prior))
    if len(missing) == Rw:
        assert o.flags == pf.NO_OBS and not o.resampled and stats[EVIDENCE] == 0.0 and same_bits(h.logw, want.logw_post)
        return
    # the evidence increment from the device's integers, to 16 ulp of its largest term
    terms = [o.m, np.log(float(counts[Q_]) / pf.UNIT), o.m_prior, np.log(float(counts[Q_PRIOR]) / pf.UNIT)]
    evidence = (terms[0] + terms[1]) - (terms[2] + terms[3])
    tolerance = 16 * np.spacing(max(abs(x) for x in terms))
    MARGINS.note('evidence N=%d Rw=%d missing=%s' % (N, Rw, list(missing)), abs(stats[EVIDENCE] - evidence) / tolerance,
                 'of 16 ulp')
    assert abs(stats[EVIDENCE] - evidence) <= tolerance
    assert abs(counts[Q_PRIOR] - want.Q_prior) <= N and stats[EVIDENCE] < 0.0


def test_a_window_that_loses_every_particle():
    from smartpy_amd import particle
    N = 257
    sim, obs = np.full((2, N), np.nan), np.array([1.0, 2.0])
    h = Host(N, seed=51, jitter=0.0, noise=pf.NOISE, tau=1.0)
    t, buffers = device_state(h, 0.0)
    o = h.step(sim=sim, obs=obs)
    particle.particle_step(t, padded(sim, 3)[0], cuda(obs))
    compare(t, buffers, h, o)
    assert o.flags == pf.DEGENERATE and (h.logw == 0).all() and t.stats.cpu().numpy()[EVIDENCE] == -np.inf
    assert o.parents.tolist() == list(range(N))


def test_same_bits_in_phases_and_on_two_launches():
    import torch
    from smartpy_amd import _lib, particle
    N = 1000
    sim, obs = window(N, 3, seed=61, missing=(1,))
    sim_d, obs_d = padded(sim, 5)[0], cuda(obs)
    results = []
    for cut in ((7,), (7,), (1, 2, 4), (1, 6), (3, 4)):
        h = Host(N, seed=62, jitter=0.02, noise=pf.NOISE, tau=0.9)
        t, buffers = device_state(h, 0.02, sigma=(0.05, 0.1))
        for phases in cut:
            particle.particle_step(t, sim_d, obs_d, phases=phases)
        assert t.k == 1 and all(b.intact() for b in buffers.values())
        results.append([getattr(t, name).clone() for name in ('rows', 'states', 'logw', 'q', 'parents', 'stats', 'counts')])
    assert results[0][6][RESAMPLED].item() == 1
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # ... and with the integers given
    q = cuda(pf.weight_patterns(N, seed=3)['zeros'], np.int64)
    results = []
    for cut in ((7,), (1, 2, 4), (1, 6)):
        h = Host(N, seed=63, jitter=0.02, noise=pf.NOISE, tau=1.0)
        t, buffers = device_state(h, 0.02)
        for phases in cut:
            particle.particle_step(t, q_in=q, phases=phases)
        results.append([getattr(t, name).clone() for name in ('rows', 'states', 'logw', 'q', 'parents', 'counts')])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert _lib.PARTICLE_WEIGH | _lib.PARTICLE_RESAMPLE | _lib.PARTICLE_MOVE == 7


# ---- montecarlo.ParticleFilter on the example catchment ---------------------------------------------------------------------
def _filter(root, days=12, warm=0, **kw):
    import datetime
    from smartpy_amd.montecarlo import ParticleFilter
    from support import EXTRA, settings_file
    name = 'Catchment.pf%d.sttngs' % days
    end = datetime.date(2007, 1, 1) + datetime.timedelta(days=days - 1)      # (the axis holds both ends)
    settings_file(root, name, '01/01/2007', end.strftime('%d/%m/%Y'), warm, simu_minutes=1440)
    args = dict(particles=250, seed=7, sigma=(0.3, 0.1), tau=0.5, state_noise=0.05, jitter=0.01, settings_filename=name)
    args.update(kw)
    a = ParticleFilter('Catchment', root, 'csv', 'csv', **args)
    a.model.extra = EXTRA
    return a


def test_driver_in_literal_mode_equals_the_statement_on_the_oracle(tmp_path):
    """states, rows, parents and bounds against the statement driven by the oracle's all_steps per particle (POW_MUL,
    SUM_GPU), bit for bit given the device's integers"""
    from oracle import smart_oracle as so
    from oracle.analyses import quantiles
    from support import EXTRA, example_root
    a = _filter(example_root(tmp_path), days=12)
    a.math_mode = 'literal'
    a.run(store=True)
    N, K = 250, 12
    model = a.model
    area, rain, peva = float(model.area), np.asarray(model.nd_rain, dtype=np.float64), np.asarray(model.nd_peva, dtype=np.float64)
    obs = np.asarray(model.nd_flow, dtype=np.float64)
    rows = np.array(a.initial_population[:, :10], dtype=np.float64)
    states = np.stack([so.initial(area, r, EXTRA)[7:] for r in rows])
    logw = np.zeros(N)
    stored = {k: v.cpu().numpy() for k, v in a.stored.items()}
    assert stored['discharge'].shape == (K, N) and stored['q'].shape == (K, N)
    prior = np.full(N, float(pf.UNIT))
    scale, noise = a.jitter * (a.hi - a.lo), a.state_noise
    resampled = 0
    for k in range(K):
        sim, start = np.empty((1, N)), np.zeros(19)
        for i in range(N):
            start[7:] = states[i]
            d, _, fin = so.all_steps(area, 86400.0, 1, rain[k:k + 1], peva[k:k + 1], rows[i], start, so.REPORT_SUMMARY, 1,
                                     pow_mode=so.POW_MUL, sum_mode=so.SUM_GPU)
            sim[0, i], states[i] = d[0], fin[7:]
        assert same_bits(stored['discharge'][k:k + 1], sim), k
        o = pf.step(rows, states, logw, k, 7, a.columns, a.lo, a.hi, scale, noise, 5, area, a.tau, sim=sim,
                    obs=obs[k:k + 1], sigma=a.sigma, q_device=stored['q'][k])
        assert np.abs(stored['q'][k] - pf.step(rows, states, logw, k, 7, a.columns, a.lo, a.hi, scale, noise, 5, area, a.tau,
                                               sim=sim, obs=obs[k:k + 1], sigma=a.sigma).q.astype(np.int64)).max() <= 1
        assert same_bits(stored['parents'][k], o.parents.astype(np.int32)), k
        assert same_bits(a.forecast_bounds[:, k:k + 1], quantiles.statement(sim, prior, a.probs)), k
        assert same_bits(a.analysis_bounds[:, k:k + 1], quantiles.statement(sim, o.q.astype(np.float64), a.probs)), k
        assert same_bits(a.ess[k], np.float64(o.ess)) and a.resampled[k] == o.resampled
        rows, states, logw = o.rows, o.states, o.logw
        prior = np.full(N, float(pf.UNIT)) if o.resampled else o.q.astype(np.float64)
        resampled += o.resampled
    assert 0 < resampled < K
    assert same_bits(a.states.cpu().numpy(), states) and same_bits(a.parameters.cpu().numpy(), rows)
    assert same_bits(a.state.logw.cpu().numpy(), logw)


@pytest.mark.parametrize('mode', ('literal', 'fast'))
def test_a_filter_that_never_updates_is_the_ensemble(tmp_path, mode):
    from support import bits_equal, example_root, rel
    a = _filter(example_root(tmp_path), days=40, warm=10, particles=300, tau=0.0, state_noise=0.0, jitter=0.0, assimilate_every=7)
    a.math_mode = mode
    a.run(store=True)
    assert not a.resampled.any() and len(a.ess) == 6            # 5 windows of 7 days and one of 5
    whole = a.model.simulate_ensemble(a.initial_population[:, :10], math_mode=mode).discharge_report_major.cpu().numpy()
    got = a.stored['discharge'].cpu().numpy()
    assert got.shape == whole.shape == (40, 300)
    if mode == 'literal':
        assert bits_equal(got, whole)
    else:
        assert rel(got, whole) < 1e-12
    assert same_bits(a.parameters.cpu().numpy(), a.initial_population[:, :10])


def test_driver_in_fast_mode(tmp_path, eng):
    import csv
    from support import example_root
    root = example_root(tmp_path)
    a = _filter(root, days=40, assimilate_every=3)
    a.run(write=True, verify=True)
    K, R, N = 14, 40, 250
    assert a.forecast_bounds.shape == a.analysis_bounds.shape == (3, R) and a.analysis_mean.shape == (R,)
    assert a.ess.shape == a.resampled.shape == (K,) and a.diagnostics.shape == (K, 6) and a.verification.shape == (5, R)
    for table in (a.forecast_bounds, a.analysis_bounds, a.analysis_mean, a.ess, a.diagnostics):
        assert np.isfinite(table).all()
    assert np.isfinite(a.log_evidence) and (a.ess >= 1.0).all() and (a.ess <= N).all()
    assert (a.analysis_bounds[0] <= a.analysis_bounds[1]).all() and (a.analysis_bounds[1] <= a.analysis_bounds[2]).all()
    assert tuple(a.states.shape) == (N, 12) and tuple(a.parameters.shape) == (N, 10) and a._sample.shape == (N, 10)
    assert abs(float(a.weights.sum()) - 1.0) < 1e-12
    params = a.parameters.cpu().numpy()
    assert (params[:, a.columns] >= a.lo).all() and (params[:, a.columns] <= a.hi).all()
    # the states are a valid start of the next launch
    f = np.stack([np.asarray(a.model.nd_rain, dtype=np.float64)[:5], np.asarray(a.model.nd_peva, dtype=np.float64)[:5]], axis=1)
    ahead = eng.run_ensemble(a.parameters, f, float(a.model.area), 86400.0, 0, 1, initial=a.states)
    assert np.isfinite(ahead.discharge.cpu().numpy()).all()
    # the files, written and read again
    assert a.file.endswith('Catchment.SMART.pf') and a.diagnostics_written == a.diagnostics_file
    with open(a.file, newline='') as fh:
        lines = list(csv.reader(fh))
    assert lines[0] == ['DateTime', 'observed', 'forecast_q0.05', 'forecast_q0.5', 'forecast_q0.95', 'analysis_q0.05',
                        'analysis_q0.5', 'analysis_q0.95', 'analysis_mean'] and len(lines) == R + 1
    again = np.array([[float(v) for v in line[1:]] for line in lines[1:]])
    assert np.allclose(again[:, 1:4], a.forecast_bounds.T, rtol=1e-6) and np.allclose(again[:, 7], a.analysis_mean, rtol=1e-6)
    text = open(a.diagnostics_file).read().split('\n')
    assert text[0] == 'window,resampled,distinct_parents,flags,ess,log_evidence' and len(text) == K + 2
    assert [int(line.split(',')[1]) for line in text[1:-1]] == a.resampled.astype(int).tolist()
    # the same seed gives the same bits
    b = _filter(root, days=40, assimilate_every=3)
    b.run()
    assert same_bits(b.analysis_bounds, a.analysis_bounds) and same_bits(b.states.cpu().numpy(), a.states.cpu().numpy())
    # a sampling run gives the initial rows: at equal strides through it where fewer are asked for
    c = _filter(root, days=40, assimilate_every=3, sampling=a, particles=100)
    assert c.particles == 100 and same_bits(c.initial_population, a._sample[(np.arange(100) * N) // 100])


def test_sampling_with_a_subset_that_varies(tmp_path):
    """rows of a sampling run whose other columns differ from row to row: a column that does not vary has one value for
    every particle, before and after the resamplings, so that no child pairs its parent's states with another row's
    parameters"""
    from support import example_root
    root = example_root(tmp_path)
    source = _filter(root, days=40)                         # a hypercube over all ten parameters
    assert (source._sample.std(axis=0) > 0).all()
    a = _filter(root, days=40, sampling=source, vary=['T', 'C'], fixed={'Z': 80.0}, jitter=0.05)
    names = list(a.param_names)
    ranges = a.model.parameters.ranges
    want = np.array([80.0 if p == 'Z' else 0.5 * (ranges[p][0] + ranges[p][1]) for p in names])
    others = [j for j, p in enumerate(names) if p not in ('T', 'C')]
    assert a.columns == [0, 1] and same_bits(a.initial_population[:, [0, 1]], source._sample[:, [0, 1]])
    assert (a.initial_population[:, others] == want[others]).all()
    a.run(store=True)
    assert a.resampled.sum() >= 3
    params, parents = a.parameters.cpu().numpy(), a.stored['parents'].cpu().numpy()
    assert (parents[a.resampled] != np.arange(a.particles)).any()
    assert (params[:, others] == want[others]).all() and (a.state.rows_next.cpu().numpy()[:, others] == want[others]).all()
    assert (params[:, [0, 1]] >= a.lo).all() and (params[:, [0, 1]] <= a.hi).all() and params[:, 0].std() > 0
    # the soil layers lie below the capacity of the Z every particle runs with
    states = a.states.cpu().numpy()
    assert np.isfinite(states).all() and (states[:, 5:11] <= ((80.0 / 6.0) / 1e3) * float(a.model.area)).all()
    assert np.isfinite(a.analysis_bounds).all() and np.isfinite(a.stored['discharge'].cpu().numpy()).all()
