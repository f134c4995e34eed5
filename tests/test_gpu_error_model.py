"""The residual error model on the device: smart_error_model_loglik_hip against the 50-digit yardstick of
oracle/analyses/error_model.py within the bounds of the issue (every N and R at which the kernel takes another path, a
leading dimension with guarded padding, the error parameters at a row stride), an exactly representable case bit for bit,
invalid rows among valid ones, observations that are all missing; smart_error_model_draw_hip against the numpy statement
with a bound carried through the recurrence, and the same bits from a call in two halves; then through the API on the
example catchment: montecarlo.DEMCz(likelihood='ar1') and MonteCarlo.predictive_bounds.

The yardstick is computed once, cumulatively along the report steps of ONE record: a record cut after R' steps is a case
of its own for the kernel and a prefix for the yardstick.  The share of each bound that is used goes to
profiles/error_model_margins.txt (SMART_MARGINS_DIR)."""
import numpy as np
import pytest

from oracle.analyses.error_model import Draws, Truth, loglik_statement, shares
from oracle.exact import U
from support import EXTRA, Guarded, Margins, eng, example_root, margins_dir, padded, same_bits, settings_file, to_device  # noqa: F401

pytestmark = pytest.mark.gpu

L = 64                                                  # SMART_ERROR_MODEL_SEGMENT
SAMPLES = (1, 63, 65, 257)
REPORTS = (1, 2, 3, L - 1, L, L + 1, 8 * L + 1)
MARGINS = Margins()
PHIS = (0.0, 0.5, 0.99, -0.7)


@pytest.fixture(scope='module', autouse=True)
def publish_margins():
    yield
    lines = ['# tests/test_gpu_error_model.py: the largest share of each bound that a comparison used (1 = the bound)',
             '%-44s %12s  %s' % ('comparison', 'share', 'where')]
    lines += ['%-44s %12.4g  %s' % (key, MARGINS[key][0], MARGINS[key][1]) for key in sorted(MARGINS)]
    Margins.publish('\n'.join(lines), margins_dir(), 'error_model_margins.txt')


@pytest.fixture(scope='module')
def record():
    """ONE record of 8 L + 1 steps and 257 columns -- lognormal flows with a 1e3-fold flood, gaps at the start, around
    both ends of the first segments, single steps and at the end --, error parameters of every kind, and the yardstick of
    every cut in REPORTS"""
    R, N = max(REPORTS), max(SAMPLES)
    rng = np.random.default_rng(2024)
    sim = np.exp(rng.normal(0.0, 1.0, size=(R, N)))
    sim[200] *= 1e3
    obs = sim[:, 0] * np.exp(rng.normal(0.0, 0.3, size=R))
    obs[rng.random(R) < 0.1] = np.nan
    obs[L - 2] = obs[L + 1] = np.nan                   # the first boundary: steps L - 1 and L observed, a chain across it
    obs[2 * L - 1] = np.nan                             # the second: step 2 L is a start
    obs[3 * L] = np.nan                                 # the third: step 3 L - 1 ends a chain, 3 L + 1 starts one
    obs[[0, 2]] = [sim[0, 0] * 1.1, sim[2, 0] * 0.9]   # R = 1, 2, 3: observed, missing, observed
    obs[1] = np.nan
    obs[R - 1] = sim[R - 1, 0]
    theta = np.stack([np.exp(rng.uniform(-4.0, 0.0, N)), rng.uniform(0.0, 0.6, N), np.resize(PHIS, N)], axis=1)
    theta[5::7, 1] = 0.0
    return dict(sim=sim, obs=obs, theta=theta, truth=Truth(sim, obs, theta, cuts=REPORTS))


def loglik(sim, ld, obs, err, err_ld, N, R):
    """the C entry on device tensors, into a guarded output -> ([3, N] numpy, whether the guards are intact)"""
    import torch
    from smartpy_amd import _lib
    own = Guarded(3 * N)
    _lib.check(_lib.lib().smart_error_model_loglik_hip(N, R, sim.data_ptr(), ld, obs.data_ptr(), err.data_ptr(), err_ld,
                                                       own.ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    values, intact = own.read()
    return values.reshape(3, N).copy(), intact


@pytest.mark.parametrize('err_ld', (3, 13))
@pytest.mark.parametrize('N', SAMPLES)
def test_the_likelihood_against_the_yardstick(eng, record, N, err_ld):
    """every R of REPORTS at this N; ld = N + 5 with NaN in the padding; the error parameters as [N, 3], or as columns
    10 .. 12 of a [N, 13] matrix of NaN (the launch matrix of DE-MCz)"""
    theta = record['theta'][:N]
    wide = np.full((N, err_ld), np.nan)
    wide[:, err_ld - 3:] = theta
    err = to_device(wide)
    err_at = err[:, err_ld - 3:]
    for R in REPORTS:
        sim, ld = padded(record['sim'][:R, :N], 5)
        obs = to_device(record['obs'][:R])
        got, intact = loglik(sim, ld, obs, err_at, err_ld, N, R)
        assert intact and np.isfinite(got).all()
        rows = record['truth'].after(R)[:N]
        for i in range(N):
            used = shares(got[:, i], rows[i], record['truth'].mp)
            for name, share in zip(('LOGLIK', 'SSQ', 'LOGSIG'), used):
                MARGINS.note('likelihood %s' % name, share, 'N=%d R=%d err_ld=%d column %d' % (N, R, err_ld, i))
                assert share <= 1.0, (name, N, R, i, share)
        # the same call again: the same bits
        again, _ = loglik(sim, ld, obs, err_at, err_ld, N, R)
        assert same_bits(again, got)
        # ... and through the API, the error parameters read in place
        api = eng.residual_log_likelihood(sim[:, :N], obs, err_at).cpu().numpy()
        assert same_bits(api, got)


def test_an_exactly_representable_case_bit_for_bit(eng):
    """integer flows and observations, theta = (1, 0, 0.5): sigma = 1, every a_t an integer, every term a multiple of
    1 / 4 far below 2^53 -- SSQ is exact whatever the order of the sums, and LOGSIG is +0.0"""
    rng = np.random.default_rng(7)
    R, N = 8 * L + 1, 130
    sim = rng.integers(0, 50, size=(R, N)).astype(np.float64)
    obs = rng.integers(0, 50, size=R).astype(np.float64)
    obs[rng.random(R) < 0.2] = np.nan
    obs[[L - 1, L]] = [3.0, 5.0]
    theta = np.tile([1.0, 0.0, 0.5], (N, 1))
    a = obs[:, None] - sim
    seen = ~np.isnan(obs)
    cont = seen & np.concatenate([[False], seen[:-1]])
    start = seen & ~cont
    before = np.vstack([np.zeros((1, N)), a[:-1]])
    want = (0.75 * a[start] ** 2).sum(axis=0) + ((a[cont] - 0.5 * before[cont]) ** 2).sum(axis=0)
    assert (want * 4 == np.round(want * 4)).all() and want.max() < 2.0 ** 40
    got = eng.residual_log_likelihood(sim, obs, theta).cpu().numpy()
    assert same_bits(got[1], want)
    assert same_bits(got[2], np.zeros(N)) and not np.signbit(got[2]).any()
    n, S = int(seen.sum()), int(start.sum())
    ll = ((-0.5 * want - 0.0) + (0.5 * S) * np.log(0.75)) - (0.5 * n) * 1.8378770664093453
    assert np.abs(got[0] - ll).max() <= 4 * U * np.abs(ll).max()


def test_invalid_rows_among_valid_ones(eng):
    rng = np.random.default_rng(8)
    R, N = 150, 70
    sim = np.exp(rng.normal(0.0, 0.5, size=(R, N)))
    obs = sim[:, 0] * 1.1
    obs[[0, 40, 41, 64, 100]] = np.nan
    theta = np.tile([0.3, 0.2, 0.6], (N, 1))
    clean = eng.residual_log_likelihood(sim, obs, theta).cpu().numpy()
    assert np.isfinite(clean).all()
    theta[3, 2] = 1.0                                   # |phi| = 1
    theta[4, 2] = -1.5
    theta[5, 1] = np.nan
    theta[6, 0] = np.inf
    theta[12] = [-0.2, 0.2, 0.6]
    sim[:, 12] = 2.0
    sim[77, 12] = 1.0                                   # sigma_t = -0.2 + 0.2 = 0 at ONE observed step, 0.2 at the others
    sim[65, 20] = np.nan                                # NaN at an observed step (the second of its segment)
    sim[128, 21] = np.inf
    sim[64, 30] = np.nan                                # NaN at a step WITHOUT an observation: valid
    sim[0, 31] = -np.inf
    invalid = [3, 4, 5, 6, 12, 20, 21]
    sigma12 = theta[12, 0] + theta[12, 1] * sim[:, 12]
    assert not np.isnan(obs[77]) and sigma12[77] == 0.0 and (np.delete(sigma12, 77) > 0.0).all()
    got = eng.residual_log_likelihood(sim, obs, theta).cpu().numpy()
    assert (got[0, invalid] == -np.inf).all() and np.isnan(got[1:, invalid]).all()
    others = np.setdiff1d(np.arange(N), invalid)
    assert same_bits(got[:, others], clean[:, others])  # the neighbours, columns 30 and 31 among them, are untouched
    want = loglik_statement(sim, obs, theta)
    assert np.array_equal(np.isnan(got[1]), np.isnan(want[1])) and np.array_equal(got[0] == -np.inf, want[0] == -np.inf)


def test_observations_that_are_all_missing(eng):
    rng = np.random.default_rng(9)
    for R, N in ((1, 1), (L + 1, 65), (300, 7)):
        sim = rng.normal(size=(R, N))
        sim[0, 0] = np.nan
        got = eng.residual_log_likelihood(sim, np.full(R, np.nan), np.tile([0.1, 0.1, 0.9], (N, 1))).cpu().numpy()
        assert same_bits(got, np.zeros((3, N))), (R, N)


# ---- the draws ----------------------------------------------------------------------------------------------------------
def draw(N, R, K, sim, ld, err, err_ld, seed, offset, truncate, out_ptr, out_ld):
    import torch
    from smartpy_amd import _lib
    _lib.check(_lib.lib().smart_error_model_draw_hip(N, R, K, sim.data_ptr(), ld, err.data_ptr(), err_ld, seed, offset,
                                                     1 if truncate else 0, out_ptr, out_ld,
                                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def draw_bound(d):
    """The bound of the issue, carried through the recurrence of the statement `d` (oracle.analyses.error_model.Draws):
    |d eps_t| <= 16 u r_t; d a_t <= |phi| d a_{t-1} + |d eps_t| + 4 u (|phi a_{t-1}| + |eps_t|) -- step 0, a quotient by
    a square root, takes |d eps_0| / sqrt(q) + 4 u |a_0| --; d y <= sigma_t d a_t + 4 u (|x| + sigma_t |a_t|)"""
    R, C = d.a.shape
    d_eps = 16 * U * d.r
    d_a = np.empty((R, C))
    with np.errstate(all='ignore'):
        root = np.sqrt((1.0 - d.phi) * (1.0 + d.phi))
        d_a[0] = d_eps[0] / root + 4 * U * np.abs(d.a[0])
        for t in range(1, R):
            d_a[t] = np.abs(d.phi) * d_a[t - 1] + d_eps[t] + 4 * U * (np.abs(d.phi * d.a[t - 1]) + np.abs(d.eps[t]))
        return d.sigma * d_a + 4 * U * (np.abs(d.x) + d.sigma * np.abs(d.a))


@pytest.mark.parametrize('K', (1, 3))
@pytest.mark.parametrize('N', (1, 63, 65, 130))
def test_the_draws_against_the_statement(eng, N, K):
    """C = N K columns: 1, 63, 65 and 130 with one replicate, 3, 189, 195 and 390 with three; R = 1, 2, 7 and 401 each;
    guarded output with out_ld = C + 3; an invalid sample among the valid ones where there is room"""
    rng = np.random.default_rng(100 * N + K)
    C = N * K
    for R in (1, 2, 7, 401):
        sim_h = np.exp(rng.normal(0.0, 1.0, size=(R, N)))
        theta = np.stack([np.exp(rng.uniform(-3.0, 0.0, N)), rng.uniform(0.0, 0.5, N), np.resize(PHIS, N)], axis=1)
        if N > 2:
            theta[1, 2] = 1.0
            sim_h[R // 2, 2] = np.nan
        seed = (N << 33) + 17 * R + K
        sim, ld = padded(sim_h, 4)
        err = to_device(theta)
        out_ld = C + 3
        for truncate in (True, False):
            out = Guarded(R * out_ld)
            out.inner().view(R, out_ld)[:, :C] = 0.0        # (the columns of the call: everything else stays a sentinel)
            draw(N, R, K, sim, ld, err, 3, seed, 0, truncate, out.ptr(), out_ld)
            flat, intact = out.read()
            got = flat.reshape(R, out_ld)
            assert intact and (got[:, C:] == out.sentinel).all()
            got = got[:, :C]
            d = Draws(sim_h, theta, replicates=K, seed=seed, truncate=truncate)
            assert np.array_equal(np.isnan(got), np.isnan(d.y))
            if N > 2:
                assert np.isnan(got[:, K:3 * K]).all() and d.bad[K:3 * K].all()
            ok = ~d.bad
            err_abs, bound = np.abs(got[:, ok] - d.y[:, ok]), draw_bound(d)[:, ok]
            share = np.where(err_abs == 0.0, 0.0, err_abs / bound)
            where = np.unravel_index(np.argmax(share), share.shape) if share.size else (0, 0)
            MARGINS.note('draws', float(share.max()) if share.size else 0.0,
                         'N=%d K=%d R=%d truncate=%s step %d' % (N, K, R, truncate, where[0]))
            assert (share <= 1.0).all(), (N, K, R, float(share.max()))
            if truncate:
                assert (got[:, ok] >= 0.0).all()
        # through the API: the same bits as the entry, into a matrix of its own or of the caller's
        api = eng.predictive_draws(sim[:, :N], err, replicates=K, seed=seed, truncate=False)
        assert same_bits(api.cpu().numpy(), got)
        import torch
        mine = torch.full((R, C + 2), -7.0, dtype=torch.float64, device='cuda')
        back = eng.predictive_draws(sim[:, :N], theta, replicates=K, seed=seed, truncate=False, out=mine[:, :C])
        assert back.data_ptr() == mine.data_ptr() and same_bits(mine[:, :C].cpu().numpy(), got)
        assert (mine[:, C:] == -7.0).all()


@pytest.mark.parametrize('K', (1, 3))
def test_the_draws_in_two_halves(eng, K):
    import torch
    rng = np.random.default_rng(31 + K)
    R, N = 37, 130
    C = N * K
    sim, ld = padded(np.exp(rng.normal(0.0, 1.0, size=(R, N))), 2)
    theta = np.stack([np.full(N, 0.2), np.full(N, 0.3), np.resize(PHIS, N)], axis=1)
    err = to_device(theta)
    seed, first = 2 ** 63 + 5, 1000

    def whole():
        out = torch.empty((R, C), dtype=torch.float64, device='cuda')
        draw(N, R, K, sim, ld, err, 3, seed, first, True, out.data_ptr(), C)
        return out.cpu().numpy()
    a, b = whole(), whole()
    assert same_bits(a, b) and np.isfinite(a).all()
    half = 61                                           # samples of the first call: not a multiple of anything
    out = torch.empty((R, C), dtype=torch.float64, device='cuda')
    draw(half, R, K, sim, ld, err, 3, seed, first, True, out.data_ptr(), C)
    draw(N - half, R, K, sim[:, half:], ld, err[half:], 3, seed, first + half * K, True, out[:, half * K:].data_ptr(), C)
    assert same_bits(out.cpu().numpy(), a)
    other = torch.empty((R, C), dtype=torch.float64, device='cuda')
    draw(N, R, K, sim, ld, err, 3, seed + 1, first, True, other.data_ptr(), C)
    assert not same_bits(other.cpu().numpy(), a)


# ---- through the API on the example catchment ---------------------------------------------------------------------------
def _sampler(root, **kw):
    from smartpy_amd.montecarlo import DEMCz
    args = dict(chains=64, generations=20, thin=5, seed=0, settings_filename='Catchment.ar1.sttngs')
    args.update(kw)
    obj = DEMCz('Catchment', root, 'csv', 'csv', **args)
    obj.model.extra = EXTRA
    return obj


@pytest.fixture(scope='module')
def ar1_runs(tmp_path_factory):
    """DEMCz(chains=64, generations=20, thin=5, likelihood='ar1', seed=0) on one year of the example catchment, twice"""
    root = example_root(tmp_path_factory.mktemp('ar1'))
    settings_file(root, 'Catchment.ar1.sttngs', '01/01/2007', '31/12/2007', 90, simu_minutes=1440)
    runs = []
    for _ in range(2):
        obj = _sampler(root, likelihood='ar1')
        obj.run(write=True)
        runs.append((obj, open(obj.db_file, 'rb').read(), open(obj.diagnostics_file).read()))
    return root, runs


def statement_bound(sim, obs, theta):
    """the bound of the issue on LOGLIK, in numpy, per column"""
    s0, s1, phi = theta[:, 0], theta[:, 1], theta[:, 2]
    seen = ~np.isnan(obs)
    cont = seen & np.concatenate([[False], seen[:-1]])
    sigma = s0 + s1 * sim
    a = (obs[:, None] - sim) / sigma
    before = np.vstack([np.zeros((1, sim.shape[1])), a[:-1]])
    B = ((np.abs(a[cont]) + np.abs(phi * before[cont])) ** 2).sum(axis=0) + (a[seen & ~cont] ** 2).sum(axis=0)
    lnsig = np.abs(np.log(sigma[seen])).sum(axis=0)
    n, S = int(seen.sum()), int((seen & ~cont).sum())
    return U * ((n + 16) * (0.5 * B + lnsig + 0.5 * S * np.abs(np.log((1.0 - phi) * (1.0 + phi)))) + 4 * n)


def test_demcz_with_the_ar1_likelihood(eng, ar1_runs):
    root, ((a, db_a, diag_a), (b, db_b, diag_b)) = ar1_runs
    # ---- one seed, the same bytes
    assert db_a == db_b and diag_a == diag_b
    assert same_bits(a._sample, b._sample) and same_bits(a.log_density.cpu().numpy(), b.log_density.cpu().numpy())
    assert same_bits(a.posterior.error_parameters.cpu().numpy(), b.posterior.error_parameters.cpu().numpy())
    # ---- shapes: five snapshots of 64 chains, the first two dropped; thirteen dimensions
    S, N, first = 5, 64, 2
    n = (S - first) * N
    theta = a.posterior.error_parameters.cpu().numpy()
    assert a._sample.shape == (n, 10) and theta.shape == (n, 3) and a.obj_fns.shape == (n, 8)
    assert a.posterior.names == a.param_names + ['sigma0', 'sigma1', 'phi'] and a.rhat.shape == (13,)
    assert a.diagnostics.shape == (S, 15) and tuple(a.posterior.history.shape) == (S, N, 13)
    assert diag_a.split('\n')[0].endswith('Rhat_RK,Rhat_sigma0,Rhat_sigma1,Rhat_phi')
    assert len(db_a.split(b'\n')) == n + 2 and len(db_a.split(b'\n')[0].split(b',')) == 8 + 10
    assert 0.0 < a.acceptance_rate < 1.0
    # ---- the error parameters lie in their ranges, the model parameters in theirs
    for k in range(3):
        assert (theta[:, k] >= a.lo[10 + k]).all() and (theta[:, k] <= a.hi[10 + k]).all(), k
    for j, p in enumerate(a.param_names):
        lo, hi = a.model.parameters.ranges[p]
        assert (a._sample[:, j] >= lo).all() and (a._sample[:, j] <= hi).all(), p
    assert same_bits(a.posterior.sample.cpu().numpy()[:, 10:], theta)
    # ---- the archived log-density of every row is the statement on a fresh stored launch of that row with its theta
    out, obs = a._launch_stored()
    sim = out.discharge_report_major.cpu().numpy()
    obs = obs.cpu().numpy()
    want = loglik_statement(sim, obs, theta)[0]
    got = a.log_density.cpu().numpy()
    bound = statement_bound(sim, obs, theta)
    share = np.abs(got - want) / bound
    print('archived log-density against the statement: largest share of the bound %.3g' % share.max())
    MARGINS.note('DEMCz archived log-density', float(share.max()), 'row %d of %d' % (int(np.argmax(share)), n))
    assert np.isfinite(got).all() and (share <= 1.0).all()
    # ---- the chains move uphill from the Latin hypercube
    history = a.posterior.history_log_density
    assert float(history[-1].median()) > float(history[0].median())
    # ---- residual_likelihood defaults to the archived parameters and writes its side file
    res = a.residual_likelihood(write=True)
    assert same_bits(res.error_parameters, theta) and res.file.endswith('Catchment.SMART.demcz.errormodel')
    assert (np.abs(res.log_likelihood - want) <= bound).all()
    assert len(open(res.file).read().split('\n')) == n + 2


def test_the_gaussian_likelihood_is_as_it_was(eng, ar1_runs):
    """DEMCz with default arguments against DEMCz with likelihood='gaussian' spelt out, the same seed: the same bytes"""
    root, _ = ar1_runs
    runs = []
    for kw in (dict(), dict(likelihood='gaussian')):
        obj = _sampler(root, **kw)
        obj.run(write=True)
        runs.append((obj, open(obj.db_file, 'rb').read(), open(obj.diagnostics_file).read()))
    (a, db_a, diag_a), (b, db_b, diag_b) = runs
    assert db_a == db_b and diag_a == diag_b and a.posterior.error_parameters is None
    assert same_bits(a._sample, b._sample) and same_bits(a.log_density.cpu().numpy(), b.log_density.cpu().numpy())
    assert same_bits(a.obj_fns, b.obj_fns) and same_bits(a.rhat, b.rhat) and a.rhat.shape == (10,)
    assert a.posterior.names == a.param_names and same_bits(a.initial_population, b.initial_population)


def test_predictive_bounds(eng, ar1_runs):
    root, ((a, _, _), _) = ar1_runs
    theta = a.posterior.error_parameters.cpu().numpy()
    n = a._sample.shape[0]
    pb = a.predictive_bounds(replicates=2, verify=True, write=True)
    assert pb.bounds.shape == pb.parametric.shape == (3, len(pb.datetime)) and pb.replicates == 2
    # ---- the bounds are weighted_quantiles of the draws matrix, bit for bit
    out, obs = a._launch_stored()
    sim = out.discharge_report_major
    draws = eng.predictive_draws(sim, theta, replicates=2, seed=0, truncate=True)
    assert tuple(draws.shape) == (sim.shape[0], 2 * n)
    assert same_bits(pb.bounds, eng.weighted_quantiles(draws, [0.05, 0.5, 0.95]).cpu().numpy())
    assert same_bits(pb.parametric, eng.weighted_quantiles(sim, [0.05, 0.5, 0.95]).cpu().numpy())
    scores = eng.ensemble_scores(draws, obs).cpu().numpy()
    assert same_bits(pb.verification.crps, scores[0]) and 0.0 <= pb.verification.reliability <= 1.0
    # ---- the total band contains the parametric band wherever truncation is not active, and at least as many observations
    # (truncation is active on a step's band where it sets the lower bound: a bound above 0 is a draw it did not touch,
    # and the quantile of the draws as they were; the upper bound is above 0 at every step)
    free = eng.predictive_draws(sim, theta, replicates=2, seed=0, truncate=False)
    lower = eng.weighted_quantiles(free, [0.05]).cpu().numpy()[0]
    active = ~(pb.bounds[0] > 0.0)
    assert np.array_equal(active, ~(lower > 0.0)) and same_bits(pb.bounds[0, ~active], lower[~active])
    print('total containment %.3f, parametric %.3f; truncation sets the lower bound at %d of %d steps'
          % (pb.containment, pb.parametric_containment, int(active.sum()), len(active)))
    assert (pb.bounds[2] > 0.0).all()
    assert (pb.bounds[0, ~active] <= pb.parametric[0, ~active]).all()
    assert (pb.bounds[2] >= pb.parametric[2]).all()
    # ... and without truncation it is active nowhere: both ends, every step
    whole = a.predictive_bounds(replicates=2, truncate=False)
    assert same_bits(whole.bounds[0], lower) and same_bits(whole.parametric, pb.parametric)
    assert (whole.bounds[0] <= pb.parametric[0]).all() and (whole.bounds[2] >= pb.parametric[2]).all()
    assert whole.containment >= whole.parametric_containment == pb.parametric_containment
    assert pb.containment >= pb.parametric_containment
    lines = open(pb.file).read().split('\n')
    assert pb.file.endswith('Catchment.SMART.demcz.predictive') and len(lines) == len(pb.datetime) + 2
    assert lines[0] == 'DateTime,q0.05,q0.5,q0.95,param_q0.05,param_q0.5,param_q0.95'
    # ---- weights repeat over the replicates; one triple serves every row
    w = np.linspace(0.0, 1.0, n)
    weighted = a.predictive_bounds([0.05, 0.1, 0.5], replicates=2, likelihood=w)
    one = eng.predictive_draws(sim, [0.05, 0.1, 0.5], replicates=2, seed=0)
    assert same_bits(weighted.bounds, eng.weighted_quantiles(one, [0.05, 0.5, 0.95], np.repeat(w, 2)).cpu().numpy())
