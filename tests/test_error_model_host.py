"""The residual error model, host side: the numpy statement of include/smart_amd.h (smart_error_model_loglik_hip,
smart_error_model_draw_hip) that tests/test_gpu_error_model.py holds the kernels to -- the likelihood against 50-digit
arithmetic (mpmath) on flows with a 1e6-fold flood, gaps of every kind, four phi and standardised residuals up to 1e6; the
draws by hand on three steps, statistically over six seeds, truncated, and NaN for invalid rows --; every refusal of the two
C entries, as literals; the bindings; montecarlo.DEMCz(likelihood='ar1') as far as it goes without a device; the side
files.  Nothing here needs a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from oracle.analyses.error_model import LN_TWO_PI, TWO_PI, Draws, Truth, flood_record, loglik_statement, shares
from oracle.exact import U
from oracle.philox import philox4x32
from smartpy_amd import _lib, errormodel
from support import E_NO_DEVICE, E_NULL, E_SIZE, FAKE, example_root, refusal, settings_file


PHIS = (0.0, 0.5, 0.99, -0.7)


def test_the_likelihood_statement_against_fifty_digits():
    R, N = 120, 8
    rng, sim, obs = flood_record(11, R, N)
    theta = np.stack([np.exp(rng.uniform(-3.0, 0.0, N)), rng.uniform(0.0, 0.5, N), np.resize(PHIS, N)], axis=1)
    theta[4:, 0] = 1e-6                     # sigma0 so small, with sigma1 = 0, that |a_t| reaches 1e6 and beyond
    theta[4:, 1] = 0.0
    got = loglik_statement(sim, obs, theta)
    truth = Truth(sim, obs, theta)
    worst = [0.0, 0.0, 0.0]
    for i, row in enumerate(truth.after(R)):
        assert row[3] == int((~np.isnan(obs)).sum()) and row[4] == 5      # n, and the starts: steps 3, 9, 12, 14, 61
        used = shares([g[i] for g in got], row, truth.mp)
        worst = [max(w, u) for w, u in zip(worst, used)]
    largest = np.abs((obs[:, None] - sim) / (theta[:, 0] + theta[:, 1] * sim))[~np.isnan(obs)].max()
    print('shares of the bounds used (LOGLIK, SSQ, LOGSIG): %s; largest |a_t| %.3g' % (worst, largest))
    assert largest >= 1e6 and max(worst) <= 1.0
    # what a cut of the record has is what the statement gives on the cut record
    cuts = Truth(sim[:, :2], obs, theta[:2], cuts=(1, 4, 10, R))
    for cut in (1, 4, 10, R):
        part = loglik_statement(sim[:cut, :2], obs[:cut], theta[:2])
        for i, row in enumerate(cuts.after(cut)):
            assert max(shares([g[i] for g in part], row, cuts.mp)) <= 1.0
    assert [row[3] for row in cuts.after(4)] == [1, 1] and [row[3] for row in cuts.after(1)] == [0, 0]


def test_the_likelihood_statement_on_its_edges():
    sim = np.array([[2.0, 2.0, 2.0, np.nan, 2.0], [4.0, 4.0, 0.0, 4.0, np.nan], [1.0, 1.0, 1.0, 1.0, 1.0]])
    obs = np.array([3.0, np.nan, 2.0])
    theta = np.array([[1.0, 0.0, 0.5], [1.0, 0.0, 1.0], [0.0, 1.0, 0.5], [1.0, 0.0, 0.5], [1.0, 0.0, 0.5]])
    ll, ssq, logsig = loglik_statement(sim, obs, theta)
    # column 0: two starts, a = 1 and 1, q = 0.75; the NaN of column 4 and the zero sigma of column 2 lie at the step
    # without an observation; |phi| = 1 and a NaN at an observed step are invalid
    assert ssq.tolist()[0] == 1.5 and logsig.tolist()[0] == 0.0
    assert ll[0] == ((-0.75 - 0.0) + math.log(0.75)) - LN_TWO_PI
    assert ll[1] == -np.inf and np.isnan(ssq[1]) and np.isnan(logsig[1])
    assert np.isfinite(ll[2]) and ssq[2] == 0.75 * (0.25 + 1.0)
    assert ll[3] == -np.inf and ll[4] == ll[0]
    none = loglik_statement(sim, np.full(3, np.nan), theta)
    for values in none:     # no observed step: +0.0 (the invalid phi stays invalid)
        assert np.array_equal(np.signbit(values[[0, 2, 3, 4]]), [False] * 4) and (values[[0, 2, 3, 4]] == 0.0).all()
    assert none[0][1] == -np.inf


def test_the_draws_by_hand():
    sim = np.array([[2.0], [4.0], [1.0]])
    theta = np.array([[0.5, 0.25, 0.5]])
    seed, offset = (7 << 32) | 9, 5
    d = Draws(sim, theta, replicates=1, seed=seed, truncate=False, column_offset=offset)
    eps = []
    for j in (0, 1):
        w = [int(v) for v in philox4x32((offset, j, 0, 0), (9, 7))]
        u1 = 1.0 - ((w[0] >> 5) * 2 ** 26 + (w[1] >> 6)) * 2.0 ** -53
        u2 = ((w[2] >> 5) * 2 ** 26 + (w[3] >> 6)) * 2.0 ** -53
        r = math.sqrt(-2.0 * math.log(u1))
        assert 0.0 < u1 <= 1.0 and 0.0 <= u2 < 1.0
        eps += [r * math.cos(TWO_PI * u2), r * math.sin(TWO_PI * u2)]
    a0 = eps[0] / math.sqrt(0.5 * 1.5)
    a1 = 0.5 * a0 + eps[1]
    a2 = 0.5 * a1 + eps[2]
    want = [2.0 + (0.5 + 0.25 * 2.0) * a0, 4.0 + (0.5 + 0.25 * 4.0) * a1, 1.0 + (0.5 + 0.25 * 1.0) * a2]
    assert np.allclose(d.y[:, 0], want, rtol=4 * U, atol=0.0) and not d.bad[0]
    assert np.allclose(d.eps[:, 0], eps[:3], rtol=4 * U, atol=0.0)
    # column c of a call with an offset is column c + offset of the call without; replicate k of sample i is column i K + k
    wide = Draws(np.repeat(sim, 2, axis=1), np.repeat(theta, 2, axis=0), replicates=3, seed=seed, truncate=False)
    assert np.array_equal(wide.y[:, 5], d.y[:, 0]) and wide.y.shape == (3, 6)
    assert not np.array_equal(wide.y[:, 4], wide.y[:, 5])


@pytest.mark.parametrize('phi', (0.0, 0.9))
@pytest.mark.parametrize('seed', range(6))
def test_the_draws_have_the_moments_of_the_model(seed, phi):
    """64 columns of 4,000 steps on sim = 0 with sigma = 1: y = a_t.  Each statistic within four standard errors, the
    standard errors those of a stationary Gaussian AR(1) of n values with v = 1 / (1 - phi^2) (Bartlett): the mean
    sqrt(v (1 + phi) / ((1 - phi) n)), the variance v sqrt(2 (1 + phi^2) / ((1 - phi^2) n)), the lag-1 correlation
    sqrt((1 - phi^2) / n), the correlation of the two halves of a Box-Muller pair 1 / sqrt(pairs).  Conditions, not
    measurements."""
    R, C = 4000, 64
    d = Draws(np.zeros((R, C)), np.tile([1.0, 0.0, phi], (C, 1)), seed=seed, truncate=False)
    y, n = d.y, float(R * C)
    v = 1.0 / (1.0 - phi * phi)
    mean, var = y.mean(), y.var()
    lag1 = ((y[1:] - mean) * (y[:-1] - mean)).mean() / var
    pair = (d.eps[0::2] * d.eps[1::2]).mean()
    z = [mean / math.sqrt(v * (1.0 + phi) / ((1.0 - phi) * n)),
         (var - v) / (v * math.sqrt(2.0 * (1.0 + phi * phi) / ((1.0 - phi * phi) * n))),
         (lag1 - phi) / math.sqrt((1.0 - phi * phi) / n), pair * math.sqrt(n / 2.0)]
    print('seed %d phi %g: z of mean, variance, lag-1 correlation, pair correlation %s' % (seed, phi, z))
    assert np.isfinite(y).all() and (np.abs(z) <= 4.0).all()


def test_truncation_and_invalid_rows_of_the_draws():
    rng = np.random.default_rng(5)
    sim = np.exp(rng.normal(-1.0, 1.0, size=(40, 6)))
    theta = np.tile([0.5, 0.5, 0.8], (6, 1))
    theta[1, 2] = 1.0                       # |phi| = 1
    theta[2, 0] = np.inf
    sim[17, 3] = np.nan                     # judged over every step: there are no observations here
    theta[4] = [-0.01, 0.0, 0.3]            # sigma_t <= 0
    free = Draws(sim, theta, replicates=2, seed=3, truncate=False)
    cut = Draws(sim, theta, replicates=2, seed=3, truncate=True)
    assert free.bad.tolist() == [False, False, True, True, True, True, True, True, True, True, False, False]
    assert np.isnan(free.y[:, 2:10]).all() and np.isnan(cut.y[:, 2:10]).all()
    ok = [0, 1, 10, 11]
    assert (free.y[:, ok] < 0.0).any() and (cut.y[:, ok] >= 0.0).all() and not np.signbit(cut.y[:, ok]).any()
    assert np.array_equal(cut.y[:, ok], np.where(free.y[:, ok] > 0.0, free.y[:, ok], 0.0))


# ---- the refusals of the two C entries ------------------------------------------------------------------------------------
TWO31, TWO32 = 2 ** 31, 2 ** 32
LL, DR = 'smart_error_model_loglik_hip', 'smart_error_model_draw_hip'
VALID = {
    LL: dict(n_samples=8, n_reports=5, sim=FAKE, ld=8, obs=FAKE, err=FAKE, err_ld=3, loglik=FAKE, stream=None),
    DR: dict(n_samples=8, n_reports=5, n_replicates=3, sim=FAKE, ld=8, err=FAKE, err_ld=3, seed=1, column_offset=0,
             truncate=1, out=FAKE, out_ld=24, stream=None),
}
LL_REQUIRED = LL + ': sim, obs, err and loglik are required (%s is NULL)'
DR_REQUIRED = DR + ': sim, err and out are required (%s is NULL)'
ONE_LAUNCH = ' is more than one launch takes (2^31 - 1)'
CASES = [
    (LL, dict(sim=None), E_NULL, LL_REQUIRED % 'sim'),
    (LL, dict(obs=None), E_NULL, LL_REQUIRED % 'obs'),
    (LL, dict(err=None), E_NULL, LL_REQUIRED % 'err'),
    (LL, dict(loglik=None), E_NULL, LL_REQUIRED % 'loglik'),
    (LL, dict(loglik=None, obs=None), E_NULL, LL_REQUIRED % 'obs'),                  # the first in the list is named
    (LL, dict(err=None, n_samples=0), E_NULL, LL_REQUIRED % 'err'),                  # pointers before sizes
    (LL, dict(n_samples=0), E_SIZE, LL + ': need n_samples, n_reports >= 1 (got 0, 5)'),
    (LL, dict(n_reports=-1), E_SIZE, LL + ': need n_samples, n_reports >= 1 (got 8, -1)'),
    (LL, dict(n_reports=0, ld=2), E_SIZE, LL + ': need n_samples, n_reports >= 1 (got 8, 0)'),
    (LL, dict(ld=7), E_SIZE, LL + ': ld 7 is less than n_samples 8'),
    (LL, dict(ld=7, err_ld=2), E_SIZE, LL + ': ld 7 is less than n_samples 8'),
    (LL, dict(err_ld=2), E_SIZE, LL + ': err_ld 2 is less than the 3 parameters of a row'),
    (LL, dict(err_ld=-3), E_SIZE, LL + ': err_ld -3 is less than the 3 parameters of a row'),
    (LL, dict(n_samples=TWO31, ld=TWO31), E_SIZE, LL + ': n_samples 2147483648' + ONE_LAUNCH),
    (LL, dict(n_reports=TWO31), E_SIZE, LL + ': n_reports 2147483648' + ONE_LAUNCH),
    (LL, dict(n_reports=TWO31, err_ld=0), E_SIZE, LL + ': err_ld 0 is less than the 3 parameters of a row'),
    (DR, dict(sim=None), E_NULL, DR_REQUIRED % 'sim'),
    (DR, dict(err=None), E_NULL, DR_REQUIRED % 'err'),
    (DR, dict(out=None), E_NULL, DR_REQUIRED % 'out'),
    (DR, dict(out=None, sim=None), E_NULL, DR_REQUIRED % 'sim'),
    (DR, dict(out=None, n_replicates=0), E_NULL, DR_REQUIRED % 'out'),
    (DR, dict(n_samples=0), E_SIZE, DR + ': need n_samples, n_reports, n_replicates >= 1 (got 0, 5, 3)'),
    (DR, dict(n_reports=0), E_SIZE, DR + ': need n_samples, n_reports, n_replicates >= 1 (got 8, 0, 3)'),
    (DR, dict(n_replicates=0), E_SIZE, DR + ': need n_samples, n_reports, n_replicates >= 1 (got 8, 5, 0)'),
    (DR, dict(n_replicates=-2, ld=1), E_SIZE, DR + ': need n_samples, n_reports, n_replicates >= 1 (got 8, 5, -2)'),
    (DR, dict(ld=7), E_SIZE, DR + ': ld 7 is less than n_samples 8'),
    (DR, dict(ld=7, out_ld=1), E_SIZE, DR + ': ld 7 is less than n_samples 8'),
    (DR, dict(err_ld=2), E_SIZE, DR + ': err_ld 2 is less than the 3 parameters of a row'),
    (DR, dict(err_ld=2, out_ld=1), E_SIZE, DR + ': err_ld 2 is less than the 3 parameters of a row'),
    (DR, dict(out_ld=23), E_SIZE, DR + ': out_ld 23 is less than the n_samples * n_replicates = 24 columns'),
    (DR, dict(out_ld=23, column_offset=-1), E_SIZE,
     DR + ': out_ld 23 is less than the n_samples * n_replicates = 24 columns'),
    (DR, dict(column_offset=-1), E_SIZE, DR + ': column_offset -1 must be in 0 .. 4294967295'),
    (DR, dict(column_offset=TWO32), E_SIZE, DR + ': column_offset 4294967296 must be in 0 .. 4294967295'),
    (DR, dict(column_offset=TWO32 - 23), E_SIZE,
     DR + ": columns 4294967273 ..: a column's number stays below 2^32 (8 samples, 3 replicates)"),
    (DR, dict(n_samples=TWO31, ld=TWO31, out_ld=2 ** 40), E_SIZE,
     DR + ": columns 0 ..: a column's number stays below 2^32 (2147483648 samples, 3 replicates)"),
    (DR, dict(n_reports=TWO31), E_SIZE, DR + ': n_reports 2147483648' + ONE_LAUNCH),
    (DR, dict(n_reports=TWO31, column_offset=TWO32), E_SIZE, DR + ': column_offset 4294967296 must be in 0 .. 4294967295'),
]


@pytest.mark.parametrize('entry,changes,code,text', CASES,
                         ids=['%02d-%s-%s' % (i, c[0].split('_')[3], '-'.join('%s=%s' % kv for kv in c[1].items()))
                              for i, c in enumerate(CASES)])
def test_refusals(entry, changes, code, text):
    assert refusal(VALID, entry, changes) == (code, text)


def test_a_well_formed_call_gets_as_far_as_the_device():
    L = _lib.lib()
    if L.smart_device_count() == 0:
        # ... and no further: there is no CPU fallback
        for entry, changes in ((LL, dict()), (LL, dict(ld=100, err_ld=13)), (LL, dict(n_samples=1, n_reports=1)),
                               (DR, dict()), (DR, dict(n_replicates=1, out_ld=8)), (DR, dict(truncate=0, seed=2 ** 64 - 1)),
                               (DR, dict(column_offset=TWO32 - 24)), (DR, dict(err_ld=13, out_ld=100))):
            rc, text = refusal(VALID, entry, changes)
            assert rc == E_NO_DEVICE and 'device' in text, (entry, changes)
    else:
        assert refusal(VALID, LL, dict(sim=None))[0] == E_NULL and refusal(VALID, DR, dict(out=None))[0] == E_NULL


def test_the_two_names_are_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'smart_amd.h')).read()
    for entry in (LL, DR):
        assert entry in _lib.SYMBOLS and getattr(_lib.lib(), entry) is not None
        assert _lib.SYMBOLS[entry][0] is ctypes.c_int and len(_lib.SYMBOLS[entry][1]) == len(VALID[entry])
        declared = re.search(r'^int %s\(([^;]*)\);' % entry, header, re.M)
        names = re.findall(r'(\w+)\s*(?:,|$)', declared.group(1).replace('\n', ' '))
        assert names == list(VALID[entry])           # the dictionary above is the entry's argument list, in its order
    for macro, value in (('SMART_ERROR_MODEL_SEGMENT', 64), ('SMART_ERROR_MODEL_LOGLIK', 0), ('SMART_ERROR_MODEL_SSQ', 1),
                         ('SMART_ERROR_MODEL_LOGSIG', 2)):
        assert re.search(r'^#define %s %d$' % (macro, value), header, re.M), macro
    assert _lib.ERROR_MODEL_SEGMENT == 64 and _lib.ERROR_MODEL_ROWS == ['LOGLIK', 'SSQ', 'LOGSIG']
    assert _lib.lib().smart_abi_version() == 7 and _lib.ABI_VERSION == 7
    from smartpy_amd import build, engine, analysis
    assert build.UNITS['smart_error_model.hip'] == ['-ffp-contract=off']
    assert engine.residual_log_likelihood is analysis.residual_log_likelihood
    assert engine.predictive_draws is analysis.predictive_draws
    assert errormodel.PARAMETER_NAMES == ['sigma0', 'sigma1', 'phi'] and errormodel.LIKELIHOOD_NAMES == _lib.ERROR_MODEL_ROWS


# ---- the error_model argument, DEMCz(likelihood='ar1') and the side files -------------------------------------------------
def test_the_error_model_argument():
    obs = np.array([1.0, np.nan, 3.0, 8.0])
    assert errormodel.default_ranges(obs) == {'sigma0': (1e-4 * 4.0, 4.0), 'sigma1': (0.0, 1.0), 'phi': (0.0, 0.99)}
    assert errormodel.resolve(None, obs) == (['sigma0', 'sigma1', 'phi'], errormodel.default_ranges(obs), {})
    sampled, ranges, fixed = errormodel.resolve({'sigma1': 0.1, 'phi': (-0.5, 0.9)}, obs)
    assert sampled == ['sigma0', 'phi'] and fixed == {'sigma1': 0.1}
    assert ranges == {'sigma0': (1e-4 * 4.0, 4.0), 'phi': (-0.5, 0.9)}
    assert errormodel.resolve({'sigma0': 1, 'sigma1': 0, 'phi': 0.5}, None) == ([], {}, {'sigma0': 1.0, 'sigma1': 0.0, 'phi': 0.5})
    for bad, text in (({'sigma': 1.0}, r"error parameter\(s\) \['sigma'\] are not among"),
                      ({'phi': (0.0, 1.0)}, r'phi must stay inside \(-1, 1\)'), ({'phi': -1.0}, r'phi must stay inside'),
                      ({'sigma0': (2.0, 1.0)}, r'needs finite lo <= hi'), ({'sigma1': (-0.1, 1.0)}, 'sigma1 must not be negative'),
                      ({'sigma0': float('nan')}, 'must be finite'), ({'sigma0': (1.0, 2.0, 3.0)}, r'takes a \(lo, hi\) range')):
        with pytest.raises(_lib.SmartEngineError, match=text) as err:
            errormodel.resolve(bad, obs)
        assert err.value.code == -2
    with pytest.raises(_lib.SmartEngineError, match='no observed flow'):
        errormodel.default_ranges([np.nan])
    table = errormodel.parameter_table([0.5, 0.1, 0.8], 3)
    assert table.shape == (3, 3) and (table == [0.5, 0.1, 0.8]).all()
    assert errormodel.parameter_table(np.arange(6.0).reshape(2, 3), 2).tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]
    with pytest.raises(_lib.SmartEngineError, match=r'must be \[4, 3\]'):
        errormodel.parameter_table(np.zeros((3, 3)), 4)


def _sampler(root, **kw):
    from smartpy_amd.montecarlo import DEMCz
    args = dict(chains=16, generations=4, thin=2, seed=0, settings_filename='Catchment.ar1.sttngs')
    args.update(kw)
    return DEMCz('Catchment', root, 'csv', 'csv', **args)


def test_demcz_with_the_ar1_likelihood_constructs(tmp_path):
    import inspect
    from smartpy_amd.montecarlo import DEMCz
    from smartpy_amd.montecarlo.montecarlo import MonteCarlo
    from smartpy_amd.sampling import latin_hypercube
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.ar1.sttngs', '01/01/2007', '31/12/2007', 90, simu_minutes=1440)
    plain = _sampler(root)
    explicit = _sampler(root, likelihood='gaussian')
    assert plain.likelihood == 'gaussian' and plain.score_kind == 'rmse' and plain.error_sampled == []
    assert plain.initial_population.shape == (16, 10) and plain.columns == list(range(10))
    assert np.array_equal(plain.initial_population, explicit.initial_population)
    assert np.array_equal(plain.initial_population, latin_hypercube(16, plain.model.parameters.ranges, seed=0))
    ar1 = _sampler(root, likelihood='ar1')
    m = float(np.nanmean(np.asarray(ar1.model.nd_flow, dtype=np.float64)))
    assert ar1.score_kind == 'logp' and ar1.error_sampled == ['sigma0', 'sigma1', 'phi'] and ar1.error_fixed == {}
    assert ar1.dimension_names == ar1.param_names + ['sigma0', 'sigma1', 'phi'] and ar1.columns == list(range(13))
    assert ar1.initial_population.shape == (16, 13) and ar1._sample.shape == (16, 10)
    assert ar1.lo[10:].tolist() == [1e-4 * m, 0.0, 0.0] and ar1.hi[10:].tolist() == [m, 1.0, 0.99]
    # one Latin hypercube call over the widened ranges: every column stratified, the model columns those of the sample
    assert np.array_equal(ar1.initial_population[:, :10], ar1._sample)
    for j in range(13):
        strata = np.floor((ar1.initial_population[:, j] - ar1.lo[j]) / (ar1.hi[j] - ar1.lo[j]) * 16).astype(int)
        assert sorted(strata.tolist()) == list(range(16)), j
    mixed = _sampler(root, likelihood='ar1', error_model={'sigma1': 0.0, 'phi': (0.2, 0.9)}, vary=['T', 'SK'])
    assert mixed.dimension_names == ['T', 'SK', 'sigma0', 'phi'] and mixed.columns == [0, 6, 10, 12]
    assert (mixed.initial_population[:, 11] == 0.0).all() and mixed.error_fixed == {'sigma1': 0.0}
    assert (mixed.initial_population[:, 12] >= 0.2).all() and (mixed.initial_population[:, 12] <= 0.9).all()
    for kw, text in ((dict(likelihood='ar1', sigma=0.5), r"sigma= and n_eff= belong to likelihood='gaussian'"),
                     (dict(likelihood='ar1', n_eff=100.0), r"sigma= and n_eff= belong to likelihood='gaussian'"),
                     (dict(error_model={'phi': 0.5}), r"error_model= belongs to likelihood='ar1'"),
                     (dict(likelihood='ar1', error_model={'phi': 1.0}), 'phi must stay inside')):
        with pytest.raises(_lib.SmartEngineError, match=text) as err:
            _sampler(root, **kw)
        assert err.value.code == -2
    with pytest.raises(_lib.SmartEngineError, match=r"likelihood 'student' unknown") as err:
        _sampler(root, likelihood='student')
    assert err.value.code == -7
    assert list(inspect.signature(MonteCarlo.predictive_bounds).parameters) == [
        'self', 'error_parameters', 'quantiles', 'replicates', 'likelihood', 'seed', 'truncate', 'verify', 'write']
    assert list(inspect.signature(MonteCarlo.residual_likelihood).parameters) == ['self', 'error_parameters', 'write']
    assert DEMCz.predictive_bounds is MonteCarlo.predictive_bounds
    with pytest.raises(_lib.SmartEngineError, match='error_parameters are needed'):
        plain._error_parameters('predictive_bounds', None)
    assert plain._error_parameters('x', [1.0, 0.0, 0.5]).shape == (16, 3)


def test_the_side_files(tmp_path):
    theta = np.array([[0.5, 0.1, 0.8], [1.0, 0.0, 1.0]])
    values = np.array([[-12.5, -np.inf], [3.0, np.nan], [0.25, np.nan]])
    path = str(tmp_path / 'Catchment.SMART.demcz.errormodel')
    errormodel.write_likelihood_file(path, theta, values)
    assert open(path).read().split('\n') == [
        'sigma0,sigma1,phi,LOGLIK,SSQ,LOGSIG', '5.000000e-01,1.000000e-01,8.000000e-01,-1.250000e+01,3.000000e+00,2.500000e-01',
        '1.000000e+00,0.000000e+00,1.000000e+00,-inf,nan,nan', '']
    res = errormodel.ResidualLikelihood(theta, values, None, path)
    assert res.log_likelihood.tolist() == [-12.5, -np.inf] and res.ssq[0] == 3.0 and res.logsig[0] == 0.25 and res.file == path
    path = str(tmp_path / 'Catchment.SMART.demcz.predictive')
    bounds_, alone = np.array([[0.0, 1.0], [2.0, 3.5]]), np.array([[0.5, 1.5], [1.0, 2.0]])
    errormodel.write_predictive_file(path, ['2007-01-01', '2007-01-02'], [0.05, 0.95], bounds_, alone)
    assert open(path).read().split('\n') == [
        'DateTime,q0.05,q0.95,param_q0.05,param_q0.95', '2007-01-01,0.000000e+00,2.000000e+00,5.000000e-01,1.000000e+00',
        '2007-01-02,1.000000e+00,3.500000e+00,1.500000e+00,2.000000e+00', '']
    pb = errormodel.PredictiveBounds([0.05, 0.95], bounds_, alone, 0.9, 0.4, ['a', 'b'], 2, 0, True, None, path)
    assert pb.containment == 0.9 and pb.parametric_containment == 0.4 and pb.replicates == 2 and pb.file == path
