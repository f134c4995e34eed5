"""Ensemble verification scores on the GPU (smartpy_amd/csrc/smart_ensemble_scores.hip) against the exact yardstick and
the numpy statement of oracle/analyses/ensemble_scores.py: both forms, the C entry with its own leading dimension and its
batches, the engine and GLUE.ensemble_verification on top.  launch_ensemble_scores chooses among ten kernel instances;
each is reached here by (instance -- with and without weights --, chosen when, the N of test_exact_cases that reach it)

    smart_ensemble_scores_lds<1024, 512, .>     LDS, N <= 1024             N = 1, 2, 1000, 1024
    smart_ensemble_scores_lds<2048, 1024, .>    LDS, 1025 <= N <= 2048     N = 1025, 2048   (general weights: 1500)
    smart_ensemble_scores_lds<4096, 1024, .>    LDS, 2049 <= N <= 4096     N = 2049, 4096
    smart_ensemble_scores_lds<8192, 1024, .>    LDS, 4097 <= N <= capacity N = 4097, cap    (general weights: cap)
    smart_ensemble_scores_global<.>             global, any N <= 2**24     every N of the list: one block of 4096 up to
                                                N = 4096, 2 blocks at 4097 and cap, 4 at cap + 1, 8 at 2**15, 32 at
                                                2**17 (general weights: cap + 1, 3 cap + 5 -> 8 blocks, 100,000 -> 32)

Without weights only the N that are powers of two are exact cases (W = N must divide exactly).  AUTO takes the LDS form up
to the capacity and the global form beyond: test_exact_cases launches it at cap and at cap + 1.

The exact cases compare with `same`: `==` everywhere, NaN for NaN.  The cases with general weights are held to
4 (N + 4) 2**-53 relative (CRPS, SPREAD), N 2**-53 absolute (the PITs) and N 2**-53 sum w |x| / W (MEAN); the largest share
of each tolerance that was used is printed at the end of the module (and written to
$SMART_MARGINS_DIR/ensemble_scores_margins.txt where that is set); profiles/ensemble_scores_margins.txt is that table."""
import os

import numpy as np
import pytest

from oracle.analyses.ensemble_scores import (yardstick, yardstick_rows, assert_all_exact, as_floats, statement, shares,
                                             CRPS, SPREAD, PIT_LOW, PIT_HIGH, MEAN)
from support import (EXTRA, NSE_MIN, SENTINEL, Margins, example_root, filled, margins_dir, padded, ptr, same, same_bits,
                     settings_file, to_device, workspace)

pytestmark = pytest.mark.gpu

AUTO, LDS, GLOBAL = 0, 1, 2
NAMES = ('CRPS', 'SPREAD', 'PIT_LOW', 'PIT_HIGH', 'MEAN')
MARGINS = Margins()     # column name -> (largest share of its tolerance, where it was seen)


def capacity():
    from smartpy_amd import engine
    return engine.ensemble_scores_lds_capacity()


def launch(matrix, weights, obs, method, pad=0, junk=np.nan, spare=0, ws_steps=None):
    """The C entry on a [R, N] host matrix laid out with ld = N + pad (the padding holds `junk`) -> numpy [5, R] (with
    `spare` more rows below, as they were before the call: SENTINEL).  The workspace is what the helper entry asks for, or
    exactly `ws_steps` steps."""
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    R, N = np.shape(matrix)
    sim, ld = padded(matrix, pad, junk)
    w, y = to_device(weights), to_device(obs)
    out = filled((5 + spare, R))
    weighted = 0 if w is None else 1
    need = int(L.smart_ensemble_scores_workspace_bytes(N, R, weighted, method))
    if ws_steps is not None:
        need = ws_steps * int(L.smart_ensemble_scores_workspace_bytes(N, 1, weighted, method))
    assert need >= 0
    work = workspace(need)
    _lib.check(L.smart_ensemble_scores_hip(N, R, sim.data_ptr(), ld, ptr(w), ptr(y), out.data_ptr(), method, ptr(work),
                                           need, torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


def forms(N):
    return (LDS, GLOBAL) if N <= capacity() else (GLOBAL,)


def record(got, exact_rows, x, w, what):
    """hold every step of `got` [5, R] to its tolerances against the references of the steps; keep the margins"""
    for r, exact in enumerate(exact_rows):
        used = shares(got[:, r], exact, x[r], w)
        for name, share in used.items():
            MARGINS.note(name, share, what)
        assert all(v <= 1.0 for v in used.values()), (what, r, used)


@pytest.fixture(scope='module', autouse=True)
def _print_the_margins():
    yield
    if not MARGINS:
        return
    text = ('largest error of this run against the exact yardstick (longdouble statement for N > 3 * capacity), as a share '
            'of the tolerance -- CRPS and SPREAD 4 (N + 4) 2**-53 relative, PIT_LOW and PIT_HIGH N 2**-53 absolute, MEAN '
            'N 2**-53 sum w |x| / W: column, share, where it was seen\n' +
            '\n'.join('%-9s %-10.3g %s' % (name, MARGINS[name][0], MARGINS[name][1]) for name in NAMES if name in MARGINS) +
            '\nexact cases (small-integer members, weights whose sum is a power of two): bit for bit\n')
    MARGINS.publish(text, margins_dir(), 'ensemble_scores_margins.txt')


# ---- exact cases ------------------------------------------------------------------------------------------------------
def power_of_two_integer_weights(rng, n):
    """n integer weights 1 .. 3, the last one raised until the total is a power of two: every partial sum is an exact
    integer, every quotient by W a dyadic number of few bits"""
    w = rng.integers(1, 4, size=n)
    total = int(w.sum())
    w[-1] += (1 << (total - 1).bit_length()) - total
    return w.astype(np.float64)


SIZES = ['1', '2', '1000', '1024', '1025', '2048', '2049', '4096', '4097', 'cap', 'cap+1', '2**15', '2**17']
# (members 0 .. 15, halves for the observation) below, above, on a member, inside a gap, on the lowest member, missing
OBSERVATIONS = np.array([-2.0, 21.5, 7.0, 3.5, 0.0, np.nan])


# without weights W = N must divide exactly: the powers of two (the module's docstring)
EXACT = [(s, True) for s in SIZES] + [(s, False) for s in SIZES if s not in ('1000', '1025', '2049', '4097', 'cap+1')]


@pytest.mark.parametrize('size,weighted', EXACT)
def test_exact_cases(size, weighted):
    cap = capacity()
    N = eval(size, {'cap': cap})
    assert weighted or N & (N - 1) == 0
    rng = np.random.default_rng(500 + 2 * SIZES.index(size) + weighted)
    R = len(OBSERVATIONS)
    x = rng.integers(0, 16, size=(R, N)).astype(np.float64)
    w = power_of_two_integer_weights(rng, N) if weighted else None
    want = np.stack([as_floats(assert_all_exact(x[r], w, OBSERVATIONS[r])) for r in range(R)], axis=1)
    assert np.isnan(want[[CRPS, PIT_LOW, PIT_HIGH], -1]).all() and not np.isnan(want[:, :-1]).any()
    assert same(want, statement(x, w, OBSERVATIONS))
    methods = forms(N) + ((AUTO,) if N in (cap, cap + 1) else ())
    for m in methods:
        got = launch(x, w, OBSERVATIONS, m, pad=3)
        assert same(got, want), (size, weighted, m, got, want)
    if not weighted:        # weights of one are no weights
        for m in forms(N):
            assert same(launch(x, np.ones(N), OBSERVATIONS, m), want), (size, m)


@pytest.mark.parametrize('size', ['1', '2', '1000', '2049', 'cap', 'cap+1'])
def test_all_members_equal(size):
    """SPREAD is exactly 0 and CRPS exactly |x - y|, whatever the weights (every gap is 0, and 0 * P is 0).  MEAN: every
    product w x and the quotient by W round once, the sums of N non-negative terms lose at most N - 1 roundings more."""
    N = eval(size, {'cap': capacity()})
    rng = np.random.default_rng(40 + N)
    obs = np.array([2.5, -1.25, 7.0, np.nan])
    x = np.full((4, N), 2.5)
    for w in (None, rng.uniform(0.1, 1.0, size=N)):
        for m in forms(N):
            got = launch(x, w, obs, m, pad=1)
            assert same(got[SPREAD], np.zeros(4)) and same(got[CRPS], np.array([0.0, 3.75, 4.5, np.nan])), (size, m, got)
            assert same(got[PIT_LOW], np.array([0.0, 0.0, 1.0, np.nan])), (size, m, got)
            assert same(got[PIT_HIGH], np.array([1.0, 0.0, 1.0, np.nan])), (size, m, got)
            assert np.allclose(got[MEAN], 2.5, rtol=(N + 2) * 2.0 ** -53, atol=0), (size, m, got[MEAN] - 2.5)


# ---- general weights and values -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', ['1500', 'cap', 'cap+1', '3*cap+5', '100000'])
def test_general_weights_and_values(size):
    from oracle.analyses.ensemble_scores import float_scores
    cap = capacity()
    N = eval(size, {'cap': cap})
    rng = np.random.default_rng(900 + N)
    R = 3 if N == 100000 else 4
    x = rng.gamma(2.0, 3.0, size=(R, N))
    x[:, ::7] = x[:, 1:2]                                       # some ties
    w = rng.uniform(0.0, 1.0, size=N)
    ranked = np.sort(x, axis=1)
    obs = np.array([ranked[0, 0] - 1.0, ranked[1, N // 2], 0.5 * (ranked[2, N // 3] + ranked[2, N // 3 + 1]),
                    ranked[3 % R, -1] + 2.0])[:R]
    if N > 3 * cap:         # Fractions are too slow here: the same definitions in longdouble (64 bits of mantissa)
        exact = [float_scores(x[r], w, obs[r], np.longdouble) for r in range(R)]
    else:
        exact = yardstick_rows(x, w, obs)
    for m in forms(N):
        got = launch(x, w, obs, m, pad=3)
        record(got, exact, x, w, 'N=%d %s weighted' % (N, 'LDS' if m == LDS else 'global'))
    exact = ([float_scores(x[r], None, obs[r], np.longdouble) for r in range(R)] if N > 3 * cap
             else yardstick_rows(x, None, obs))
    for m in forms(N):
        got = launch(x, None, obs, m, pad=3)
        record(got, exact, x, None, 'N=%d %s equal weights' % (N, 'LDS' if m == LDS else 'global'))


# ---- special cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', ['700', 'cap', 'cap+1'])
def test_members_of_weight_zero_take_no_part(size):
    N = eval(size, {'cap': capacity()})
    rng = np.random.default_rng(60 + N)
    R = 4
    x, w = rng.gamma(2.0, 3.0, size=(R, N)), rng.uniform(0.1, 1.0, size=N)
    dead = rng.permutation(N)[:N // 3]
    w[dead] = 0.0
    x[:, dead[0::4]], x[:, dead[1::4]], x[:, dead[2::4]] = np.nan, np.inf, -np.inf
    obs = np.array([x[0, ~np.isin(np.arange(N), dead)].min() - 1.0, np.median(x[1, w > 0]), 5.0, np.nan])
    keep = w > 0
    exact = yardstick_rows(x[:, keep], w[keep], obs)
    assert exact == yardstick_rows(x, w, obs) and exact[0][0] is not None
    for m in forms(N):
        got = launch(x, w, obs, m, pad=2)
        assert not np.isnan(got[:, :3]).any() and not np.isnan(got[[SPREAD, MEAN], 3]).any()
        record(got, exact, x[:, keep], w[keep], 'N=%d %s a third weightless' % (N, 'LDS' if m == LDS else 'global'))
        record(launch(x[:, keep], w[keep], obs, m), exact, x[:, keep], w[keep], 'N=%d without them' % keep.sum())
    # exact weights and values: not even the last bits
    xi = rng.integers(0, 16, size=(R, N)).astype(np.float64)
    wi = power_of_two_integer_weights(rng, N)
    obs = np.array([-2.0, 7.0, 3.5, np.nan])
    want = launch(xi, wi, obs, forms(N)[0])
    assert same(want, statement(xi, wi, obs))
    wide = np.concatenate([xi, np.full((R, 5), np.nan), np.full((R, 3), np.inf)], axis=1)
    order = rng.permutation(N + 8)
    for m in forms(N + 8):
        assert same(launch(wide[:, order], np.concatenate([wi, np.zeros(8)])[order], obs, m), want), (size, m)


@pytest.mark.parametrize('size', ['700', 'cap', 'cap+1'])
def test_a_live_member_that_is_not_finite_spoils_its_step_only(size):
    N = eval(size, {'cap': capacity()})
    rng = np.random.default_rng(70 + N)
    x = rng.integers(0, 16, size=(6, N)).astype(np.float64)
    obs = np.full(6, 3.5)
    for w in (None, power_of_two_integer_weights(rng, N)):
        clean = {m: launch(x, w, obs, m) for m in forms(N)}
        bad = x.copy()
        bad[1, N // 2], bad[3, 0], bad[4, N - 1] = np.nan, np.inf, -np.inf
        for m in forms(N):
            got = launch(bad, w, obs, m, pad=1)
            assert np.isnan(got[:, [1, 3, 4]]).all(), (size, m, got)
            assert same(got[:, [0, 2, 5]], clean[m][:, [0, 2, 5]]) and not np.isnan(got[:, [0, 2, 5]]).any()


@pytest.mark.parametrize('size', ['700', 'cap+1'])
def test_missing_observations_zero_total_weight_and_signed_zeros(size):
    N = eval(size, {'cap': capacity()})
    rng = np.random.default_rng(80 + N)
    x = rng.integers(0, 16, size=(5, N)).astype(np.float64)
    w = power_of_two_integer_weights(rng, N)
    obs = np.array([3.5, np.nan, np.inf, -np.inf, 7.0])
    want = statement(x, w, obs)
    for m in forms(N):
        got = launch(x, w, obs, m)
        assert same(got, want)
        assert np.isnan(got[[CRPS, PIT_LOW, PIT_HIGH], 1:4]).all() and not np.isnan(got[[SPREAD, MEAN]]).any()
        # obs == NULL: as if every observation were missing
        none = launch(x, w, None, m)
        assert np.isnan(none[[CRPS, PIT_LOW, PIT_HIGH]]).all() and same(none[[SPREAD, MEAN]], want[[SPREAD, MEAN]])
        # W == 0
        assert np.isnan(launch(x, np.zeros(N), obs, m)).all()
    # -0.0 and +0.0 are one value, among the members and as the observation
    z = rng.choice(np.array([0.0, -0.0, 1.0, -1.0]), size=(4, N))
    z[:, :4] = [0.0, -0.0, 1.0, -1.0]
    obs = np.array([0.0, -0.0, 0.5, -1.0])
    want = statement(np.where(z == 0.0, 0.0, z), w, np.array([0.0, 0.0, 0.5, -1.0]))
    assert not np.isnan(want).any() and (want[PIT_LOW, :2] < want[PIT_HIGH, :2]).all()
    for m in forms(N):
        got = launch(z, w, obs, m)
        assert same(got, want), (size, m)
        assert same_bits(launch(z, w, -obs, m)[:, :2], got[:, :2])


# ---- layout and batching ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', ['1000', 'cap', 'cap+1'])
def test_leading_dimension_spare_rows_and_two_launches(size):
    N = eval(size, {'cap': capacity()})
    rng = np.random.default_rng(90 + N)
    x, w = rng.gamma(2.0, 3.0, size=(5, N)), rng.uniform(0.0, 1.0, size=N)
    obs = rng.gamma(2.0, 3.0, size=5)
    for m in forms(N):
        plain = launch(x, w, obs, m)
        assert not np.isnan(plain).any()
        roomy = launch(x, w, obs, m, pad=5, junk=np.nan, spare=2)
        assert roomy.shape == (7, 5) and same_bits(roomy[:5], plain) and (roomy[5:] == SENTINEL).all()
        assert same_bits(launch(x, w, obs, m, pad=1, junk=1e300), plain)
        assert same_bits(launch(x, w, obs, m), plain)               # two launches give the same bits
        assert same_bits(launch(x, None, obs, m), launch(x, None, obs, m, pad=3))


@pytest.mark.parametrize('weighted', [True, False])
def test_global_form_in_batches(weighted):
    """A workspace for exactly two steps and five report steps: three launches (2, 2, 1), the bits of the one-batch run."""
    N = capacity() + 1
    rng = np.random.default_rng(95 + weighted)
    x = rng.gamma(2.0, 3.0, size=(5, N))
    w = rng.uniform(0.0, 1.0, size=N) if weighted else None
    obs = rng.gamma(2.0, 3.0, size=5)
    whole = launch(x, w, obs, GLOBAL)
    assert not np.isnan(whole).any() and len(set(whole[CRPS].tolist())) == 5
    assert same_bits(launch(x, w, obs, GLOBAL, ws_steps=2, spare=1)[:5], whole)
    assert same_bits(launch(x, w, obs, AUTO, ws_steps=1), whole)
    from smartpy_amd._lib import SmartEngineError
    with pytest.raises(SmartEngineError, match='workspace') as err:
        launch(x, w, obs, GLOBAL, ws_steps=0)
    assert err.value.code == -1


# ---- the engine and GLUE on top -------------------------------------------------------------------------------------------
def test_engine_against_the_c_entry():
    import torch
    from smartpy_amd import engine
    cap = capacity()
    rng = np.random.default_rng(17)
    for N in (1500, cap + 1):
        x, w = rng.gamma(2.0, 3.0, size=(6, N)), rng.uniform(0.0, 1.0, size=N)
        obs = rng.gamma(2.0, 3.0, size=6)
        obs[4] = np.nan
        wide = torch.from_numpy(np.concatenate([x, np.full((6, 9), np.nan)], axis=1)).cuda()
        view = wide[:, :N]                                      # a matrix with a leading dimension of its own
        assert view.stride(0) == N + 9
        for name, m in (('auto', AUTO), ('lds', LDS), ('global', GLOBAL)):
            if m == LDS and N > cap:
                with pytest.raises(engine.SmartEngineError, match='at most %d samples' % cap):
                    engine.ensemble_scores(view, obs, w, method=name)
                continue
            got = engine.ensemble_scores(view, obs, w, method=name)
            assert got.is_cuda and got.dtype == torch.float64 and got.shape == (5, 6)
            assert same_bits(got.cpu().numpy(), launch(x, w, obs, m)), (N, name)
            assert same_bits(engine.ensemble_scores(x, torch.from_numpy(obs), w, method=name).cpu().numpy(), got.cpu().numpy())
        plain = engine.ensemble_scores(view).cpu().numpy()
        assert same_bits(plain, launch(x, None, None, AUTO)) and np.isnan(plain[[CRPS, PIT_LOW, PIT_HIGH]]).all()
        bad = w.copy()
        bad[3], bad[5] = -1.0, np.inf
        with pytest.raises(engine.SmartEngineError, match='2 of the %d weights' % N):
            engine.ensemble_scores(view, obs, bad)
    with pytest.raises(engine.SmartEngineError, match="method 'median' unknown"):
        engine.ensemble_scores(view, obs, w, method='median')


def test_glue_ensemble_verification_end_to_end(tmp_path):
    from smartpy_amd.montecarlo import LHS, GLUE
    from smartpy_amd import verification
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sampling.sttngs', '01/01/2007', '31/12/2007', 180)
    settings_file(root, 'Catchment.evaluating.sttngs', '01/01/2008', '30/06/2008', 90)
    np.random.seed(2024)
    lhs = LHS('Catchment', root, 'csv', 'csv', sample_size=256, settings_filename='Catchment.sampling.sttngs')
    lhs.model.extra = EXTRA
    lhs.run()
    glue = GLUE('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (NSE_MIN,))}, sampling=lhs,
                settings_filename='Catchment.evaluating.sttngs')
    glue.model.extra = EXTRA
    n = glue.behavioural_params.shape[0]
    assert 10 <= n <= 200
    nse = glue.behavioural_obj_fns[:, 0].astype(np.float64)
    R = len(glue.model.timeseries_report) - 1
    out = glue.model.simulate_ensemble(glue._sample, save_discharge=True, math_mode=glue.math_mode)
    dis = out.discharge.cpu().numpy()
    assert dis.shape == (n, R)
    obs = np.asarray(glue.model.nd_flow, dtype=np.float64)
    assert np.isfinite(obs).sum() > 10
    for likelihood, w in (('NSE', nse), (None, None)):
        ev = glue.ensemble_verification(likelihood=likelihood, bins=5, write=True)
        scores = np.stack([ev.crps, ev.spread, ev.pit_low, ev.pit_high, ev.mean])
        assert scores.shape == (5, R) and scores.dtype == np.float64 and ev.datetime == glue.model.timeseries_report[1:]
        record(scores, yardstick_rows(dis.T, w, obs), dis.T, w, 'GLUE, %d behavioural rows, likelihood=%s' % (n, likelihood))
        valid = np.isfinite(obs)
        assert np.array_equal(np.isfinite(ev.crps), valid) and ev.n_valid == valid.sum()
        assert np.isfinite(ev.spread).all() and np.isfinite(ev.mean).all()
        assert (ev.pit_low[valid] <= ev.pit_high[valid]).all() and (ev.crps[valid] >= 0).all()
        # the aggregates are the host statement on these scores
        ref = verification.EnsembleVerification(scores, obs, bins=5)
        assert ev.mean_crps == ref.mean_crps == ev.crps[valid].mean() and ev.mean_spread == ev.spread[valid].mean()
        assert ev.skill == ref.skill == 1.0 - ev.mean_crps / verification.crps_climatology(obs, obs[valid]).mean()
        assert ev.skill < 1.0 and np.array_equal(ev.pit_histogram, ref.pit_histogram) and ev.reliability == ref.reliability
        assert ev.pit_histogram.shape == (5,) and abs(ev.pit_histogram.sum() - ev.n_valid) < 1e-9
        assert 0.0 <= ev.reliability <= 1.0
        # the file: the dates and the '%e' of the modelled flow file
        assert ev.file == os.path.join(glue.model.out_f, 'Catchment.SMART.glue.verification')
        lines = open(ev.file, newline='').read().split('\r\n')
        assert lines[0] == 'DateTime,crps,spread,pit_low,pit_high,mean' and len(lines) == R + 2 and lines[-1] == ''
        assert [ln.split(',')[0] for ln in lines[1:-1]] == [str(dt) for dt in ev.datetime]
        assert [ln.split(',')[1:] for ln in lines[1:-1]] == [['%e' % v for v in col] for col in scores.T]
        parsed = np.array([[float(v) for v in ln.split(',')[1:]] for ln in lines[1:-1]]).T
        assert np.allclose(parsed, scores, rtol=5e-7, atol=0, equal_nan=True)
    assert glue.ensemble_verification().file is None
    shifted = glue.ensemble_verification(likelihood=nse - nse.min())
    record(np.stack([shifted.crps, shifted.spread, shifted.pit_low, shifted.pit_high, shifted.mean]),
           yardstick_rows(dis.T, nse - nse.min(), obs), dis.T, nse - nse.min(), 'GLUE, one likelihood of zero')
    with pytest.raises(Exception, match='negative or not finite'):
        glue.ensemble_verification(likelihood=-np.ones(n))
    # no behavioural set (from the database the sampling run has written): everything NaN, nothing is launched
    nobody = GLUE('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (2.0,))},
                  settings_filename='Catchment.evaluating.sttngs')
    nobody.model.extra = EXTRA
    assert nobody.behavioural_params.shape[0] == 0
    empty = nobody.ensemble_verification(likelihood='NSE', bins=4)
    for col in (empty.crps, empty.spread, empty.pit_low, empty.pit_high, empty.mean, empty.crps_climatology):
        assert col.shape == (R,) and np.isnan(col).all()
    assert empty.n_valid == 0 and empty.file is None and empty.pit_histogram.tolist() == [0.0] * 4
    assert all(np.isnan(v) for v in (empty.mean_crps, empty.mean_spread, empty.skill, empty.reliability))
    assert empty.datetime == nobody.model.timeseries_report[1:]
