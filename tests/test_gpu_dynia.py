"""Dynamic identifiability analysis on the GPU (smartpy_amd/csrc/smart_dynia.hip) against the statement and the exact
yardsticks of oracle/analyses/dynia.py: the C entry with its own leading dimensions and its batches, the engine and
MonteCarlo.dynamic_identifiability on top.  launch_dynia runs five kernel instances; each is reached here by (instance,
chosen when, the cases that reach it)

    smart_dynia_count                   always, once per call           every case
    smart_dynia_sums                    always, once per batch          every case: one chunk of blocks for R <= 8 w, several
                                                                        beyond (R = 100 at h = 0, 1; the general data at h = 1);
                                                                        a batch that begins inside a block (workspaces of one
                                                                        and of two steps)
    smart_dynia_shares<2048, 256>       N <= 2048                       N = 1, 2, 63, 64, 65, 257, 1000, 2048
    smart_dynia_shares<16384, 1024>     2049 <= N <= lds capacity       N = 2049, cap
    smart_dynia_shares<0, 1024>         N > lds capacity                N = cap + 1, 20000 (general data: 16400)

The exact cases (integers 0 .. 15: every E, s and S an exact integer, a share one division) compare with `same`: `==`
everywhere, NaN for NaN.  The general data hold stage one, the window sums, to exact arithmetic -- (w + 2) 2**-53 relative
against the Fraction yardstick, on a spread of columns (every column costs R w Fraction additions) -- and stage two to stage
one: the statement evaluated on the err the kernel returned makes the same selection from the same doubles, so cut and
retained compare with `==`, and the shares within 2 (K + 2) 2**-53 relative, K = retained[r] (two sums of at most K
non-negative terms in another order).  The largest share of each tolerance that was used is printed at the end of the
module (and written to $SMART_MARGINS_DIR/dynia_margins.txt where that is set); profiles/dynia_margins.txt is that table."""
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle.analyses.dynia import dynia_statement, exact_sums, EQUAL, LINEAR
from oracle.exact import U
from support import (EXTRA, SENTINEL, Margins, example_root, filled, margins_dir, padded, same, same_bits, settings_file, to_device,
                     workspace)

pytestmark = pytest.mark.gpu

MARGINS = Margins()     # what -> (largest share of its tolerance, where it was seen)
SMALL = 2048            # the largest N of the small instance of smart_dynia_shares (smart_dynia.hip: kDyniaSmallCapacity)


def capacity():
    from smartpy_amd import engine
    return engine.dynia_lds_capacity()


def launch(sim, obs, cat, B, h, min_valid, fraction, support, pad=0, junk=np.nan, spare=0, ws_steps=None, keep=True,
           pad_err=0):
    """The C entry on a [R, N] host matrix laid out with ld = N + pad (the padding holds `junk`) -> dict of numpy arrays:
    shares [R + spare, P, B], cut, retained, count [R + spare] (the spare rows as they were before the call: SENTINEL), err
    [R + spare, N + pad_err] or None.  The workspace is what the helper entry asks for, or exactly `ws_steps` steps."""
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    R, N = np.shape(sim)
    P = len(cat)
    d_sim, ld = padded(sim, pad, junk)
    d_obs, d_cat = to_device(obs), to_device(cat, np.uint8)
    shares, cut = filled((R + spare, P, B)), filled((R + spare,))
    retained, count = filled((R + spare,), 'int32'), filled((R + spare,), 'int32')
    err = filled((R + spare, N + pad_err)) if keep else None
    need = int(L.smart_dynia_workspace_bytes(N, R, h, P, B))
    if ws_steps is not None:
        need = ws_steps * int(L.smart_dynia_workspace_bytes(N, 1, h, P, B))
    assert need >= 0
    work = workspace(need, least=1)
    _lib.check(L.smart_dynia_hip(N, R, d_sim.data_ptr(), ld, d_obs.data_ptr(), h, min_valid, float(fraction),
                                 d_cat.data_ptr(), P, B, support, shares.data_ptr(), cut.data_ptr(), retained.data_ptr(),
                                 count.data_ptr(), None if err is None else err.data_ptr(), N + pad_err, work.data_ptr(),
                                 need, torch.cuda.current_stream().cuda_stream))
    return dict(shares=shares.cpu().numpy(), cut=cut.cpu().numpy(), retained=retained.cpu().numpy(),
                count=count.cpu().numpy(), err=None if err is None else err.cpu().numpy())


def all_same_bits(a, b, keys=('shares', 'cut', 'retained', 'count')):
    return all(same_bits(a[k], b[k]) for k in keys)


@pytest.fixture(scope='module', autouse=True)
def _print_the_margins():
    yield
    if not MARGINS:
        return
    text = ('largest error of this run as a share of its tolerance -- err: the window sums against the Fraction yardstick, '
            '(w + 2) 2**-53 relative; shares: against the statement evaluated on the err the kernel returned, '
            '2 (K + 2) 2**-53 relative, K = retained[r]: what, share, where it was seen\n' +
            '\n'.join('%-9s %-10.3g %s' % (name, MARGINS[name][0], MARGINS[name][1]) for name in sorted(MARGINS)) +
            '\ncut and retained of the general data: equal to the statement on the returned err\n'
            'exact cases (integers 0 .. 15): bit for bit\n')
    MARGINS.publish(text, margins_dir(), 'dynia_margins.txt')


# ---- exact cases ------------------------------------------------------------------------------------------------------
SIZES = ['1', '2', '63', '64', '65', '257', '1000', 'small', 'small+1', 'cap', 'cap+1', '20000']
FRACTIONS = (0.1, 1.0, 1e-9)      # 1e-9: k = 1


def exact_inputs(rng, N, R, h, equal_columns=False):
    """integers 0 .. 15 with everything the definition has a rule for (what fits into R and N)"""
    w = 2 * h + 1
    sim = rng.integers(0, 16, size=(R, N)).astype(np.float64)
    if N >= 2:
        sim[:, N // 2:] = sim[:, :N - N // 2]                  # duplicated columns: ties at the cut
    if equal_columns:
        sim[:] = sim[:, :1]                                     # every row at the cut: S == 0, the fallback
    obs = rng.integers(0, 16, size=R).astype(np.float64)
    if R > 3 * w:
        obs[w + 2:2 * w + 4] = np.nan                           # w + 2 missing in a row: steps not assessed
    if R >= 3:
        obs[R - 2] = np.inf                                     # the last step keeps h of its h + 1: min_valid - 1
    if R > 5:
        sim[5, 0] = np.nan                                      # not eligible exactly where the window covers row 5
        sim[3, (N - 1) // 3] = np.inf
    return sim, obs


@pytest.mark.parametrize('size', SIZES)
def test_exact_cases(size):
    cap = capacity()
    N = eval(size, {'cap': cap, 'small': SMALL})
    rng = np.random.default_rng(900 + SIZES.index(size))
    P, B = (16, 64) if N in (65, cap + 1) else (2, 4)
    cat = rng.integers(0, B, size=(P, N)).astype(np.uint8)
    cat[0, 0] = 255                                             # a row that takes no part in factor 0
    cat[P - 1, N - 1] = B if B < 255 else 255                   # ... and a bin beyond n_bins does the same
    launches = 0
    for h in (0, 1, 7):
        w = 2 * h + 1
        min_valid = h + 1                                       # the first step has exactly min_valid observed steps
        for i, R in enumerate(sorted({1, max(1, w - 1), w, w + 1, 3 * w + 1, 100})):
            fraction = FRACTIONS[(i + h) % 3]
            sim, obs = exact_inputs(rng, N, R, h, equal_columns=(i % 3 == 2 and h == 1))
            for support in (EQUAL, LINEAR):
                catref = np.where(cat >= B, 255, cat)
                want = dynia_statement(sim, obs, catref, B, h, min_valid, fraction, support)
                got = launch(sim, obs, cat, B, h, min_valid, fraction, support, pad=3, spare=1, pad_err=5)
                launches += 1
                where = (N, R, h, fraction, support)
                assert same(got['count'][:R], want['count']), where
                assert same(got['err'][:R, :N], want['E']), where
                assert same(got['cut'][:R], want['cut']), where
                assert same(got['retained'][:R], want['retained']), where
                assert same(got['shares'][:R], want['shares']), where
                assert (want['retained'] >= want['k']).all()
                # the spare rows and the padding of err are untouched
                assert (got['shares'][R:] == SENTINEL).all() and got['cut'][R] == SENTINEL and got['retained'][R] == SENTINEL
                assert got['count'][R] == SENTINEL and (got['err'][R:] == SENTINEL).all() and (got['err'][:, N:] == SENTINEL).all()
                if support == LINEAR and R in (3 * w + 1, 100):
                    # the same bits from a second launch, without err (the sums in the workspace), and whatever the
                    # batches: a workspace of one step, of two, of all
                    assert all_same_bits(launch(sim, obs, cat, B, h, min_valid, fraction, support, pad=3, spare=1, pad_err=5),
                                         dict(got, err=None))
                    whole = launch(sim, obs, cat, B, h, min_valid, fraction, support, keep=False)
                    assert all_same_bits(whole, {k: v[:R] for k, v in got.items() if k != 'err'}), where
                    for steps in (1, 2, R):
                        assert all_same_bits(launch(sim, obs, cat, B, h, min_valid, fraction, support, keep=False,
                                                    ws_steps=steps), whole), (where, steps)
                    launches += 5
    # what the inputs were built to hold did occur (the last case: h = 7, R = 100)
    assert (want['count'] < min_valid).sum() >= 3 and want['count'][0] == min_valid and want['count'][R - 1] == min_valid - 1
    assert not np.isfinite(want['E'][5, 0]) and np.isfinite(want['E'][5 + h + 1, 0])
    assert launches > 30


def test_the_workspace_must_hold_a_step():
    from smartpy_amd._lib import SmartEngineError
    rng = np.random.default_rng(3)
    sim, obs = exact_inputs(rng, 10, 9, 1)
    cat = np.zeros((1, 10), dtype=np.uint8)
    with pytest.raises(SmartEngineError, match='workspace_bytes 0, need 80') as err:
        launch(sim, obs, cat, 2, 1, 2, 0.5, LINEAR, ws_steps=0)
    assert err.value.code == -2


# ---- general data -----------------------------------------------------------------------------------------------------
def flood_data(rng, N, R, flood_at):
    """lognormal flows over six decades; a flood of 1e6 times the level around it that lasts two steps: a window sum
    falls by 1e6 within w steps of its end"""
    sim = np.exp(rng.normal(0.0, 2.3, size=(R, N)))
    obs = np.exp(rng.normal(0.0, 2.3, size=R))
    sim[flood_at:flood_at + 2] *= 1e6
    obs[flood_at:flood_at + 2] *= 1e6
    obs[R // 2] = np.nan
    return sim, obs


@pytest.mark.parametrize('h,N', [(1, 1000), (15, 1000), ('cap', 1000), (1, 16400), (15, 16400), ('cap', 16400)])
def test_general_data(h, N):
    from smartpy_amd import engine
    if h == 'cap':
        h = engine.dynia_max_half_width()
    assert N <= SMALL or N > capacity()
    w = 2 * h + 1
    R = {1: 40, 15: 100, 63: 300}[h]
    rng = np.random.default_rng(1000 * h + N)
    sim, obs = flood_data(rng, N, R, flood_at=R // 4)
    P, B = 3, 7
    cat = rng.integers(0, B, size=(P, N)).astype(np.uint8)
    cat[1, ::17] = 255
    min_valid = h + 1
    columns = sorted({0, 1, 63, 64, 65, N // 2, N - 2, N - 1} | set(rng.integers(0, N, size=8).tolist()))
    exact = exact_sums(sim[:, columns], obs, h, min_valid)
    for support in (LINEAR, EQUAL):
        got = launch(sim, obs, cat, B, h, min_valid, 0.1, support, pad=1)
        where = 'N = %d, R = %d, h = %d, support %d' % (N, R, h, support)
        # stage one against exact arithmetic
        for r in range(R):
            for j, n in enumerate(columns):
                if exact[r][j] is None:
                    assert np.isnan(got['err'][r, n])
                    continue
                share = float(abs(Fraction(float(got['err'][r, n])) - exact[r][j]) / ((w + 2) * U * exact[r][j]))
                print('err', where, r, n, share) if share > 0.5 else None
                MARGINS.note('err', share, where)
                assert share <= 1.0, (where, r, n, share)
        with np.errstate(invalid='ignore', divide='ignore'):
            falls = got['err'][:-1] / got['err'][1:]
        dropped = float(np.nanmax(np.where(np.isfinite(falls), falls, np.nan)))
        assert dropped > 1e6, dropped          # the flood did leave a window: a sum fell by 1e6 from one step to the next
        # stage two against the statement on the sums the kernel returned
        want = dynia_statement(sim, obs, cat, B, h, min_valid, 0.1, support, err=got['err'])
        assert same(got['count'], want['count']) and same(got['cut'], want['cut']), where
        assert same(got['retained'], want['retained']) and (want['retained'] >= want['k']).all(), where
        assessed = want['count'] >= min_valid
        assert assessed.sum() > R // 2 and np.isnan(got['shares'][~assessed]).all()
        assert (np.isnan(got['err']).all(axis=1) == ~assessed).all()
        for r in np.flatnonzero(assessed):
            tol = 2.0 * (want['retained'][r] + 2) * U
            a, b = got['shares'][r], want['shares'][r]
            assert ((b == 0) == (a == 0)).all(), (where, r)
            share = float((np.abs(a - b)[b > 0] / (tol * b[b > 0])).max())
            MARGINS.note('shares', share, where)
            assert share <= 1.0, (where, r, share)
        assert np.allclose(got['shares'][assessed][:, 0].sum(axis=1), 1.0, rtol=1e-12, atol=0)
        # the same bits without err, and from the batches of a small workspace
        plain = launch(sim, obs, cat, B, h, min_valid, 0.1, support, keep=False, ws_steps=7)
        assert all_same_bits(plain, got), where


# ---- the engine and MonteCarlo on top ---------------------------------------------------------------------------------
def test_engine_against_the_c_entry():
    import torch
    from smartpy_amd import engine
    rng = np.random.default_rng(23)
    N, R, h, B = 1500, 30, 2, 6
    sim, obs = flood_data(rng, N, R, flood_at=8)
    cat = rng.integers(0, B, size=(4, N)).astype(np.uint8)
    ref = launch(sim, obs, cat, B, h, 3, 0.1, LINEAR)
    wide = torch.from_numpy(np.concatenate([sim, np.full((R, 9), np.nan)], axis=1)).cuda()
    view = wide[:, :N]                                      # a matrix with a leading dimension of its own
    assert view.stride(0) == N + 9
    for errors in (False, True):
        res = engine.dynamic_identifiability(view, obs, cat, B, h, keep_errors=errors)
        assert res.shares.is_cuda and res.shares.shape == (R, 4, B) and res.shares.dtype == torch.float64
        assert res.retained.dtype == torch.int32 and res.count.dtype == torch.int32 and res.cut.shape == (R,)
        got = dict(shares=res.shares.cpu().numpy(), cut=res.cut.cpu().numpy(), retained=res.retained.cpu().numpy(),
                   count=res.count.cpu().numpy())
        assert all_same_bits(got, ref)                      # fraction 0.1, min_valid (w + 1) // 2 = 3, 'linear' by default
        assert (res.errors is None) == (not errors)
        if errors:
            assert same_bits(res.errors.cpu().numpy(), ref['err'])
    eq = engine.dynamic_identifiability(sim, torch.from_numpy(obs), torch.from_numpy(cat).cuda(), B, h, fraction=0.25,
                                        min_valid=1, support='equal')
    ref = launch(sim, obs, cat, B, h, 1, 0.25, EQUAL)
    assert same_bits(eq.shares.cpu().numpy(), ref['shares']) and same_bits(eq.retained.cpu().numpy(), ref['retained'])
    with pytest.raises(engine.SmartEngineError, match='half_width 64 must be in 0 .. 63'):
        engine.dynamic_identifiability(view, obs, cat, B, 64)
    with pytest.raises(engine.SmartEngineError, match=r'fraction 0 is outside \(0, 1\]'):
        engine.dynamic_identifiability(view, obs, cat, B, h, fraction=0.0)


def test_a_planted_parameter_is_the_one_identified():
    """ten factors drawn independently; on the steps 20 .. 39 the error of a row is decided by factor 3 alone (its
    distance from 0.3), elsewhere by noise that knows nothing of the factors: on that stretch, and only there, factor 3
    carries the most information of the ten"""
    from smartpy_amd import engine, identifiability as ident
    rng = np.random.default_rng(5)
    N, R, P, h, B = 2000, 60, 10, 2, 10
    theta = rng.uniform(0.0, 1.0, size=(N, P))
    ranges = [(0.0, 1.0)] * P
    obs = rng.gamma(2.0, 3.0, size=R) + 5.0
    sim = obs[:, None] + rng.normal(0.0, 1.0, size=(R, N))
    sim[20:40] = obs[20:40, None] + 10.0 * np.abs(theta[:, 3] - 0.3)[None, :] + rng.normal(0.0, 0.01, size=(20, N))
    cat = ident.bin_table(theta, ranges, B)
    res = engine.dynamic_identifiability(sim, obs, cat, B, h, fraction=0.1)
    shares = res.shares.cpu().numpy()
    info = ident.information_content(ident.confidence_limits(shares, ranges, 0.9), ranges)
    assert info.shape == (R, P) and np.isfinite(info).all() and (info >= 0).all() and (info <= 1).all()
    inside = info[20 + h:40 - h]
    assert (inside.argmax(axis=1) == 3).all() and (inside[:, 3] > 0.8).all()
    assert (np.delete(inside, 3, axis=1) < 0.5).all()
    limits = ident.confidence_limits(shares, ranges, 0.9)[20 + h:40 - h, 3]
    assert (limits[:, 0] >= 0.2).all() and (limits[:, 1] <= 0.4).all()
    outside = np.concatenate([info[:20 - h], info[40 + h:]])
    assert (outside[:, 3] < 0.5).all()


def test_lhs_dynamic_identifiability_end_to_end(tmp_path):
    from smartpy_amd.montecarlo import LHS
    from smartpy_amd import engine, identifiability as ident
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sampling.sttngs', '01/01/2007', '31/12/2007', 180)
    np.random.seed(2024)
    lhs = LHS('Catchment', root, 'csv', 'csv', sample_size=300, settings_filename='Catchment.sampling.sttngs')
    lhs.model.extra = EXTRA
    res = lhs.dynamic_identifiability(half_width=3, bins=5, write=True)
    R, P = len(lhs.model.timeseries_report) - 1, 10
    assert res.names == lhs.param_names and res.datetime == lhs.model.timeseries_report[1:] and len(res.names) == P
    assert res.ranges.tolist() == [list(lhs.model.parameters.ranges[name]) for name in res.names]
    assert res.shares.shape == (R, P, 5) and res.limits.shape == (R, P, 2) and res.information.shape == (R, P)
    assert res.cut.shape == res.mean_error.shape == (R,) and res.retained.shape == res.count.shape == (R,)
    assert (res.half_width, res.fraction, res.support, res.min_valid, res.level) == (3, 0.1, 'linear', 4, 0.9)
    obs = np.asarray(lhs.model.nd_flow, dtype=np.float64)
    counts = np.array([np.isfinite(obs[max(0, r - 3):r + 4]).sum() for r in range(R)])
    assert np.array_equal(res.count, counts)
    assessed = counts >= 4
    assert assessed.sum() > 10
    assert np.isfinite(res.information[assessed]).all() and np.isnan(res.information[~assessed]).all()
    assert (res.information[assessed] >= 0).all() and (res.information[assessed] <= 1).all()
    assert (res.retained[assessed] >= 30).all() and (res.retained[~assessed] == 0).all()
    assert np.allclose(res.shares[assessed].sum(axis=2), 1.0, rtol=1e-12, atol=0)      # every drawn row lies in its range
    assert np.array_equal(res.mean_error[assessed], (res.cut / res.count)[assessed])
    # the same as the engine called by hand on the same launch
    out = lhs.model.simulate_ensemble(lhs._sample, save_discharge=True, math_mode=lhs.math_mode)
    cat = ident.bin_table(lhs._sample, res.ranges, 5)
    by_hand = engine.dynamic_identifiability(out.discharge_report_major, obs, cat, 5, 3, fraction=0.1, min_valid=4,
                                             support='linear')
    assert same_bits(by_hand.shares.cpu().numpy(), res.shares) and same_bits(by_hand.cut.cpu().numpy(), res.cut)
    assert same_bits(res.device_shares.cpu().numpy(), res.shares)
    assert np.array_equal(by_hand.retained.cpu().numpy(), res.retained)
    # the file
    assert res.file == lhs.dynia_file == os.path.join(lhs.model.out_f, 'Catchment.SMART.lhs.dynia')
    lines = open(res.file).read().split('\n')
    assert lines[0] == 'DateTime,' + ','.join('IC@%s,LO@%s,HI@%s' % (n, n, n) for n in res.names)
    assert len(lines) == R + 2 and lines[-1] == ''
    assert [ln.split(',')[0] for ln in lines[1:-1]] == [str(dt) for dt in res.datetime]
    r = int(np.flatnonzero(assessed)[0])
    cells = []
    for p in range(P):
        cells += ['%.6e' % res.information[r, p], '%.6e' % res.limits[r, p, 0], '%.6e' % res.limits[r, p, 1]]
    assert lines[1 + r].split(',')[1:] == cells
    # equal support and other ranges; nothing is written unless asked for
    wide = dict(lhs.model.parameters.ranges, T=(0.5, 1.5))
    eq = lhs.dynamic_identifiability(half_width=3, bins=5, support='equal', ranges=wide, fraction=0.2)
    assert eq.file is None and eq.ranges[0].tolist() == [0.5, 1.5]
    assert np.array_equal(eq.shares[assessed][:, :, :].sum(axis=2) > 0.999, np.ones((assessed.sum(), P), dtype=bool))
    assert (eq.shares[assessed][:, 0, [0, 1, 3, 4]] == 0).all()         # T was drawn from (0.9, 1.1): the middle bin of five
    assert np.array_equal(eq.retained[assessed], np.round(eq.shares[assessed][:, 0, 2] * eq.retained[assessed]))
    assert (eq.retained[assessed] >= 60).all()
    # no row (a GLUE without a behavioural set): everything NaN, nothing is launched, the file still has its lines
    lhs._set_sample(np.empty((0, P)))
    empty = lhs.dynamic_identifiability(half_width=3, bins=5, write=True)
    assert empty.shares.shape == (R, P, 5) and np.isnan(empty.shares).all() and np.isnan(empty.information).all()
    assert (empty.retained == 0).all() and (empty.count == 0).all() and empty.device_shares is None
    assert len(open(empty.file).read().split('\n')) == R + 2
