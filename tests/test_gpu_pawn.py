"""PAWN sensitivity on the GPU (smartpy_amd/csrc/smart_pawn.hip) against the numpy statement of oracle/analyses/pawn.py: the
C entry with a leading dimension of its own, spare output rows and its batches, the engine and MonteCarlo.pawn_sensitivity
on top.  EVERY comparison is an equality of bytes (NaN for NaN): the result is a ratio of integers and there is no
tolerance anywhere in this file.  launch_pawn runs six kernel instances; each is reached here by (instance, chosen when,
the sizes that reach it)

    smart_pawn_counts                   always, once per call           every case
    smart_pawn_lds<1024, 512>           N <= 1024                       N = 1, 2, 63, 64, 65, 257, 1000, 1024
    smart_pawn_lds<2048, 1024>          1025 <= N <= 2048               N = 1025, 2048
    smart_pawn_lds<4096, 1024>          2049 <= N <= 4096               N = 2049, 4096
    smart_pawn_lds<8192, 1024>          4097 <= N <= lds capacity       N = 4097, cap - 1, cap
    smart_pawn_global                   N > lds capacity, or asked for  N = 1000 and cap (asked for: one block of 4096, and
                                                                        two with one long stage), cap + 1 (four blocks: a
                                                                        long stage alone and two in one pass), 20000 (eight
                                                                        blocks: two in one pass and then one alone); the
                                                                        batches of a workspace of one and of two steps

Values (two sets of rows a size): lognormal flows; integers 0 .. 15 with duplicated columns, so that runs of ties cross
every segment boundary; a row of equal values; a row where -0.0 and +0.0 mix with other values; a row with one NaN, one
with +inf, one with -inf between rows that must not notice.  Categories (five tables a size): 16 factors x 64 bins (one
factor a pass of the walk), 1 x 1 (no 255: ks is 0.0), 1 x 7, 13 x 10 (six factors a pass: 6 + 6 + 1), 16 x 3 (21 a
pass: all 16 in one) -- with a factor of many 255, one with an empty bin and a bin of a single row, one that is all 255,
one whose bins are the ranks of the first row's values (ks = (B - 1) / B in the outer bins where B divides N) and
one with values beyond the bins."""
import functools
import os

import numpy as np
import pytest

from oracle.analyses.pawn import pawn_statement
from support import EXTRA, SENTINEL, example_root, filled, padded, same_bits, settings_file, workspace

pytestmark = pytest.mark.gpu

AUTO, LDS, GLOBAL = 0, 1, 2
TABLES = [(16, 64), (1, 1), (1, 7), (13, 10), (16, 3)]         # (factors, bins); 64 // bins factors are walked together


def capacity():
    from smartpy_amd import engine
    return engine.pawn_lds_capacity()


def launch(y, cat, B, method=AUTO, pad=3, spare=1, ws_steps=None):
    """The C entry on a [R, N] host matrix laid out with ld = N + pad (the padding holds NaN) -> (ks [R + spare, P, B],
    counts [P + spare, B]); the spare rows as they were before the call: SENTINEL.  The workspace is what the helper entry asks
    for, or exactly `ws_steps` steps."""
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    R, N = np.shape(y)
    P = len(cat)
    d_y, ld = padded(y, pad)
    d_cat = torch.from_numpy(np.array(cat, dtype=np.uint8)).cuda()         # (a copy: the shared case is read-only)
    ks, counts = filled((R + spare, P, B)), filled((P + spare, B), 'int32')
    need = int(L.smart_pawn_workspace_bytes(N, R, method))
    if ws_steps is not None:
        need = ws_steps * int(L.smart_pawn_workspace_bytes(N, 1, method))
    need = max(need, 0)         # (sizes the helper refuses: the entry refuses them too, with its text)
    work = workspace(need, least=1)
    _lib.check(L.smart_pawn_ks_hip(N, R, d_y.data_ptr(), ld, d_cat.data_ptr(), P, B, ks.data_ptr(), counts.data_ptr(),
                                   method, work.data_ptr(), need,
                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return ks.cpu().numpy(), counts.cpu().numpy()


def nan_bits(a):
    """every NaN the one quiet NaN of numpy: the statement's NaN and the kernel's are both 0x7ff8000000000000, and this says
    so where they are compared"""
    assert (a.view(np.uint64)[np.isnan(a)] == np.uint64(0x7ff8000000000000)).all()
    return a


def values(rng, N, which):
    flows = np.exp(rng.normal(0.0, 2.0, size=(5, N)))
    if which == 'ties':
        y = flows[:4].copy()
        y[1] = rng.integers(0, 16, size=N)
        if N >= 2:
            y[1, N // 2:] = y[1, :N - N // 2]                  # duplicated columns
        y[2] = 3.25                                            # one run
        zero = rng.random(N) < 0.5
        y[3] = np.where(zero, np.where(rng.random(N) < 0.5, -0.0, 0.0), rng.normal(0.0, 1.0, size=N))
        y[3, 0], y[3, N - 1] = -0.0, 0.0
    else:
        y = flows
        y[1, N // 3] = np.nan
        y[2, N - 1] = np.inf
        y[3, 0] = -np.inf
    return y


def categories(rng, N, P, B, ranks_of):
    cat = rng.integers(0, B, size=(P, N)).astype(np.uint8)
    if B == 1:
        return cat                                              # one bin that holds every row
    cat[0, rng.random(N) < 0.1] = 255
    cat[0, 0] = 255
    if P > 1:                                                   # an empty bin and a bin of a single row
        cat[1][cat[1] == 1] = 0
        cat[1][cat[1] == 2] = 0
        cat[1, N // 2] = 2
    if P > 2:
        cat[2] = 255
    if P > 3:                                                   # the bins are the ranks of the first row's values
        rank = np.argsort(np.argsort(ranks_of, kind='stable'), kind='stable')
        cat[3] = np.minimum(B - 1, rank * B // N)
    if P > 4:
        cat[4, ::3] = B                                         # beyond the bins: as good as 255
    return cat


@functools.lru_cache(maxsize=None)
def case(N, table, which):
    """(y, cat, B, the statement's ks, its counts) -- made once, shared by every test that launches it, never written to"""
    P, B = TABLES[table]
    rng = np.random.default_rng(7000 + 10 * N + table)
    y = values(rng, N, which)
    cat = categories(rng, N, P, B, y[0])
    ks, counts = pawn_statement(y, np.where(cat >= B, 255, cat), B)
    for a in (y, cat, ks, counts):
        a.setflags(write=False)
    return y, cat, B, nan_bits(ks), counts


def check(N, method, table, which):
    y, cat, B, want_ks, want_counts = case(N, table, which)
    R, P = len(y), len(cat)
    ks, counts = launch(y, cat, B, method)
    where = (N, method, TABLES[table], which)
    assert (counts[:P] == want_counts).all() and (counts[P:] == SENTINEL).all(), where
    assert same_bits(nan_bits(ks[:R]), want_ks), (where, np.argwhere(~((ks[:R] == want_ks) | np.isnan(want_ks)))[:5])
    assert (ks[R:] == SENTINEL).all(), where
    return ks[:R]


SIZES = ['1', '2', '63', '64', '65', '257', '1000', '1024', '1025', '2048', '2049', '4096', '4097', 'cap-1', 'cap']
CASES = [(s, AUTO) for s in SIZES] + [('1000', GLOBAL), ('cap', GLOBAL), ('cap', LDS), ('cap+1', GLOBAL), ('cap+1', AUTO),
                                      ('20000', GLOBAL), ('20000', AUTO)]


@pytest.mark.parametrize('size,method', CASES, ids=['%s-%s' % (s, ('auto', 'lds', 'global')[m]) for s, m in CASES])
def test_against_the_statement(size, method):
    N = eval(size, {'cap': capacity()})
    for table, (P, B) in enumerate(TABLES):
        for which in ('ties', 'holes'):
            ks = check(N, method, table, which)
            y, cat, _, want, counts = case(N, table, which)
            if which == 'holes':
                assert np.isnan(ks[1:4]).all() and not np.isnan(ks[0, 0, counts[0] > 0]).any()
                assert not np.isnan(ks[4, 0, counts[0] > 0]).any()
                continue
            assert (ks[2][:, :][np.broadcast_to(counts > 0, ks[2].shape)] == 0.0).all()         # the row of equal values
            assert same_bits(np.isnan(ks[0]), counts == 0)                                      # NaN exactly where n_b == 0
            if B == 1:
                assert (ks == 0.0).all() and counts.tolist() == [[N]] * P
            if P > 2:
                assert np.isnan(ks[:, 2]).all() and (counts[2] == 0).all()                      # the factor of 255 alone
            if P > 1 and N >= 3:
                assert counts[1, 1] == 0 and counts[1, 2] == 1
            if P > 3 and N % B == 0:
                assert ks[0, 3, 0] == ks[0, 3, B - 1] == (B - 1) / B and (ks[0, 3] <= (B - 1) / B).all()
    if size == 'cap' and method == GLOBAL:
        # both forms: the same bytes (each equals the statement; said once more, directly)
        for table in range(len(TABLES)):
            y, cat, B, _, _ = case(N, table, 'ties')
            a, b = launch(y, cat, B, LDS), launch(y, cat, B, GLOBAL)
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.parametrize('size', ['1000', 'cap+1', '20000'])
def test_the_same_bytes_from_every_launch_and_every_workspace(size):
    N = eval(size, {'cap': capacity()})
    for table in (0, 3):
        y, cat, B, want, _ = case(N, table, 'ties')
        R = len(y)
        first = launch(y, cat, B, AUTO)
        again = launch(y, cat, B, AUTO)
        assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])
        for steps in (1, 2, R):
            got = launch(y, cat, B, GLOBAL, ws_steps=steps)
            assert same_bits(got[0], first[0]) and same_bits(got[1], first[1]), (N, table, steps)
        plain = launch(y, cat, B, AUTO, pad=0, spare=0)
        assert same_bits(plain[0], first[0][:R]) and same_bits(nan_bits(plain[0]), want)


def test_the_workspace_must_hold_a_step():
    from smartpy_amd._lib import SmartEngineError
    y, cat, B, _, _ = case(1000, 3, 'ties')
    with pytest.raises(SmartEngineError, match='workspace_bytes 0, need 49152') as err:
        launch(y, cat, B, GLOBAL, ws_steps=0)
    assert err.value.code == -2
    with pytest.raises(SmartEngineError, match='the LDS form takes at most 8192 samples, not 8193') as err:
        launch(np.zeros((1, 8193)), np.zeros((1, 8193), dtype=np.uint8), 1, LDS)
    assert err.value.code == -2


# ---- the engine and MonteCarlo on top ---------------------------------------------------------------------------------
def test_engine_against_the_c_entry():
    import torch
    from smartpy_amd import engine
    N = 1000
    y, cat, B, want, want_counts = case(N, 3, 'ties')
    y, cat = np.array(y), np.array(cat)                    # (copies: the shared case is read-only)
    R, P = len(y), len(cat)
    wide = torch.from_numpy(np.concatenate([y, np.full((R, 9), np.nan)], axis=1)).cuda()
    view = wide[:, :N]                                      # a matrix with a leading dimension of its own
    assert view.stride(0) == N + 9
    for method in ('auto', 'lds', 'global'):
        res = engine.pawn_ks(view, cat, B, method=method)
        assert res.ks.is_cuda and res.ks.shape == (R, P, B) and res.ks.dtype == torch.float64
        assert res.counts.is_cuda and res.counts.shape == (P, B) and res.counts.dtype == torch.int32
        ks, counts = res.numpy()
        assert same_bits(nan_bits(ks), want) and same_bits(counts, want_counts)
    res = engine.pawn_ks(y, torch.from_numpy(cat).cuda(), B)      # a host matrix, a device table
    assert same_bits(res.ks.cpu().numpy(), want)
    with pytest.raises(engine.SmartEngineError, match='n_bins 65 must be in 1 .. 64'):
        engine.pawn_ks(view, cat, 65)
    with pytest.raises(engine.SmartEngineError, match='n_factors 17 must be in 1 .. 16'):
        engine.pawn_ks(view, np.zeros((17, N), dtype=np.uint8), 4)


def test_a_planted_parameter_is_the_influential_one():
    """ten factors drawn independently; rows 0 .. 19 of the matrix depend on factor 3 alone (plus a little noise), the
    others on nothing: there, and only there, factor 3 lies above the dummy factors"""
    from smartpy_amd import engine, pawn
    rng = np.random.default_rng(5)
    N, R, P, B, D = 3000, 40, 10, 10, 3
    theta = rng.uniform(0.0, 1.0, size=(N, P))
    y = rng.normal(0.0, 1.0, size=(R, N))
    y[:20] = np.sin(3.0 * theta[:, 3])[None, :] + 0.05 * y[:20]
    cat = np.concatenate([pawn.bin_table(theta, [(0.0, 1.0)] * P, B), pawn.dummy_table(N, B, D, seed=1)])
    ks, counts = engine.pawn_ks(y, cat, B).numpy()
    index = pawn.pawn_indices(ks, counts, 'median', min_count=pawn.default_min_count(N, B))
    dummy = index[:, P:].max(axis=1)
    assert (index[:20, 3] > 0.3).all() and (index[:20, 3] > 4 * dummy[:20]).all()
    assert (np.delete(index[:, :P], 3, axis=1) < 0.12).all() and (index[20:, 3] < 0.12).all()
    assert (dummy < 2 * pawn.critical_value(N, N // B)).all()


def test_lhs_pawn_sensitivity_end_to_end(tmp_path):
    from smartpy_amd.montecarlo import LHS
    from smartpy_amd import identifiability as ident, pawn
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sampling.sttngs', '01/01/2007', '31/12/2007', 180)
    np.random.seed(2024)
    lhs = LHS('Catchment', root, 'csv', 'csv', sample_size=300, settings_filename='Catchment.sampling.sttngs')
    lhs.model.extra = EXTRA
    res = lhs.pawn_sensitivity(of='discharge', bins=5, write=True)
    R, P, D, N = len(lhs.model.timeseries_report) - 1, 10, 3, 300
    assert res.names == lhs.param_names and res.datetime == lhs.model.timeseries_report[1:] and len(res.names) == P
    assert res.ks.shape == (R, P + D, 5) and res.counts.shape == (P + D, 5) and res.categories.shape == (P + D, N)
    assert (res.bins, res.dummies, res.statistic, res.min_count) == (5, D, 'median', 15)
    # the categories the method used: the bins of the sample on the ranges it was drawn from, then the dummy factors
    assert np.array_equal(res.categories[:P], ident.bin_table(lhs._sample, ident._ranges(lhs.model.parameters.ranges,
                                                                                         res.names), 5))
    assert np.array_equal(res.categories[P:], pawn.dummy_table(N, 5, D, 0))
    assert (res.counts.sum(axis=1) == N).all() and (res.counts[P:] == N // 5).all()
    # ks: the statement on the discharge of the same launch and those categories, bit for bit
    out = lhs.model.simulate_ensemble(lhs._sample, save_discharge=True, math_mode=lhs.math_mode)
    discharge = out.discharge_report_major.cpu().numpy()
    want, want_counts = pawn_statement(discharge, res.categories, 5)
    assert same_bits(nan_bits(res.ks), nan_bits(want)) and same_bits(res.counts, want_counts)
    assert same_bits(res.device_ks.cpu().numpy(), res.ks) and np.isfinite(res.ks).all()
    # index, dummy and influential: pawn_indices on that ks
    index = pawn.pawn_indices(res.ks, res.counts, 'median', 15)
    assert same_bits(res.index, index[:, :P]) and same_bits(res.dummy, index[:, P:].max(axis=1))
    assert np.array_equal(res.influential, res.index > res.dummy[:, None]) and res.influential.any()
    # the file: R lines of P + 2 columns
    assert res.file == lhs.pawn_file == os.path.join(lhs.model.out_f, 'Catchment.SMART.lhs.pawn')
    lines = open(res.file).read().split('\n')
    assert lines[0] == 'DateTime,' + ','.join(res.names) + ',dummy' and len(lines) == R + 2 and lines[-1] == ''
    assert all(len(ln.split(',')) == P + 2 for ln in lines[:-1])
    assert [ln.split(',')[0] for ln in lines[1:-1]] == [str(dt) for dt in res.datetime]
    assert lines[1].split(',')[1:] == ['%.6e' % v for v in res.index[0]] + ['%.6e' % res.dummy[0]]
    # the scores of every row as the outputs; nothing is written unless asked for
    obj = lhs.pawn_sensitivity(of='objective_functions', bins=5, statistic='max', dummies=2, seed=3, min_count=1,
                               method='global')
    table = lhs._score_table().cpu().numpy()
    assert table.shape == (8, N) and obj.datetime == ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE', 'GW_RATIO']
    assert obj.file is None and obj.ks.shape == (8, P + 2, 5) and np.array_equal(obj.categories[P:], pawn.dummy_table(N, 5, 2, 3))
    want, _ = pawn_statement(table, obj.categories, 5)
    assert same_bits(nan_bits(obj.ks), nan_bits(want))
    assert same_bits(obj.index, pawn.pawn_indices(obj.ks, obj.counts, 'max', 1)[:, :P])
    # an array of the caller's, other ranges
    wide = dict(lhs.model.parameters.ranges, T=(0.5, 1.5))
    own = lhs.pawn_sensitivity(of=discharge[:3], bins=5, dummies=0, ranges=wide)
    assert own.datetime == [0, 1, 2] and own.dummies == 0 and np.isnan(own.dummy).all() and not own.influential.any()
    assert (own.counts[0, [0, 1, 3, 4]] == 0).all() and own.counts[0, 2] == N     # T was drawn from (0.9, 1.1): the middle bin
    assert (own.ks[:, 0, 2] == 0.0).all() and np.isnan(own.ks[:, 0, [0, 1, 3, 4]]).all()
    assert same_bits(own.ks[:, 1:], res.ks[:3, 1:P])
    # no row (a GLUE without a behavioural set): everything NaN, nothing is launched, the file still has its lines
    lhs._set_sample(np.empty((0, P)))
    empty = lhs.pawn_sensitivity(bins=5, write=True)
    assert empty.ks.shape == (R, P + D, 5) and np.isnan(empty.ks).all() and np.isnan(empty.index).all()
    assert (empty.counts == 0).all() and empty.device_ks is None and not empty.influential.any()
    assert len(open(empty.file).read().split('\n')) == R + 2
