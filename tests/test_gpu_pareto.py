"""smart_pareto_counts_hip on the GPU against the numpy statement of oracle/analyses/pareto.py.  The results are
integers: every comparison is exact equality of int32 arrays, no tolerance anywhere.

Launch conditions (launch below): the score matrix has C = M + 2 columns of which M are selected, in an order that is not
ascending, NaN in the two that are not, ld = C + 3 with NaN in the padding; dominated_by lies support.GUARD integers inside a
buffer of sentinels whose guards are checked; every launch is made twice and the two answers compared.

Shapes stand on both sides of every switch the implementation has: the wavefront (63 / 64 / 65 rows), the workgroup of
256 candidates (255 / 256 / 257; 1,023 / 1,025), the four instances of the pair kernel (M = 1, 2 | 3, 4 | 5, 8 | 9, 16),
their loop trips of 8, 4, 2, 1 challengers with a ragged end, and the slices of the challenger range: S = min(16, ceil(E /
64)) slices of L = ceil(E / S) rounded up to a multiple of 8, so E = 64 is one slice and 65 two; E = 1,023 (L = 64) has a
last slice of 63 challengers; E = 1,025 (L = 72) has 17 challengers in slice 14 and NONE in slice 15.  E is the number of
rows that take part: the cases that aim at a slice boundary run with eligible=None and without NaN, where E = N."""
import os

import numpy as np
import pytest

from oracle.analyses.pareto import pareto_statement, pareto_rank_statement, pareto_keys, dominance_counts
from support import EXTRA, Guarded, example_root, padded, settings_file, to_device, ptr

pytestmark = pytest.mark.gpu

SENTINEL = -77
WGUARD = 256         # bytes around the workspace (its parts stay on the boundaries the kernels' wide loads like)
WORDS = ['max', 'min', ('target', 0.5)]
CODES = {'max': 0, 'min': 1, 'target': 2}


def directions(M):
    return [WORDS[m % 3] for m in range(M)]


def columns_of(M):
    """M of the M + 2 columns, not in ascending order"""
    return [(3 * m + 1) % (M + 2) for m in range(M)] if (M + 2) % 3 else list(range(M + 1, 1, -1))


def make_scores(seed, N, M, nan=0.03, ineligible=0.10):
    """seeded normal scores in the selected columns, NaN elsewhere; a share of the rows gets a NaN in one selected
    column, a share is ineligible -> (scores [N, M + 2], columns, eligible uint8 [N] or None)"""
    rng = np.random.default_rng(seed)
    cols = columns_of(M)
    assert len(set(cols)) == M and max(cols) < M + 2
    scores = np.full((N, M + 2), np.nan)
    scores[:, cols] = rng.standard_normal((N, M))
    if nan:
        hit = np.nonzero(rng.random(N) < nan)[0]
        scores[hit, np.asarray(cols)[rng.integers(0, M, hit.size)]] = np.nan
    eligible = (rng.random(N) >= ineligible).astype(np.uint8) if ineligible else None
    return scores, cols, eligible


def launch(scores, words, cols, eligible=None, pad=3, twice=True):
    """The C entry on a host matrix laid out with ld = C + pad (NaN in the padding) -> int32 [N]."""
    import ctypes
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    N, C = scores.shape
    M = len(words)
    d_s, ld = padded(scores, pad)
    d_e = to_device(eligible, np.uint8)
    code = (ctypes.c_int32 * M)(*[CODES[w[0] if isinstance(w, tuple) else w] for w in words])
    target = (ctypes.c_double * M)(*[w[1] if isinstance(w, tuple) else float('nan') for w in words])
    col = (ctypes.c_int32 * M)(*cols)
    need = int(L.smart_pareto_workspace_bytes(N, M))
    assert need > 0
    answers = []
    for _ in range(2 if twice else 1):
        work = Guarded(need, dtype='uint8', guard=WGUARD, sentinel=0x5a)
        buf = Guarded(N, dtype='int32', sentinel=SENTINEL)              # (GUARD int32 entries around dominated_by)
        rc = L.smart_pareto_counts_hip(N, d_s.data_ptr(), ld, col, code, target, M, ptr(d_e), buf.ptr(), work.ptr(), need,
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _lib.check(rc)
        (counts, around_counts), (_, around_work) = buf.read(), work.read()
        assert around_counts and around_work
        answers.append(counts.copy())
    if twice:
        assert np.array_equal(answers[0], answers[1])
    assert answers[0].dtype == np.int32
    return answers[0]


def check(scores, words, cols, eligible, what):
    got = launch(scores, words, cols, eligible)
    want = pareto_statement(scores, words, None, cols, eligible)
    part = want >= 0
    print('%s: %d rows, %d take part, %d on the front, largest count %d'
          % (what, len(want), part.sum(), (want == 0).sum(), want.max(initial=-1)))
    assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:10])
    return want


@pytest.mark.parametrize('N,M', [(1, 1), (2, 2), (63, 3), (64, 4), (65, 5), (255, 8), (256, 9), (257, 16), (1023, 2),
                                 (1025, 7), (4097, 16), (1000, 2), (4097, 4), (1025, 1)])
def test_counts_with_nan_and_ineligible_rows(N, M):
    scores, cols, eligible = make_scores(100 * N + M, N, M)
    want = check(scores, directions(M), cols, eligible, 'N %d M %d' % (N, M))
    if N >= 1000:       # such inputs give answers that are not trivial
        assert 0 < (want == 0).sum() < (want >= 0).sum() < N and (want == -1).sum() > 0


@pytest.mark.parametrize('M', [1, 2, 3, 4, 5, 8, 9, 16])
@pytest.mark.parametrize('N', [64, 65, 1023, 1025])
def test_slice_boundaries_where_every_row_takes_part(N, M):
    """E = N: one slice / two; a ragged last slice (1,023); a ragged slice 14 and an empty slice 15 (1,025) -- in every
    instance and on both sides of it"""
    scores, cols, _ = make_scores(7 * N + M, N, M, nan=0.0, ineligible=0.0)
    want = check(scores, directions(M), cols, None, 'E = N = %d, M %d' % (N, M))
    assert (want >= 0).all()


def test_one_of_the_two_alone():
    """eligible=None with NaN rows, and an eligible mask without any NaN"""
    scores, cols, eligible = make_scores(11, 1025, 3, ineligible=0.0)
    want = check(scores, directions(3), cols, eligible, 'NaN only')
    assert eligible is None and (want == -1).sum() > 0
    scores, cols, eligible = make_scores(12, 1025, 3, nan=0.0)
    want = check(scores, directions(3), cols, eligible, 'eligible only')
    assert np.array_equal(want == -1, eligible == 0)


def test_ties():
    rng = np.random.default_rng(5)
    # scores rounded to halves, M = 2: many equal keys in one column, equal rows among them
    scores, cols, eligible = make_scores(21, 1000, 2)
    scores = np.round(scores * 2.0) / 2.0
    keys = scores[:, cols][~np.isnan(scores[:, cols]).any(axis=1)]
    assert len(np.unique(keys, axis=0)) < len(keys)
    check(scores, ['max', 'min'], cols, eligible, 'halves')
    check(scores, ['max', ('target', 0.5)], cols, None, 'halves, a target between two of them')
    # 5 % of the rows copied verbatim over other rows: a front with duplicates keeps them all
    scores, cols, _ = make_scores(22, 1025, 3, nan=0.0)
    src, dst = rng.integers(0, 1025, 51), rng.integers(0, 1025, 51)
    scores[dst] = scores[src]
    want = check(scores, directions(3), cols, None, 'copied rows')
    on_front = scores[want == 0][:, cols]
    assert len(np.unique(on_front, axis=0)) < len(on_front)
    # every row the same: nobody dominates anybody
    same = np.tile(scores[:1], (300, 1))
    assert (check(same, directions(3), cols, None, 'identical rows') == 0).all()
    # nobody takes part
    assert (check(scores, directions(3), cols, np.zeros(1025, dtype=np.uint8), 'no eligible row') == -1).all()
    # signed zeros and infinities
    scores, cols, _ = make_scores(23, 257, 2, nan=0.0, ineligible=0.0)
    scores[::5, cols[0]] = 0.0
    scores[1::5, cols[0]] = -0.0
    scores[::7, cols[1]] = np.inf
    scores[3::7, cols[1]] = -np.inf
    check(scores, ['max', 'min'], cols, None, 'zeros and infinities')
    check(scores, [('target', 0.0), ('target', 0.5)], cols, None, 'zeros and infinities against targets')


@pytest.mark.parametrize('word', ['max', 'min'])
def test_counts_beyond_sixteen_bits(word):
    """N = 70,001, M = 1, integer-valued scores with ties: the truth is the number of strictly greater keys, from a sort"""
    N = 70001
    scores = np.random.default_rng(3).integers(0, 20000, N).astype(np.float64)[:, None]
    got = launch(scores, [word], [0])
    keys = np.sort(scores[:, 0] if word == 'max' else -scores[:, 0])
    want = (N - np.searchsorted(keys, scores[:, 0] if word == 'max' else -scores[:, 0], side='right')).astype(np.int32)
    assert want.max() > 65536 and (want == 0).sum() >= 1
    assert np.array_equal(got, want)


def test_compaction_does_not_depend_on_where_the_rows_lie():
    """N = 4,097 with 2 % of the rows eligible: E^2 pairs, and the same rows at other places give the same counts"""
    N, M = 4097, 5
    scores, cols, _ = make_scores(31, N, M, ineligible=0.0)
    rng = np.random.default_rng(32)
    eligible = (rng.random(N) < 0.02).astype(np.uint8)
    want = check(scores, directions(M), cols, eligible, '2 % eligible')
    assert 40 < (want >= 0).sum() < 130
    perm = rng.permutation(N)
    moved = check(scores[perm], directions(M), cols, eligible[perm], 'the same rows, permuted')
    assert np.array_equal(moved, want[perm])
    front_only = np.zeros(N, dtype=np.uint8)        # the front alone: every one of its rows stays on it
    front_only[want == 0] = 1
    again = check(scores, directions(M), cols, front_only, 'the front alone')
    assert np.array_equal(again == 0, want == 0)


def test_ranks():
    import torch
    from smartpy_amd import engine
    scores, cols, eligible = make_scores(41, 1000, 2)
    want = pareto_rank_statement(scores, directions(2), None, cols, eligible, max_rank=None)
    got = engine.pareto_ranks(scores, directions(2), columns=cols, eligible=eligible, max_rank=None)
    assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    print('N 1000 M 2: %d fronts, %d rows on the first' % (want.max(), (want == 1).sum()))
    assert want.max() > 10 and (want != 0).all()                    # every row that takes part is ranked, once
    counts = engine.pareto_counts(scores, directions(2), columns=cols, eligible=eligible).cpu().numpy()
    assert np.array_equal(counts, pareto_statement(scores, directions(2), None, cols, eligible))
    assert np.array_equal(want == 1, counts == 0) and np.array_equal(want == -1, counts == -1)
    # three fronts of three objectives, on a device matrix with a leading dimension of its own (NaN beside it) ...
    scores, cols, eligible = make_scores(42, 1000, 3)
    as32 = scores.astype(np.float32).astype(np.float64)
    wide = torch.full((1000, 9), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :5] = torch.from_numpy(as32).cuda()
    view = wide[:, :5]
    assert view.stride(0) == 9
    want = pareto_rank_statement(as32, directions(3), None, cols, eligible, max_rank=3)
    got = engine.pareto_ranks(view, directions(3), columns=cols, eligible=torch.from_numpy(eligible).cuda(), max_rank=3)
    assert np.array_equal(got.cpu().numpy(), want) and sorted(set(want.tolist())) == [-1, 0, 1, 2, 3]
    # ... and on float32, host and device: widened exactly
    for single in (scores.astype(np.float32), torch.from_numpy(scores.astype(np.float32)).cuda()):
        first = engine.pareto_ranks(single, directions(3), columns=cols, eligible=eligible)
        assert np.array_equal(first.cpu().numpy(), np.where(want > 1, 0, want))
    # 'target' with its value in targets=, one column [N]
    one = engine.pareto_counts(scores[:, cols[2]], ['target'], targets=[0.5]).cpu().numpy()
    assert np.array_equal(one, pareto_statement(scores[:, cols[2]], [('target', 0.5)]))


def test_pareto_rows_from_numpy_and_from_a_device_tensor():
    import torch
    from smartpy_amd.montecarlo.selection import pareto_rows
    rng = np.random.default_rng(51)
    fns = np.round(rng.standard_normal((500, 3)), 1)        # ties
    fns[rng.random(500) < 0.03, 1] = np.nan
    allowed = rng.random(500) < 0.8
    words = ['max', ('target', 0.0), 'min']
    want = pareto_rank_statement(fns, words, eligible=allowed, max_rank=2)
    order = np.array(sorted(np.nonzero(want > 0)[0], key=lambda r: (want[r], r)))
    rows, ranks = pareto_rows(fns, words, allowed, max_rank=2)
    assert isinstance(rows, np.ndarray) and np.array_equal(rows, order) and np.array_equal(ranks, want[order])
    assert set(ranks.tolist()) == {1, 2}
    d_rows, d_ranks = pareto_rows(torch.from_numpy(fns).cuda(), words, torch.from_numpy(allowed).cuda(), max_rank=2)
    assert d_rows.is_cuda and np.array_equal(d_rows.cpu().numpy(), order) and np.array_equal(d_ranks.cpu().numpy(), ranks)
    everything, _ = pareto_rows(fns, words, max_rank=None)
    assert len(everything) == int((~np.isnan(fns).any(axis=1)).sum())


def test_pareto_end_to_end(tmp_path):
    from datetime import datetime
    from smartpy_amd.montecarlo import LHS, Pareto
    from smartpy_amd.montecarlo.selection import as_stored
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sampling.sttngs', '01/01/2007', '30/09/2007', 90)
    settings_file(root, 'Catchment.evaluating.sttngs', '01/01/2008', '31/03/2008', 30)
    np.random.seed(2025)
    lhs = LHS('Catchment', root, 'csv', 'csv', sample_size=256, settings_filename='Catchment.sampling.sttngs')
    lhs.model.extra = EXTRA
    lhs.run()
    names = ['NSE', 'PBias', 'RMSE']
    kw = dict(objectives=names, settings_filename='Catchment.evaluating.sttngs')
    dev = Pareto('Catchment', root, 'csv', 'csv', sampling=lhs, **kw)
    fil = Pareto('Catchment', root, 'csv', 'csv', **kw)
    assert dev.directions == ['max', ('target', 0.0), 'min'] == fil.directions
    assert np.array_equal(dev.pareto_index, fil.pareto_index) and np.array_equal(dev.pareto_rank, fil.pareto_rank)
    assert dev.pareto_params.dtype == np.float32 and dev.pareto_params.tobytes() == fil.pareto_params.tobytes()
    assert np.array_equal(dev.pareto_obj_fns, fil.pareto_obj_fns, equal_nan=True)
    stored = as_stored(lhs.obj_fns).astype(np.float64)
    cols = [lhs.obj_fn_names.index(n) for n in names]
    want = pareto_statement(stored, dev.directions, None, cols)
    n = int((want == 0).sum())
    print('Pareto set of NSE, |PBias|, RMSE: %d of 256 rows' % n)
    assert 1 < n < 256 and np.array_equal(dev.pareto_index, np.nonzero(want == 0)[0]) and (dev.pareto_rank == 1).all()
    assert dev._sample.shape == (n, 10) and np.array_equal(dev._sample, dev.pareto_params.astype(np.float64))
    # no selected row is dominated by any row of the sample: brute force, row by row
    keys = pareto_keys(stored, dev.directions, None, cols)
    for r in dev.pareto_index:
        ge, le = (keys >= keys[r]).all(axis=1), (keys <= keys[r]).all(axis=1)
        assert not (ge & ~le).any(), r
    dev.model.extra = EXTRA
    dev.run()
    path = os.path.join(root, 'out', 'Catchment', 'Catchment.SMART.pareto')
    assert os.path.normpath(dev.db_file) == path
    table = np.loadtxt(path, delimiter=',', skiprows=1, ndmin=2)
    assert table.shape == (n, 8 + 10) and np.array_equal(table[:, 8:].astype(np.float32), dev.pareto_params)
    # two fronts, in the documented order; a conditioning that leaves a part, and one that leaves nothing
    two = Pareto('Catchment', root, 'csv', 'csv', max_rank=2, sampling=lhs, **kw)
    ranks = pareto_rank_statement(stored, dev.directions, None, cols, max_rank=2)
    order = np.array(sorted(np.nonzero(ranks > 0)[0], key=lambda r: (ranks[r], r)))
    assert np.array_equal(two.pareto_index, order) and np.array_equal(two.pareto_rank, ranks[order])
    level = float(np.sort(stored[:, 0])[128])           # (a value of the sample: the same number in float32)
    cond = {'NSE': ('max', (level,))}                   # the worse half by NSE, as GLUE reads 'max': value <= level
    for half in (Pareto('Catchment', root, 'csv', 'csv', conditioning=cond, sampling=lhs, **kw),
                 Pareto('Catchment', root, 'csv', 'csv', conditioning=cond, **kw)):
        want_half = pareto_statement(stored, dev.directions, None, cols, as_stored(lhs.obj_fns)[:, 0] <= np.float32(level))
        assert np.array_equal(half.pareto_index, np.nonzero(want_half == 0)[0]) and len(half.pareto_index) > 0
    none = Pareto('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (2.0,))}, sampling=lhs, **kw)
    assert none.pareto_index.shape == (0,) and none.pareto_params.shape == (0, 10)
    none.run()
    lines = open(path).read().splitlines()
    assert len(lines) == 1 and lines[0].startswith('NSE,')
    # calibration-period KGE against validation-period KGE: two periods of the sampling run itself
    win = lhs.window_objective_functions('split', split=datetime(2007, 7, 1))
    assert len(win.labels) == 2 and tuple(win.device_values.shape) == (2, 256, 7)
    extra = {'KGE@calibration': (win.device_values[0, :, 1], 'max'), 'KGE@validation': (win.device_values[1, :, 1], 'max')}
    both = Pareto('Catchment', root, 'csv', 'csv', objectives={'PBias': ('target', 0.0)}, sampling=lhs, extra=extra,
                  settings_filename='Catchment.evaluating.sttngs')
    joined = np.concatenate([stored[:, [5]], win.values[0][:, [1]], win.values[1][:, [1]]], axis=1)
    want = pareto_statement(joined, [('target', 0.0), 'max', 'max'])
    assert both.objective_names == ['PBias', 'KGE@calibration', 'KGE@validation']
    assert np.array_equal(both.pareto_index, np.nonzero(want == 0)[0]) and 0 < len(both.pareto_index) < 256
    host = {k: (v[0].cpu().numpy(), v[1]) for k, v in extra.items()}
    from_file = Pareto('Catchment', root, 'csv', 'csv', objectives={'PBias': ('target', 0.0)}, extra=host,
                       settings_filename='Catchment.evaluating.sttngs')
    assert np.array_equal(from_file.pareto_index, both.pareto_index)
