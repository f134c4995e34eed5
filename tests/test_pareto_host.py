"""Pareto selection without a device: the numpy statement of the dominance counts and ranks (oracle/analyses/pareto.py, the
truth of tests/test_gpu_pareto.py) on hand-worked cases written as literals, every refusal of the two new C entries as
(return code, text) literals, and the refusals of the Python layer that come before any device call."""
import ctypes
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle.analyses.pareto import pareto_keys, pareto_rank_statement, pareto_statement
from support import E_MODE, E_NULL, E_SIZE, FAKE, example_root, refusal, settings_file

NAN, INF = float('nan'), float('inf')


# ---- hand-worked cases -----------------------------------------------------------------------------------------------
SIX = [[1.0, 5.0], [2.0, 4.0], [3.0, 3.0], [2.0, 2.0], [1.0, 1.0], [3.0, 1.0]]


def test_six_points_two_objectives():
    # (1,5), (2,4), (3,3) beat nobody among themselves; (2,2) loses to (2,4) and (3,3); (1,1) to everybody; (3,1) to (3,3)
    assert pareto_statement(SIX, ['max', 'max']).tolist() == [0, 0, 0, 2, 5, 1]
    assert pareto_rank_statement(SIX, ['max', 'max'], max_rank=None).tolist() == [1, 1, 1, 2, 3, 2]
    assert pareto_rank_statement(SIX, ['max', 'max'], max_rank=1).tolist() == [1, 1, 1, 0, 0, 0]
    assert pareto_rank_statement(SIX, ['max', 'max'], max_rank=2).tolist() == [1, 1, 1, 2, 0, 2]


def test_six_points_min_and_target():
    # keys (-x, -|y - 0.5|): (-1,-4.5) (-2,-3.5) (-3,-2.5) (-2,-1.5) (-1,-0.5) (-3,-0.5); row 4 is best in both
    want = [1, 2, 3, 1, 0, 1]
    assert pareto_statement(SIX, ['min', ('target', 0.5)]).tolist() == want
    assert pareto_statement(SIX, ['min', 'target'], targets=[0.0, 0.5]).tolist() == want
    assert pareto_keys(SIX, ['min', ('target', 0.5)]).tolist() == [[-1.0, -4.5], [-2.0, -3.5], [-3.0, -2.5], [-2.0, -1.5],
                                                                     [-1.0, -0.5], [-3.0, -0.5]]
    # the same through columns= on a wider matrix whose other columns hold NaN: they are never looked at
    wide = np.full((6, 4), NAN)
    wide[:, 3], wide[:, 1] = np.array(SIX)[:, 0], np.array(SIX)[:, 1]
    assert pareto_statement(wide, ['min', ('target', 0.5)], columns=[3, 1]).tolist() == want


def test_duplicates_stay_on_the_front():
    assert pareto_statement([[1.0, 2.0]] * 3, ['max', 'max']).tolist() == [0, 0, 0]
    assert pareto_statement([[1.0, 2.0]] * 3 + [[0.0, 0.0]], ['max', 'max']).tolist() == [0, 0, 0, 3]
    assert pareto_statement([[1.0, 2.0], [1.0, 2.0], [2.0, 2.0]], ['max', 'max']).tolist() == [1, 1, 0]
    assert pareto_rank_statement([[1.0, 2.0]] * 3 + [[0.0, 0.0]], ['max', 'max'], max_rank=None).tolist() == [1, 1, 1, 2]


def test_a_strict_chain_in_one_objective():
    chain = np.arange(7.0)
    assert pareto_statement(chain, ['max']).tolist() == [6, 5, 4, 3, 2, 1, 0]
    assert pareto_statement(chain, ['min']).tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert pareto_statement(chain, [('target', 3.0)]).tolist() == [5, 3, 1, 0, 1, 3, 5]
    assert pareto_rank_statement(chain, ['min'], max_rank=None).tolist() == [1, 2, 3, 4, 5, 6, 7]


def test_nan_eligible_infinities_and_zeros():
    s = [[1.0, 1.0, NAN], [2.0, NAN, 0.0], [0.0, 0.0, NAN], [NAN, 3.0, 0.0]]
    assert pareto_statement(s, ['max', 'max']).tolist() == [0, -1, 1, -1]          # column 2 is not selected
    assert pareto_statement(s, ['max', 'max', 'max']).tolist() == [-1, -1, -1, -1]
    assert pareto_statement(s, ['max'], columns=[0]).tolist() == [1, 0, 2, -1]
    assert pareto_statement(SIX, ['max', 'max'], eligible=[1, 1, 0, 1, 1, 1]).tolist() == [0, 0, -1, 1, 4, 0]
    assert pareto_statement(SIX, ['max', 'max'], eligible=[0] * 6).tolist() == [-1] * 6
    assert pareto_rank_statement(SIX, ['max', 'max'], eligible=[1, 1, 0, 1, 1, 1], max_rank=None).tolist() == \
        [1, 1, -1, 2, 3, 1]
    assert pareto_statement([INF, -INF, 0.0], ['max']).tolist() == [0, 2, 1]
    assert pareto_statement([INF, -INF, 0.0], ['min']).tolist() == [2, 0, 1]
    assert pareto_statement([INF, -INF, 0.0, INF], [('target', 0.0)]).tolist() == [1, 1, 0, 1]   # both keys are -inf
    assert pareto_statement([[0.0, 1.0], [-0.0, 1.0]], ['max', 'min']).tolist() == [0, 0]
    assert pareto_statement([0.0, -0.0, -1.0], ['max']).tolist() == [0, 0, 2]


# ---- the C entries ---------------------------------------------------------------------------------------------------
P = 'smart_pareto_counts_hip'
VALID = dict(n_rows=4, scores=FAKE, ld=3, columns=(0, 2), direction=(0, 2), target=(0.0, 0.5), n_objectives=2,
             eligible=None, dominated_by=FAKE, workspace=FAKE, workspace_bytes=1 << 20, stream=None)
SIXTEEN = tuple(range(16))


def call(changes):
    """support.refusal on the one entry, its two lists of integers as int32 arrays (a tuple left to it becomes doubles)"""
    def arrays(args):
        return {k: (ctypes.c_int32 * len(v))(*v) if k in ('columns', 'direction') and v is not None else v
                for k, v in args.items()}
    return refusal({P: arrays(VALID)}, P, arrays(changes))


CASES = [
    (dict(scores=None), E_NULL, P + ': scores, columns, direction and dominated_by are required (scores is NULL)'),
    (dict(columns=None), E_NULL, P + ': scores, columns, direction and dominated_by are required (columns is NULL)'),
    (dict(direction=None), E_NULL, P + ': scores, columns, direction and dominated_by are required (direction is NULL)'),
    (dict(dominated_by=None), E_NULL,
     P + ': scores, columns, direction and dominated_by are required (dominated_by is NULL)'),
    (dict(n_rows=0), E_SIZE, P + ': n_rows 0 must be in 1 .. 2^31 - 1'),
    (dict(n_rows=-5), E_SIZE, P + ': n_rows -5 must be in 1 .. 2^31 - 1'),
    (dict(n_rows=2 ** 31), E_SIZE, P + ': n_rows 2147483648 must be in 1 .. 2^31 - 1'),
    (dict(n_objectives=0), E_SIZE, P + ': n_objectives 0 must be in 1 .. 16'),
    (dict(n_objectives=17), E_SIZE, P + ': n_objectives 17 must be in 1 .. 16'),
    (dict(columns=(-1, 2)), E_SIZE, P + ': column -1 of objective 0 is outside 0 .. ld - 1 = 2'),
    (dict(columns=(0, 3)), E_SIZE, P + ': column 3 of objective 1 is outside 0 .. ld - 1 = 2'),
    (dict(ld=2), E_SIZE, P + ': column 2 of objective 1 is outside 0 .. ld - 1 = 1'),
    (dict(columns=(2, 2)), E_SIZE, P + ': column 2 is named twice (objectives 0 and 1)'),
    (dict(direction=(0, 3)), E_MODE, P + ": direction '3' of objective 1 unknown."),
    (dict(direction=(-1, 2)), E_MODE, P + ": direction '-1' of objective 0 unknown."),
    (dict(target=None), E_NULL, P + ': objective 1 is a TARGET (target is NULL)'),
    (dict(target=(0.0, NAN)), E_SIZE, P + ': target nan of objective 1 must be finite'),
    (dict(target=(0.0, INF)), E_SIZE, P + ': target inf of objective 1 must be finite'),
    (dict(target=(0.0, -INF)), E_SIZE, P + ': target -inf of objective 1 must be finite'),
    (dict(workspace=None), E_NULL, P + ': a workspace of 1024 bytes is needed (workspace is NULL)'),
    (dict(workspace_bytes=1023), E_SIZE, P + ': workspace_bytes 1023, need 1024'),
    # two rules broken at once: which refusal wins
    (dict(scores=None, n_rows=0), E_NULL,
     P + ': scores, columns, direction and dominated_by are required (scores is NULL)'),
    (dict(n_rows=0, n_objectives=17), E_SIZE, P + ': n_rows 0 must be in 1 .. 2^31 - 1'),
    (dict(columns=(0, 3), direction=(0, 7)), E_SIZE, P + ': column 3 of objective 1 is outside 0 .. ld - 1 = 2'),
    (dict(direction=(0, 7), target=None), E_MODE, P + ": direction '7' of objective 1 unknown."),
    (dict(target=(0.0, NAN), workspace_bytes=0), E_SIZE, P + ': target nan of objective 1 must be finite'),
    # 16 objectives pass the size rule (the workspace is what is missing); a NaN target of a MAX column is not looked at
    (dict(n_objectives=16, ld=16, columns=SIXTEEN, direction=(0,) * 16, target=None, workspace_bytes=0), E_SIZE,
     P + ': workspace_bytes 0, need 1280'),
    (dict(direction=(0, 1), target=(NAN, NAN), workspace_bytes=8), E_SIZE, P + ': workspace_bytes 8, need 1024'),
]


@pytest.mark.parametrize('changes,code,text', CASES, ids=[str(i) for i in range(len(CASES))])
def test_refusals_of_the_entry(changes, code, text):
    assert call(changes) == (code, text)


def test_workspace_bytes_and_the_cap():
    from smartpy_amd import _lib, engine
    L = _lib.lib()
    assert L.smart_pareto_max_objectives() == 16 == engine.pareto_max_objectives() == _lib.PARETO_MAX_OBJECTIVES
    need = L.smart_pareto_workspace_bytes
    for bad in ((0, 2), (-1, 2), (2 ** 31, 2), (4, 0), (4, 17), (4, -3)):
        assert need(*bad) == 0, bad
    sizes = [1, 2, 63, 64, 65, 1000, 100000, 2 ** 31 - 1]
    for m in range(1, 17):
        row = [need(n, m) for n in sizes]
        assert all(a > 0 for a in row) and all(a <= b for a, b in zip(row, row[1:])), m
        assert row[5] < row[6] < row[7]
    for n in sizes:
        col = [need(n, m) for m in range(1, 17)]
        assert all(a <= b for a, b in zip(col, col[1:])), n
    # the keys of a row are padded to 2, 4, 8 or 16 doubles; 4 bytes of list and 16 partial counts per row
    assert need(100000, 16) - need(100000, 8) == 100000 * 8 * 8
    assert need(100000, 7) == need(100000, 8) and need(100000, 2) < need(100000, 3)
    assert need(4, 2) == 1024 and need(100000, 7) >= 100000 * (8 * 8 + 4 + 16 * 4)


# ---- the Python layer: refused before anything is moved to a device ---------------------------------------------------
def test_engine_refusals_come_before_the_device():
    from smartpy_amd import engine
    s = np.zeros((5, 3))
    for fn in (engine.pareto_counts, engine.pareto_ranks):
        with pytest.raises(engine.SmartEngineError, match="direction 'up' unknown") as e:
            fn(s, ['max', 'up'])
        assert e.value.code == E_MODE
        with pytest.raises(engine.SmartEngineError, match='must be finite') as e:
            fn(s, ['max', ('target', NAN)])
        assert e.value.code == E_SIZE
        with pytest.raises(engine.SmartEngineError, match='must be finite'):
            fn(s, ['max', 'target'], targets=[0.0, INF])
        with pytest.raises(engine.SmartEngineError, match="without a value"):
            fn(s, ['max', 'target'])
        with pytest.raises(engine.SmartEngineError, match='17 objectives, between 1 and 16') as e:
            fn(np.zeros((5, 17)), ['max'] * 17)
        assert e.value.code == E_SIZE
        with pytest.raises(engine.SmartEngineError, match='0 objectives'):
            fn(s, [])
        with pytest.raises(engine.SmartEngineError, match=r'eligible has shape \(4,\)') as e:
            fn(s, ['max', 'min'], eligible=np.ones(4, dtype=bool))
        assert e.value.code == E_SIZE
        with pytest.raises(engine.SmartEngineError, match='columns'):
            fn(s, ['max', 'min'], columns=[0, 3])
        with pytest.raises(engine.SmartEngineError, match='columns'):
            fn(s, ['max', 'min'], columns=[1, 1])
        with pytest.raises(engine.SmartEngineError, match='columns'):
            fn(s, ['max'] * 4)                         # four objectives, three columns
        with pytest.raises(engine.SmartEngineError, match='not shape'):
            fn(np.zeros((2, 2, 2)), ['max'])
    with pytest.raises(engine.SmartEngineError, match='max_rank'):
        engine.pareto_ranks(s, ['max'], max_rank=0)


NAMES = ['T', 'C', 'H', 'D', 'S', 'Z', 'SK', 'FK', 'GK', 'RK']
OBJ = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE', 'GW']


@pytest.fixture()
def root(tmp_path):
    """the inputs of the golden catchment, a short period, and the database of a sampling run of 48 rows (KAT-12)"""
    from smartpy_amd.montecarlo.database import SamplingCsv
    r = example_root(tmp_path)
    settings_file(r, 'Catchment.short.sttngs', '01/01/2007', '01/03/2007', 10)
    z = load_golden('kat12_selection.npz')
    os.makedirs(os.path.join(r, 'out', 'Catchment'), exist_ok=True)
    db = SamplingCsv(os.path.join(r, 'out', 'Catchment', 'Catchment.SMART.lhs'), OBJ, NAMES).create(len(z['params']))
    db.write_table(z['obj_fns'], z['params'])
    db.close()
    return r


def test_default_directions_cover_the_objective_functions():
    from smartpy_amd import engine
    from smartpy_amd.montecarlo import Pareto
    assert sorted(Pareto.DEFAULT_DIRECTIONS) == sorted(engine.OBJ_FN_NAMES)
    assert Pareto.DEFAULT_DIRECTIONS == {'NSE': 'max', 'KGE': 'max', 'KGEc': 'max', 'GW': 'max', 'KGEa': ('target', 1.0),
                                         'KGEb': ('target', 1.0), 'PBias': ('target', 0.0), 'RMSE': 'min'}


def test_pareto_refusals_come_before_the_device(root):
    from smartpy_amd import engine
    from smartpy_amd.montecarlo import Pareto
    kw = dict(settings_filename='Catchment.short.sttngs')
    with pytest.raises(Exception, match='not recognised'):
        Pareto('Catchment', root, 'csv', 'csv', objectives=['NSE', 'Nash'], **kw)
    with pytest.raises(Exception, match='not recognised'):
        Pareto('Catchment', root, 'csv', 'csv', objectives={'nse': 'max'}, **kw)
    with pytest.raises(Exception, match='at least one objective'):
        Pareto('Catchment', root, 'csv', 'csv', objectives=[], **kw)
    with pytest.raises(Exception, match='at least one objective'):
        Pareto('Catchment', root, 'csv', 'csv', objectives={}, **kw)
    with pytest.raises(Exception, match='for conditioning in Pareto is not recognised'):
        Pareto('Catchment', root, 'csv', 'csv', objectives=['NSE'], conditioning={'Nash': ('min', (0.0,))}, **kw)
    with pytest.raises(Exception, match=r"'validation' has shape \(47,\) where one value per sampled set \(48,\)"):
        Pareto('Catchment', root, 'csv', 'csv', objectives=['NSE'], extra={'validation': (np.zeros(47), 'max')}, **kw)
    with pytest.raises(engine.SmartEngineError, match="direction 'best' unknown"):
        Pareto('Catchment', root, 'csv', 'csv', objectives={'NSE': 'best'}, **kw)
    with pytest.raises(engine.SmartEngineError, match="direction 'up' unknown"):
        Pareto('Catchment', root, 'csv', 'csv', objectives=['NSE'], extra={'validation': (np.zeros(48), 'up')}, **kw)
    with pytest.raises(engine.SmartEngineError, match='17 objectives'):
        Pareto('Catchment', root, 'csv', 'csv', objectives=OBJ,
               extra={'x%d' % k: (np.zeros(48), 'max') for k in range(9)}, **kw)
    with pytest.raises(FileNotFoundError, match='Catchment.SMART.lhs'):
        os.remove(os.path.join(root, 'out', 'Catchment', 'Catchment.SMART.lhs'))
        Pareto('Catchment', root, 'csv', 'csv', objectives=['NSE'], **kw)
