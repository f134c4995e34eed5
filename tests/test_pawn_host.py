"""PAWN sensitivity, host side: the numpy statement of include/smart_amd.h (smart_pawn_ks_hip) that tests/test_gpu_pawn.py
holds the kernels to BIT FOR BIT, against the brute-force definition of the supremum in exact arithmetic (and scipy's
two-sample statistic where scipy is there); the host functions of smartpy_amd/pawn.py; every refusal of the C entries, as
literals; the `.pawn` writer.  Nothing here needs a device."""
import ctypes
import math

import numpy as np
import pytest

from oracle.analyses.pawn import pawn_brute, pawn_statement, random_case
from oracle.exact import U
from smartpy_amd import _lib, pawn
from support import E_MODE, E_NO_DEVICE, E_NULL, E_SIZE, FAKE, refusal, same


def test_the_statement_is_the_supremum():
    rng = np.random.default_rng(11)
    seen_empty = seen_none = 0
    for i in range(60):
        y, cat, B = random_case(rng, i)
        ks, counts = pawn_statement(y, cat, B)
        assert same(ks, pawn_brute(y, cat, B)), i
        assert counts.tolist() == [[int((row == b).sum()) for b in range(B)] for row in cat]
        assert same(np.isnan(ks[0]), counts == 0) and (ks[~np.isnan(ks)] >= 0).all() and (ks[~np.isnan(ks)] < 1).all()
        seen_empty += int((counts == 0).any())
        seen_none += int((cat == 255).any())
    assert seen_empty > 20 and seen_none > 20


def test_the_rules_of_the_definition():
    # a row worked by hand: values 1 2 2 3, the rows of bin 0 hold 2 and 3, bin 1 holds 1, the other 2 is in no bin
    y = np.array([[2.0, 1.0, 3.0, 2.0]])
    cat = np.array([[0, 1, 0, 255]], dtype=np.uint8)
    ks, counts = pawn_statement(y, cat, 3)
    # sorted 1 2 2 3; evaluation points i = 0, 2, 3; bin 0 (n = 2): c = 0, 1, 2: |1*2 - 0|, |3*2 - 1*4|, 0 -> 2 / 8
    # bin 1 (n = 1): c = 1, 1, 1: |1 - 4|, |3 - 4|, 0 -> 3 / 4; bin 2: empty
    assert counts.tolist() == [[2, 1, 0]] and ks[0, 0, :2].tolist() == [0.25, 0.75] and np.isnan(ks[0, 0, 2])
    # all values equal: one evaluation point, the last, where every CDF is 1
    ks, _ = pawn_statement(np.full((1, 9), 4.5), np.arange(9, dtype=np.uint8)[None, :] % 3, 3)
    assert (ks == 0.0).all()
    # -0.0 and +0.0 are one run
    zeros = np.array([[0.0, -0.0, 0.0, -0.0, 1.0]])
    ks, _ = pawn_statement(zeros, np.array([[0, 0, 1, 1, 1]], dtype=np.uint8), 2)
    assert ks[0, 0].tolist() == [abs(4 * 2 - 2 * 5) / 10.0, abs(4 * 3 - 2 * 5) / 15.0]
    # a value that is not finite: the whole row NaN, the others as they are
    y = np.array([[1.0, 2.0, 3.0], [1.0, np.nan, 3.0], [np.inf, 2.0, 3.0], [1.0, 2.0, -np.inf], [3.0, 2.0, 1.0]])
    ks, _ = pawn_statement(y, np.array([[0, 1, 1]], dtype=np.uint8), 2)
    assert np.isnan(ks[1:4]).all() and ks[0, 0].tolist() == [2 / 3, 1 / 3] and ks[4, 0].tolist() == [2 / 3, 1 / 3]
    # one bin that holds every row: the two CDFs are one
    ks, counts = pawn_statement(np.arange(7.0)[None, :], np.zeros((1, 7), dtype=np.uint8), 1)
    assert ks.tolist() == [[[0.0]]] and counts.tolist() == [[7]]
    # the bins are the ranks of the values: (B - 1) / B per bin
    N, B = 40, 8
    v = np.random.default_rng(1).permutation(N).astype(np.float64)
    ks, _ = pawn_statement(v[None, :], (v // (N // B)).astype(np.uint8)[None, :], B)
    assert ks[0, 0, 0] == ks[0, 0, B - 1] == (B - 1) / B and (ks[0, 0] <= (B - 1) / B).all()


def test_scipy_reads_the_literature_alike():
    stats = pytest.importorskip('scipy.stats')
    rng = np.random.default_rng(5)
    for _ in range(10):
        N, B = int(rng.integers(20, 65)), 4
        y = np.exp(rng.normal(0.0, 2.0, size=(1, N)))               # tie-free
        cat = rng.integers(0, B, size=(1, N)).astype(np.uint8)
        ks, counts = pawn_statement(y, cat, B)
        for b in range(B):
            if counts[0, b]:
                assert abs(stats.ks_2samp(y[0], y[0][cat[0] == b]).statistic - ks[0, 0, b]) <= 4 * U


# ---- pawn.py ------------------------------------------------------------------------------------------------------------
def test_dummy_table():
    for n, bins, dummies in ((103, 10, 3), (64, 64, 2), (5, 8, 1), (1000, 1, 4), (0, 3, 2), (50, 7, 0)):
        table = pawn.dummy_table(n, bins, dummies, seed=4)
        assert table.dtype == np.uint8 and table.shape == (dummies, n)
        for row in table:
            sizes = np.bincount(row, minlength=bins)
            assert len(sizes) == bins and sizes.max() - sizes.min() <= 1
        assert np.array_equal(table, pawn.dummy_table(n, bins, dummies, seed=4))
    a, b = pawn.dummy_table(500, 10, 3, seed=0), pawn.dummy_table(500, 10, 3, seed=1)
    assert not np.array_equal(a, b) and not np.array_equal(a[0], a[1])
    assert np.array_equal(pawn.dummy_table(500, 10, 3), a)          # seed 0 by default
    with pytest.raises(ValueError, match='bins must be in 1 .. 64'):
        pawn.dummy_table(10, 65, 1)
    assert pawn.bin_table is __import__('smartpy_amd.identifiability', fromlist=['x']).bin_table


def test_pawn_indices():
    import torch
    rng = np.random.default_rng(8)
    R, P, B = 6, 4, 5
    ks = rng.uniform(0.0, 1.0, size=(R, P, B))
    counts = np.array([[20, 20, 20, 20, 20], [20, 3, 20, 9, 20], [1, 2, 3, 4, 5], [0, 30, 0, 30, 0]], dtype=np.int32)
    ks[:, counts == 0] = np.nan                                       # an empty bin
    ks[4] = np.nan                                                    # a row that held a NaN
    for name, fn in (('median', np.nanmedian), ('mean', np.nanmean), ('max', np.nanmax)):
        got = pawn.pawn_indices(ks, counts, name, min_count=10)
        assert got.shape == (R, P)
        for r in range(R):
            if r == 4:
                assert np.isnan(got[r]).all()
                continue
            assert got[r, 0] == fn(ks[r, 0]) and got[r, 1] == fn(ks[r, 1, [0, 2, 4]]) and np.isnan(got[r, 2])
            assert got[r, 3] == fn(ks[r, 3, [1, 3]])
        every = pawn.pawn_indices(ks, counts, name)                    # min_count 1: the bins that hold a row
        assert every[0, 2] == fn(ks[0, 2]) and every[0, 3] == fn(ks[0, 3, [1, 3]])
        on_tensor = pawn.pawn_indices(torch.from_numpy(ks), torch.from_numpy(counts), name, min_count=10)
        assert isinstance(on_tensor, torch.Tensor) and same(on_tensor.numpy(), got)
    assert pawn.default_min_count(100000, 10) == 2500 and pawn.default_min_count(300, 10) == 10
    with pytest.raises(ValueError, match="statistic 'mode' unknown"):
        pawn.pawn_indices(ks, counts, 'mode')
    with pytest.raises(ValueError, match=r'ks must be \[R, P, B\]'):
        pawn.pawn_indices(ks, counts[:, :4])


def test_critical_value():
    assert pawn.critical_value(1000, 100) == math.sqrt(-math.log(0.025) / 2.0) * math.sqrt(1100.0 / 100000.0)
    assert abs(pawn.critical_value(1000, 100) - 1.3581 * math.sqrt(0.011)) < 1e-5       # the 1.36 of the tables
    got = pawn.critical_value(500, np.array([50, 25, 0]), alpha=0.01)
    c = math.sqrt(-math.log(0.005) / 2.0)
    assert got[:2].tolist() == [c * math.sqrt(550 / 25000.0), c * math.sqrt(525 / 12500.0)] and np.isinf(got[2])
    with pytest.raises(ValueError, match='alpha'):
        pawn.critical_value(10, 5, alpha=1.0)


def test_the_result_object_and_the_pawn_writer(tmp_path):
    names = ['T', 'C']
    ks = np.zeros((3, 4, 2))                                          # two parameters, two dummies, two bins
    ks[0] = [[0.5, 0.25], [0.125, 0.125], [0.25, 0.0], [0.0625, 0.0625]]
    ks[1] = [[0.0, 0.0], [0.5, 0.5], [0.25, 0.25], [0.5, 0.5]]
    ks[2] = np.nan
    counts = np.full((4, 2), 50, dtype=np.int32)
    res = pawn.PawnSensitivity(['a', 'b', 'c'], names, ks, counts, statistic='mean', min_count=10)
    assert (res.bins, res.dummies, res.statistic, res.min_count) == (2, 2, 'mean', 10)
    assert res.index.tolist()[:2] == [[0.375, 0.125], [0.0, 0.5]] and np.isnan(res.index[2]).all()
    assert res.dummy.tolist()[:2] == [0.125, 0.5] and np.isnan(res.dummy[2])
    assert res.influential.tolist() == [[True, False], [False, False], [False, False]]
    assert res.file is None and res.device_ks is None and res.categories is None
    top = pawn.PawnSensitivity(['a', 'b', 'c'], names, ks, counts, statistic='max')
    assert top.index.tolist()[0] == [0.5, 0.125] and top.dummy[0] == 0.25
    alone = pawn.PawnSensitivity(['a', 'b', 'c'], names, ks[:, :2], counts[:2])
    assert alone.dummies == 0 and np.isnan(alone.dummy).all() and not alone.influential.any()
    assert pawn.header_line(names) == 'DateTime,T,C,dummy\n'
    path = str(tmp_path / 'Catchment.SMART.lhs.pawn')
    pawn.write_file(path, res.datetime, res.names, res.index, res.dummy)
    lines = open(path).read().split('\n')
    assert lines == ['DateTime,T,C,dummy', 'a,3.750000e-01,1.250000e-01,1.250000e-01',
                     'b,0.000000e+00,5.000000e-01,5.000000e-01', 'c,nan,nan,nan', '']
    back = np.genfromtxt(path, delimiter=',', skip_header=1, usecols=(1, 2, 3))
    assert same(back[:, :2], res.index) and same(back[:, 2], res.dummy)


# ---- the refusals of the C entries --------------------------------------------------------------------------------------
TWO24, TWO31 = 2 ** 24, 2 ** 31
AUTO, LDS, GLOBAL = 0, 1, 2
K_, WS = 'smart_pawn_ks_hip', 'smart_pawn_workspace_bytes'
STEP = 4096 * 12                    # the workspace of one step of up to 4096 samples

VALID = {
    K_: dict(n_samples=4, n_rows=7, y=FAKE, ld=4, cat=FAKE, n_factors=2, n_bins=2, ks=FAKE, counts=FAKE, method=GLOBAL,
             workspace=FAKE, workspace_bytes=STEP, stream=None),
    WS: dict(n_samples=4, n_rows=7, method=GLOBAL),
}
REQUIRED = 'smart_pawn_ks_hip: y, cat, ks and counts are required (%s is NULL)'

CASES = [
    (K_, dict(y=None), E_NULL, REQUIRED % 'y'),
    (K_, dict(cat=None), E_NULL, REQUIRED % 'cat'),
    (K_, dict(ks=None), E_NULL, REQUIRED % 'ks'),
    (K_, dict(counts=None), E_NULL, REQUIRED % 'counts'),
    (K_, dict(cat=None, counts=None), E_NULL, REQUIRED % 'cat'),                        # the first in the list is named
    (K_, dict(ks=None, n_samples=0), E_NULL, REQUIRED % 'ks'),                          # pointers before sizes
    (K_, dict(n_samples=0), E_SIZE, 'smart_pawn_ks_hip: need n_samples, n_rows >= 1 (got 0, 7)'),
    (K_, dict(n_rows=0), E_SIZE, 'smart_pawn_ks_hip: need n_samples, n_rows >= 1 (got 4, 0)'),
    (K_, dict(n_samples=-3, n_rows=TWO31), E_SIZE, 'smart_pawn_ks_hip: need n_samples, n_rows >= 1 (got -3, 2147483648)'),
    (K_, dict(n_samples=TWO24 + 1, ld=TWO24 + 1), E_SIZE, 'smart_pawn_ks_hip: n_samples 16777217, at most 16777216 (2^24)'),
    (K_, dict(n_samples=TWO24 + 1, n_rows=TWO31), E_SIZE, 'smart_pawn_ks_hip: n_samples 16777217, at most 16777216 (2^24)'),
    (K_, dict(n_rows=TWO31), E_SIZE, 'smart_pawn_ks_hip: n_rows 2147483648 is more than one launch takes (2^31 - 1)'),
    (K_, dict(n_rows=TWO31, ld=3), E_SIZE, 'smart_pawn_ks_hip: n_rows 2147483648 is more than one launch takes (2^31 - 1)'),
    (K_, dict(ld=3), E_SIZE, 'smart_pawn_ks_hip: ld 3 is less than n_samples 4'),
    (K_, dict(ld=3, n_factors=0), E_SIZE, 'smart_pawn_ks_hip: ld 3 is less than n_samples 4'),
    (K_, dict(n_factors=0), E_SIZE, 'smart_pawn_ks_hip: n_factors 0 must be in 1 .. 16'),
    (K_, dict(n_factors=17), E_SIZE, 'smart_pawn_ks_hip: n_factors 17 must be in 1 .. 16'),
    (K_, dict(n_factors=17, n_bins=65), E_SIZE, 'smart_pawn_ks_hip: n_factors 17 must be in 1 .. 16'),
    (K_, dict(n_bins=0), E_SIZE, 'smart_pawn_ks_hip: n_bins 0 must be in 1 .. 64'),
    (K_, dict(n_bins=65), E_SIZE, 'smart_pawn_ks_hip: n_bins 65 must be in 1 .. 64'),
    (K_, dict(n_bins=65, method=3), E_SIZE, 'smart_pawn_ks_hip: n_bins 65 must be in 1 .. 64'),        # sizes before the method
    (K_, dict(method=3), E_MODE, "smart_pawn_ks_hip: method '3' unknown."),
    (K_, dict(method=-1), E_MODE, "smart_pawn_ks_hip: method '-1' unknown."),
    (K_, dict(method=3, workspace=None), E_MODE, "smart_pawn_ks_hip: method '3' unknown."),            # ... before the workspace
    (K_, dict(method=LDS, n_samples=8193, ld=8193), E_SIZE,
     'smart_pawn_ks_hip: the LDS form takes at most 8192 samples, not 8193'),
    (K_, dict(workspace=None), E_NULL, 'smart_pawn_ks_hip: a workspace of 49152 bytes is needed (workspace is NULL)'),
    (K_, dict(method=AUTO, n_samples=8193, ld=8193, workspace=None), E_NULL,
     'smart_pawn_ks_hip: a workspace of 196608 bytes is needed (workspace is NULL)'),
    (K_, dict(workspace_bytes=STEP - 1), E_SIZE, 'smart_pawn_ks_hip: workspace_bytes 49151, need 49152'),
    (K_, dict(workspace_bytes=0), E_SIZE, 'smart_pawn_ks_hip: workspace_bytes 0, need 49152'),
    (K_, dict(n_samples=4097, ld=4097), E_SIZE, 'smart_pawn_ks_hip: workspace_bytes 49152, need 98304'),
    # ---- smart_pawn_workspace_bytes: the rules of the entry that its arguments can break, with the entry's code
    (WS, dict(n_samples=0), E_SIZE, None),
    (WS, dict(n_rows=0), E_SIZE, None),
    (WS, dict(n_samples=TWO24 + 1), E_SIZE, None),
    (WS, dict(n_rows=TWO31), E_SIZE, None),
    (WS, dict(method=3), E_MODE, None),
    (WS, dict(method=3, n_rows=0), E_SIZE, None),
    (WS, dict(method=LDS, n_samples=8193), E_SIZE, None),
]


@pytest.mark.parametrize('entry,changes,code,text', CASES,
                         ids=['%s-%s' % (c[0][6:], '-'.join('%s=%s' % kv for kv in c[1].items())) for c in CASES])
def test_refusals(entry, changes, code, text):
    assert refusal(VALID, entry, changes) == (code, text)


def test_a_well_formed_call_gets_as_far_as_the_device():
    L = _lib.lib()
    if L.smart_device_count() == 0:
        # ... and no further: there is no CPU fallback
        for changes in (dict(), dict(method=LDS, workspace=None, workspace_bytes=0),
                        dict(method=AUTO, workspace=None, workspace_bytes=0),
                        dict(method=LDS, n_samples=8192, ld=8192, workspace=None),
                        dict(method=AUTO, n_samples=8193, ld=8200, workspace_bytes=16384 * 12),
                        dict(n_samples=TWO24, ld=TWO24, n_rows=TWO31 - 1, n_factors=16, n_bins=64,
                             workspace_bytes=TWO24 * 12)):
            rc, text = refusal(VALID, K_, changes)
            assert rc == E_NO_DEVICE and 'device' in text, changes
    else:
        # with a device the refusals leave the error text as they set it, and the entry is run for real by
        # tests/test_gpu_pawn.py
        assert refusal(VALID, K_, dict(y=None))[0] == E_NULL


def test_workspace_and_capacities():
    L = _lib.lib()
    cap = L.smart_pawn_lds_capacity()
    assert cap == 8192
    for method in (AUTO, LDS):
        assert L.smart_pawn_workspace_bytes(cap, 100, method) == 0 and L.smart_pawn_workspace_bytes(1, 1, method) == 0
    assert L.smart_pawn_workspace_bytes(4, 7, GLOBAL) == 7 * STEP                      # every step, padded to 4096
    assert L.smart_pawn_workspace_bytes(4096, 3, GLOBAL) == 3 * STEP
    assert L.smart_pawn_workspace_bytes(4097, 3, GLOBAL) == 3 * 8192 * 12
    assert L.smart_pawn_workspace_bytes(cap + 1, 5, AUTO) == 5 * 16384 * 12
    step = 131072 * 12                                                                  # 1e5 padded to 2^17
    assert L.smart_pawn_workspace_bytes(100000, 3653, AUTO) == (2 ** 28 // step) * step == 170 * step
    assert L.smart_pawn_workspace_bytes(TWO24, 10, GLOBAL) == TWO24 * 12               # at least one step
    from smartpy_amd import analysis, engine
    assert analysis.pawn_lds_capacity() == engine.pawn_lds_capacity() == cap
    assert _lib.PAWN_MAX_FACTORS == 16 and _lib.PAWN_MAX_BINS == 64
    assert _lib.PAWN_METHODS == {'auto': AUTO, 'lds': LDS, 'global': GLOBAL}
    assert L.smart_abi_version() == 7


def test_the_new_names_are_bound_and_the_words_are_checked_first():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'smart_amd.h')).read()
    for name, n_args, res in (('smart_pawn_ks_hip', 13, ctypes.c_int), ('smart_pawn_workspace_bytes', 3, ctypes.c_int64),
                              ('smart_pawn_lds_capacity', 0, ctypes.c_int64)):
        assert name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None
        assert _lib.SYMBOLS[name][0] is res and len(_lib.SYMBOLS[name][1]) == n_args
        declared = re.search(r'^int(?:64_t)? %s\(([^;]*)\);' % name, header, re.M)
        assert declared, name
        args = declared.group(1).strip()
        assert (0 if args == 'void' else args.count(',') + 1) == n_args
    for macro, value in (('SMART_PAWN_MAX_FACTORS', 16), ('SMART_PAWN_MAX_BINS', 64), ('SMART_PAWN_AUTO', 0),
                         ('SMART_PAWN_LDS', 1), ('SMART_PAWN_GLOBAL', 2)):
        assert re.search(r'^#define %s %d$' % (macro, value), header, re.M), macro
    from smartpy_amd import analysis, engine
    assert engine.pawn_ks is analysis.pawn_ks and engine.PawnResult is analysis.PawnResult
    # what can be refused from the words and the shapes is refused before a device is looked for
    y = np.zeros((2, 4))
    cat = np.zeros((1, 4), dtype=np.uint8)
    with pytest.raises(engine.SmartEngineError, match="method 'radix' unknown") as err:
        engine.pawn_ks(y, cat, 2, method='radix')
    assert err.value.code == -7
    with pytest.raises(engine.SmartEngineError, match=r'categories must be uint8 \[factors, 4\]') as err:
        engine.pawn_ks(y, cat.astype(np.int32), 2)
    assert err.value.code == -2
    with pytest.raises(engine.SmartEngineError, match=r'categories must be uint8 \[factors, 4\]'):
        engine.pawn_ks(y, cat[:, :3], 2)
    from smartpy_amd.montecarlo import LHS, GLUE, Total, Best, Sobol
    for cls in (LHS, GLUE, Total, Best, Sobol):
        assert callable(cls.pawn_sensitivity) and isinstance(cls.pawn_file, property)


def test_no_cpu_fallback():
    L = _lib.lib()
    from smartpy_amd import engine
    if L.smart_device_count() == 0:
        with pytest.raises(Exception, match='no CPU fallback'):
            engine.pawn_ks(np.zeros((2, 4)), np.zeros((1, 4), dtype=np.uint8), 2)
