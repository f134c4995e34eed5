"""Dynamic identifiability analysis, host side: the row-by-row statement of include/smart_amd.h (smart_dynia_hip) that
tests/test_gpu_dynia.py holds the kernels to, with its exact (Fraction) yardsticks; a record worked by hand; the host
functions of smartpy_amd/identifiability.py; every refusal of the two C entries, as literals; the `.dynia` writer.
Nothing here needs a device."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle.analyses.dynia import EQUAL, LINEAR, dynia_statement, exact_shares, exact_sums
from oracle.exact import U
from smartpy_amd import _lib, identifiability as ident
from support import E_MODE, E_NULL, E_SIZE, FAKE, refusal, same


# ---- a record worked by hand ------------------------------------------------------------------------------------------
# absolute errors d[s][n] of R = 7 steps and N = 4 samples; step 2 has no observation
D = np.array([[1, 0, 2, 1],
              [0, 1, 2, 0],
              [9, 9, 9, 9],
              [2, 2, 0, 2],
              [1, 1, 3, 1],
              [0, 0, 1, 0],
              [2, 1, 1, 3]], dtype=np.float64)
OBS = np.array([1.0, 2.0, np.nan, 4.0, 1.0, 0.0, 3.0])
SIM = np.where(np.isnan(OBS)[:, None], 9.0, np.nan_to_num(OBS)[:, None] + D)
CAT = np.array([[0, 1, 0, 1], [0, 0, 1, 255]], dtype=np.uint8)
T = 1 / 3


def test_the_record_worked_by_hand():
    got = dynia_statement(SIM, OBS, CAT, 2, 1, 2, 0.5, EQUAL)
    assert got['count'].tolist() == [2, 2, 2, 2, 3, 3, 2]
    assert got['E'].tolist() == [[1, 1, 4, 1], [1, 1, 4, 1], [2, 3, 2, 2], [3, 3, 3, 3], [3, 3, 4, 3], [3, 2, 5, 4],
                                 [2, 1, 2, 3]]
    assert got['k'].tolist() == [2] * 7                                # ceil(0.5 * 4)
    assert got['cut'].tolist() == [1, 1, 2, 3, 3, 3, 2]
    assert got['rows'] == [[0, 1, 3], [0, 1, 3], [0, 2, 3], [0, 1, 2, 3], [0, 1, 3], [0, 1], [0, 1, 2]]
    assert got['retained'].tolist() == [3, 3, 3, 4, 3, 2, 3]           # ties at the cut stay in: retained > k five times
    equal = [[[T, 2 * T], [2 * T, 0]], [[T, 2 * T], [2 * T, 0]], [[2 * T, T], [T, T]], [[0.5, 0.5], [0.5, 0.25]],
             [[T, 2 * T], [2 * T, 0]], [[0.5, 0.5], [1, 0]], [[2 * T, T], [2 * T, T]]]
    assert got['shares'].tolist() == equal
    # LINEAR: steps 0 .. 4 retain only rows AT the cut, S == 0, and fall back to 1 each; step 5 has s = (0, 1), step 6
    # s = (0, 1, 0): all of the support is sample 1's, bin 1 of factor 0 and bin 0 of factor 1
    lin = dynia_statement(SIM, OBS, CAT, 2, 1, 2, 0.5, LINEAR)
    assert lin['shares'].tolist() == equal[:5] + [[[0, 1], [1, 0]], [[0, 1], [1, 0]]]
    for key in ('count', 'E', 'k', 'cut', 'retained', 'rows'):
        assert same(lin[key], got[key]) if key != 'rows' else lin[key] == got[key]
    # k = ceil(0.75 * 4) = 3: step 5 sorted (2, 3, 4, 5), cut 4, s = (1, 2, -, 0), S = 3
    three = dynia_statement(SIM, OBS, CAT, 2, 1, 2, 0.75, LINEAR)
    assert three['k'][5] == 3 and three['cut'][5] == 4 and three['rows'][5] == [0, 1, 3]
    assert three['shares'][5].tolist() == [[T, 2 * T], [1, 0]]
    # a window of three observed steps asked for: only steps 4 and 5 are assessed
    strict = dynia_statement(SIM, OBS, CAT, 2, 1, 3, 0.5, LINEAR)
    assert strict['count'].tolist() == got['count'].tolist() and strict['retained'].tolist() == [0, 0, 0, 0, 3, 2, 0]
    assert np.isnan(strict['cut'][[0, 1, 2, 3, 6]]).all() and np.isnan(strict['shares'][[0, 1, 2, 3, 6]]).all()
    assert np.isnan(strict['E'][[0, 1, 2, 3, 6]]).all() and same(strict['shares'][4:6], lin['shares'][4:6])
    # a sample that is not finite inside a window is not eligible there, and only there
    sim = SIM.copy()
    sim[0, 2], sim[2, 1] = np.inf, np.nan                           # (step 2 has no observation: its NaN is never read)
    hole = dynia_statement(sim, OBS, CAT, 2, 1, 2, 0.5, EQUAL)
    assert np.isinf(hole['E'][0, 2]) and np.isinf(hole['E'][1, 2]) and np.isfinite(hole['E'][2:]).all()
    assert hole['k'].tolist() == [2, 2, 2, 2, 2, 2, 2] and hole['rows'][0] == [0, 1, 3] and same(hole['E'][2:], got['E'][2:])


def test_the_statement_against_exact_arithmetic():
    rng = np.random.default_rng(7)
    R, N, h, B = 40, 37, 3, 5
    sim = np.exp(rng.normal(0.0, 3.0, size=(R, N)))
    obs = np.exp(rng.normal(0.0, 3.0, size=R))
    obs[10:13] = np.nan
    sim[20, 4] = np.nan
    cat = rng.integers(0, B, size=(2, N)).astype(np.uint8)
    cat[1, 5] = 255
    exact = exact_sums(sim, obs, h, min_valid=4)
    for support in (EQUAL, LINEAR):
        got = dynia_statement(sim, obs, cat, B, h, 4, 0.2, support)
        for r in range(R):
            for n in range(N):
                if exact[r][n] is None:
                    assert not math.isfinite(got['E'][r, n])
                else:
                    assert abs(Fraction(got['E'][r, n]) - exact[r][n]) <= (2 * h + 3) * U * exact[r][n]
            ref = exact_shares(got['E'][r], cat, B, 0.2, support)
            if got['count'][r] < 4:
                assert got['retained'][r] == 0 and np.isnan(got['shares'][r]).all()
                continue
            c, rows, sh = ref
            assert c == got['cut'][r] and rows == got['rows'][r] and len(rows) >= got['k'][r] == 8
            tol = 2 * (len(rows) + 2) * U
            for p in range(2):
                for b in range(B):
                    assert abs(Fraction(got['shares'][r, p, b]) - sh[p][b]) <= tol * sh[p][b]
            # a factor without a row of category 255 among the retained sums to one; with one, to less (or to one still,
            # where that row lies at the cut and its support is zero)
            assert sum(sh[0]) == 1 and sum(sh[1]) <= 1 and (5 in rows or sum(sh[1]) == 1)


# ---- identifiability.py -------------------------------------------------------------------------------------------------
def test_bin_table_edges():
    ranges = [(0.0, 1.0), (10.0, 20.0)]
    sample = np.array([[0.0, 10.0], [1.0, 20.0], [0.25, 12.5], [0.2499999, 14.999], [-1e-9, 20.0000001], [np.nan, np.inf],
                       [0.999999, 19.99], [0.5, 15.0]])
    table = ident.bin_table(sample, ranges, 4)
    assert table.dtype == np.uint8 and table.shape == (2, 8)
    assert table.tolist() == [[0, 3, 1, 0, 255, 255, 3, 2], [0, 3, 1, 1, 255, 255, 3, 2]]
    import torch
    on_tensor = ident.bin_table(torch.from_numpy(sample), ranges, 4)
    assert on_tensor.dtype == torch.uint8 and on_tensor.numpy().tolist() == table.tolist()
    assert ident.bin_table(sample, {'a': (0.0, 1.0), 'b': (10.0, 20.0)}, 1).tolist() == [[0, 0, 0, 0, 255, 255, 0, 0]] * 2
    assert ident.bin_table(sample, ranges, 64).max() == 255 and ident.bin_table(sample, ranges, 64)[0, 1] == 63
    for bad in (0, 65):
        with pytest.raises(ValueError, match='bins must be in 1 .. 64'):
            ident.bin_table(sample, ranges, bad)
    with pytest.raises(ValueError, match='a column per factor'):
        ident.bin_table(sample[:, :1], ranges, 4)
    with pytest.raises(ValueError, match='lo < hi'):
        ident.bin_table(sample, [(0.0, 1.0), (2.0, 2.0)], 4)


def test_confidence_limits_and_information_content():
    import torch
    ranges = np.array([[0.0, 10.0], [100.0, 300.0]])
    B, level = 5, 0.9
    shares = np.zeros((3, 2, B))
    shares[0, 0, 3] = 1.0                   # all mass in bin 3 of factor 0: [6, 8)
    shares[0, 1, 0] = 0.5                   # ... and in bin 0 of factor 1, half of it lost to category 255: renormalised
    shares[1] = 1.0 / B                     # uniform
    shares[2] = np.nan                      # a step not assessed
    for array in (shares, torch.from_numpy(shares)):
        limits = ident.confidence_limits(array, ranges, level)
        info = ident.information_content(limits, ranges)
        if array is not shares:
            assert isinstance(limits, torch.Tensor) and isinstance(info, torch.Tensor)
            limits, info = limits.numpy(), info.numpy()
        assert limits.shape == (3, 2, 2) and info.shape == (3, 2)
        assert np.allclose(limits[0, 0], [6.0 + 0.05 * 2.0, 6.0 + 0.95 * 2.0], rtol=1e-14, atol=0)
        assert np.allclose(limits[0, 1], [100.0 + 0.05 * 40.0, 100.0 + 0.95 * 40.0], rtol=1e-14, atol=0)
        assert 6.0 <= limits[0, 0, 0] < limits[0, 0, 1] <= 8.0
        assert np.allclose(info[0], 1.0 - level / B, rtol=1e-14, atol=0)
        assert np.allclose(limits[1, 0], [0.5, 9.5], rtol=1e-13, atol=0)
        assert np.allclose(limits[1, 1], [110.0, 290.0], rtol=1e-13, atol=0)
        assert np.allclose(info[1], 1.0 - level, rtol=1e-12, atol=0)
        assert np.isnan(limits[2]).all() and np.isnan(info[2]).all()
    # a factor without any share is NaN; level = 1 spans the bins that hold the mass
    none = ident.confidence_limits(np.zeros((1, 2, B)), ranges)
    assert np.isnan(none).all()
    full = ident.confidence_limits(shares[:2], ranges, 1.0)
    assert np.allclose(full[0, 0], [6.0, 8.0]) and np.allclose(full[1, 1], [100.0, 300.0])
    with pytest.raises(ValueError, match='level'):
        ident.confidence_limits(shares, ranges, 0.0)


def test_the_result_object_and_the_dynia_writer(tmp_path):
    ranges = {'T': (0.9, 1.1), 'C': (0.0, 1.0)}
    shares = np.zeros((2, 2, 4))
    shares[0, 0, 1] = shares[0, 1, 2] = 1.0
    shares[1] = np.nan
    res = ident.DynamicIdentifiability(['2007-01-01 09:00:00', '2007-01-02 09:00:00'], ['T', 'C'], ranges, shares,
                                       [6.0, np.nan], [3, 0], [3, 1], level=0.9, errors=[[3.0, 6.0], [np.nan, np.nan]])
    assert res.ranges.tolist() == [[0.9, 1.1], [0.0, 1.0]] and res.mean_error[0] == 2.0 and np.isnan(res.mean_error[1])
    assert res.mean_errors[0].tolist() == [1.0, 2.0] and res.file is None and res.device_shares is None
    assert res.information.shape == (2, 2) and np.allclose(res.information[0], 1.0 - 0.9 / 4) and np.isnan(res.information[1]).all()
    assert ident.header_line(['T', 'C']) == 'DateTime,IC@T,LO@T,HI@T,IC@C,LO@C,HI@C\n'
    path = str(tmp_path / 'Catchment.SMART.lhs.dynia')
    ident.write_file(path, res.datetime, res.names, res.information, res.limits)
    lines = open(path).read().split('\n')
    assert lines[0] == 'DateTime,IC@T,LO@T,HI@T,IC@C,LO@C,HI@C' and len(lines) == 4 and lines[3] == ''
    assert lines[1] == '2007-01-01 09:00:00,7.750000e-01,9.525000e-01,9.975000e-01,7.750000e-01,5.125000e-01,7.375000e-01'
    assert lines[2] == '2007-01-02 09:00:00,nan,nan,nan,nan,nan,nan'


# ---- the refusals of the C entries --------------------------------------------------------------------------------------
NAN = float('nan')
TWO31 = 2 ** 31
D_, WS = 'smart_dynia_hip', 'smart_dynia_workspace_bytes'

VALID = {
    D_: dict(n_samples=4, n_reports=7, sim=FAKE, ld=4, obs=FAKE, half_width=1, min_valid=2, fraction=0.5, cat=FAKE,
             n_factors=2, n_bins=2, support=1, shares=FAKE, cut=FAKE, retained=FAKE, count=FAKE, err=None, ld_err=0,
             workspace=FAKE, workspace_bytes=32, stream=None),
    WS: dict(n_samples=4, n_reports=7, half_width=1, n_factors=2, n_bins=2),
}
REQUIRED = 'smart_dynia_hip: sim, obs, cat, shares, cut, retained and count are required (%s is NULL)'

CASES = [
    (D_, dict(sim=None), E_NULL, REQUIRED % 'sim'),
    (D_, dict(obs=None), E_NULL, REQUIRED % 'obs'),
    (D_, dict(cat=None), E_NULL, REQUIRED % 'cat'),
    (D_, dict(shares=None), E_NULL, REQUIRED % 'shares'),
    (D_, dict(cut=None), E_NULL, REQUIRED % 'cut'),
    (D_, dict(retained=None), E_NULL, REQUIRED % 'retained'),
    (D_, dict(count=None), E_NULL, REQUIRED % 'count'),
    (D_, dict(obs=None, count=None), E_NULL, REQUIRED % 'obs'),                         # the first in the list is named
    (D_, dict(cut=None, n_samples=0), E_NULL, REQUIRED % 'cut'),                        # pointers before sizes
    (D_, dict(n_samples=0), E_SIZE, 'smart_dynia_hip: need n_samples, n_reports >= 1 (got 0, 7)'),
    (D_, dict(n_reports=0), E_SIZE, 'smart_dynia_hip: need n_samples, n_reports >= 1 (got 4, 0)'),
    (D_, dict(n_samples=TWO31, ld=TWO31), E_SIZE, 'smart_dynia_hip: n_samples 2147483648 must be in 1 .. 2^31 - 1'),
    (D_, dict(n_reports=TWO31), E_SIZE, 'smart_dynia_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (D_, dict(half_width=-1), E_SIZE, 'smart_dynia_hip: half_width -1 must be in 0 .. 63'),
    (D_, dict(half_width=64, min_valid=1), E_SIZE, 'smart_dynia_hip: half_width 64 must be in 0 .. 63'),
    (D_, dict(n_factors=0), E_SIZE, 'smart_dynia_hip: n_factors 0 must be in 1 .. 16'),
    (D_, dict(n_factors=17), E_SIZE, 'smart_dynia_hip: n_factors 17 must be in 1 .. 16'),
    (D_, dict(n_bins=0), E_SIZE, 'smart_dynia_hip: n_bins 0 must be in 1 .. 64'),
    (D_, dict(n_bins=65), E_SIZE, 'smart_dynia_hip: n_bins 65 must be in 1 .. 64'),
    (D_, dict(n_factors=17, n_bins=65), E_SIZE, 'smart_dynia_hip: n_factors 17 must be in 1 .. 16'),
    (D_, dict(ld=3), E_SIZE, 'smart_dynia_hip: ld 3 is less than n_samples 4'),
    (D_, dict(err=FAKE, ld_err=3), E_SIZE, 'smart_dynia_hip: ld_err 3 is less than n_samples 4'),
    (D_, dict(min_valid=0), E_SIZE, 'smart_dynia_hip: min_valid 0 must be in 1 .. 3 (the window)'),
    (D_, dict(min_valid=4), E_SIZE, 'smart_dynia_hip: min_valid 4 must be in 1 .. 3 (the window)'),
    (D_, dict(half_width=0, min_valid=2), E_SIZE, 'smart_dynia_hip: min_valid 2 must be in 1 .. 1 (the window)'),
    (D_, dict(fraction=0.0), E_SIZE, 'smart_dynia_hip: fraction 0 is outside (0, 1]'),
    (D_, dict(fraction=1.5), E_SIZE, 'smart_dynia_hip: fraction 1.5 is outside (0, 1]'),
    (D_, dict(fraction=NAN), E_SIZE, 'smart_dynia_hip: fraction nan is outside (0, 1]'),
    (D_, dict(fraction=-0.1, support=2), E_SIZE, 'smart_dynia_hip: fraction -0.1 is outside (0, 1]'),    # sizes before the mode
    (D_, dict(support=2), E_MODE, "smart_dynia_hip: support '2' unknown."),
    (D_, dict(support=-1), E_MODE, "smart_dynia_hip: support '-1' unknown."),
    (D_, dict(support=2, workspace=None), E_MODE, "smart_dynia_hip: support '2' unknown."),             # the mode before the workspace
    (D_, dict(workspace=None), E_NULL, 'smart_dynia_hip: a workspace of 32 bytes is needed (workspace is NULL)'),
    (D_, dict(workspace_bytes=31), E_SIZE, 'smart_dynia_hip: workspace_bytes 31, need 32'),
    (D_, dict(workspace_bytes=0), E_SIZE, 'smart_dynia_hip: workspace_bytes 0, need 32'),
    # ---- smart_dynia_workspace_bytes: the size rules of the entry, SMART_E_SIZE for each
    (WS, dict(n_samples=0), E_SIZE, None),
    (WS, dict(n_reports=0), E_SIZE, None),
    (WS, dict(n_samples=TWO31), E_SIZE, None),
    (WS, dict(n_reports=TWO31), E_SIZE, None),
    (WS, dict(half_width=-1), E_SIZE, None),
    (WS, dict(half_width=64), E_SIZE, None),
    (WS, dict(n_factors=0), E_SIZE, None),
    (WS, dict(n_factors=17), E_SIZE, None),
    (WS, dict(n_bins=0), E_SIZE, None),
    (WS, dict(n_bins=65), E_SIZE, None),
]


@pytest.mark.parametrize('entry,changes,code,text', CASES,
                         ids=['%s-%s' % (c[0][6:], '-'.join('%s=%s' % kv for kv in c[1].items())) for c in CASES])
def test_refusals(entry, changes, code, text):
    assert refusal(VALID, entry, changes) == (code, text)


def test_workspace_and_capacities():
    L = _lib.lib()
    assert L.smart_dynia_max_half_width() == 63 >= 63 and L.smart_dynia_lds_capacity() == 16384
    assert L.smart_dynia_workspace_bytes(4, 7, 1, 2, 2) == 7 * 32                     # every step
    assert L.smart_dynia_workspace_bytes(100000, 3653, 15, 10, 20) == (2 ** 28 // 800000) * 800000     # 335 steps in 256 MiB
    assert L.smart_dynia_workspace_bytes(2 ** 26, 10, 63, 16, 64) == 2 ** 29         # at least one step
    from smartpy_amd import analysis, engine
    assert analysis.dynia_max_half_width() == engine.dynia_max_half_width() == 63
    assert engine.dynia_lds_capacity() == 16384
    assert _lib.DYNIA_MAX_FACTORS == 16 and _lib.DYNIA_MAX_BINS == 64 and _lib.DYNIA_SUPPORTS == {'equal': 0, 'linear': 1}


def test_the_new_names_are_bound_and_the_words_are_checked_first():
    for name in ('smart_dynia_hip', 'smart_dynia_workspace_bytes', 'smart_dynia_max_half_width', 'smart_dynia_lds_capacity'):
        assert name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None
    assert _lib.SYMBOLS['smart_dynia_hip'][0] is ctypes.c_int and len(_lib.SYMBOLS['smart_dynia_hip'][1]) == 21
    from smartpy_amd import analysis, engine
    assert engine.dynamic_identifiability is analysis.dynamic_identifiability and engine.DyniaResult is analysis.DyniaResult
    # what can be refused from the words and the shapes is refused before a device is looked for
    with pytest.raises(engine.SmartEngineError, match="support 'quadratic' unknown") as err:
        engine.dynamic_identifiability(SIM, OBS, CAT, 2, 1, support='quadratic')
    assert err.value.code == -7
    with pytest.raises(engine.SmartEngineError, match=r'categories must be uint8 \[factors, 4\]') as err:
        engine.dynamic_identifiability(SIM, OBS, CAT.astype(np.int32), 2, 1)
    assert err.value.code == -2
    with pytest.raises(engine.SmartEngineError, match=r'categories must be uint8 \[factors, 4\]'):
        engine.dynamic_identifiability(SIM, OBS, CAT[:, :3], 2, 1)


def test_no_cpu_fallback():
    import torch
    from smartpy_amd import engine
    if torch.cuda.is_available():
        pytest.skip('a GPU is present: tests/test_gpu_dynia.py runs the analysis for real')
    with pytest.raises(Exception, match='no CPU fallback'):
        engine.dynamic_identifiability(SIM, OBS, CAT, 2, 1)
