"""Sobol sensitivity indices, host side: the numpy statement of smart_sobol_indices_hip (the truth of
tests/test_gpu_sobol.py as well) with its sums in math.fsum, that statement against the analytic indices of the Ishigami
function, the Saltelli design, the bootstrap counts, the C entry's validation without a device and the two file writers."""
import inspect
import math

import numpy as np
import pytest

from oracle.analyses.sobol import design_values, ishigami, sobol_statement
from support import E_NO_DEVICE, E_NULL, E_SIZE, FAKE

NAMES = ['T', 'C', 'H', 'D', 'S', 'Z', 'SK', 'FK', 'GK', 'RK']
RANGES = {p: (float(i + 1), float(3 * i + 5)) for i, p in enumerate(NAMES)}


# ---- the design ------------------------------------------------------------------------------------------------------
def test_saltelli_design_blocks_strata_and_fixed_parameters():
    from smartpy_amd.sampling import saltelli_design, PARAMETER_NAMES
    assert list(inspect.signature(saltelli_design).parameters) == ['base_size', 'ranges', 'names', 'vary', 'fixed', 'seed']
    n = 37
    X, vary = saltelli_design(n, RANGES, seed=5)
    assert vary == PARAMETER_NAMES == NAMES and X.shape == (n * 12, 10) and X.dtype == np.float64
    A, B = X[:n], X[n:2 * n]
    for j in range(10):
        AB = X[(2 + j) * n:(3 + j) * n]
        others = [c for c in range(10) if c != j]
        assert np.array_equal(AB[:, others].view(np.int64), A[:, others].view(np.int64))
        assert np.array_equal(AB[:, j].view(np.int64), B[:, j].view(np.int64)) and not np.array_equal(AB[:, j], A[:, j])
    for block in (A, B):
        for j, p in enumerate(NAMES):
            lo, hi = RANGES[p]
            unit = (block[:, j] - lo) / (hi - lo)
            assert sorted(np.floor(unit * n + 1e-9).astype(int).tolist()) == list(range(n)), p
    assert not np.array_equal(A, B)
    # vary / fixed: the others are constant, at the midpoint unless told
    X3, vary3 = saltelli_design(n, RANGES, vary=['SK', 'T', 'Z'], fixed={'C': 2.25}, seed=5)
    assert vary3 == ['SK', 'T', 'Z'] and X3.shape == (n * 5, 10)
    for j, p in enumerate(NAMES):
        if p in vary3:
            assert len(set(X3[:, j].tolist())) > n
        else:
            assert set(X3[:, j].tolist()) == {2.25 if p == 'C' else 0.5 * (RANGES[p][0] + RANGES[p][1])}
    assert np.array_equal(X3[4 * n:, 5], X3[n:2 * n, 5]) and np.array_equal(X3[4 * n:, 0], X3[:n, 0])   # AB_2 moves 'Z'
    assert np.array_equal(X3[2 * n:3 * n, 6], X3[n:2 * n, 6])                                             # AB_0 moves 'SK'


def test_saltelli_design_is_seeded_and_leaves_the_legacy_stream_alone():
    from smartpy_amd.sampling import saltelli_design
    np.random.seed(77)
    before = np.random.rand(3)
    np.random.seed(77)
    a, _ = saltelli_design(16, RANGES, seed=9)
    after = np.random.rand(3)
    assert np.array_equal(before, after)
    b, _ = saltelli_design(16, RANGES, seed=9)
    c, _ = saltelli_design(16, RANGES, seed=10)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    with pytest.raises(Exception, match="'XK'"):
        saltelli_design(16, RANGES, vary=['T', 'XK'])
    for bad in (0, -3):
        with pytest.raises(Exception, match='base_size'):
            saltelli_design(bad, RANGES)


# ---- the counts ------------------------------------------------------------------------------------------------------
def test_bootstrap_counts():
    from smartpy_amd import engine, _lib
    cap = engine.sobol_max_resamples()
    assert cap == _lib.lib().smart_sobol_max_resamples() >= 128
    c = engine.sobol_counts(100, 37, seed=3)
    assert c.shape == (100, 37) and c.dtype == np.uint16 and c.flags['C_CONTIGUOUS']
    assert np.all(c.sum(axis=0) == 100)
    assert np.array_equal(c, engine.sobol_counts(100, 37, seed=3)) and not np.array_equal(c, engine.sobol_counts(100, 37, seed=4))
    draws = np.random.Generator(np.random.PCG64(3)).integers(100, size=(37, 100))
    assert np.array_equal(c[:, 5], np.bincount(draws[5], minlength=100))
    assert engine.sobol_counts(5, 0).shape == (5, 0) and engine.sobol_counts(7, cap).shape == (7, cap)
    with pytest.raises(engine.SmartEngineError, match='resamples') as e:
        engine.sobol_counts(10, cap + 1)
    assert e.value.code == E_SIZE
    with pytest.raises(engine.SmartEngineError, match='n_base'):
        engine.sobol_counts(0, 4)


# ---- the statement against analytic truth ----------------------------------------------------------------------------
ISHIGAMI_S1 = [0.3139, 0.4424, 0.0, 0.0]
ISHIGAMI_ST = [0.5576, 0.4424, 0.2437, 0.0]


def ishigami_values(n, seed):
    from smartpy_amd.sampling import saltelli_design
    names = ['x1', 'x2', 'x3', 'x4']
    X, vary = saltelli_design(n, {p: (-math.pi, math.pi) for p in names}, names=names, seed=seed)
    assert vary == names and X.shape == (6 * n, 4)
    return ishigami(X)


def test_statement_finds_the_ishigami_indices():
    """A sampling error, not a rounding one: with this construction the worst deviation over seeds 0-19 at n = 4,096 was
    0.043; gate 0.06.  A design with A and B swapped, or the wrong column exchanged, misses it by tenths."""
    n = 4096
    y = ishigami_values(n, seed=11)
    got = sobol_statement(y, n, 4)
    print('S1', got['S1'][0], 'ST', got['ST'][0])
    assert np.max(np.abs(got['S1'][0] - ISHIGAMI_S1)) < 0.06 and np.max(np.abs(got['ST'][0] - ISHIGAMI_ST)) < 0.06
    assert abs(got['mu'][0] - 3.5) < 0.1 and abs(got['V'][0] - 13.845) < 0.5
    # the inert input: exactly +0.0, not a small number
    for name in ('S1', 'ST'):
        assert got[name][0, 3] == 0.0 and not np.signbit(got[name][0, 3])
    # the wrong column exchanged (AB_0 and AB_1 swapped) fails the same gate
    wrong = y.copy()
    wrong[2 * n:3 * n], wrong[3 * n:4 * n] = y[3 * n:4 * n], y[2 * n:3 * n]
    assert np.max(np.abs(sobol_statement(wrong, n, 4)['S1'][0] - ISHIGAMI_S1)) > 0.06


def test_statement_rules_and_bootstrap():
    from smartpy_amd import engine
    n, k = 50, 3
    y = design_values(1, n, k, 4, inert=1)
    y[2, 17] = np.inf
    y[3, :] = 2.5
    counts = engine.sobol_counts(n, 9, seed=0)
    counts[:, 0] = 1                                    # a replicate of all ones is the point estimate
    got = sobol_statement(y, n, k, counts, bounds=True)
    for name in ('S1', 'ST', 'S1_std', 'ST_std'):
        assert np.isnan(got[name][2:]).all() and not np.isnan(got[name][:2]).any()
        assert np.all(got[name][:2, 1] == 0.0) and not np.signbit(got[name][:2, 1]).any()
        assert np.all(got['bound_' + name][:2] < 1e-12)
    assert np.isnan(got['mu'][2]) and got['mu'][3] == 2.5 and got['V'][3] == 0.0
    one = sobol_statement(y[:2], n, k, np.ones((n, 1), dtype=np.uint16))
    assert np.isnan(one['S1_std']).all()                # B = 1
    assert sobol_statement(y[:2], n, k)['S1_std'] is None
    # replicates that all hold every base row once are all the point estimate: no spread
    same = sobol_statement(y[:2], n, k, np.ones((n, 4), dtype=np.uint16))
    assert np.all(same['S1_std'] == 0.0) and np.all(same['ST_std'] == 0.0)
    assert np.array_equal(same['S1'], got['S1'][:2]) and np.array_equal(sobol_statement(y[0], n, k)['ST'][0], got['ST'][0])


# ---- the C entry -----------------------------------------------------------------------------------------------------
def test_symbols_and_constants():
    from smartpy_amd import _lib, engine
    L = _lib.lib()
    for name in ('smart_sobol_indices_hip', 'smart_sobol_workspace_bytes', 'smart_sobol_max_resamples',
                 'smart_sobol_lds_capacity'):
        assert name in _lib.SYMBOLS
    assert L.smart_abi_version() == 7
    assert engine.sobol_lds_capacity() == L.smart_sobol_lds_capacity() == 8192      # 16 bytes per base row in 128 KiB
    assert L.smart_sobol_workspace_bytes(8192, 10, 3653, 128) >= 0
    for bad in ((0, 10, 1, 0), (5, 0, 1, 0), (5, 17, 1, 0), (5, 3, 0, 0), (5, 3, 1, -1),
                (5, 3, 1, L.smart_sobol_max_resamples() + 1)):
        assert L.smart_sobol_workspace_bytes(*bad) == E_SIZE, bad


def test_validation_comes_before_the_device():
    from smartpy_amd import _lib
    L = _lib.lib()
    cap = L.smart_sobol_max_resamples()

    def call(n=64, k=3, rows=2, y=FAKE, ld=None, s1=FAKE, st=FAKE, mom=FAKE, counts=None, B=0, s1_std=None, st_std=None,
             work=None, work_bytes=0):
        rc = L.smart_sobol_indices_hip(n, k, rows, y, n * (k + 2) if ld is None else ld, s1, st, mom, counts, B, s1_std,
                                       st_std, work, work_bytes, None)
        return rc, L.smart_last_error().decode()

    for name in ('y', 's1', 'st', 'mom'):
        rc, text = call(**{name: None})
        assert rc == E_NULL and 'smart_sobol_indices_hip' in text and '(%s is NULL)' % {'mom': 'moments'}.get(name, name) in text
    for kw, name in ((dict(), 'counts'), (dict(counts=FAKE), 's1_std'), (dict(counts=FAKE, s1_std=FAKE), 'st_std')):
        rc, text = call(B=4, **kw)
        assert rc == E_NULL and '(%s is NULL)' % name in text
    for kw, word in ((dict(n=0), 'n_base'), (dict(n=-1), 'n_base'), (dict(n=2 ** 31), 'n_base'), (dict(k=0), 'n_params'),
                     (dict(k=17), 'n_params'), (dict(rows=0), 'n_rows'), (dict(B=-1), 'n_resamples'),
                     (dict(B=cap + 1, counts=FAKE, s1_std=FAKE, st_std=FAKE), 'n_resamples'),
                     (dict(ld=64 * 5 - 1), 'ld'), (dict(work_bytes=-8), 'workspace_bytes')):
        rc, text = call(**kw)
        assert rc == E_SIZE and 'smart_sobol_indices_hip' in text and word in text, (kw, text)
    assert call(y=None, n=0)[0] == E_NULL                   # NULL before SIZE
    if L.smart_device_count() == 0:
        # a well-formed call gets as far as the device, and no further: there is no CPU fallback
        for kw in (dict(), dict(ld=64 * 5 + 3), dict(n=1, k=16, rows=1), dict(B=cap, counts=FAKE, s1_std=FAKE, st_std=FAKE),
                   dict(n=100000, k=10, rows=8)):
            assert call(**kw)[0] == E_NO_DEVICE, kw


def test_engine_and_workflow_surface():
    from smartpy_amd import engine
    from smartpy_amd.montecarlo import Sobol
    from smartpy_amd.montecarlo.montecarlo import MonteCarlo
    assert list(inspect.signature(engine.sobol_indices).parameters) == ['values', 'n_base', 'n_params', 'counts']
    assert list(inspect.signature(engine.sobol_counts).parameters) == ['n_base', 'resamples', 'seed']
    with pytest.raises(engine.SmartEngineError, match='columns are not n_base') as e:
        engine.sobol_indices(np.ones((2, 99)), 20, 3)
    assert e.value.code == E_SIZE
    with pytest.raises(engine.SmartEngineError, match='counts must be uint16'):
        engine.sobol_indices(np.ones((2, 100)), 20, 3, counts=np.ones((20, 4)))
    assert issubclass(Sobol, MonteCarlo) and Sobol.run is MonteCarlo.run
    assert list(inspect.signature(Sobol.__init__).parameters) == ['self', 'catchment', 'root_f', 'in_format', 'out_format',
                                                                  'base_size', 'parallel', 'save_sim', 'settings_filename',
                                                                  'vary', 'fixed', 'seed']
    sig = inspect.signature(Sobol.sensitivity)
    assert {k: p.default for k, p in sig.parameters.items() if k != 'self'} == \
        dict(targets=None, resamples=128, conf_level=0.95, seed=None, write=False)
    sig = inspect.signature(Sobol.sensitivity_series)
    assert {k: p.default for k, p in sig.parameters.items() if k != 'self'} == \
        dict(resamples=0, conf_level=0.95, seed=None, write=False)
    from smartpy_amd.montecarlo.sobol import normal_quantile
    assert abs(normal_quantile(0.95) - 1.959964) < 1e-6
    with pytest.raises(Exception, match='between 0 and 1'):
        normal_quantile(1.0)


# ---- the files -------------------------------------------------------------------------------------------------------
def test_the_indices_and_series_files(tmp_path):
    from datetime import datetime, timedelta
    from smartpy_amd.montecarlo.sobol import _write_indices_file, _write_series_file, series_header_line, INDICES_HEADER
    M, k = 2, 3
    S1 = (np.arange(M * k, dtype=np.float64).reshape(M, k) + 0.25) / 7.0
    ST = S1 * 1.5 + 1.0 / 3.0
    c1, ct = S1 / 11.0, ST / 13.0
    S1[1, 2] = np.nan
    path = str(tmp_path / 'x.indices')
    _write_indices_file(path, ['NSE', 'GW'], ['T', 'SK', 'RK'], S1, c1, ST, ct)
    lines = open(path).read().split('\n')
    assert lines[0] + '\n' == INDICES_HEADER == 'target,parameter,S1,S1_conf,ST,ST_conf\n'
    assert lines[-1] == '' and len(lines) == M * k + 2
    want = []
    for m, t in enumerate(['NSE', 'GW']):
        for j, p in enumerate(['T', 'SK', 'RK']):
            want.append([t, p] + ['%.6e' % np.float32(v) for v in (S1[m, j], c1[m, j], ST[m, j], ct[m, j])])
    assert [line.split(',') for line in lines[1:-1]] == want
    _write_indices_file(path, ['NSE', 'GW'], ['T', 'SK', 'RK'], S1, None, ST, None)      # no resamples: NaN columns
    assert open(path).read().split('\n')[1].split(',')[3] == '%.6e' % np.float32(np.nan)
    R = 5
    stamps = [datetime(2007, 1, 1, 9) + timedelta(days=r) for r in range(R)]
    S1, ST = np.linspace(0.0, 1.0, R * k).reshape(R, k) / 3.0, np.linspace(1.0, 2.0, R * k).reshape(R, k) / 7.0
    path = str(tmp_path / 'x.series')
    _write_series_file(path, stamps, ['T', 'SK', 'RK'], S1, ST)
    lines = open(path).read().split('\n')
    assert lines[0] + '\n' == series_header_line(['T', 'SK', 'RK']) == 'DateTime,S1_T,S1_SK,S1_RK,ST_T,ST_SK,ST_RK\n'
    assert len(lines) == R + 2 and lines[-1] == ''
    for r in range(R):
        assert lines[1 + r].split(',') == [stamps[r].strftime('%Y-%m-%d %H:%M:%S')] + \
            ['%.6e' % np.float32(v) for v in list(S1[r]) + list(ST[r])]
    assert not [f for f in tmp_path.iterdir() if f.name.endswith('.rows')]
