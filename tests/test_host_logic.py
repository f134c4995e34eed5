"""Host-side logic around the hot path, on CPU: time axes, input pipeline, settings / parameters files,
sampler, conditioning rules, database format, sharding arithmetic.  Expected values come from the reference
(tests/golden/*.npz) or from its documented file formats."""
import gzip
import os
from datetime import datetime, timedelta

import numpy as np
import pytest

from conftest import load_golden, GOLDEN

DATA = os.path.join(GOLDEN, 'data')
CATCH = os.path.join(DATA, 'in', 'Catchment', 'Catchment')
START, END = datetime(2007, 1, 1, 9), datetime(2016, 12, 31, 9)


# ---- time axes (timeframe.py:50-115) -----------------------------------------------------------------------
def test_timeframe_axes():
    from smartpy_amd.timeframe import TimeFrame
    tf = TimeFrame(START, END, timedelta(hours=1), timedelta(days=1))
    assert (tf.n_steps, tf.n_reports, tf.report_gap) == (87672, 3653, 24)
    assert tf.simu_series[0] == datetime(2006, 12, 31, 9) and tf.simu_series[1] == datetime(2006, 12, 31, 10)
    assert tf.simu_series[-1] == END and tf.save_series[0] == datetime(2006, 12, 31, 9) and tf.save_series[-1] == END
    assert tf.get_series_simu() is tf.simu_series and tf.get_gap_report() == timedelta(days=1)
    td = TimeFrame(START, END, timedelta(days=1), timedelta(days=1))
    assert (td.n_steps, td.n_reports, td.report_gap) == (3653, 3653, 1) and td.simu_series[1] == START
    with pytest.raises(Exception, match='Save Start is greater'):
        TimeFrame(END, START, timedelta(hours=1), timedelta(days=1))
    with pytest.raises(Exception, match='not compatible'):
        TimeFrame(START, END + timedelta(hours=5), timedelta(hours=1), timedelta(days=1))
    with pytest.raises(Exception, match='multiple of Simulation Gap'):
        TimeFrame(START, END, timedelta(hours=7), timedelta(days=1))


# ---- input pipeline: the arrays the engine consumes, bit-identical to the reference's (smart.py:130-143) ------
@pytest.mark.parametrize('delta,per', [(timedelta(hours=1), 24), (timedelta(days=1), 1), (timedelta(hours=6), 4)])
def test_forcing_arrays_match_the_reference(delta, per):
    from smartpy_amd.timeframe import TimeFrame
    from smartpy_amd import inout
    g = load_golden('forcing_example.npz')
    tf = TimeFrame(START, END, delta, timedelta(days=1))
    rain = inout.get_rain_series_simu(CATCH + '.rain', 'csv', tf.simu_series[1], tf.simu_series[-1], delta)
    peva = inout.get_peva_series_simu(CATCH + '.peva', 'csv', tf.simu_series[1], tf.simu_series[-1], delta)
    if per in (24, 1):          # produced by the reference itself
        assert np.array_equal(rain, np.repeat(g['rain_daily'] / per, per))
        assert np.array_equal(peva, np.repeat(g['peva_daily'] / per, per))
    else:                       # 6-hourly on 09:00 daily data: resolution gcd = 6 h, a quarter of the day each
        assert np.array_equal(rain, np.repeat(g['rain_daily'] / 4, 4))
    assert abs(rain.sum() - g['rain_daily'].sum()) < 1e-8 * g['rain_daily'].sum()      # mass is conserved


@pytest.mark.parametrize('tag,hh', [('aligned', 9), ('shifted', 12)])
def test_resampling_with_reaggregation_matches_the_reference(tag, hh):
    """KAT-10: 6-hourly steps; shifted to 12:00 the common resolution is 3 h and every step sums two portions,
    and the observation windows straddle two daily means (timeframe.py:158-309)."""
    from smartpy_amd.timeframe import TimeFrame
    from smartpy_amd import inout
    g = load_golden('kat10_resampling.npz')
    tf = TimeFrame(datetime(2007, 1, 1, hh), datetime(2007, 12, 31, hh), timedelta(hours=6), timedelta(days=1))
    for var, fn in (('rain', inout.get_rain_series_simu), ('peva', inout.get_peva_series_simu)):
        got = fn(CATCH + '.' + var, 'csv', tf.simu_series[1], tf.simu_series[-1], timedelta(hours=6))
        assert np.array_equal(got, g[var + '_' + tag])
    obs = inout.get_discharge_series(CATCH + '.flow', 'csv', tf.save_series[1], tf.save_series[-1], 175.46e6, 175.97e6)
    assert np.array_equal(obs, g['flow_' + tag], equal_nan=True)


def test_observation_array_matches_the_reference_and_g3():
    from smartpy_amd.timeframe import TimeFrame
    from smartpy_amd import inout
    g = load_golden('forcing_example.npz')
    g3 = load_golden('g2_g3_example_flows.npz')['obs_flow']
    tf = TimeFrame(START, END, timedelta(hours=1), timedelta(days=1))
    obs = inout.get_discharge_series(CATCH + '.flow', 'csv', tf.save_series[1], tf.save_series[-1],
                                     175.46e6, 175.97e6)
    assert np.array_equal(obs, g['flow_obs'], equal_nan=True) and int(np.isnan(obs).sum()) == 425
    ok = ~np.isnan(obs)
    assert ['%e' % v for v in obs[ok]] == ['%e' % v for v in g3[ok]]       # examples/out/.../ExampleDaily.obs.flow


def test_insufficient_or_irregular_data_raise(tmp_path):
    from smartpy_amd import inout
    with pytest.raises(Exception, match='Rain data not sufficient'):
        inout.get_rain_series_simu(CATCH + '.rain', 'csv', datetime(1999, 1, 1, 9), datetime(1999, 2, 1, 9),
                                   timedelta(days=1))
    with pytest.raises(Exception, match='could not be found'):
        inout.get_peva_series_simu(str(tmp_path / 'nope.peva'), 'csv', START, END, timedelta(days=1))
    bad = tmp_path / 'gap.rain'
    bad.write_text('DateTime,rain\n2000-01-01 09:00:00,1.0\n2000-01-02 09:00:00,1.0\n2000-01-04 09:00:00,1.0\n')
    with pytest.raises(Exception, match='Inconsistent Interval'):
        inout.get_rain_series_simu(str(bad), 'csv', datetime(2000, 1, 2, 9), datetime(2000, 1, 3, 9), timedelta(days=1))
    with pytest.raises(Exception, match="netCDF4"):
        inout.get_rain_series_simu(CATCH + '.rain.nc', 'netcdf', START, END, timedelta(days=1))


def test_settings_and_parameters_files(tmp_path):
    from smartpy_amd import inout
    from smartpy_amd.parameters import Parameters
    s = inout.get_dict_simulation_settings(CATCH + '.sttngs')
    assert s == (175.46e6, 175.97e6, START, END, timedelta(hours=1), timedelta(days=1), 365, 0.12667)
    minimal = tmp_path / 'm.sttngs'
    minimal.write_text('ARGUMENT,VALUE\ncatchment_area_km2,10\nstart_datetime,01/01/2007 09:00:00\n'
                       'end_datetime,02/01/2007 09:00:00\nsimu_timedelta_min,60\nreport_timedelta_min,1440\n'
                       'warm_up_days,0\n')
    m = inout.get_dict_simulation_settings(str(minimal))
    assert m[1] == m[0] == 10e6 and m[7] is None                                   # inout.py:98,137
    minimal.write_text('ARGUMENT,VALUE\ncatchment_area_km2,ten\n')
    with pytest.raises(Exception, match='CATCHMENT AREA could not be converted'):
        inout.get_dict_simulation_settings(str(minimal))
    p = Parameters()
    assert p.names == ['T', 'C', 'H', 'D', 'S', 'Z', 'SK', 'FK', 'GK', 'RK'] and p.ranges['RK'] == (1.0, 96.0)
    p.set_parameters_with_file(CATCH + '.parameters')
    assert np.array_equal([p.values[n] for n in p.names], load_golden('forcing_example.npz')['params'])
    with pytest.raises(Exception, match='not available in the dictionary'):
        Parameters().set_parameters_with_dict({'T': 1.0})


def test_flow_writer_format(tmp_path):
    """'%e' values, csv.writer line endings (inout.py:291-296); round trip through the G2 numbers."""
    from smartpy_amd import inout
    g2 = load_golden('g2_g3_example_flows.npz')['mod_flow']
    stamps = [START + timedelta(days=k) for k in range(len(g2))]
    out = tmp_path / 'x.mod.flow'
    inout.write_flow_file_from_nds(stamps, g2, str(out), 'csv')
    raw = out.read_bytes().split(b'\r\n')
    assert raw[0] == b'DateTime,flow' and raw[1] == b'2007-01-01 09:00:00,4.135082e+00' and raw[-1] == b''
    with pytest.raises(Exception, match='cannot be written by SMARTpy'):
        inout.write_flow_file_from_nds(stamps, g2, str(out), 'xlsx')


# ---- sampler (lhs.py:133-167) ----------------------------------------------------------------------------------
def test_latin_hypercube_is_the_reference_stream():
    from smartpy_amd.sampling import latin_hypercube
    from smartpy_amd.parameters import Parameters
    g = load_golden('kat7_lhs.npz')
    for key in g.files:
        seed, n = key.split('_')
        assert np.array_equal(latin_hypercube(int(n[1:]), Parameters().ranges, seed=int(seed[4:])), g[key]), key
    np.random.seed(42)                                  # seed=None continues the global stream like the reference
    assert np.array_equal(latin_hypercube(64, Parameters().ranges), g['seed42_n64'])
    narrow = dict(Parameters().ranges, T=(1.0, 1.0))
    assert np.all(latin_hypercube(10, narrow, seed=1)[:, 0] == 1.0)


# ---- conditioning rules (glue.py:222-289, best.py:221-287) ------------------------------------------------------
def test_glue_and_best_selection_rules():
    from smartpy_amd.montecarlo.glue import GLUE
    from smartpy_amd.montecarlo.best import Best
    rng = np.random.default_rng(0)
    params = rng.random((50, 10)).astype(np.float32)
    fns = rng.normal(size=(50, 3)).astype(np.float32)
    fns[:, 2] = rng.integers(0, 2, 50)
    sel = GLUE._get_behavioural_sets(params, fns, [(0.0,), (-0.5, 0.5), (1.0,)], ['min', 'inside', 'equal'])
    want = params[(fns[:, 0] >= 0) & (fns[:, 1] >= -0.5) & (fns[:, 1] <= 0.5) & (fns[:, 2] == 1)]
    assert np.array_equal(sel, want) and 0 < len(sel) < 50
    assert len(GLUE._get_behavioural_sets(params, fns[:, :1], [(0.3,)], ['max'])) == int((fns[:, 0] <= 0.3).sum())
    # 'outside' is written (x <= lo) & (x >= hi) in the reference: never true
    assert len(GLUE._get_behavioural_sets(params, fns[:, :1], [(-0.5, 0.5)], ['outside'])) == 0
    with pytest.raises(Exception, match='inconsistent'):
        GLUE._get_behavioural_sets(params, fns[:, :1], [(0.5, -0.5)], ['inside'])
    with pytest.raises(Exception, match='not in the database'):
        GLUE._get_behavioural_sets(params, fns[:, :1], [(0.5,)], ['above'])
    with pytest.raises(Exception, match='compatible dimensions'):
        GLUE._get_behavioural_sets(params, fns, [(0.5,)], ['min'])
    # Best keeps the LARGEST nb_best values of the target, after the constraints
    best = Best._get_best_sets(params, fns[:, 2:3], [(1.0,)], ['equal'], fns[:, 0:1], 5)
    keep = fns[:, 2] == 1
    order = np.argsort(fns[keep, 0])
    assert np.array_equal(best, params[keep][order][-5:])
    assert np.array_equal(Best._get_best_sets(params, fns[:, :0], [], [], fns[:, 1:2], 3),
                          params[np.argsort(fns[:, 1])][-3:])
    with pytest.raises(Exception, match='higher than the sample size'):
        Best._get_best_sets(params, fns[:, :0], [], [], fns[:, 0:1], 51)
    with pytest.raises(Exception, match='restrained sample size'):
        Best._get_best_sets(params, fns[:, 2:3], [(1.0,)], ['equal'], fns[:, 0:1], 49)


def test_selection_on_tensors_matches_numpy():
    """The same rules on torch tensors (device-side selection of behavioural / best rows)."""
    import torch
    from smartpy_amd.montecarlo.selection import condition_mask, best_rows
    rng = np.random.default_rng(3)
    fns = rng.normal(size=(500, 4))
    vals, kinds = [(0.0,), (-1.0, 0.5), (0.2,), (-0.3, 0.3)], ['min', 'inside', 'max', 'outside']
    m_np = condition_mask(fns[:, :3], vals[:3], kinds[:3])
    m_t = condition_mask(torch.from_numpy(fns[:, :3]), vals[:3], kinds[:3])
    assert isinstance(m_t, torch.Tensor) and np.array_equal(m_t.numpy(), m_np) and 0 < m_np.sum() < 500
    assert int(condition_mask(torch.from_numpy(fns), vals, kinds).sum()) == 0          # 'outside' never holds
    b_np = best_rows(fns[:, 3], m_np, 7)
    b_t = best_rows(torch.from_numpy(fns[:, 3]), m_t, 7)
    assert np.array_equal(b_t.numpy(), b_np) and np.all(np.diff(fns[b_np, 3]) >= 0)
    assert set(b_np) == set(np.nonzero(m_np)[0][np.argsort(fns[m_np, 3])][-7:])


def test_device_latin_hypercube_is_latin():
    import torch
    from smartpy_amd.sampling import latin_hypercube_device
    from smartpy_amd.parameters import Parameters
    p = Parameters()
    x = latin_hypercube_device(1000, p.ranges, seed=5, device='cpu')
    assert x.shape == (1000, 10) and x.dtype == torch.float64
    lo = np.array([p.ranges[n][0] for n in p.names])
    hi = np.array([p.ranges[n][1] for n in p.names])
    strata = np.floor((x.numpy() - lo) / (hi - lo) * 1000).astype(int)
    assert all(sorted(np.clip(strata[:, j], 0, 999)) == list(range(1000)) for j in range(10))   # one per stratum
    assert torch.equal(x, latin_hypercube_device(1000, p.ranges, seed=5, device='cpu'))
    assert not torch.equal(x, latin_hypercube_device(1000, p.ranges, seed=6, device='cpu'))
    assert abs(np.corrcoef(x[:, 0].numpy(), x[:, 5].numpy())[0, 1]) < 0.15                      # columns independent


# ---- sampling database format (montecarlo.py:123-127, 211-262) ---------------------------------------------------
@pytest.mark.parametrize('save_sim', [False, True])
def test_sampling_database_csv_round_trip(tmp_path, save_sim):
    """montecarlo/database.py: header, float32 '%.6e' rows (bulk writer and the per-sample one give the same text),
    reading back by column name, gzip."""
    from smartpy_amd.montecarlo.database import database_for, SamplingCsv
    g4 = load_golden('g4_example_lhs.npz')
    names = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE', 'GW']
    pnames = ['T', 'C', 'H', 'D', 'S', 'Z', 'SK', 'FK', 'GK', 'RK']
    stamps = [START + timedelta(days=k) for k in range(3)] if save_sim else None
    sims = g4['discharge'][:, :3]
    path = str(tmp_path / 'C.SMART.lhs')
    db = database_for('csv', path, names, pnames)
    assert isinstance(db, SamplingCsv)
    db.create(10, stamps)
    db.write_table(g4['objfns'], g4['params'], sims)
    db.close()
    lines = open(path).read().split('\n')
    head = ','.join(names + pnames + (['2007-01-01 09:00:00', '2007-01-02 09:00:00', '2007-01-03 09:00:00']
                                      if save_sim else []))
    assert lines[0] == head and len(lines) == 12 and lines[-1] == ''
    row = [g4['objfns'][0], g4['params'][0]] + ([sims[0]] if save_sim else [])
    assert lines[1] == ','.join('%.6e' % np.float32(x) for x in np.concatenate(row))      # montecarlo.py:225-231
    params, fns = db.read()
    # '%.6e' keeps 7 significant digits: the second stage sees the sample to ~1e-7, as in the reference
    assert params.dtype == np.float32 and np.allclose(params, g4['params'], rtol=1e-6, atol=0)
    assert np.allclose(fns, g4['objfns'], rtol=1e-6)
    # ... which is what selection.as_stored reproduces without a database (device-side second stages)
    from smartpy_amd.montecarlo.selection import as_stored
    assert np.array_equal(as_stored(g4['params']), params) and np.array_equal(as_stored(g4['objfns']), fns)
    # a reader asking for fewer / reordered objective functions finds them by header name
    p_again, nse_rmse = database_for('csv', path, ['RMSE', 'NSE'], pnames).read()
    assert np.array_equal(p_again, params) and np.array_equal(nse_rmse, fns[:, [6, 0]])
    with pytest.raises(KeyError):
        database_for('csv', path, ['NSE', 'Bias'], pnames).read()
    # the per-sample writer of the reference protocol gives the same text
    one = database_for('csv', str(tmp_path / 'D.SMART.lhs'), names, pnames).create(10, stamps)
    for r in range(10):
        one.write_sample(None, list(g4['objfns'][r]), g4['params'][r], sims[r])
    one.close()
    assert open(one.path).read() == open(path).read()
    db.compress(None)
    assert os.path.exists(path)
    db.compress(True)                                                                      # montecarlo.py:171-177
    assert not os.path.exists(path) and gzip.open(path + '.gz', 'rt').readline().strip() == head
    p2, f2 = db.read(gzipped=True)
    assert np.array_equal(p2, params) and np.array_equal(f2, fns)


def test_native_row_writer_prints_what_python_prints(tmp_path):
    """smart_db_append_rows (the library's host-side writer behind _write_rows) against '%.6e' % numpy.float32(x),
    character for character: random bit patterns over the whole float32 range, rounding ties, decade boundaries,
    subnormals, signed zeros, infinities and NaN."""
    import ctypes
    import io
    from smartpy_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(4)
    bits = rng.integers(0, 2 ** 32, size=(20000, 9), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.array([1999999.5, 2999999.5, 1000000.5, 9999999.5, 9999999.0, 1e7, 999999.94, 0.1, 1e-5, 1e10,
                        9.9999995e9, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 3.4028235e38], dtype=np.float32)
    halves = (np.arange(1000003, 1000003 + 7 * 18 * 50, 7, dtype=np.float32) + np.float32(0.5)).reshape(-1, 18)
    subnormal = np.arange(1, 18 * 40 + 1, dtype=np.uint32).view(np.float32).reshape(-1, 18)
    for table in (bits, np.stack([special, -special]), halves, subnormal):
        table = np.ascontiguousarray(table, dtype=np.float32)
        path = str(tmp_path / 'rows.csv')
        open(path, 'w').write('header\n')
        _lib.check(L.smart_db_append_rows(path.encode(), table.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                          table.shape[0], table.shape[1], 3))
        want = io.StringIO()
        for row in table:
            want.write(','.join('%.6e' % x for x in row) + '\n')
        assert open(path).read() == 'header\n' + want.getvalue()
    with pytest.raises(_lib.SmartEngineError, match='cannot open'):
        _lib.check(L.smart_db_append_rows(str(tmp_path / 'no' / 'dir.csv').encode(),
                                          table.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 1, 18, 0))


def test_native_row_parser_reads_what_numpy_reads():
    """smart_db_parse_rows (behind _get_sampled_sets_from_file) against str -> float64 -> float32, the conversion
    numpy.array(rows_of_str, dtype=float32) performs in the reference (montecarlo.py:262)."""
    import ctypes
    from smartpy_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(9)
    t = (rng.standard_normal((3000, 12)) * 10.0 ** rng.integers(-20, 20, (3000, 12))).astype(np.float32)
    t[3, 2], t[4, 5], t[5, 7] = np.nan, np.inf, -np.inf
    text = ''.join(','.join('%.6e' % x for x in row) + ('\r\n' if i % 7 == 0 else '\n') for i, row in enumerate(t))
    text = text + '\n'                                   # a trailing empty line is not a row
    want = np.array([[np.float32(float(c)) for c in ln.split(',')] for ln in text.split()], dtype=np.float32)
    cols = np.array([11, 0, 4, 4, 7], dtype=np.int32)
    out = np.full((3001, 5), -1, dtype=np.float32)
    body = text.encode()
    n = L.smart_db_parse_rows(body, len(body), 12, cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 5,
                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 3001, 3)
    assert n == 3000 and np.array_equal(out[:n], want[:, cols], equal_nan=True)
    bad = body.replace(b',', b';', 1)
    assert L.smart_db_parse_rows(bad, len(bad), 12, cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 5,
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 3001, 1) < 0
    assert b'malformed' in L.smart_last_error()
    assert L.smart_db_parse_rows(body, len(body), 12, cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 5,
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 10, 1) < 0      # no room


def test_dictionary_helpers_match_the_reference():
    """The reference's dictionary-keyed helpers (timeframe.py:167-309, inout.py:35-78,143-274) under their own
    names: the calls of tests/golden/make_golden.py::dict_helper_vectors repeated here, keys and values bit for bit."""
    from collections import OrderedDict
    from smartpy_amd import timeframe as tf, inout as io
    g = load_golden('kat11_dict_helpers.npz')
    epoch = datetime(1970, 1, 1)

    def same(d, tag):
        keys = list(d)
        t = np.array([(k - epoch).total_seconds() for k in keys])
        v = np.array([d[k] for k in keys], dtype=np.float64)
        assert np.array_equal(t, g[tag + '_t']), tag
        assert np.array_equal(v.view(np.int64), g[tag + '_v'].view(np.int64)), tag

    def as_dict(tag, kind=dict):
        return kind((epoch + timedelta(seconds=float(t)), float(v)) for t, v in zip(g[tag + '_t'], g[tag + '_v']))

    start = datetime(2010, 3, 1, 9)
    daily = as_dict('reg_in')
    res = tf.get_required_resolution(start, datetime(2010, 3, 2, 12), timedelta(days=1), timedelta(hours=3))
    assert res.total_seconds() == float(g['reg_res_sec'])
    inc = tf.increase_time_resolution_of_regular_cumulative_data(daily, start, start + timedelta(days=39),
                                                                 timedelta(days=1), res)
    same(inc, 'reg_inc')
    same(tf.decrease_time_resolution_of_regular_cumulative_data(inc, datetime(2010, 3, 2, 12), datetime(2010, 4, 5, 12),
                                                                timedelta(hours=6), res), 'reg_dec')
    same(tf.rescale_time_resolution_of_regular_cumulative_data(daily, start, start + timedelta(days=39),
                                                               timedelta(days=1), res, datetime(2010, 3, 2, 12),
                                                               datetime(2010, 4, 5, 12), timedelta(hours=3)), 'reg_resc')
    flows = as_dict('irr_in', OrderedDict)
    same(tf.increase_time_resolution_of_irregular_mean_data(flows, timedelta(days=1), timedelta(hours=1)), 'irr_inc')
    same(tf.rescale_time_resolution_of_irregular_mean_data(flows, datetime(2010, 3, 1, 9), datetime(2010, 3, 15, 9),
                                                           timedelta(days=1), timedelta(hours=1)), 'irr_resc')
    with pytest.raises(Exception, match='Time Deltas are not multiples of each other'):
        tf.increase_time_resolution_of_regular_cumulative_data(daily, start, start, timedelta(days=1), timedelta(hours=5))
    with pytest.raises(Exception, match='Decrease Resolution: Time Deltas are not multiples'):
        tf.decrease_time_resolution_of_regular_cumulative_data(daily, start, start, timedelta(hours=1), timedelta(hours=2))
    loc = os.path.join(GOLDEN, 'data', 'in', 'Catchment', 'Catchment')
    same(io.get_dict_rain_series_simu(loc + '.rain', 'csv', datetime(2007, 1, 1, 12), datetime(2007, 2, 1, 9),
                                      timedelta(hours=3)), 'rain_3h')
    same(io.get_dict_discharge_series(loc + '.flow', 'csv', datetime(2007, 1, 1, 9), datetime(2007, 3, 1, 9),
                                      175.46e6, 175.97e6), 'flow')
    raw, first, last, step = io.read_peva_file(loc + '.peva', 'csv')
    assert len(raw) == int(g['peva_raw_n']) and (first - epoch).total_seconds() == float(g['peva_raw_first']) and \
        (last - epoch).total_seconds() == float(g['peva_raw_last']) and step.total_seconds() == float(g['peva_raw_step'])
    assert len(io.read_flow_file(loc + '.flow', 'csv')) == int(g['flow_raw_n'])
    with pytest.raises(Exception, match='Rain data not sufficient'):
        io.get_dict_rain_series_simu(loc + '.rain', 'csv', datetime(2007, 1, 1, 12), datetime(2030, 2, 1, 9),
                                     timedelta(hours=3))
    assert io.valid_file_format('CSV') == 'csv' and tf.valid_delta_min('90') == timedelta(minutes=90)
    assert tf.valid_date('01/02/2007_09:00:00') == datetime(2007, 2, 1, 9)
    frame = tf.TimeFrame(datetime(2007, 1, 1, 9), datetime(2007, 1, 3, 9), timedelta(hours=6), timedelta(days=1))
    assert frame._get_list_save_dt_with_initial_conditions() == frame.save_series and \
        frame._get_list_simu_dt_with_initial_conditions() == frame.simu_series


def test_public_surface_has_every_name_of_the_reference():
    """tests/golden/api_surface.json lists the public functions, classes and methods of the reference's modules with
    their parameter names (generated by make_golden.py); the package must offer each under the same name with the
    same parameters, so that a script written against the reference runs after `import smartpy_amd as smartpy`."""
    import importlib
    import inspect
    import json
    with open(os.path.join(GOLDEN, 'api_surface.json')) as fh:
        ref = json.load(fh)
    problems = []
    for mod_name, names in ref.items():
        mine = importlib.import_module(mod_name.replace('smartpy', 'smartpy_amd', 1))
        for name, spec in names.items():
            obj = getattr(mine, name, None)
            if obj is None:
                problems.append('%s.%s missing' % (mod_name, name))
            elif isinstance(spec, list):
                if list(inspect.signature(obj).parameters) != spec:
                    problems.append('%s.%s%s' % (mod_name, name, inspect.signature(obj)))
            else:
                for meth, params in spec.items():
                    fn = getattr(obj, meth, None)
                    if fn is None:
                        problems.append('%s.%s.%s missing' % (mod_name, name, meth))
                    elif params is not None and list(inspect.signature(fn).parameters) != params:
                        problems.append('%s.%s.%s%s' % (mod_name, name, meth, inspect.signature(fn)))
    assert not problems, problems


def test_the_three_statements_of_the_row_classes_agree():
    """The rule that sends a parameter row to its arithmetic class is written down three times: on the device
    (smart_fast_model.h: wave_class, authoritative), in torch for whole matrices (engine.variant_classes, which groups
    the rows of a launch), and since round 5 in C on the host for ONE row (smart_row_class: smartcpp.allsteps and
    SMART.simulate() name one kernel per call with it).  The two host statements are compared here on default-range
    rows, daily and hourly, on rows with every kind of parameter that is none, and on given initial states; the GPU
    suite compares the torch one with the device (smart_plan_ensemble's bits)."""
    import ctypes
    import torch
    from smartpy_amd import engine, _lib
    from oracle import lhs_oracle
    L = _lib.lib()

    def one(row, dt, init=None, area=0.0):
        row = np.ascontiguousarray(row, dtype=np.float64)
        st = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
        return L.smart_row_class(row.ctypes.data, dt, None if st is None else st.ctypes.data, area)

    rng = np.random.default_rng(77)
    p = lhs_oracle.lhs_params(4000, seed=21)
    # a tenth of the rows get one parameter that is none, of every kind the rules name
    odd = rng.choice(len(p), 400, replace=False)
    kinds = [(0, -0.3), (0, 0.1), (1, -0.2), (2, 1.4), (2, -0.01), (3, 3.0), (3, -1.0), (4, 0.7), (4, -0.1), (5, 0.0),
             (5, 0.4), (5, 5e3), (6, 0.0), (7, -2.0), (8, 0.0), (9, -1.0), (9, 0.3), (6, 0.5), (0, np.nan), (4, np.inf),
             (9, np.nan), (5, -np.inf)]
    for n, r in enumerate(odd):
        col, val = kinds[n % len(kinds)]
        p[r, col] = val
    for dt in (86400.0, 3600.0, 900.0):
        want = engine.variant_classes(torch.from_numpy(p), dt).numpy()
        got = np.array([one(p[r], dt) for r in range(len(p))])
        assert np.array_equal(got, want), (dt, np.nonzero(got != want)[0][:5])
        assert set(np.unique(want)) >= {0, 2, 3}
    # given initial states: NaN, infinity, a negative volume, -0.0 (a zero like any other), soil above capacity
    q = lhs_oracle.lhs_params(256, seed=22)
    init = np.full((256, 12), 1e5)
    init[3, 0], init[9, 7], init[17, 11], init[25, 6], init[33, 4] = np.nan, np.inf, -1.0, 1e13, -0.0
    init[40:80, 5:11] = rng.uniform(0.0, 6e6, (40, 6))          # some of these stand far above capacity
    area = 175.46e6
    want = engine.variant_classes(torch.from_numpy(q), 3600.0, torch.from_numpy(init), [area]).numpy()
    got = np.array([one(q[r], 3600.0, init[r], area) for r in range(len(q))])
    assert np.array_equal(got, want) and (want[[3, 9, 17, 25]] == 3).all() and want[33] == 0 and (want[40:80] == 3).any()


def test_rccl_or_host_staging_is_decided_by_the_devices_the_ranks_sit_on():
    """distributed.init(): device tensors go through RCCL unless two ranks share one physical GPU -- told from the
    ranks' (host, UUID) identities, not from WORLD_SIZE against device_count() (round 4's rule, which sent a launch with
    one visible device per rank, or one over several nodes, through the host: advisor)."""
    from smartpy_amd import distributed as sdist
    eight = ['node-a/GPU-%02x' % k for k in range(8)]
    assert not sdist.shares_a_device(eight)                                     # one node, eight GPUs
    assert not sdist.shares_a_device(eight + ['node-b/GPU-%02x' % k for k in range(8)])     # two nodes, same UUID-less numbering
    assert not sdist.shares_a_device(['node-a/GPU-07'])
    assert sdist.shares_a_device(['box/GPU-00'] * 8)                            # the one-GPU box running the 8-rank path
    assert sdist.shares_a_device(eight[:7] + eight[:1])
    import os
    assert os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY') is not None            # set at import, ahead of any GPU call


# ---- sharding arithmetic -----------------------------------------------------------------------------------------
def test_rows_are_classified_and_grouped_by_arithmetic_variant():
    """engine.variant_classes mirrors wave_class() of csrc/smart_fast_model.h: 1 stiff (some k*3600 < dt), 2 guarded
    (S outside [0, 0.5], C < 0, Z <= 0), 3 ill-conditioned (dt / RK > 2 -- the river constant only: the catchment
    reservoirs' clamp at zero forgets a perturbation) or any NaN / infinite parameter; the most
    demanding wins.  _variant_grouping
    puts each class into whole wavefronts of 64 (padded with copies of its last row), keeps every row, and with
    sort_rows orders a class by T (64 bins), then S * Z."""
    import torch
    from smartpy_amd import engine
    from oracle import lhs_oracle
    p = lhs_oracle.lhs_params(3000, seed=9)
    dt = 86400.0
    p[:40, 6] = 0.5                 # dt / SK = 48: stiff, NOT ill-conditioned
    p[:40, 9] = 50.0
    p[40:60, 9] = 11.9              # dt / RK just above 2
    p[60:70, 9] = 12.0              # exactly 2: still the fast arithmetic (its STIFF variant: RK * 3600 < dt)
    p[60:70, 6:9] = 100.0
    p[70:80, 4] = 0.6               # S > 0.5: guarded ...
    p[80:90, 4], p[80:90, 9] = 0.6, 1.0     # ... unless the river sends the row to the literal model anyway
    cls = engine.variant_classes(torch.from_numpy(p), dt).numpy()
    k = p[:, 6:10] * 3600.0
    want = np.zeros(len(p), dtype=np.int64)
    want[(k < dt).any(axis=1)] = 1
    want[~((p[:, 4] >= 0) & (p[:, 4] <= 0.5) & (p[:, 1] >= 0) & (p[:, 5] > 0))] = 2
    want[k[:, 3] < 0.5 * dt] = 3
    assert np.array_equal(cls, want)
    assert (cls[:40] == 1).all() and (cls[40:60] == 3).all() and (cls[60:70] == 1).all()
    assert (cls[70:80][k[70:80, 3] >= 0.5 * dt] == 2).all() and (cls[80:90] == 3).all()
    assert engine.variant_classes(torch.from_numpy(p), 3600.0).max() == 2      # hourly steps: nothing stiff by default
    # a NaN or an infinite parameter anywhere in the row: the literal model decides what comes of it, at any step length
    q = lhs_oracle.lhs_params(64, seed=10)
    for row, (col, val) in enumerate([(0, np.nan), (2, np.inf), (3, -np.inf), (5, np.nan), (8, np.inf), (9, np.nan)]):
        q[row * 7, col] = val
    got = engine.variant_classes(torch.from_numpy(q), 3600.0).numpy()
    assert (got[[0, 7, 14, 21, 28, 35]] == 3).all() and (np.delete(got, [0, 7, 14, 21, 28, 35]) == 0).all()
    # ... or a share that is none (round 4): D or H outside [0, 1], a negative T -- negative inflows, the reference's clamps
    q = lhs_oracle.lhs_params(96, seed=13)
    for row, (col, val) in enumerate([(3, 300.0), (3, -0.1), (2, 1.5), (2, -1e-9), (0, -0.5), (6, -3.0), (8, 0.0),
                                      (5, 0.0), (0, 0.15), (5, 2.0e4), (5, 0.5), (3, 1.0), (2, 1.0)]):
        q[row * 7, col] = val
    got = engine.variant_classes(torch.from_numpy(q), 3600.0).numpy()
    odd = [0, 7, 14, 21, 28, 35, 42, 49, 56, 63, 70]  # (the bounds of the shares themselves are fine; a k or a Z <= 0 is not)
    assert (got[odd] == 3).all() and (np.delete(got, odd) == 0).all()
    # (... and T < 0.2 or Z > 1 m, rows 56 and 63: discharges orders below the rain's, where the last place of
    # the fast arithmetic's sums shows; Z < 1 mm, row 70)
    # ... and wild INITIAL states: a NaN, an infinity, a negative volume, soil so far above capacity that S tot / Z > 0.5
    q = lhs_oracle.lhs_params(64, seed=11)
    init = np.full((64, 12), 1e5)
    init[3, 0], init[9, 7], init[17, 11], init[25, 6], init[33, 4] = np.nan, np.inf, -1.0, 1e13, -0.0
    got = engine.variant_classes(torch.from_numpy(q), 3600.0, torch.from_numpy(init), [175.46e6]).numpy()
    assert (got[[3, 9, 17, 25]] == 3).all() and (np.delete(got, [3, 9, 17, 25]) == 0).all()
    # ... or that the overland share H tot / Z of the first rainy step's excess is beyond one (round 4): with Z = 100 mm and
    # H = 0.3, soil of more than 333 mm -- here 6 x 1e5 m3 on 1e6 m2 = 600 mm
    h = lhs_oracle.lhs_params(64, seed=12)
    h[:, 2], h[:, 5], h[40, 2] = 0.1, 100.0, 0.3
    got_h = engine.variant_classes(torch.from_numpy(h), 3600.0, torch.from_numpy(np.full((64, 12), 1e5)), [1e6]).numpy()
    assert got_h[40] == 3 and (np.delete(got_h, 40) == 0).all()
    two = np.stack([np.full((64, 12), 1e5), init])            # [C = 2, N, 12]: wild in any catchment counts
    assert np.array_equal(engine.variant_classes(torch.from_numpy(q), 3600.0, torch.from_numpy(two), [1e8, 175.46e6]).numpy(), got)

    for sort_rows in (False, True):
        gather, inverse = engine._variant_grouping(torch.from_numpy(p), dt, sort_rows)
        gather, inverse = gather.numpy(), inverse.numpy()
        assert len(gather) % 64 == 0 and np.array_equal(gather[inverse], np.arange(len(p)))     # every row, once
        g = cls[gather]
        assert np.all(np.diff(g) >= 0)                                                           # class by class
        for c in np.unique(cls):
            assert (g == c).sum() % 64 == 0 and (g == c).sum() - (cls == c).sum() < 64          # whole wavefronts
        if sort_rows:
            rows = gather[g == 0]
            t = p[rows, 0]
            bins = np.minimum(np.floor((t - t.min()) / (t.max() - t.min()) * 64), 63)
            assert np.all(np.diff(bins) >= 0)
            first = rows[bins == bins[0]]
            assert np.all(np.diff(p[first, 4] * p[first, 5]) >= 0)
    one = engine._variant_grouping(torch.from_numpy(p[cls == 0][:500]), dt, False)
    assert one is None                                        # a single class and no ordering asked for: rows as drawn


def test_shard_bounds_cover_the_rows_exactly():
    from smartpy_amd.distributed import shard_bounds, shard_counts
    for n in (0, 1, 7, 8, 9, 100000, 1000000):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert sum(shard_counts(n, world)) == n and max(shard_counts(n, world)) == -(-n // world)
    assert shard_bounds(1000000, 8, 3) == (375000, 500000)


def test_package_surface():
    import smartpy_amd
    assert smartpy_amd.__version__ and smartpy_amd.Parameters
    from smartpy_amd import objfunctions, structure, smartcpp
    assert objfunctions.groundwater_constraint([0.12667], [0.2]) == 1.0
    assert objfunctions.groundwater_constraint([0.12667], [0.23]) == 0.0
    assert structure.model_variables[6] == 'Q_out' and len(structure.model_variables) == 19
    assert callable(smartcpp.allsteps) and callable(smartcpp.onestep)
    with pytest.raises(Exception, match="Reporting type 'hourly' unknown."):
        structure.run(1.0, timedelta(hours=1), [0.0] * 24, [0.0] * 24, [1.0] * 10, None, list(range(25)),
                      list(range(2)), 'hourly', warm_up=0)
    with pytest.raises(Exception, match='warm-up duration'):
        structure.run(1.0, timedelta(hours=1), [0.0] * 24, [0.0] * 24, [1.0] * 10, None, list(range(25)),
                      list(range(2)), 'summary', warm_up=2)


# ---- the NetCDF flavours, driven through a test double of netCDF4.Dataset (the package is absent from this image) ----
@pytest.fixture()
def fake_netcdf(monkeypatch):
    from fake_netcdf import FakeDataset
    import smartpy_amd.inout as inout
    import smartpy_amd.montecarlo.database as database
    FakeDataset.opened = []
    monkeypatch.setattr(inout, 'Dataset', FakeDataset)
    monkeypatch.setattr(database, 'Dataset', FakeDataset)
    return FakeDataset


@pytest.mark.parametrize('save_sim', [False, True])
def test_sampling_database_netcdf_schema_and_round_trip(tmp_path, fake_netcdf, save_sim):
    """montecarlo.py:91-118 (schema), :211-224 (rows), :157-169 (zlib rewrite), :236-243 (reading back): dimension
    and variable names, dtypes, units strings, DateTime in seconds since the epoch, float32 storage."""
    from smartpy_amd.montecarlo.database import database_for, SamplingNetcdf
    from smartpy_amd.version import __version__
    g4 = load_golden('g4_example_lhs.npz')
    names = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE', 'GW']
    pnames = ['T', 'C', 'H', 'D', 'S', 'Z', 'SK', 'FK', 'GK', 'RK']
    stamps = [START + timedelta(days=k) for k in range(3)] if save_sim else None
    sims = g4['discharge'][:, :3]
    path = str(tmp_path / 'C.SMART.lhs.nc')
    db = database_for('netcdf', path, names, pnames)
    assert isinstance(db, SamplingNetcdf)
    db.create(10, stamps, parallel=True)
    assert fake_netcdf.opened[-1] == (path, 'w', True)                 # montecarlo.py:93 opens with parallel=self.p
    db.write_table(g4['objfns'], g4['params'], sims)
    db.close()
    nc = fake_netcdf(path, 'r')
    assert nc.description == "Monte Carlo Simulation outputs with SMARTpy v{}.".format(__version__)
    want_dims = {'NbSamples': 10, 'NbParameters': 10, 'NbObjFunctions': 8}
    if save_sim:
        want_dims['DateTime'] = 3
    assert {k: len(v) for k, v in nc.dimensions.items()} == want_dims
    v = nc.variables
    assert sorted(v) == sorted(['Parameters', 'ObjFunctions'] + (['DateTime', 'Simulations'] if save_sim else []))
    assert v['Parameters'].datatype == np.float32 and v['Parameters'].dimensions == ('NbSamples', 'NbParameters')
    assert v['Parameters'].units == 'T, C, H, D, S, Z, SK, FK, GK, RK'
    assert v['ObjFunctions'].datatype == np.float32 and v['ObjFunctions'].units == ', '.join(names)
    assert np.array_equal(v['Parameters'][:, :], g4['params'].astype(np.float32))
    assert np.array_equal(v['ObjFunctions'][:, :], g4['objfns'].astype(np.float32), equal_nan=True)
    if save_sim:
        assert v['DateTime'].datatype == np.float64 and v['DateTime'].units == "seconds since 1970-01-01 00:00:00.0"
        assert v['DateTime'][0] == (START - datetime(1970, 1, 1)).total_seconds() and v['DateTime'][2] - v['DateTime'][0] == 172800
        assert v['Simulations'].dimensions == ('NbSamples', 'DateTime') and v['Simulations'].units == "Discharge in m3/s"
        assert np.array_equal(v['Simulations'][:, :], sims.astype(np.float32))
    params, fns = db.read()
    assert params.dtype == np.float32 and np.array_equal(params, g4['params'].astype(np.float32))
    assert np.array_equal(fns, g4['objfns'].astype(np.float32), equal_nan=True)
    # the per-sample writer of the reference protocol lands every row at its own index, in any order
    one = database_for('netcdf', str(tmp_path / 'D.SMART.lhs.nc'), names, pnames).create(10, stamps)
    for r in (3, 0, 9, 1, 2, 8, 4, 7, 5, 6):
        one.write_sample(r, list(g4['objfns'][r]), g4['params'][r], sims[r])
    one.close()
    again = fake_netcdf(one.path, 'r')
    for name in v:
        assert np.array_equal(again.variables[name][:], v[name][:], equal_nan=True)
    # compression: None / False leave the file alone; True = zlib level 6; a number = that level (montecarlo.py:158-169)
    db.compress(None)
    db.compress(False)
    assert not fake_netcdf(path, 'r').variables['Parameters'].filters['zlib']
    for level, want in ((True, 6), (3, 3)):
        db.compress(level)
        packed = fake_netcdf(path, 'r')
        assert not os.path.exists(path.replace('.nc', '_.nc')) and packed.description == nc.description
        for name in v:
            assert packed.variables[name].filters == {'zlib': True, 'complevel': want}
            assert packed.variables[name].units == v[name].units
            assert np.array_equal(packed.variables[name][:], v[name][:], equal_nan=True)


def test_netcdf_flow_files_and_forcing_readers(tmp_path, fake_netcdf):
    """inout.py:299-310 (flow writer), :212-231 / :256-274 (readers) through the same double: what is written as a
    flow file reads back as an observation series with its NaN entries dropped, and a regular series reads back with
    its interval checked."""
    import smartpy_amd.inout as io
    stamps = [START + timedelta(days=k) for k in range(6)]
    flow = np.array([1.5, np.nan, 2.25, 3.0, np.nan, 0.125])
    base = str(tmp_path / 'C.obs.flow')
    io.write_flow_file_from_nds(stamps, flow, base, out_file_format='netcdf', parallel=False)
    nc = fake_netcdf(base + '.nc', 'r')
    assert nc.description.startswith('Discharge file generated with SMARTpy v')
    assert nc.variables['flow'].datatype == np.float32 and nc.variables['DateTime'].datatype == np.float64
    assert nc.variables['DateTime'].units == 'seconds since 1970-01-01 00:00:00.0'
    data = io.read_netcdf_time_series_with_missing_check(base + '.nc', 'DateTime', 'flow')
    assert list(data) == [stamps[0], stamps[2], stamps[3], stamps[5]] and list(data.values()) == [1.5, 2.25, 3.0, 0.125]
    got_stamps, got_values = io._read_flow_arrays(base + '.nc', 'netcdf')
    assert got_stamps == list(data) and np.array_equal(got_values, [1.5, 2.25, 3.0, 0.125])
    # a regular rain series
    rain = np.array([0.0, 2.5, 1.25, 0.0, 7.0, 0.5])
    with fake_netcdf(str(tmp_path / 'C.rain.nc'), 'w') as f:
        f.createDimension('DateTime', 6)
        f.createVariable('DateTime', np.float64, ('DateTime',))
        f.createVariable('rain', np.float32, ('DateTime',))
        f.variables['DateTime'][0:6] = [(s - datetime(1970, 1, 1)).total_seconds() for s in stamps]
        f.variables['rain'][0:6] = rain
    data, first, last, delta = io.read_netcdf_time_series_with_delta_check(str(tmp_path / 'C.rain.nc'), 'DateTime', 'rain')
    assert (first, last, delta) == (stamps[0], stamps[-1], timedelta(days=1)) and [data[s] for s in stamps] == list(rain)
    with pytest.raises(Exception, match='Variable DateTime or peva does not exist'):
        io.read_netcdf_time_series_with_delta_check(str(tmp_path / 'C.rain.nc'), 'DateTime', 'peva')
    with pytest.raises(Exception, match='could not be found'):
        io.read_netcdf_time_series_with_missing_check(str(tmp_path / 'nothing.nc'), 'DateTime', 'flow')


def test_without_netcdf4_the_reference_message_is_raised(tmp_path, monkeypatch):
    import smartpy_amd.inout as io
    import smartpy_amd.montecarlo.database as database
    monkeypatch.setattr(io, 'Dataset', None)
    monkeypatch.setattr(database, 'Dataset', None)
    with pytest.raises(Exception, match="requires the package 'netCDF4'"):
        database.database_for('netcdf', str(tmp_path / 'x.nc'), ['NSE'], ['T']).create(1)
    with pytest.raises(Exception, match="requires the package 'netCDF4'"):
        database.database_for('netcdf', str(tmp_path / 'x.nc'), ['NSE'], ['T']).read()
    with pytest.raises(Exception, match="requires the package 'netCDF4'"):
        io.write_flow_file_from_nds([START], [1.0], str(tmp_path / 'y'), out_file_format='netcdf')


@pytest.mark.parametrize('sanitizers', ['address,undefined', 'thread'])
def test_host_side_native_code_under_sanitizers(tmp_path, sanitizers):
    """smart_hostio.cpp (the only host-side native code with loops over caller data: database row writer / parser,
    threaded) built with -fsanitize=address,undefined, then with -fsanitize=thread, and driven with random tables,
    special values and malformed input (tests/native/hostio_sanitize.cpp).  GPU sanitizers do not exist on this pool; the kernels are covered by the
    parity tests."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'hostio_sanitize')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=' + sanitizers, '-fno-sanitize-recover=all',
                           '-pthread', os.path.join(root, 'tests', 'native', 'hostio_sanitize.cpp'),
                           os.path.join(root, 'smartpy_amd', 'csrc', 'smart_hostio.cpp'), '-o', exe])
    r = subprocess.run([exe, str(tmp_path / 'rows.csv')], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0 and 'hostio sanitize ok' in r.stdout, r.stdout + r.stderr
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr


def test_reciprocal_correction_step_gives_the_bits_of_the_division():
    """csrc/smart_literal_model.h (RECIP): q0 = RN(a y); r = a - b q0 [exact: one FMA]; q = RN(q0 + r y) with
    y = RN(1 / b) is claimed to be RN(a / b) for every normal a unless b's significand is all ones.  The three
    operations replayed in exact rational arithmetic (fractions: RN = float(Fraction), round-half-even) on pairs drawn
    to stress them: significands next to 1 and next to 2 on either side, random ones, and divisors of the model's own
    kind (k * 3600, areas, 1e3, 2 ... 6, step lengths).  (The remainder is NOT always exact: q0 can be more than an
    ulp off when the quotient's significand is next to 2, ~1 % of these pairs; the final rounding still lands on the
    division's result in every case -- which is what the kernel relies on, and what this test pins.)"""
    from fractions import Fraction
    rng = np.random.default_rng(20261003)
    n = 40000

    def near(edge, count):            # significands within a few hundred ulps of 1.0 (edge 0) or 2.0 (edge 1)
        k = rng.integers(0, 400, count).astype(np.float64) * 2.0 ** -52
        return (1.0 + k) if edge == 0 else (2.0 - 2.0 ** -52 - k)

    def scaled(sig, count):
        return sig * 2.0 ** rng.integers(-300, 300, count)

    kinds = [(scaled(rng.uniform(1.0, 2.0, n), n), scaled(rng.uniform(1.0, 2.0, n), n))]
    for ea in (0, 1):
        for eb in (0, 1):
            kinds.append((scaled(near(ea, n // 4), n // 4), scaled(near(eb, n // 4), n // 4)))
    model_b = np.concatenate([rng.uniform(1, 2000, n // 4) * 3600.0, rng.uniform(1e4, 1e10, n // 4),
                              np.tile([1e3, 2.0, 3.0, 4.0, 5.0, 6.0, 3600.0, 86400.0, 900.0], n // 36)])
    kinds.append((rng.uniform(0.0, 1e9, len(model_b)) * rng.uniform(0, 1, len(model_b)) ** 8, model_b))
    kinds.append((scaled(rng.uniform(1.0, 2.0, n), n), rng.integers(1, 1 << 20, n).astype(np.float64)))
    checked = inexact = 0
    for a_all, b_all in kinds:
        for a, b in zip(a_all.tolist(), b_all.tolist()):
            if a == 0.0 or (np.float64(b).view(np.uint64) & np.uint64(0x000fffffffffffff)) == np.uint64(0x000fffffffffffff):
                continue
            fa, fb = Fraction(a), Fraction(b)
            y = float(1 / fb)
            q0 = float(fa * Fraction(y))
            r = float(fa - fb * Fraction(q0))                 # one FMA: a single rounding of the exact remainder
            inexact += Fraction(r) != fa - fb * Fraction(q0)
            q = float(Fraction(q0) + Fraction(r) * Fraction(y))
            assert q == float(fa / fb), (a.hex(), b.hex())
            checked += 1
    assert checked > 140000
    print('inexact remainders', inexact, 'of', checked)


# ---- the engine's host side: the memo behind its handle, the plan word, broadcasting over catchments --------------
def _memo_pair():
    import torch
    return torch.zeros(4, 10, dtype=torch.float64), torch.zeros(6, 2, dtype=torch.float64)


@pytest.fixture
def memo():
    """engine._Memo with an empty process-wide list (restored afterwards)."""
    from smartpy_amd import engine
    kept = list(engine._Memo._entries)
    engine._Memo._entries[:] = []
    yield engine._Memo
    engine._Memo._entries[:] = kept


def test_memo_hits_on_the_same_objects_at_the_same_versions_only(memo):
    """What prepare_ensemble() remembers is tied to the two tensor OBJECTS and their in-place version counters: the
    same objects come back -> hit; an in-place write to either, a fresh tensor with equal contents, another key -> miss."""
    import torch
    cpu = torch.device('cpu')
    p, f = _memo_pair()
    assert memo((p, f), 'key', cpu).lookup() is None
    memo((p, f), 'key', cpu).store(('grouping', 0x123))
    assert memo((p, f), 'key', cpu).lookup() == ('grouping', 0x123)
    assert memo((p, f), 'other key', cpu).lookup() is None
    assert memo((p.clone(), f), 'key', cpu).lookup() is None and memo((p, f.clone()), 'key', cpu).lookup() is None
    assert memo((f, p), 'key', cpu).lookup() is None
    for written in (p, f):
        a, b = _memo_pair()
        memo((a, b), 'key', cpu).store('before')
        (a if written is p else b)[0, 0] = 1.0
        assert memo((a, b), 'key', cpu).lookup() is None
        memo((a, b), 'key', cpu).store('after')              # the newest entry for the objects at their versions wins
        assert memo((a, b), 'key', cpu).lookup() == 'after'
    assert memo((p, f), 'key', cpu).lookup() == ('grouping', 0x123)


def test_memo_forget_removes_exactly_that_entry_and_refresh_takes_the_new_versions(memo):
    import torch
    cpu = torch.device('cpu')
    p, f = _memo_pair()
    q, g = _memo_pair()
    h = memo((p, f), 'key', cpu)
    h.store('mine')
    memo((p, f), 'other key', cpu).store('other key')
    memo((q, g), 'key', cpu).store('other tensors')
    p[0, 0] = 2.0               # forget() goes by objects and key, not by version: what went stale is what it drops
    h.forget()
    assert [ent.value for ent in memo._entries] == ['other key', 'other tensors']
    h.store('stale versions')   # what verify() does after a stale plan: forget, refresh, re-plan, store
    assert memo((p, f), 'key', cpu).lookup() is None
    h.forget()
    h.refresh()
    h.store('fresh')
    assert memo((p, f), 'key', cpu).lookup() == 'fresh' and len(memo._entries) == 3


def test_memo_keeps_eight_entries_and_drops_those_whose_tensor_died(memo):
    import gc
    import torch
    cpu = torch.device('cpu')
    assert memo.SIZE == 8
    pairs = [_memo_pair() for _ in range(9)]
    for i, pair in enumerate(pairs):
        memo(pair, 'key', cpu).store(i)
    assert len(memo._entries) == 8 and memo(pairs[0], 'key', cpu).lookup() is None           # the oldest went out
    assert [memo(pair, 'key', cpu).lookup() for pair in pairs[1:]] == list(range(1, 9))
    h = memo(pairs[3], 'key', cpu)
    del pairs[3:5]
    gc.collect()
    assert memo(pairs[1], 'key', cpu).lookup() == 1
    assert sorted(ent.value for ent in memo._entries) == [1, 2, 5, 6, 7, 8]                 # pruned by that lookup
    h.refresh()
    h.store('about dead tensors')
    h.forget()
    assert h.lookup() is None and len(memo._entries) == 6                                    # ... which nothing touches


def test_memo_does_not_apply_to_converted_inputs_initial_states_or_literal_mode(memo):
    """An input that is not a tensor on the device is converted on the way in (a fresh object each call); with initial
    states the rows' classes depend on them too; the plan belongs to fast mode.  Then nothing is stored or found."""
    import torch
    cpu = torch.device('cpu')
    p, f = _memo_pair()
    assert memo((p, f), 'key', cpu).applies
    for h in (memo((p.numpy(), f), 'key', cpu), memo((p, f.tolist()), 'key', cpu), memo((p, f), 'key', torch.device('meta')),
              memo((p, f), 'key', cpu, initial=torch.zeros(4, 12)), memo((p, f), 'key', cpu, fast=False)):
        assert not h.applies
        h.store('never')
        assert h.lookup() is None and memo._entries == []
    memo((p, f), 'key', cpu).store('kept')
    memo((p, f), 'key', cpu, fast=False).forget()
    assert memo((p, f), 'key', cpu).lookup() == 'kept'


def test_plan_word_keeps_the_row_order_mark_and_aims_at_one_class():
    """engine._compose_plan: a re-plan carries PLAN_ROWS_ORDERED over from the word it replaces (and nothing else of
    it); the plan of a single row is PLAN_VALID, the forcing bits of the plan in force and the kernel of its class."""
    from smartpy_amd import engine, _lib
    forcing = (_lib.PLAN_FORCING_PIECEWISE, _lib.PLAN_FORCING_VARYING, _lib.PLAN_FORCING_RUNS)
    old = _lib.PLAN_VALID | _lib.PLAN_ROWS_ORDERED | _lib.PLAN_CLASS_BITS[1] | _lib.PLAN_FORCING_VARYING
    new = _lib.PLAN_VALID | _lib.PLAN_CLASS_BITS[0] | _lib.PLAN_FORCING_RUNS | (5 << _lib.PLAN_ILLCOND_BLOCKS_SHIFT)
    assert engine._compose_plan(new, old) == new | _lib.PLAN_ROWS_ORDERED
    assert engine._compose_plan(new, old & ~_lib.PLAN_ROWS_ORDERED) == new and engine._compose_plan(new) == new
    assert engine._compose_plan(new, _lib.PLAN_ROWS_ORDERED) == new | _lib.PLAN_ROWS_ORDERED
    for cls in range(4):
        for bits in (0, forcing[0], forcing[1] | forcing[2], forcing[0] | forcing[1] | forcing[2]):
            in_force = new | _lib.PLAN_ROWS_ORDERED | _lib.PLAN_CLASS_BITS[3] | bits
            assert engine._compose_plan(in_force, row_class=cls) == _lib.PLAN_VALID | (in_force & sum(forcing)) | \
                _lib.PLAN_CLASS_BITS[cls]
    assert engine._compose_plan(new, row_class=2) == _lib.PLAN_VALID | _lib.PLAN_FORCING_RUNS | _lib.PLAN_CLASS_BITS[2]


def test_inputs_are_broadcast_over_the_catchments():
    """engine._per_catchment: a scalar or an array the catchments share -> contiguous [C, ...]; one entry per catchment
    -> reshaped; the bytes that cross to a device are counted by as_device as before (none on the host)."""
    import torch
    from smartpy_amd import engine
    cpu, C = torch.device('cpu'), 3
    assert engine._per_catchment(None, cpu, C) is None and engine._per_catchment(None, cpu, C, (7,)) is None
    area = engine._per_catchment(175.46e6, cpu, C)
    assert area.shape == (C,) and area.dtype == torch.float64 and area.tolist() == [175.46e6] * C
    assert engine._per_catchment([1.0, 2.0, 3.0], cpu, C).tolist() == [1.0, 2.0, 3.0]
    assert engine._per_catchment(np.float32(0.5), cpu, 1).tolist() == [0.5]
    with pytest.raises(RuntimeError):
        engine._per_catchment([1.0, 2.0], cpu, C)
    seven = np.arange(7.0)
    shared = engine._per_catchment(seven, cpu, C, (7,))
    assert shared.shape == (C, 7) and shared.is_contiguous() and all(np.array_equal(r.numpy(), seven) for r in shared)
    own = engine._per_catchment(np.arange(21.0), cpu, C, (7,))
    assert own.shape == (C, 7) and own.is_contiguous() and np.array_equal(own.numpy().ravel(), np.arange(21.0))
    init = engine._per_catchment(torch.arange(5 * 12, dtype=torch.float64), cpu, C, (5, 12))
    assert init.shape == (C, 5, 12) and init.is_contiguous() and torch.equal(init[2], init[0])
    assert engine._per_catchment(np.zeros((C, 5, 12)), cpu, C, (5, 12)).shape == (C, 5, 12)
    obs = engine._per_catchment(np.arange(4.0), cpu, 1, (4,))
    assert obs.shape == (1, 4) and obs.is_contiguous()
    with pytest.raises(RuntimeError):
        engine._per_catchment(np.arange(5.0), cpu, C, (4,))
