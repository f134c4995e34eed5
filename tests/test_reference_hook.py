"""The plug-in contract, held against what the REAL reference did (tests/golden/reference_hook.npz, recorded from the
unmodified reference by tests/golden/make_reference_hook.py): the calls its structure.run makes through the
`smartcpp` hook are replayed through smartpy_amd.smartcpp, and our input pipeline is held against the arrays the
reference's readers and resamplers produced on the same random files.  No GPU here, so the launch behind allsteps
is replaced by the CPU oracle; on the GPU box the same call path ends in smart_allsteps_hip
(tests/test_gpu_api.py::test_smartcpp_module_contract)."""
import importlib
import os
from datetime import datetime, timedelta

import numpy as np
import pytest

from conftest import load_golden

FIXTURE = 'reference_hook.npz'


@pytest.fixture(scope='module')
def recorded():
    with load_golden(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_unmodified_reference_runs_through_our_smartcpp(monkeypatch, recorded):
    from oracle import smart_oracle as so
    from smartpy_amd import engine
    calls = []

    def allsteps_on_cpu(area, dt, length, rain, peva, params, initial, report_type, gap):
        calls.append((length, len(rain), np.asarray(initial).shape, report_type, gap))
        return so.all_steps(area, dt, length, rain, peva, params, initial, report_type, gap)

    monkeypatch.setattr(engine, 'allsteps', allsteps_on_cpu)
    import smartpy_amd.smartcpp as shim
    importlib.reload(shim)                       # re-binds allsteps to the patched engine function
    try:
        assert shim.__version__ >= '0.2.0' and callable(shim.allsteps)      # structure.py:56-58 takes allsteps
        # the warm-up call and the run, with the arguments the reference passed (structure.py:118-121,143-146)
        out = []
        for k in range(int(recorded['n_calls'])):
            c = 'call%d_' % k
            out.append(shim.allsteps(float(recorded[c + 'area']), float(recorded[c + 'dt']), int(recorded[c + 'length']),
                                     recorded['rain'], recorded['peva'], recorded[c + 'params'],
                                     recorded[c + 'initial'], int(recorded[c + 'report_type']),
                                     int(recorded[c + 'gap'])))
    finally:
        importlib.reload(shim)
    # warm-up call: full-length forcing with the shorter length, then the run
    assert calls == [(8760, 87672, (19,), 1, 24), (87672, 87672, (19,), 1, 24)]
    # the run starts from the final state the warm-up call handed back (structure.py:118-121: `[2]`)
    assert np.array_equal(np.asarray(out[0][2]), recorded['call1_initial'])
    for k, (dis, gw, final) in enumerate(out):
        c = 'call%d_' % k
        assert np.array_equal(np.asarray(dis), recorded[c + 'discharge']) and gw == float(recorded[c + 'gw'])
        assert np.array_equal(np.asarray(final), recorded[c + 'final'])
    discharge = np.asarray(out[-1][0])
    g1 = load_golden('g1_reference_test.npz')
    for i, v in zip(g1['report_index'], g1['expected']):
        assert '%.6e' % discharge[i] == '%.6e' % v
    assert np.array_equal(discharge, load_golden('kat1_hourly.npz')['discharge_summary'])


def _write_series(path, header, stamps, values, fmt='%.6e'):
    with open(path, 'w') as f:
        f.write('DateTime,%s\n' % header)
        for s, v in zip(stamps, values):
            f.write('%s,%s\n' % (s.strftime('%Y-%m-%d %H:%M:%S'), v if isinstance(v, str) else fmt % v))


def random_input_files(root, seed):
    """Random rain / PE / flow files of one seed under root/in/C -> the arguments of the SMART constructor (the
    fixture's generator writes the same files for the reference)."""
    rng = np.random.default_rng(1000 + seed)
    d_data = timedelta(hours=int(rng.choice([1, 3, 24])))
    d_simu = timedelta(hours=int(rng.choice([1, 2, 3, 6, 12, 24])))
    d_save = timedelta(hours=24)
    if d_save.total_seconds() % d_simu.total_seconds():
        d_simu = timedelta(hours=6)
    t0 = datetime(2001, 3, 1, int(rng.integers(0, 24)))
    n_data = int(rng.integers(24 * 40, 24 * 60) * 3600 // d_data.total_seconds())
    stamps = [t0 + k * d_data for k in range(n_data)]
    cat = os.path.join(str(root), 'in', 'C')
    os.makedirs(cat)
    _write_series(os.path.join(cat, 'C.rain'), 'rain', stamps, rng.gamma(0.5, 3.0, n_data) * (rng.random(n_data) < 0.6))
    _write_series(os.path.join(cat, 'C.peva'), 'peva', stamps, rng.random(n_data) * 0.3)
    # daily mean flows at some clock time, with holes
    f0 = datetime(2001, 2, 20, int(rng.integers(0, 24)))
    fst, fval = [], []
    for k in range(90):
        u = rng.random()
        if u < 0.08:
            continue                                    # missing row
        fst.append(f0 + timedelta(days=k))
        fval.append('' if u < 0.12 else ('-99' if u < 0.16 else '%.3f' % (rng.random() * 20)))
    _write_series(os.path.join(cat, 'C.flow'), 'flow', fst, fval)
    start = datetime(2001, 3, 8, int(rng.integers(0, 24))) + timedelta(days=int(rng.integers(0, 5)))
    end = start + timedelta(days=int(rng.integers(5, 25)))
    return ('C', 50e6, start, end, d_simu, d_save, 0, 'csv', 'csv', str(root) + os.sep)


def as_datetime64(series):
    return np.array(series, dtype='datetime64[us]')


@pytest.mark.parametrize('seed', range(16))
def test_input_pipeline_against_the_reference_on_random_files(tmp_path, recorded, seed):
    """Random rain / PE files (hourly, 3-hourly or daily stamps at random offsets) and irregular flow files (missing
    days, '', -99, different clock time), random simulation and report steps: the arrays our readers + resamplers
    produce must equal the reference's (smart.py:130-143), exceptions included."""
    import smartpy_amd
    args = random_input_files(tmp_path / 'data', seed)
    try:
        ours = smartpy_amd.SMART(*args, gauged_area_m2=47e6)
        our_err = None
    except Exception as e:
        ours, our_err = None, e
    s = 'seed%d_' % seed
    ref_err = str(recorded[s + 'error'])
    assert (ref_err == '') == (our_err is None), (ref_err, our_err)
    if our_err is not None:
        assert str(our_err) == ref_err or type(our_err).__name__ == str(recorded[s + 'error_type'])
        print('both raise:', ref_err)
        return
    assert np.array_equal(as_datetime64(ours.timeseries), recorded[s + 'timeseries'])
    assert np.array_equal(as_datetime64(ours.timeseries_report), recorded[s + 'timeseries_report'])
    assert np.array_equal(ours.nd_rain, recorded[s + 'nd_rain']) and np.array_equal(ours.nd_peva, recorded[s + 'nd_peva'])
    assert np.array_equal(ours.nd_flow, recorded[s + 'nd_flow'], equal_nan=True)
