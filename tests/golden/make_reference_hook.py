"""Generate tests/golden/reference_hook.npz by RUNNING THE UNMODIFIED REFERENCE (ThibHlln/smartpy v0.2.2).

Run from the repo root:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_hook.py <reference checkout>

The reference is imported from the checkout given, never copied.  What is stored are numbers only:
  call<k>_*        the arguments of every smartcpp.allsteps call the reference's structure.run makes for the shipped
                   example (a recording `smartcpp` registered before `import smartpy`, answering with the reference's
                   own run_all_steps), and what that call returned; rain / peva are the same for both calls
  seed<s>_*        for the random input files of tests/test_reference_hook.py (seeds 0-15): the reference's
                   timeseries, timeseries_report (datetime64[us]), nd_rain, nd_peva, nd_flow -- or the message and
                   type of the exception its SMART constructor raised (error '' when it raised none)
"""
import importlib
import os
import shutil
import sys
import tempfile
import types
from datetime import datetime, timedelta

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))

from test_reference_hook import FIXTURE, as_datetime64, random_input_files  # noqa: E402


def fresh_reference(ref, smartcpp=None):
    for name in [m for m in sys.modules if m == 'smartpy' or m.startswith('smartpy.')] + ['smartcpp']:
        sys.modules.pop(name, None)
    if smartcpp is not None:
        sys.modules['smartcpp'] = smartcpp
    if ref not in sys.path:
        sys.path.insert(0, ref)
    return importlib.import_module('smartpy')


def record_calls(ref, out):
    calls = []
    hook = types.ModuleType('smartcpp')
    hook.__version__ = '0.2.0'

    def allsteps(*args):
        got = sys.modules['smartpy.structure'].run_all_steps(*args)
        calls.append((args, got))
        return got
    hook.allsteps = allsteps
    # (run_all_steps itself steps through smartcpp.onestep once the hook is there, structure.py:171-174)
    hook.onestep = lambda *args: sys.modules['smartpy.structure'].run_one_step(*args)
    smartpy = fresh_reference(ref, hook)
    from smartpy import structure
    assert structure.smart_in_cpp and structure.smartcpp is hook
    g = np.load(os.path.join(HERE, 'forcing_example.npz'))
    extra = {'aar': float(g['extra'][0]), 'r-o_ratio': float(g['extra'][1]), 'r-o_split': tuple(g['extra'][2:])}
    tmp = tempfile.mkdtemp(prefix='smart_hook_')
    try:
        data = os.path.join(tmp, 'data')
        shutil.copytree(os.path.join(ref, 'tests', 'data'), data)
        for dirpath, _, _ in os.walk(data):
            os.chmod(dirpath, 0o755)
        sm = smartpy.SMART('Catchment', 175.46e6, datetime(2007, 1, 1, 9), datetime(2016, 12, 31, 9),
                           timedelta(hours=1), timedelta(days=1), 365, 'csv', 'csv', data + os.sep,
                           gauged_area_m2=175.97e6)
        sm.extra = extra
        sm.parameters.set_parameters_with_file(sm.in_f + 'Catchment.parameters')
        sm.simulate(sm.parameters.values)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out['n_calls'] = np.array(len(calls))
    for k, (args, got) in enumerate(calls):
        area, dt, length, rain, peva, params, initial, report_type, gap = args
        assert np.array_equal(rain, calls[0][0][3]) and np.array_equal(peva, calls[0][0][4])
        c = 'call%d_' % k
        out.update({c + 'area': np.array(area, dtype=np.float64), c + 'dt': np.array(dt, dtype=np.float64),
                    c + 'length': np.array(length), c + 'params': np.asarray(params, dtype=np.float64),
                    c + 'initial': np.asarray(initial, dtype=np.float64), c + 'report_type': np.array(report_type),
                    c + 'gap': np.array(gap), c + 'discharge': np.asarray(got[0], dtype=np.float64),
                    c + 'gw': np.array(got[1], dtype=np.float64), c + 'final': np.asarray(got[2], dtype=np.float64)})
    out['rain'] = np.asarray(calls[0][0][3], dtype=np.float64)
    out['peva'] = np.asarray(calls[0][0][4], dtype=np.float64)


def record_pipeline(ref, out):
    smartpy = fresh_reference(ref)
    for seed in range(16):
        tmp = tempfile.mkdtemp(prefix='smart_files_')
        s = 'seed%d_' % seed
        try:
            args = random_input_files(os.path.join(tmp, 'data'), seed)
            try:
                sm = smartpy.SMART(*args, gauged_area_m2=47e6)
            except Exception as e:                      # e.g. data not sufficient, time deltas not multiples
                out[s + 'error'], out[s + 'error_type'] = np.array(str(e)), np.array(type(e).__name__)
                continue
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        out[s + 'error'], out[s + 'error_type'] = np.array(''), np.array('')
        out.update({s + 'timeseries': as_datetime64(sm.timeseries),
                    s + 'timeseries_report': as_datetime64(sm.timeseries_report),
                    s + 'nd_rain': np.asarray(sm.nd_rain, dtype=np.float64),
                    s + 'nd_peva': np.asarray(sm.nd_peva, dtype=np.float64),
                    s + 'nd_flow': np.asarray(sm.nd_flow, dtype=np.float64)})


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], 'smartpy')):
        raise SystemExit('usage: make_reference_hook.py <checkout of the reference (holds smartpy/)>')
    ref = os.path.abspath(sys.argv[1])
    out = {}
    record_pipeline(ref, out)
    record_calls(ref, out)
    path = os.path.join(HERE, FIXTURE)
    np.savez_compressed(path, **out)
    print('%-28s %8.1f kB' % (FIXTURE, os.path.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
