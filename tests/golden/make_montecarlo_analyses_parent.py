"""Every analysis method of the Monte-Carlo workflows on the example catchment, as the PARENT commit's host code drives
the library -> tests/golden/montecarlo_analyses_parent.npz: every numpy attribute of the results bit for bit, the bytes of
the side files and of the sampling databases, and the number of model.simulate_ensemble calls each method made.  Needs an
MI355X; run once at the parent commit:

    python tests/golden/make_montecarlo_analyses_parent.py [out.npz]

The change the fixture was made for moved the analyses of the stored discharge matrix out of montecarlo.py into
smartpy_amd/montecarlo/analyses.py and folded their shared preamble, the side-file block, the weights rule, the containment
and the rank-0 write into one helper each.  No kernel and no launch changed, so equality is exact: no tolerance is
involved.  The calls live here, so that tests/test_gpu_montecarlo_analyses.py repeats exactly what the fixture recorded.

The objects, all on half a year of the example catchment (181 daily reports, hourly steps, 30 days of warm-up):
  host     an LHS of 16 rows, seed 5, the sample a host matrix
  device   the same 16 rows handed over as a device tensor (_launch_rows takes its other branch)
  nobody   a GLUE of `host` after its run() that nothing passes: zero behavioural rows, no launch anywhere
  sobol    a Saltelli design of base size 4 over two parameters (16 rows): run(), sensitivity, sensitivity_series
  demcz    16 chains, 4 generations, every 2nd archived: run(write=True)
Each of host and device makes the eight analyses with write=True before its run() (pawn_sensitivity on the objective
functions then launches for itself), run(), and afterwards the calls that take what run() left: pawn_sensitivity on the
objective functions again and predictive_bounds weighted by KGEb (a ratio of means: never negative)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'tests'))

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'montecarlo_analyses_parent.npz')
SETTINGS = 'Catchment.analyses.sttngs'
ROWS = 16
THETA = [0.1, 0.2, 0.5]         # sigma0, sigma1, phi of every row


def counted(obj):
    """wrap obj.model.simulate_ensemble on the instance -> the list whose only element counts its calls"""
    inner, calls = obj.model.simulate_ensemble, [0]

    def simulate_ensemble(*args, **kw):
        calls[0] += 1
        return inner(*args, **kw)
    obj.model.simulate_ensemble = simulate_ensemble
    return calls


def arrays_of(result, prefix=''):
    """every numpy attribute of a result (numbers as arrays of one element; the attributes of a result it holds, such as
    the verification of predictive_bounds, under `<attribute>.`) -> {name: array}"""
    out = {}
    for name, value in sorted(vars(result).items()):
        if isinstance(value, (bool, int, float, np.number)):
            value = np.asarray(value)
        if isinstance(value, np.ndarray):
            if value.dtype.kind in 'biuf':
                out[prefix + name] = value
        elif type(value).__module__.startswith('smartpy_amd.') and hasattr(value, '__dict__'):
            out.update(arrays_of(value, prefix + name + '.'))
    return out


def file_bytes(path):
    with open(path, 'rb') as f:
        return np.frombuffer(f.read(), dtype=np.uint8)


class Record(dict):
    """key -> array: `<object>|<call>|<attribute>`, `<object>|<call>|file`, `<object>|<call>|launches`"""

    def call(self, who, name, calls, method, *args, **kw):
        before = calls[0]
        result = method(*args, **kw)
        self['%s|%s|launches' % (who, name)] = np.asarray(calls[0] - before)
        if result is not None:
            for attribute, value in arrays_of(result).items():
                self['%s|%s|%s' % (who, name, attribute)] = value
            path = getattr(result, 'file', None) or getattr(result, 'path', None)     # (two results call it `path`)
            assert kw.get('write') is not True or path is not None, (who, name)
            if path is not None:
                self['%s|%s|file' % (who, name)] = file_bytes(path)
        return result

    def state(self, who, name, obj):
        """what a run() leaves on the object, and the database it wrote"""
        self['%s|%s|sample' % (who, name)] = obj._sample
        self['%s|%s|obj_fns' % (who, name)] = obj.obj_fns
        self['%s|%s|gw_contributions' % (who, name)] = obj.gw_contributions
        self['%s|%s|database' % (who, name)] = file_bytes(obj.db_file)


def analyses(record, who, obj, calls, after_run):
    """the eight analyses of the stored matrix on one object, write=True each"""
    tag = '@run' if after_run else ''
    if not after_run:
        record.call(who, 'window_objective_functions', calls, obj.window_objective_functions, 'month', transform='log',
                    write=True)
        record.call(who, 'flow_duration_curves', calls, obj.flow_duration_curves, exceedance=(0.1, 0.9), windows='month',
                    transform='sqrt', segment=(0.0, 0.5), write=True)
        record.call(who, 'hydrological_signatures', calls, obj.hydrological_signatures, windows='all', write=True)
        record.call(who, 'score_uncertainty', calls, obj.score_uncertainty, windows='month', resamples=16, seed=3,
                    quantiles=(0.05, 0.95), min_steps=20, write=True)
        record.call(who, 'dynamic_identifiability', calls, obj.dynamic_identifiability, fraction=0.25, bins=4, write=True)
        record.call(who, 'pawn_sensitivity', calls, obj.pawn_sensitivity, of='discharge', bins=2, dummies=1, seed=0,
                    min_count=1, write=True)
        record.call(who, 'residual_likelihood', calls, obj.residual_likelihood, error_parameters=THETA, write=True)
    record.call(who, 'pawn_sensitivity:objective_functions' + tag, calls, obj.pawn_sensitivity, of='objective_functions',
                bins=2, dummies=1, seed=0, min_count=1, write=True)
    record.call(who, 'predictive_bounds' + tag, calls, obj.predictive_bounds, error_parameters=THETA,
                quantiles=(0.05, 0.95), replicates=2, likelihood='KGEb' if after_run else None, seed=1, verify=True,
                write=True)


def run_all(folder):
    """every object, every call -> Record"""
    import torch
    from support import EXTRA, example_root, settings_file
    from smartpy_amd.montecarlo import DEMCz, GLUE, LHS, Sobol
    assert torch.cuda.is_available(), 'the analyses run on the GPU'
    root = example_root(folder)
    settings_file(root, SETTINGS, '01/01/2007', '30/06/2007', 30)
    record = Record()

    def made(obj):
        obj.model.extra = EXTRA
        return obj, counted(obj)
    host, host_calls = made(LHS('Catchment', root, 'csv', 'csv', sample_size=ROWS, settings_filename=SETTINGS, seed=5))
    for who, sample in (('host', None), ('device', torch.from_numpy(host._sample).cuda())):
        obj, calls = (host, host_calls) if sample is None else \
            made(LHS('Catchment', root, 'csv', 'csv', sample_size=ROWS, settings_filename=SETTINGS, seed=5))
        if sample is not None:
            obj._set_sample(sample)
        assert (obj.device_sample is not None) == (who == 'device') and np.array_equal(obj._sample, host._sample)
        analyses(record, who, obj, calls, after_run=False)
        record.call(who, 'run', calls, obj.run)
        record.state(who, 'run', obj)
        analyses(record, who, obj, calls, after_run=True)
    nobody, calls = made(GLUE('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (2.0,))}, sampling=host,
                              settings_filename=SETTINGS))
    assert nobody._sample.shape == (0, 10)
    analyses(record, 'nobody', nobody, calls, after_run=False)
    record.call('nobody', 'prediction_bounds', calls, nobody.prediction_bounds, quantiles=(0.05, 0.95), write=True)
    record.call('nobody', 'ensemble_verification', calls, nobody.ensemble_verification, write=True)
    record.call('nobody', 'run', calls, nobody.run)
    record.state('nobody', 'run', nobody)
    sobol, calls = made(Sobol('Catchment', root, 'csv', 'csv', base_size=4, settings_filename=SETTINGS, vary=['T', 'SK'],
                              seed=4))
    record.call('sobol', 'run', calls, sobol.run)
    record.state('sobol', 'run', sobol)
    record.call('sobol', 'sensitivity', calls, sobol.sensitivity, resamples=8, seed=2, write=True)
    record.call('sobol', 'sensitivity_series', calls, sobol.sensitivity_series, write=True)
    demcz, calls = made(DEMCz('Catchment', root, 'csv', 'csv', chains=ROWS, generations=4, thin=2, seed=0,
                              settings_filename=SETTINGS))
    record.call('demcz', 'run', calls, demcz.run, write=True)
    record.state('demcz', 'run', demcz)
    record['demcz|run|diagnostics'] = demcz.diagnostics
    record['demcz|run|file'] = file_bytes(demcz.posterior.file)
    return record


def main(path):
    import tempfile
    from smartpy_amd import _lib
    print('library:', _lib.LIB_PATH)
    with tempfile.TemporaryDirectory() as folder:
        record = run_all(folder)
    np.savez_compressed(path, **record)
    for key in sorted(record):
        print('%-64s %-8s %s' % (key, record[key].dtype, record[key].shape))
    print('%d entries, %d bytes -> %s' % (len(record), os.path.getsize(path), path))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
