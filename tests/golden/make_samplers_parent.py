"""The two generational samplers of the Monte-Carlo workflows, DEMCz and NSGA2, as the PARENT commit's host code builds
and drives them -> tests/golden/samplers_parent.npz.  Run once at the parent commit:

    python tests/golden/make_samplers_parent.py [out.npz] [--host-only]

The change the fixture was made for gave the two classes a common base (smartpy_amd/montecarlo/generational.py), the two
bindings a common module (smartpy_amd/generational.py) and the two propose / vary kernels one differential-evolution move
(csrc/smart_de_move.h).  Every output of both steps is defined to the bit, so equality is exact: no tolerance is involved.
The constructions and the calls live here, so that tests/test_samplers_host.py and tests/test_gpu_samplers_parent.py repeat
exactly what the fixture recorded.  The recorder is the one of make_montecarlo_analyses_parent.py.

The host part (keys `host|...`, no device needed): `initial_population`, `columns`, `lo`, `hi` and `vary` of the five
constructions of CONSTRUCTIONS, and `text` / `code` of every refusal of REFUSALS (the class of the exception leads the text;
code 0: a plain Exception, which carries none).

The device part (keys `<run>|run|...`, needs an MI355X): the three runs of RUNS, 16 rows each on one year of daily steps
with 90 days of warm-up -- sample, obj_fns, gw_contributions, diagnostics, what is the sampler's own (rank / crowding / keys,
or log_density / accepted / rhat / error_parameters), the bytes of the database and of the diagnostics file, and the number
of ensemble launches.  (The Gaussian DEMCz run is in montecarlo_analyses_parent.npz.)

The device part was made twice at the parent before it was committed; every entry was equal between the two, so none is
left out as the parent's own nondeterminism."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'tests'))

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'samplers_parent.npz')
SETTINGS = 'Catchment.samplers.sttngs'
ROWS = 16
SUBSET = dict(vary=['T', 'SK', 'FK', 'GK'], fixed={'C': 0.5})
THREE = {'NSE': 'max', 'PBias': ('target', 0.0), 'RMSE': 'min'}

#: name -> (class, positional arguments after the formats, keywords)
CONSTRUCTIONS = {
    'demcz': ('DEMCz', (), dict(chains=ROWS, generations=4, thin=2, seed=0)),
    'demcz_subset': ('DEMCz', (), dict(chains=ROWS, generations=4, thin=2, seed=1, **SUBSET)),
    'demcz_ar1': ('DEMCz', (), dict(chains=ROWS, generations=4, thin=2, seed=2, likelihood='ar1', error_model={'phi': 0.3})),
    'nsga2': ('NSGA2', (['NSE', 'PBias'],), dict(population=ROWS, generations=3, thin=2, seed=3)),
    'nsga2_three': ('NSGA2', (THREE,), dict(population=ROWS, generations=3, thin=2, seed=4, **SUBSET)),
}
#: the runs of the device part
RUNS = {
    'demcz_ar1': ('DEMCz', (), dict(chains=ROWS, generations=4, thin=2, seed=5, likelihood='ar1', gw_prior=True, **SUBSET)),
    'nsga2_two': ('NSGA2', (['NSE', 'PBias'],), dict(population=ROWS, generations=3, thin=2, seed=6)),
    'nsga2_three': ('NSGA2', (THREE,), dict(population=ROWS, generations=3, thin=2, seed=7, gw_constraint=True, **SUBSET)),
}
TWO = (['NSE', 'PBias'],)
#: label -> (class, positional arguments, keywords): every vary / fixed / size refusal of the two constructors
REFUSALS = {
    'demcz:chains': ('DEMCz', (), dict(chains=1)),
    'demcz:generations': ('DEMCz', (), dict(chains=ROWS, generations=0)),
    'demcz:thin': ('DEMCz', (), dict(chains=ROWS, thin=0)),
    'demcz:burn_in': ('DEMCz', (), dict(chains=ROWS, burn_in=1.0)),
    'demcz:likelihood': ('DEMCz', (), dict(chains=ROWS, likelihood='student')),
    'demcz:ar1_sigma': ('DEMCz', (), dict(chains=ROWS, likelihood='ar1', sigma=1.0)),
    'demcz:error_model': ('DEMCz', (), dict(chains=ROWS, error_model={'phi': 0.3})),
    'demcz:p_jump': ('DEMCz', (), dict(chains=ROWS, p_jump=2.0)),
    'demcz:cr': ('DEMCz', (), dict(chains=ROWS, cr=1.5)),
    'demcz:vary_none': ('DEMCz', (), dict(chains=ROWS, vary=[])),
    'demcz:vary_twice': ('DEMCz', (), dict(chains=ROWS, vary=['T', 'T'])),
    'demcz:vary_unknown': ('DEMCz', (), dict(chains=ROWS, vary=['T', 'Q'])),
    'demcz:fixed_varies': ('DEMCz', (), dict(chains=ROWS, fixed={'T': 1.0})),
    'demcz:fixed_unknown': ('DEMCz', (), dict(chains=ROWS, vary=['T'], fixed={'Q': 1.0})),
    'nsga2:objectives_few': ('NSGA2', (['NSE'],), dict(population=ROWS)),
    'nsga2:objectives_many': ('NSGA2', (['NSE', 'KGE', 'KGEc', 'RMSE', 'PBias'],), dict(population=ROWS)),
    'nsga2:objective_unknown': ('NSGA2', (['NSE', 'nse'],), dict(population=ROWS)),
    'nsga2:population_small': ('NSGA2', TWO, dict(population=3)),
    'nsga2:population_large': ('NSGA2', TWO, dict(population=8193)),
    'nsga2:generations': ('NSGA2', TWO, dict(population=ROWS, generations=0)),
    'nsga2:thin': ('NSGA2', TWO, dict(population=ROWS, thin=0)),
    'nsga2:cr': ('NSGA2', TWO, dict(population=ROWS, cr=1.5)),
    'nsga2:direction': ('NSGA2', ({'NSE': 'up', 'PBias': 'min'},), dict(population=ROWS)),
    'nsga2:dimensions': ('NSGA2', TWO, dict(population=ROWS, vary=['T'] * 17)),
    'nsga2:vary_none': ('NSGA2', TWO, dict(population=ROWS, vary=[])),
    'nsga2:vary_twice': ('NSGA2', TWO, dict(population=ROWS, vary=['T', 'T'])),
    'nsga2:vary_unknown': ('NSGA2', TWO, dict(population=ROWS, vary=['T', 'Q'])),
    'nsga2:fixed_varies': ('NSGA2', TWO, dict(population=ROWS, fixed={'T': 1.0})),
    'nsga2:fixed_unknown': ('NSGA2', TWO, dict(population=ROWS, vary=['T'], fixed={'Q': 1.0})),
}


def recorder():
    """make_montecarlo_analyses_parent.py as a module: Record, counted and file_bytes are its"""
    from support import golden_script
    return golden_script('make_montecarlo_analyses_parent')


def example(folder):
    """the example catchment under `folder` with the settings file of every construction here -> its root"""
    from support import example_root, settings_file
    root = example_root(folder)
    settings_file(root, SETTINGS, '01/01/2007', '31/12/2007', 90, simu_minutes=1440)
    return root


def construct(root, spec):
    from support import EXTRA
    from smartpy_amd import montecarlo
    name, args, kw = spec
    obj = getattr(montecarlo, name)('Catchment', root, 'csv', 'csv', *args, settings_filename=SETTINGS, **kw)
    obj.model.extra = EXTRA
    return obj


def host_part(folder):
    """the constructions and the refusals -> {key: array}"""
    root = example(folder)
    record = {}
    for who, spec in CONSTRUCTIONS.items():
        obj = construct(root, spec)
        record['host|%s|initial_population' % who] = np.array(obj.initial_population)
        record['host|%s|columns' % who] = np.asarray(obj.columns, dtype=np.int64)
        record['host|%s|lo' % who] = np.array(obj.lo)
        record['host|%s|hi' % who] = np.array(obj.hi)
        record['host|%s|vary' % who] = np.asarray(obj.vary, dtype=np.str_)
    for label, spec in REFUSALS.items():
        try:
            construct(root, spec)
        except Exception as e:      # (the parent raises plain Exception for vary / fixed)
            record['host|refusal|%s|text' % label] = np.asarray('%s: %s' % (type(e).__name__, e), dtype=np.str_)
            record['host|refusal|%s|code' % label] = np.asarray(getattr(e, 'code', 0))
        else:
            raise AssertionError('%s was not refused' % label)
    return record


def device_part(folder):
    """the three runs -> Record"""
    import torch
    assert torch.cuda.is_available(), 'the samplers run on the GPU'
    rec = recorder()
    root = example(folder)
    record = rec.Record()
    for who, spec in RUNS.items():
        obj = construct(root, spec)
        calls = rec.counted(obj)
        record.call(who, 'run', calls, obj.run, write=True)
        record.state(who, 'run', obj)
        record['%s|run|diagnostics' % who] = obj.diagnostics
        record['%s|run|file' % who] = rec.file_bytes(obj.diagnostics_file)
        if spec[0] == 'NSGA2':
            record['%s|run|rank' % who] = obj.rank
            record['%s|run|crowding' % who] = obj.crowding
            record['%s|run|keys' % who] = obj.keys.cpu().numpy()
        else:
            record['%s|run|log_density' % who] = obj.log_density.cpu().numpy()
            record['%s|run|accepted' % who] = obj.posterior.accepted
            record['%s|run|rhat' % who] = obj.rhat
            record['%s|run|error_parameters' % who] = obj.posterior.error_parameters.cpu().numpy()
    return record


def main(path, host_only=False):
    import tempfile
    from smartpy_amd import _lib
    print('library:', _lib.LIB_PATH)
    with tempfile.TemporaryDirectory() as folder:
        record = host_part(os.path.join(folder, 'host'))
        if not host_only:
            record.update(device_part(os.path.join(folder, 'device')))
    np.savez_compressed(path, **record)
    for key in sorted(record):
        print('%-56s %-8s %s' % (key, record[key].dtype, record[key].shape))
    print('%d entries, %d bytes -> %s' % (len(record), os.path.getsize(path), path))


if __name__ == '__main__':
    names = [a for a in sys.argv[1:] if not a.startswith('--')]
    main(names[0] if names else FIXTURE, host_only='--host-only' in sys.argv)
