"""The thirteen side files of the Monte-Carlo workflows, byte for byte, as the PARENT commit's host code writes them ->
tests/golden/side_files_parent.json (file name -> its text, the line endings kept as they are: the files are read with
open(..., 'rb'), and JSON escapes a carriage return and a line feed, it does not translate them).  Needs no device; run once
at the parent commit:

    python tests/golden/make_side_files_parent.py [out.json]

The change the fixture was made for moved the analyses of the stored discharge matrix into
smartpy_amd/montecarlo/analyses.py and put every hand-written "header, then a line per stamp or label" loop behind one
writer; every file has to keep its bytes, whichever line terminator it had: the csv.writer ones '\\r\\n', the others '\\n'.
The calls live here, so that tests/test_side_files_host.py makes exactly the calls the fixture recorded (the four
`_write_*_file` functions of the float32 family are looked up in the module that holds them: analyses.py, at the parent
montecarlo.py).

Shapes: 2 windows, 3 samples, 2 probabilities, 4 report stamps, the 10 parameters.  The tables are filled, in turn, from
POOL: NaN, both infinities, -0.0, 1e-310 and 1e39 (the last two underflow and overflow the float32 of the '%.6e' family)
among ordinary values.  `<name>.empty` is the same call on a table with N = 0 rows.  `.bounds` and `.verification` have no
writer function at the parent: they come out of GLUE.prediction_bounds / ensemble_verification, on a GLUE with no behavioural
set (no launch: the NaN tables) and on one with three behavioural rows whose _launch_stored and engine calls are replaced by
stubs that hand back fixed CPU tensors."""
import datetime
import json
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'tests'))

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'side_files_parent.json')
SUFFIXES = ['.windows', '.fdc', '.signatures', '.uncertainty', '.dynia', '.pawn', '.errormodel', '.predictive', '.bounds',
            '.verification', '.indices', '.series', '.diagnostics']
#: the line terminator of every line of the file, the header's included
TERMINATOR = {'.windows': '\n', '.fdc': '\n', '.signatures': '\n', '.uncertainty': '\n', '.dynia': '\n', '.pawn': '\n',
              '.errormodel': '\r\n', '.predictive': '\r\n', '.bounds': '\r\n', '.verification': '\r\n', '.indices': '\n',
              '.series': '\n', '.diagnostics': '\n'}
POOL = [0.5, np.nan, -1.25, np.inf, 3.0e-5, -np.inf, 12345.678, -0.0, 1e-310, 0.1, 1e39, -7.0e20, 2.0 / 3.0]
W, N, K, R = 2, 3, 2, 4
NAMES = ['T', 'C', 'H', 'D', 'S', 'Z', 'SK', 'FK', 'GK', 'RK']
OBJ = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE', 'GW']
LABELS = ['2007', '2008']
PROBS = [0.05, 0.95]
STAMPS = [datetime.datetime(2007, 1, 1, 9) + datetime.timedelta(days=d) for d in range(R)]
SETTINGS = 'Catchment.short.sttngs'


def table(*shape, start=0):
    """an array of `shape` filled from POOL in turn, beginning at its element `start`"""
    size = int(np.prod(shape))
    return np.array([POOL[(start + i) % len(POOL)] for i in range(size)], dtype=np.float64).reshape(shape)


def float32_writers():
    """the module that holds _write_windows_file, _write_fdc_file, _write_signatures_file and _write_uncertainty_file"""
    try:
        from smartpy_amd.montecarlo import analyses as home
    except ImportError:
        from smartpy_amd.montecarlo import montecarlo as home
    return home


def written_by_functions(folder):
    """the eleven files that a function writes, and each once more from a table without rows -> {name: path}"""
    from smartpy_amd import demcz, errormodel, identifiability, pawn
    from smartpy_amd.montecarlo import sobol
    home = float32_writers()
    paths = {}

    def at(name):
        paths[name] = os.path.join(folder, 'Catchment.SMART.lhs' + name)
        return paths[name]
    for n, tag in ((N, ''), (0, '.empty')):
        home._write_windows_file(at('.windows' + tag), LABELS, 'log', table(W, n, 7))
        home._write_fdc_file(at('.fdc' + tag), PROBS, LABELS, 'sqrt', table(W, K, n, start=1), table(W, n, 7, start=2))
        home._write_signatures_file(at('.signatures' + tag), LABELS, table(W, 12, n, start=3))
        home._write_uncertainty_file(at('.uncertainty' + tag), PROBS, table(n, 7, start=4), table(7, n, start=5),
                                     table(7, n, start=6), table(7, K, n, start=7))
        errormodel.write_likelihood_file(at('.errormodel' + tag), table(n, 3, start=8), table(3, n, start=9))
    for r, tag in ((R, ''), (0, '.empty')):
        stamps = STAMPS[:r]
        identifiability.write_file(at('.dynia' + tag), stamps, NAMES, table(r, 10, start=10), table(r, 10, 2, start=11))
        pawn.write_file(at('.pawn' + tag), stamps, NAMES, table(r, 10, start=12), table(r, start=1))
        errormodel.write_predictive_file(at('.predictive' + tag), stamps, PROBS, table(K, r, start=2), table(K, r, start=3))
        sobol._write_series_file(at('.series' + tag), stamps, NAMES, table(r, 10, start=4), table(r, 10, start=5))
        demcz.write_diagnostics(at('.diagnostics' + tag), NAMES, np.concatenate(
            [10.0 * np.arange(r)[:, None], table(r, 11, start=6)], axis=1))
    # the labels of a table of objective functions, and indices without confidence half-widths
    pawn.write_file(at('.pawn.labels'), OBJ[:7] + ['GW_RATIO'], NAMES, table(8, 10, start=7), table(8, start=8))
    sobol._write_indices_file(at('.indices'), ['NSE', 'GW'], NAMES, table(2, 10, start=9), table(2, 10, start=10),
                              table(2, 10, start=11), table(2, 10, start=12))
    sobol._write_indices_file(at('.indices.no_conf'), ['target0'], NAMES[:3], table(1, 3, start=1), None, table(1, 3, start=2),
                              None)
    sobol._write_indices_file(at('.indices.empty'), [], NAMES, table(0, 10), None, table(0, 10), None)
    return paths


class _Stored(object):
    def __init__(self, matrix):
        self.discharge_report_major = matrix


def glue(folder, level):
    """a GLUE on four report steps of the example catchment, built from a sampling database of N rows whose objective
    functions are 0.1, 0.5 and 0.9 in every column, conditioned on NSE >= level"""
    import shutil
    from support import settings_file
    from conftest import GOLDEN
    from smartpy_amd.montecarlo import GLUE
    from smartpy_amd.montecarlo.database import SamplingCsv
    root = os.path.join(folder, 'data')
    if not os.path.isdir(root):
        shutil.copytree(os.path.join(GOLDEN, 'data', 'in'), os.path.join(root, 'in'))
        settings_file(root, SETTINGS, '01/01/2007', '04/01/2007', 1)
        os.makedirs(os.path.join(root, 'out', 'Catchment'))
        db = SamplingCsv(os.path.join(root, 'out', 'Catchment', 'Catchment.SMART.lhs'), OBJ, NAMES).create(N)
        db.write_table(np.tile(np.array([[0.1], [0.5], [0.9]]), (1, len(OBJ))), np.arange(10.0 * N).reshape(N, 10))
        db.close()
    return GLUE('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (level,))}, settings_filename=SETTINGS)


def written_by_glue(folder):
    """`.bounds` and `.verification`: of a GLUE without a behavioural set, and of one with three behavioural rows whose
    launch and engine calls are stubs -> {name: bytes} (both objects write the same two paths)"""
    import torch
    from smartpy_amd import engine
    files = {}
    for tag, level in (('.empty', 2.0), ('', 0.0)):
        obj = glue(folder, level)
        assert obj._sample.shape[0] == (0 if tag else N) and len(obj.model.timeseries_report) - 1 == R
        obj._launch_stored = lambda: (_Stored(torch.from_numpy(table(R, N))), torch.from_numpy(table(R, start=4)))
        held = engine.weighted_quantiles, engine.ensemble_scores
        engine.weighted_quantiles = lambda sim, q, weights=None: torch.from_numpy(table(len(q), R, start=5))
        engine.ensemble_scores = lambda sim, obs, weights=None: torch.from_numpy(table(5, R, start=6))
        try:
            bounds = obj.prediction_bounds(quantiles=PROBS, likelihood=None if tag else 'KGE', write=True)
            scores = obj.ensemble_verification(write=True)
        finally:
            engine.weighted_quantiles, engine.ensemble_scores = held
        for name, path in (('.bounds', bounds.file), ('.verification', scores.file)):
            with open(path, 'rb') as f:
                files[name + tag] = f.read()
    return files


def side_files(folder):
    """every call -> {name: the bytes of the file it wrote}"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)        # (1e39 becomes the inf of float32 on purpose)
        paths, files = written_by_functions(folder), written_by_glue(folder)
    for name, path in paths.items():
        with open(path, 'rb') as f:
            files[name] = f.read()
    assert all(any(name == s or name.startswith(s + '.') for name in files) for s in SUFFIXES)
    return files


def main(path):
    with tempfile.TemporaryDirectory() as folder:
        files = {name: raw.decode('utf8') for name, raw in side_files(folder).items()}
    with open(path, 'w', newline='\n', encoding='utf8') as f:
        json.dump(files, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d files, %d bytes -> %s' % (len(files), os.path.getsize(path), path))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
