"""The host layer of the Monte-Carlo analyses, without a device: every side file byte for byte as the commit before
analyses.py wrote it (tests/golden/make_side_files_parent.py holds the calls, side_files_parent.json the bytes), the line
terminator of each file said out loud, the likelihood-to-weights rule through both of its callers with their full texts, and
the parameters of every public analysis method and side-file property on the four classes that offer them."""
import inspect
import json

import pytest

from support import golden_script

cases = golden_script('make_side_files_parent')


@pytest.fixture(scope='module')
def written(tmp_path_factory):
    return cases.side_files(str(tmp_path_factory.mktemp('side_files')))


def test_every_side_file_keeps_its_bytes(written):
    with open(cases.FIXTURE, encoding='utf8', newline='') as f:
        parent = {name: text.encode('utf8') for name, text in json.load(f).items()}
    assert sorted(written) == sorted(parent)
    different = [name for name in sorted(parent) if written[name] != parent[name]]
    assert not different, {name: (written[name], parent[name]) for name in different[:2]}
    # all thirteen, each with values and each (but the two a GLUE writes, which always has its report steps) without a row
    assert sorted(name for name in parent if name.count('.') == 1) == sorted(cases.SUFFIXES)
    # the awkward values are in both families of cells: float64 printed by Python ('%e', '%.6e'), which keeps 1e-310 and
    # 1e39, and the float32 '%.6e' of the sampling database, which loses both
    python = b''.join(parent[s] for s in ('.dynia', '.pawn', '.errormodel', '.predictive', '.bounds', '.verification'))
    float32 = b''.join(parent[s] for s in ('.windows', '.fdc', '.signatures', '.uncertainty', '.indices', '.series'))
    for token in (b',nan', b',inf', b',-inf', b',-0.000000e+00'):
        assert token in python and token in float32, token
    assert b'1.000000e-310' in python and b'1.000000e+39' in python
    assert b'e-310' not in float32 and b'e+39' not in float32


def test_the_line_terminator_of_each_file(written):
    """'\\r\\n' in the four files that began as csv.writer output, '\\n' in the nine others: the header's and every row's"""
    assert sorted(cases.TERMINATOR) == sorted(cases.SUFFIXES)
    assert sorted(s for s, end in cases.TERMINATOR.items() if end == '\r\n') == \
        ['.bounds', '.errormodel', '.predictive', '.verification']
    for name, raw in written.items():
        end = cases.TERMINATOR[[s for s in cases.SUFFIXES if name == s or name.startswith(s + '.')][0]].encode()
        lines = raw.split(b'\n')
        assert lines[-1] == b'' and len(lines) >= 2, name
        for line in lines[:-1]:
            assert line.endswith(b'\r') == (end == b'\r\n'), (name, line)
        assert raw.count(b'\r') == (len(lines) - 1 if end == b'\r\n' else 0), name


NAMES = 'NSE, KGE, KGEc, KGEa, KGEb, PBias, RMSE, GW'
REFUSALS = [   # (likelihood, what GLUE.prediction_bounds says, what MonteCarlo.predictive_bounds says): the parent's texts
    ('Nash',
     "The likelihood 'Nash' is not one of the objective functions of the sampling run (%s)." % NAMES,
     "predictive_bounds: the likelihood 'Nash' is not one of the objective functions of a finished run() of this object "
     "(%s)." % NAMES),
    ([1.0, 2.0],
     "The likelihood array has shape (2,) where one value per behavioural set (3) is expected.",
     "predictive_bounds: the likelihood array has shape (2,) where one value per row of the sample (3) is expected."),
    ([[1.0, 2.0, 3.0]],
     "The likelihood array has shape (1, 3) where one value per behavioural set (3) is expected.",
     "predictive_bounds: the likelihood array has shape (1, 3) where one value per row of the sample (3) is expected."),
    ([1.0, -0.5, float('nan')],
     "2 of the 3 likelihood values are negative or not finite: they cannot be used as weights (shift or select them first, "
     "nothing is clipped here).",
     "predictive_bounds: 2 of the 3 likelihood values are negative or not finite: they cannot be used as weights."),
]


def test_the_weights_rule_through_both_callers(tmp_path):
    import numpy as np
    glue = cases.glue(str(tmp_path), 0.0)
    assert glue._sample.shape == (3, 10)
    for likelihood, by_glue, by_montecarlo in REFUSALS:
        with pytest.raises(Exception) as err:
            glue.prediction_bounds(likelihood=likelihood)
        assert type(err.value) is Exception and str(err.value) == by_glue
        with pytest.raises(Exception) as err:
            glue.ensemble_verification(likelihood=likelihood)
        assert str(err.value) == by_glue
        with pytest.raises(Exception) as err:
            glue.predictive_bounds(error_parameters=[0.1, 0.2, 0.5], likelihood=likelihood)
        assert type(err.value) is Exception and str(err.value) == by_montecarlo
    # a name the object knows: GLUE takes the sampling run's column of its behavioural rows; the analyses of the base class
    # take the column of the object's own finished run(), and there has been none
    assert glue._likelihood_weights('KGE').tolist() == [float(np.float32(v)) for v in (0.1, 0.5, 0.9)]
    with pytest.raises(Exception) as err:
        glue._row_weights('residual_likelihood', 'KGE')
    assert str(err.value) == "residual_likelihood: the likelihood 'KGE' is not one of the objective functions of a finished " \
                             "run() of this object (%s)." % NAMES
    glue.obj_fns = np.arange(24.0).reshape(3, 8)
    assert glue._row_weights('x', 'KGE').tolist() == [1.0, 9.0, 17.0]
    for weights in (glue._likelihood_weights([0.0, 1.0, 2.0]), glue._row_weights('x', np.array([0, 1, 2]))):
        assert weights.dtype == np.float64 and weights.tolist() == [0.0, 1.0, 2.0]
    assert glue._likelihood_weights(None) is None and glue._row_weights('x', None) is None


ANALYSES = {
    'window_objective_functions': ['self', 'windows', 'transform', 'eps', 'start_month', 'split', 'write'],
    'flow_duration_curves': ['self', 'exceedance', 'windows', 'transform', 'eps', 'segment', 'start_month', 'split', 'write'],
    'hydrological_signatures': ['self', 'windows', 'alpha', 'high', 'low', 'thresholds', 'start_month', 'split', 'write'],
    'score_uncertainty': ['self', 'windows', 'resamples', 'seed', 'quantiles', 'transform', 'eps', 'min_steps', 'start_month',
                          'split', 'write'],
    'dynamic_identifiability': ['self', 'half_width', 'fraction', 'bins', 'support', 'min_valid', 'level', 'ranges', 'write'],
    'pawn_sensitivity': ['self', 'of', 'bins', 'statistic', 'dummies', 'seed', 'min_count', 'ranges', 'method', 'write'],
    'residual_likelihood': ['self', 'error_parameters', 'write'],
    'predictive_bounds': ['self', 'error_parameters', 'quantiles', 'replicates', 'likelihood', 'seed', 'truncate', 'verify',
                          'write'],
}
FILES = ['dynia_file', 'fdc_file', 'pawn_file', 'signatures_file', 'uncertainty_file', 'windows_file']
SURFACE = {     # class -> (its methods beyond ANALYSES, run() among them; its `*_file` properties beyond FILES)
    'MonteCarlo': ({'run': ['self', 'compression']}, []),
    'GLUE': ({'run': ['self', 'compression'], 'prediction_bounds': ['self', 'quantiles', 'likelihood', 'write'],
              'ensemble_verification': ['self', 'likelihood', 'bins', 'write']}, []),
    'Sobol': ({'run': ['self', 'compression'], 'sensitivity': ['self', 'targets', 'resamples', 'conf_level', 'seed', 'write'],
               'sensitivity_series': ['self', 'resamples', 'conf_level', 'seed', 'write']}, ['indices_file', 'series_file']),
    'DEMCz': ({'run': ['self', 'compression', 'write']}, ['diagnostics_file']),
}


def test_the_parameters_of_every_analysis_method_and_file_property():
    from smartpy_amd import montecarlo
    from smartpy_amd.montecarlo.analyses import Analyses
    from smartpy_amd.montecarlo.montecarlo import MonteCarlo
    for name, (methods, files) in SURFACE.items():
        cls = MonteCarlo if name == 'MonteCarlo' else getattr(montecarlo, name)
        assert issubclass(cls, MonteCarlo) and issubclass(MonteCarlo, Analyses)
        for method, parameters in dict(ANALYSES, **methods).items():
            assert list(inspect.signature(getattr(cls, method)).parameters) == parameters, (name, method)
        for method in ANALYSES:       # one definition, inherited: nobody overrides an analysis
            assert getattr(cls, method) is getattr(Analyses, method), (name, method)
        found = sorted(n for n in dir(cls) if n.endswith('_file') and isinstance(getattr(cls, n), property))
        assert found == sorted(FILES + files), name
