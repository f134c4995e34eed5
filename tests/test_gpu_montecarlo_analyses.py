"""Every analysis method of the Monte-Carlo workflows against what the commit before analyses.py left: the arrays of the
results bit for bit, the side files and the sampling databases byte for byte, and the number of model.simulate_ensemble
calls each method makes (tests/golden/make_montecarlo_analyses_parent.py holds the objects and the calls,
montecarlo_analyses_parent.npz what they gave on the MI355X).  The kernels are the same, so nothing here has a tolerance.
Needs an MI355X."""
import numpy as np
import pytest

from conftest import load_golden
from support import golden_script, same_bits

pytestmark = pytest.mark.gpu

cases = golden_script('make_montecarlo_analyses_parent')


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    """(what the calls give on this tree, what they gave at the parent), key by key"""
    parent = load_golden('montecarlo_analyses_parent.npz')
    return cases.run_all(str(tmp_path_factory.mktemp('analyses'))), {key: parent[key] for key in parent.files}


def kind(key):
    last = key.split('|')[-1]
    return 'launches' if last == 'launches' else 'bytes' if last in ('file', 'database') else 'array'


def test_the_calls_are_the_ones_recorded(both):
    got, parent = both
    assert sorted(got) == sorted(parent)
    calls = {key.split('|')[1].split(':')[0].split('@')[0] for key in parent if key.startswith('host|')}
    assert calls == {'window_objective_functions', 'flow_duration_curves', 'hydrological_signatures', 'score_uncertainty',
                     'dynamic_identifiability', 'pawn_sensitivity', 'residual_likelihood', 'predictive_bounds', 'run'}
    # every analysis wrote its file, on the object without rows too
    for who in ('host', 'device', 'nobody'):
        assert sum(1 for key in parent if key.startswith(who + '|') and key.endswith('|file')) >= 9, who
    assert parent['nobody|run|sample'].shape == (0, 10) and parent['host|run|sample'].shape == (cases.ROWS, 10)


def test_the_arrays_are_equal_bit_for_bit(both):
    got, parent = both
    different = [key for key in sorted(parent) if kind(key) == 'array' and not same_bits(got[key], parent[key])]
    assert not different, different
    # the sample as a device tensor goes another way into the launch and gives the same bits
    for key in sorted(parent):
        if key.startswith('host|') and kind(key) == 'array':
            assert same_bits(got[key], got['device|' + key[len('host|'):]]), key


def test_the_files_are_equal_byte_for_byte(both):
    got, parent = both
    different = [key for key in sorted(parent) if kind(key) == 'bytes' and got[key].tobytes() != parent[key].tobytes()]
    assert not different, different
    assert sum(1 for key in parent if kind(key) == 'bytes') >= 40


def test_the_launch_counts_are_equal(both):
    got, parent = both
    counts = {key: (int(got[key]), int(parent[key])) for key in sorted(parent) if kind(key) == 'launches'}
    assert not {key: pair for key, pair in counts.items() if pair[0] != pair[1]}
    # one launch per analysis of the stored matrix, none where there are no rows or run() has left the scores
    assert counts['host|predictive_bounds|launches'] == (1, 1) and counts['demcz|run|launches'] == (5, 5)
    assert counts['host|pawn_sensitivity:objective_functions|launches'] == (1, 1)
    assert counts['host|pawn_sensitivity:objective_functions@run|launches'] == (0, 0)
    assert all(pair == (0, 0) for key, pair in counts.items() if key.startswith('nobody|'))
