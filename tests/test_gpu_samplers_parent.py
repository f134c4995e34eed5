"""montecarlo.DEMCz (likelihood='ar1') and montecarlo.NSGA2 end to end against what the commit before their common base, the
shared binding module and the shared differential-evolution move left: the sample, the tables and the diagnostics bit for
bit, the database and the diagnostics file byte for byte, and the number of ensemble launches
(tests/golden/make_samplers_parent.py holds the runs, samplers_parent.npz what they gave on the MI355X).  Every output of
both steps is defined to the bit, so nothing here has a tolerance.  Needs an MI355X."""
import pytest

from conftest import load_golden
from support import golden_script, same_bits

pytestmark = pytest.mark.gpu

cases = golden_script('make_samplers_parent')


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    """(what the runs give on this tree, what they gave at the parent), key by key"""
    parent = load_golden('samplers_parent.npz')
    return cases.device_part(str(tmp_path_factory.mktemp('samplers'))), \
        {key: parent[key] for key in parent.files if not key.startswith('host|')}


def kind(key):
    last = key.split('|')[-1]
    return 'launches' if last == 'launches' else 'bytes' if last in ('file', 'database') else 'array'


def test_the_runs_are_the_ones_recorded(both):
    got, parent = both
    assert sorted(got) == sorted(parent)
    assert {key.split('|')[0] for key in parent} == set(cases.RUNS)
    common = {'sample', 'obj_fns', 'gw_contributions', 'diagnostics', 'database', 'file', 'launches'}
    for who, own in (('demcz_ar1', {'log_density', 'accepted', 'rhat', 'error_parameters'}),
                     ('nsga2_two', {'rank', 'crowding', 'keys'}), ('nsga2_three', {'rank', 'crowding', 'keys'})):
        assert {key.split('|')[2] for key in parent if key.startswith(who + '|')} == common | own, who
    # the runs did something: proposals were accepted, more than one front was peeled
    assert parent['demcz_ar1|run|accepted'].sum() > 0 and parent['nsga2_three|run|rank'].max() > 1
    assert parent['demcz_ar1|run|error_parameters'].shape == (2 * cases.ROWS, 3)


def test_the_arrays_are_equal_bit_for_bit(both):
    got, parent = both
    different = [key for key in sorted(parent) if kind(key) == 'array' and not same_bits(got[key], parent[key])]
    assert not different, different


def test_the_files_are_equal_byte_for_byte(both):
    got, parent = both
    different = [key for key in sorted(parent) if kind(key) == 'bytes' and got[key].tobytes() != parent[key].tobytes()]
    assert not different, different
    assert sum(1 for key in parent if kind(key) == 'bytes') == 2 * len(cases.RUNS)


def test_the_launch_counts_are_equal(both):
    got, parent = both
    counts = {key: (int(got[key]), int(parent[key])) for key in sorted(parent) if kind(key) == 'launches'}
    # one launch per generation and the initial one
    assert counts == {'demcz_ar1|run|launches': (5, 5), 'nsga2_two|run|launches': (4, 4), 'nsga2_three|run|launches': (4, 4)}
