"""montecarlo.DEMCz and montecarlo.NSGA2 as far as they go without a device, against what the commit before their common
base (smartpy_amd/montecarlo/generational.py) built: the starting population, the varying columns and their box of five
constructions bit for bit, and the text and code of every refusal of the two constructors as strings
(tests/golden/make_samplers_parent.py holds the constructions, samplers_parent.npz what they gave)."""
import pytest

from conftest import load_golden
from support import golden_script, same_bits

cases = golden_script('make_samplers_parent')


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    """(what the constructions give on this tree, what they gave at the parent), key by key"""
    parent = load_golden('samplers_parent.npz')
    return cases.host_part(str(tmp_path_factory.mktemp('samplers'))), \
        {key: parent[key] for key in parent.files if key.startswith('host|')}


def test_the_constructions_and_refusals_are_the_ones_recorded(both):
    got, parent = both
    assert sorted(got) == sorted(parent)
    assert len([key for key in parent if key.endswith('|initial_population')]) == len(cases.CONSTRUCTIONS) == 5
    assert len([key for key in parent if key.endswith('|text')]) == len(cases.REFUSALS)
    # what the constructions are there for: a subset that varies, error parameters as further columns
    assert parent['host|demcz_subset|columns'].tolist() == parent['host|nsga2_three|columns'].tolist() == [0, 6, 7, 8]
    assert parent['host|demcz_ar1|initial_population'].shape == (cases.ROWS, 13)
    assert parent['host|demcz_ar1|columns'].tolist() == list(range(10)) + [10, 11]        # phi is fixed


@pytest.mark.parametrize('who', sorted(cases.CONSTRUCTIONS))
def test_the_constructions_are_equal_bit_for_bit(both, who):
    got, parent = both
    for what in ('initial_population', 'columns', 'lo', 'hi'):
        key = 'host|%s|%s' % (who, what)
        assert same_bits(got[key], parent[key]), key
    assert got['host|%s|vary' % who].tolist() == parent['host|%s|vary' % who].tolist()


@pytest.mark.parametrize('label', sorted(cases.REFUSALS))
def test_the_refusals_are_equal_as_strings(both, label):
    got, parent = both
    key = 'host|refusal|%s|' % label
    assert str(got[key + 'text']) == str(parent[key + 'text'])
    assert int(got[key + 'code']) == int(parent[key + 'code'])
