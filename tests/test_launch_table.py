"""The decisions of the engine's C side, held as a whole: for every row of tests/golden/engine_launch_table.json (a
SmartEnsemble with dummy pointers plus environment overrides; tests/golden/make_engine_launch_table.py made the rows and
recorded, from the PARENT commit's library, what it answered) the verdict of smart_check_ensemble, the number
smart_workspace_bytes asks for and the text of smart_describe_launch are what they were.  Nothing is allocated, nothing
is launched."""
import ctypes
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location(
    'make_engine_launch_table', os.path.join(ROOT, 'tests', 'golden', 'make_engine_launch_table.py'))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

TABLE = json.load(open(maker.FIXTURE))
ROWS = TABLE['rows']


@pytest.fixture(scope='module')
def L():
    from smartpy_amd import build as hip_build
    hip_build.build()                       # no-op when up to date; hipcc cross-compiles without a GPU
    from smartpy_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def answers(L):
    """every row asked once: {name: what make_engine_launch_table.ask() returns}"""
    buf = (ctypes.c_double * 16)()
    with_device = maker.device_cus(L) > 0
    return {r['name']: maker.ask(L, r, ctypes.addressof(buf), with_device) for r in ROWS}


def test_the_table_is_the_one_its_maker_describes():
    """the rows in the file are the rows of the maker script, every column recorded"""
    fresh = maker.rows()
    assert [r['name'] for r in fresh] == [r['name'] for r in ROWS] and len(ROWS) >= 150
    for new, old in zip(fresh, ROWS):
        assert all(new[k] == old[k] for k in ('e', 'pointers', 'workspace', 'env')), new['name']
        assert all(k in old for k in ('check', 'bytes_no_device', 'bytes_device', 'describe')), new['name']
    assert TABLE['multi_processor_count'] * 4 == maker.N_SIMD


def test_check_refuses_what_it_refused_with_the_same_words(L, answers):
    assert L.smart_check_ensemble(None) == -1 and L.smart_last_error() == b'SmartEnsemble pointer is NULL'
    codes = set()
    for r in ROWS:
        assert answers[r['name']]['check'] == r['check'], r['name']
        assert (r['check'][0] == 0) == (r['check'][1] == ''), r['name']
        codes.add(r['check'][0])
    assert codes == {0, -1, -2, -3, -4, -5, -7}     # every code check() can return
    assert sum(1 for r in ROWS if r['check'][0]) >= 25


def test_workspace_bytes_of_every_row(L, answers):
    cus = maker.device_cus(L)
    if cus and cus != TABLE['multi_processor_count']:
        pytest.skip('the table was recorded on a device of %d CUs, this one has %d' % (TABLE['multi_processor_count'], cus))
    column = 'bytes_device' if cus else 'bytes_no_device'
    assert L.smart_workspace_bytes(None) == 0
    for r in ROWS:
        assert answers[r['name']]['bytes'] == r[column], r['name']
        # (the workspace the caller then brings does not change what is asked for)
        assert answers[r['name']]['bytes_with_workspace'] == r[column], r['name']


@pytest.mark.gpu
def test_describe_launch_of_every_row(L, answers):
    cus = maker.device_cus(L)
    if cus != TABLE['multi_processor_count']:
        pytest.skip('the table was recorded on a device of %d CUs, this one has %d' % (TABLE['multi_processor_count'], cus))
    for r in ROWS:
        assert answers[r['name']]['describe'] == r['describe'], r['name']
        assert answers[r['name']]['bytes'] == r['bytes_device'], r['name']
    # every kernel of the family is named somewhere in the table, and each form of a launch's description
    text = ' '.join(r['describe'][1] for r in ROWS)
    for name in ('intervals_exits', 'intervals', 'intervals_states', 'steps', 'steps_states', 'plain', 'stiff', 'guard',
                 'illcond', 'runs_exits', 'runs', 'runs_states', 'steps_raw', 'intervals_raw', 'steps_every',
                 'illcond_lanes'):
        assert 'smart_fast_%s[' % name in text, name
    assert 'smart_ensemble_literal' in text and ' slices x ' in text and 'DPP row x 16 wavefronts' in text
