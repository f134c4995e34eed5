"""The order-statistics kernels along the sample axis where their workgroup primitives change behaviour: at the thread
count and the capacity of every (CAP, THREADS) instance and one past each, in the four ways the long stages of the global
ensemble form run, across the wavefront, the workgroup and both LDS capacities of smart_dynia_shares
(tests/golden/make_order_stats_parent.py has the cases and says why).  Needs an MI355X.

Every case is held to the bits of tests/golden/order_stats_parent.npz, made by the library of the commit BEFORE the bitonic
network in LDS and the weight scan became one definition each (csrc/smart_order_stats.h), shared by smart_quantiles_sort --
which took the two-stages-a-pass network for its own one-stage one -- and smart_ensemble_scores_lds / _global.  No
comparator, no order of summation and no launch geometry changed, so those kernels have to reproduce every bit (compared as
int64: a NaN only equals a NaN of the same payload, -0.0 is not 0.0) -- whole arrays element by element, and through their
sha256.  A differing bit is a defect of the code, never a reason to record the fixture again.
smart_quantiles_select, smart_dynia_shares and the one bootstrap case (whose quantiles are the flow-duration sort form,
launch_flow_duration, not smart_quantiles_sort) run none of the shared code; they are held to the parent's bits all the
same, so that a later fold of their workgroup sums finds its cases here.
"""
import importlib.util
import os

import numpy as np
import pytest

from support import eng        # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_order_stats_parent',
                                               os.path.join(HERE, 'golden', 'make_order_stats_parent.py'))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


@pytest.fixture(scope='module')
def parent():
    return cases.load_fixture()


def test_the_cases_are_where_the_shared_code_changes_behaviour(eng, parent):
    """what the cases claim, from the arrays and the library's own capacities"""
    cases.check_inputs()        # a finite (and live) value in every step of every case
    cap = eng.quantiles_sort_capacity()
    assert cap == cases.SORT_CAPACITY == eng.ensemble_scores_lds_capacity()
    sizes = set(cases.QUANTILE_SIZES)
    for instance in (1024, 2048, 4096, cap):                # the capacities of the sort instances, and one past each
        assert instance in sizes and (instance + 1 in sizes or instance == cap)
    for threads in (512, 1024):                             # their thread counts, one below and one past
        assert {threads - 1, threads, threads + 1} <= sizes
    assert cap - 1 in sizes and cases.SELECT_ONLY == [cap + 1]
    # the global form pads to a power of two of at least 4096: no long stage, one, a fused pair, a pair and one
    padded = [max(4096, 1 << int(np.ceil(np.log2(N)))) for N in cases.GLOBAL_SIZES]
    assert sorted(set(padded)) == [4096, 8192, 16384, 32768]
    lds = eng.dynia_lds_capacity()
    assert {63, 64, 65, 2048, 2049, lds, lds + 1} <= set(cases.DYNIA_SIZES)
    for N in (65, 1025):
        sim = cases.matrix(N)
        assert sim.shape == (cases.R, N + cases.PAD) and np.isnan(sim[:, N:]).all()
        assert len(set(sim[1, :N])) == 7
        special = sim[2, :N]
        assert np.isnan(special).any() and np.isposinf(special).any() and np.isneginf(special).any()
        assert (np.signbit(special) & (special == 0)).any() and (~np.signbit(special) & (special == 0)).any()
        assert (cases.weights(N, 'zero') == 0).sum() == N // 3
    # every group is in the fixture, and nothing else
    assert {k.split('|')[0] + '|' + k.split('|')[1] for k in parent} == {'%s|N%d' % g for g in cases.GROUPS}


@pytest.mark.parametrize('entry, N', cases.GROUPS, ids=['%s-%d' % g for g in cases.GROUPS])
def test_the_parent_commits_bits(eng, parent, entry, N):
    got = cases.run_group(eng, entry, N)
    assert got and set(cases.key(entry, N, name) for name in got) == {k for k in parent
                                                                      if k.startswith('%s|N%d|' % (entry, N))}
    for name, a in got.items():
        bits, sha = cases.kept(a)
        want_bits, want_sha = parent[cases.key(entry, N, name)]
        differ = int((bits != want_bits).sum()) if bits.shape == want_bits.shape else -1
        print('%s N=%d %s: %d values, %d differ' % (entry, N, name, bits.size, differ))
        assert np.array_equal(bits, want_bits), (entry, N, name)
        assert sha == want_sha, (entry, N, name)
