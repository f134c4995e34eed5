"""The four kernels that list "the valid rows of window w, in row order" (csrc/smart_window_rows.h) where the list can go
wrong: rows of one window on both sides of a 1,024-row chunk boundary, a first chunk that lists nothing, a window of
exactly the two rows 1023 and 1024 (tests/golden/make_window_rows_parent.py has the cases and says why).  Needs an MI355X.

Every case is held to two things:
  (a) the bits of tests/golden/window_rows_parent.npz, made by the library of the commit BEFORE the four copies of the
      compaction were folded into one: the fold changed no arithmetic and no order of summation, so smart_objfn_windows,
      smart_bootstrap_*, smart_signatures and smart_fdc_observed / smart_fdc_sort have to reproduce every bit (compared as
      int64: a NaN only equals a NaN of the same payload, -0.0 is not 0.0) -- the kept sample columns element by element,
      the whole array through its sha256.  AC1 of smart_signatures was re-centred since (each pair list about a member of
      its own): the two signature arrays are held to the pins `<name>|but_ac1` -- the eleven other columns, every bit of
      every sample, made by the library of the commit before that change, which reproduced the full-array pins first --
      and AC1 of the kept columns to the exact truth of oracle/analyses/signatures.py within the bounds derived
      there;
  (b) for smart_objfn_windows_hip, the numpy statement of oracle/analyses/windows.py at the gate of
      tests/test_gpu_objfn_windows.py (rel < 1e-9, |want| floored at 1e-12) on the kept columns: whatever the parent did at
      a chunk boundary, the list has to be the right one.
"""
import importlib.util
import os

import numpy as np
import pytest

from oracle.analyses.signatures import exact, bounds, margins
from oracle.analyses.windows import statement
from support import GATE, rel_to_want, eng      # noqa: F401 (eng is a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_window_rows_parent',
                                               os.path.join(HERE, 'golden', 'make_window_rows_parent.py'))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


@pytest.fixture(scope='module')
def parent():
    return cases.load_fixture()


def test_the_cases_straddle_the_chunk_boundary():
    """what the cases claim, from the arrays: lists that continue across row 1024, a first chunk without an entry, and a
    window of exactly the rows 1023 and 1024"""
    C = cases.CHUNK
    assert {R for R, _ in cases.SHAPES} == {1, 2, C - 1, C, C + 1, 2 * C + 1}
    assert {N for R, N in cases.SHAPES if R == C + 1} == {1, 65, 257}
    for R, N in cases.SHAPES:
        if R <= C:
            continue
        for obs_kind in cases.obs_kinds(R):
            valid = {}
            for kind in cases.WINDOW_KINDS:
                _, obs, win, W = cases.inputs(R, N, kind, obs_kind)
                assert win.min() >= -1 and win.max() < W
                valid[kind] = [np.flatnonzero((win == w) & ~np.isnan(obs)) for w in range(W)]
                assert np.isnan(obs[:C - 1]).all() if obs_kind == 'late' else 0.10 < np.isnan(obs).mean() < 0.20
            for v in valid['one'] + valid['mod3'][C % 3:C % 3 + 1] + (valid['mod3'] if R > 2 * C else []):
                assert (v < C).any() == (obs_kind == 'some') and (v >= C).any()
            assert (valid['blocks'][1] >= C).all() and len(valid['blocks'][1]) >= 1
            assert valid['pair'][1].tolist() == [C - 1, C]
            assert 0.05 < (cases.inputs(R, N, 'minus', obs_kind)[2] == -1).mean() < 0.15
            if obs_kind == 'late':
                assert all((v >= C).all() for v in valid['one'] + valid['mod3'] + valid['minus'])


@pytest.mark.parametrize('R, N', cases.SHAPES)
def test_the_parent_commits_bits_and_the_statement(eng, parent, R, N):
    cols = cases.columns(N)
    for window_kind in cases.WINDOW_KINDS:
        for obs_kind in cases.obs_kinds(R):
            sim, obs, win, W = cases.inputs(R, N, window_kind, obs_kind)
            got = cases.run_case(eng, R, N, window_kind, obs_kind)
            tag = 'R=%d N=%d %s %s' % (R, N, window_kind, obs_kind)
            # (b) the statement
            for transform, eps in (('none', 0.0), ('log', cases.LOG_EPS)):
                want = statement(sim[:, cols], obs, win, W, transform, eps)
                err = rel_to_want(got['windows_' + transform][0][:, cols], want)
                print('%s %s: rel %.3e against the statement, %d NaN entries' % (tag, transform, err,
                                                                                 int(np.isnan(want).sum())))
                assert err < GATE, (tag, transform)
            # (a) the parent commit's bits
            reference = exact(sim[:, cols], obs, win, W)
            bound = bounds(sim[:, cols], obs, win, W, reference=reference)[:, cases.AC1]
            for name, (a, axis) in got.items():
                if name in cases.SIGNATURE_ARRAYS:
                    ac1 = a[:, cases.AC1][:, cols]
                    ratio = margins(ac1, reference[0][:, cases.AC1], bound)
                    print('%s %s: AC1 at %.3g of its bound, %d NaN entries' % (tag, name, ratio.max(),
                                                                              int(np.isnan(ac1).sum())))
                    assert np.all(ratio <= 1.0), (tag, name)
                    a, name = cases.but_ac1(a), name + cases.BUT_AC1
                bits, sha = cases.kept(a, axis, N)
                want_bits, want_sha = parent[cases.key(R, N, window_kind, obs_kind, name)]
                assert np.array_equal(bits.ravel(), want_bits), (tag, name)
                assert sha == want_sha, (tag, name)
