"""The scores of smart_flow_duration_hip against the exact scores of oracle/analyses/flow_duration.py.

Every case of that module's list -- one R per instance of the sort form (1,024 x 16, 2,048 x 8, 4,096 x 4, 8,192 x 2,
16,384 x 1), an N that leaves the instance's last workgroup partial, the four transforms, the whole curve, its top 2 %,
its bottom 30 % and the mid segment (0.3, 0.7), one window without an array and seven uneven ones (rows in no window, a
window without an observation) -- goes through the C entry with ld = N + 3, NaN in the padding and guarded outputs, and
is held to `truth` (fractions.Fraction on the pairs of the segment) within `bounds(S, E, 0)`: what any order of the
float64 additions may differ by when the one-pass moments are taken about the column's value at rank i0, THE FIRST RANK
OF THE SEGMENT.  The pattern of NaN and of infinities is equal.  The order statistics of the same launch stay bit-equal
to the numpy statement.

The host module holds the data to the conditions that make this one bite: on the `plateau` family the moments about rank
0 of the window (or about any value from outside the segment) miss the bound 1e5-fold and more, under every instance.
The tolerance is the derived bound and nothing else; the largest used fraction per (instance, transform) is printed at
the end of the module (and written to $SMART_MARGINS_DIR/flow_duration_margins.txt where that is set);
profiles/flow_duration_margins.txt is that table."""
import numpy as np
import pytest

import support
from cases_flow_duration import (CASES, EMPTY, INSTANCES, SEGMENTS, TRANSFORMS, case_data, case_id, case_reference, launch,
                                 plateau, window_array)
from cases_objfn import EPS
from oracle.analyses.flow_duration import curve_reference, statement
from support import Margins, bits_equal, margins_dir, same_values

pytestmark = pytest.mark.gpu

PAD = 3             # ld = N + 3, the padding holds NaN
PROBS = [0.0, 0.05, 0.5, 1.0 / 3.0, 0.95, 1.0]
MARGINS = Margins()


def path_of(R, transform):
    return 'smart_fdc_sort %s, %s' % (INSTANCES[R][0], transform)


def hold(R, transform, what, got, want, bnd):
    support.hold(MARGINS, path_of(R, transform), what, got, want, bnd)


@pytest.fixture(scope='module', autouse=True)
def _print_the_margins():
    yield
    if not MARGINS:
        return
    paths = [path_of(R, t) for R in sorted(INSTANCES) for t in TRANSFORMS]
    text = ('largest |result - truth| of this run as a fraction of bounds(S, E, 0) of oracle/analyses/flow_duration.py '
            '(truth in fractions.Fraction on the pairs of the segment; the bound is what any order of the float64 additions '
            'about the first in-segment rank may differ by): instance of the sort form (rows x columns) and transform, '
            'fraction, where it was seen\n' +
            '\n'.join('%-38s %-10.3g %s' % (p, MARGINS[p][0], MARGINS[p][1])
                      for p in paths + sorted(set(MARGINS) - set(paths)) if p in MARGINS) + '\n')
    MARGINS.publish(text, margins_dir(), 'flow_duration_margins.txt')


def scores_of(case):
    """one launch of the case -> (order statistics [W, K, N], scores [W, N, 7])"""
    R, N, W, windows, transform, segment, family = case
    sim, obs, win, eps = case_data(case)
    # (copies: the case's arrays are shared and read-only, and torch wants to own what it wraps)
    return launch(sim, PROBS, obs.copy(), None if win is None else win.copy(), W, transform, eps, segment, objfn=True,
                  pad=PAD)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_scores_of_the_curve_about_the_first_rank_of_the_segment(case):
    R, N, W, windows, transform, segment, family = case
    sim, obs, win, eps = case_data(case)
    want, bnd = case_reference(case)
    quant, got = scores_of(case)
    assert same_values(quant, statement(sim, PROBS, obs, win, W)[0]), case_id(case)
    hold(R, transform, case_id(case), got, want, bnd)


@pytest.mark.parametrize('R', sorted(INSTANCES))
def test_two_launches_give_the_same_bits(R):
    case = [c for c in CASES if c[0] == R and c[2] == 7 and c[6] == 'plateau'][0]
    (quant, got), (quant2, again) = scores_of(case), scores_of(case)
    assert np.isfinite(got).any() and bits_equal(got, again) and bits_equal(quant, quant2)


def test_through_the_engine_on_a_strided_view():
    """a plateau through engine.flow_duration, the matrix a view of a wider device tensor whose other columns hold NaN"""
    import torch
    from smartpy_amd import engine
    R, n, transform, segment = 1025, 130, 'sqrt', SEGMENTS[3]
    W, win = window_array(R, 'uneven')
    sim, obs = plateau(20250, R, n, win, W, transform, segment)
    obs[win == EMPTY] = np.nan
    want, bnd = curve_reference(sim, obs, win, W, transform, EPS[transform], segment)
    assert np.isfinite(want).sum() == (W - 1) * n * 7            # (the window without an observation is among the seven)
    wide = torch.full((R, n + 63), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :n] = torch.from_numpy(sim).cuda()
    quant, scores = engine.flow_duration(wide[:, :n], PROBS, torch.from_numpy(obs).cuda(), torch.from_numpy(win).cuda(),
                                         n_windows=W, transform=transform, eps=EPS[transform], segment=segment, objfn=True)
    assert tuple(quant.shape) == (W, len(PROBS), n) and tuple(scores.shape) == (W, n, 7)
    assert same_values(quant.cpu().numpy(), statement(sim, PROBS, obs, win, W)[0])
    hold(R, transform, 'engine, strided view, R=%d N=%d W=%d %r plateau' % (R, n, W, segment), scores.cpu().numpy(), want, bnd)
