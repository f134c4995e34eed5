"""smart_signatures_hip on the GPU against the statement of oracle/analyses/signatures.py.

Shapes are the smallest at which the kernel can go wrong.  R: 1, 2, 3 (no pair, one pair, the first limb); 7, 8, 9 (the load
batch of kSigUnroll = 8 rows: one short, full, one over -- the first listed row is walked ahead of the batches, so 9 and
10 are the batch's own boundary as well: 10 rides with 9); 501; 1025 (one compaction chunk of 1,024 rows plus a row); 4097.
N: 1, 63, 65, 257, 300 (a partial wavefront, a second wavefront, a second workgroup that is partly filled).  Every R
meets every kind of window array (none, two halves, r % 7 -- which has no pair anywhere --, sixteen blocks with 10 % of the
rows in no window), with and without observations, at alpha 0.925 and 0.5.  ld = N + pad with NaN in the padding; the output
lies 64 doubles inside a buffer of sentinels with a spare window behind it.

Data: per column an exponential recession with random events, s <- k s + event, x = 0.05 + s, k in [0.80, 0.98], events
on 15 % of the rows; the observations are a perturbed column with 15 % missing.  Thresholds are the tests' own: the 30th
and the 80th percentile of the window's simulated values, so that both kinds of run occur; window 0 gets two values of
the matrix itself (strictness), the last of several windows a NaN pair.

Gates.  PEAK, PEAK_ROW, HIGH_COUNT, LOW_COUNT and the five columns that are plain additions in row order or one quotient of
two counts -- MEAN, FLASHINESS, RLD, HIGH_DURATION, LOW_DURATION -- are bit-equal to the statement (a zero compared by
value): a row that is dropped, doubled or added out of order shows however small its value.  The pattern of NaN is equal
in every column; AC1 is held to 1e-9 absolute; BFI and RECESSION to the gate the suite holds the sibling kernels to:
rel < 1e-9 with |want| floored at 1e-12, every compared |want| asserted to be 0 or above 1e-6 (a seed that fails this is
changed, not the gate).

The stress family.  oracle/analyses/signatures.py has the twelve columns in exact arithmetic (`truth`), what the
kernel's documented form may differ from them by (`bounds`, derived there) and columns on which a badly centred AC1 shows:
a window that opens on a flood peak (in a pair, and before a gap), series that barely move, a 1e6-fold flood, stretches of
exact zeros, columns that are constant but for one row.  R = 9, 501, 1025 at N = 65, the family in the last columns (they
straddle the two wavefronts), all twelve columns within `bounds` of `truth`, the pattern of NaN exact -- AC1 = NaN for both
constant-but-for-one-row kinds, whose variance is exactly 0.

The largest margins of a run are printed at the end of the module (and written to
$SMART_MARGINS_DIR/signatures_margins.txt where that is set); profiles/signatures_margins.txt is that table."""
import os

import numpy as np
import pytest

from cases_signatures import data, thresholds, stress_case, stress_reference, KINDS, CONSTANT_KINDS, STRESS_R
from oracle.analyses.signatures import (statement, margins, NAMES, PAIR_COLUMNS, MEAN, BFI, FLASHINESS, AC1, RLD, RECESSION,
                                        PEAK, PEAK_ROW, HIGH_COUNT, HIGH_DURATION, LOW_COUNT, LOW_DURATION)
from support import (EXTRA, E_SIZE, GATE, Guarded, Margins, bits_equal, example_root, margins_dir, padded, ptr, same_values,
                     settings_file, to_device, window_arrays)

pytestmark = pytest.mark.gpu

EXACT = [PEAK, PEAK_ROW, HIGH_COUNT, LOW_COUNT, MEAN, FLASHINESS, RLD, HIGH_DURATION, LOW_DURATION]
CLOSE = [BFI, RECESSION]
# R -> the N it is run with
SHAPES = {1: (1, 65), 2: (1, 63, 257), 3: (65, 300), 7: (1, 257), 8: (63, 65), 9: (1, 300), 10: (65,), 501: (63, 300),
          1025: (1, 257), 4097: (65,)}
MARGINS = Margins()     # column name -> (largest margin as a fraction of its gate, where it was seen)
STRESS_MARGINS = Margins()  # column name -> (largest |got - truth| / bound on the stress family, where it was seen)
FILLER = 65 - len(KINDS)


def launch(sim, obs=None, win=None, W=1, alpha=0.925, pulse=None, pad=0, expect=0):
    """The C entry on a [R, N] host matrix laid out with ld = N + pad (the padding holds NaN) -> sig [W, 12, N] as numpy.
    The output lies support.GUARD doubles inside a buffer of support.SENTINEL with a spare window behind it; everything around what the
    call owns is checked to be as it was."""
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    R, N = sim.shape
    d_sim, ld = padded(sim, pad)
    d_obs, d_win, d_pulse = to_device(obs), to_device(win, np.int32), to_device(pulse)
    sig = Guarded(W * 12 * N, tail=12 * N)
    rc = L.smart_signatures_hip(N, R, d_sim.data_ptr(), ld, ptr(d_obs), ptr(d_win), W, float(alpha), ptr(d_pulse), sig.ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, (rc, L.smart_last_error().decode())
        assert sig.untouched()
        return L.smart_last_error().decode()
    _lib.check(rc)
    sig, intact = sig.read()
    assert intact
    return sig.reshape(W, 12, N)


def hold(got, want, what):
    """every gate of the module's docstring on one launch"""
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ': the pattern of NaN'
    assert same_values(got[:, EXACT], want[:, EXACT], any_nan=True), what + ': the columns that are bit-equal: ' + ', '.join(
        NAMES[c] for c in EXACT if not same_values(got[:, c], want[:, c], any_nan=True))
    compared = want[:, CLOSE][~np.isnan(want[:, CLOSE])]
    assert compared.size == 0 or np.all((compared == 0.0) | (np.abs(compared) > 1e-6)), what      # (change the seed)
    for c in CLOSE + [AC1]:
        g, w = got[:, c], want[:, c]
        ok = ~np.isnan(w)
        if not ok.any():
            continue
        err = float(np.max(np.abs(g[ok] - w[ok]) / (1.0 if c == AC1 else np.maximum(np.abs(w[ok]), 1e-12))))
        MARGINS.note(NAMES[c], err / GATE, what)
        assert err < GATE, '%s: %s off by %.3e' % (what, NAMES[c], err)


@pytest.fixture(scope='module', autouse=True)
def _print_the_margins():
    yield
    if not MARGINS and not STRESS_MARGINS:
        return
    text = ('largest error of this run against the statement, as a fraction of its gate (relative 1e-9 with |want| floored '
            'at 1e-12; AC1 absolute 1e-9): column, margin, the launch it was seen in\n' +
            '\n'.join('%-14s %-10.3g %s' % (name, MARGINS[name][0], MARGINS[name][1]) for name in NAMES if name in MARGINS) +
            '\n' + ', '.join(NAMES[c] for c in EXACT) + ': bit-equal\n'
            '\nthe stress family (tests/cases_signatures.py) against exact truth: the largest |got - truth| / bound, '
            'the bound derived there (0 = equal to the correctly rounded truth; a bound of 0 admits nothing else): column, '
            'margin, the launch it was seen in\n' +
            '\n'.join('%-14s %-10.3g %s' % (name, STRESS_MARGINS[name][0], STRESS_MARGINS[name][1])
                      for name in NAMES if name in STRESS_MARGINS) + '\n')
    MARGINS.publish(text, margins_dir(), 'signatures_margins.txt')


@pytest.mark.parametrize('R', sorted(SHAPES))
def test_signatures_are_the_statement(R):
    for n in SHAPES[R]:
        rng, obs, sim = data(1000 * R + n, R, n)
        for W, win in window_arrays(rng, R, None):
            for with_obs in (obs, None):
                pulse = thresholds(sim, with_obs, win, W)
                for alpha in (0.925, 0.5):
                    what = 'R=%d n=%d W=%d obs=%s alpha=%g' % (R, n, W, with_obs is not None, alpha)
                    want = statement(sim, with_obs, win, W, alpha, pulse)
                    got = launch(sim, with_obs, win, W, alpha, pulse, pad=3)
                    hold(got, want, what)
                    if W == 7 and R >= 7:               # r % 7: no pair anywhere
                        assert np.isnan(got[:, PAIR_COLUMNS]).all(), what
                        rows = np.ones(R, dtype=bool) if with_obs is None else ~np.isnan(with_obs)
                        seen = [w for w in range(7) if rows[w::7].any()]
                        assert not np.isnan(got[seen][:, [MEAN, BFI, PEAK]]).any(), what
                    if W == 16:
                        assert np.isnan(got[15, HIGH_COUNT:]).all(), what            # the NaN pair of thresholds
    # without thresholds the four pulse columns are NaN and the other eight are what they were
    bare = launch(sim, with_obs, win, W, alpha, None)
    assert np.isnan(bare[:, HIGH_COUNT:]).all() and bits_equal(bare[:, :HIGH_COUNT], got[:, :HIGH_COUNT])


@pytest.mark.parametrize('R', STRESS_R)
def test_the_stress_family_is_the_exact_truth_within_its_bounds(R):
    sim, obs, _, kinds = stress_case(R)
    _, _, filler = data(9000 + R, R, FILLER)
    matrix = np.concatenate([filler, sim], axis=1)                      # N = 65: the family in columns 35 .. 64
    assert matrix.shape == (R, 65)
    for W, win, pulse, want, bnd in stress_reference(R):
        what = 'stress R=%d W=%d' % (R, W)
        got = launch(matrix, obs, win, W, 0.925, pulse, pad=3)
        hold(got[:, :, :FILLER], statement(filler, obs, win, W, 0.925, pulse), what + ', the benign columns beside it')
        got = got[:, :, FILLER:]
        ratio = margins(got, want, bnd)
        for c, name in enumerate(NAMES):
            worst = np.unravel_index(np.argmax(ratio[:, c]), ratio[:, c].shape)
            print('%s %-14s %.3g (window %d, %s)' % (what, name, ratio[:, c][worst], worst[0], kinds[worst[1]]))
            STRESS_MARGINS.note(name, float(ratio[:, c][worst]), '%s window %d %s' % (what, worst[0], kinds[worst[1]]))
        assert np.array_equal(np.isnan(got), np.isnan(want)), what + ': the pattern of NaN'
        assert np.isnan(got[:, AC1][:, CONSTANT_KINDS]).all(), what + ': a constant list has a variance of exactly 0'
        assert np.all(ratio <= 1.0), '%s: %s' % (what, {NAMES[c]: float(ratio[:, c].max()) for c in range(12)
                                                        if ratio[:, c].max() > 1.0})


def test_both_kinds_of_run_occur_and_thresholds_are_strict():
    R, n = 501, 65
    rng, obs, sim = data(77, R, n)
    pulse = thresholds(sim, obs, None, 1)
    assert (sim == pulse[0, 0]).any() and (sim == pulse[0, 1]).any()     # window 0: two values of the matrix itself
    want = statement(sim, obs, None, 1, 0.925, pulse)
    assert (want[0, HIGH_COUNT] > 1).any() and (want[0, LOW_COUNT] > 1).any()
    assert np.nanmax(want[0, HIGH_DURATION]) > 1.0 and np.nanmax(want[0, LOW_DURATION]) > 1.0
    hold(launch(sim, obs, None, 1, 0.925, pulse), want, 'strict thresholds')
    # thresholds no value passes: no run and a NaN duration, on both sides
    none = np.array([[0.0, 1e6]])
    want = statement(sim, obs, None, 1, 0.925, none)
    got = launch(sim, obs, None, 1, 0.925, none)
    hold(got, want, 'no run')
    assert np.all(got[0, [LOW_COUNT, HIGH_COUNT]] == 0.0) and np.isnan(got[0, [LOW_DURATION, HIGH_DURATION]]).all()


def test_planted_columns():
    R, n, W = 501, 65, 3
    rng, obs, sim = data(5, R, n)
    win = (np.arange(R) * 2 // R).astype(np.int32)                      # 0 and 1 occur, window 2 never does
    valid = ~np.isnan(obs)
    sim[:, 0] = 2.5                                                     # constant
    sim[:, 1] = 0.125 * (1.0 + np.arange(R))                            # strictly rising
    sim[:, 2] = 0.0                                                     # all zero
    sim[:, 3] = rng.choice([0.0, -0.0], R)                              # ... of both signs
    first, second = np.flatnonzero(valid & (win == 0))[[3, 40]]
    sim[first, 4] = sim[second, 4] = 1000.0                             # a tie at the peak
    sim[np.flatnonzero(valid & (win == 1))[7], 5] = np.nan              # a NaN in a valid row of window 1
    sim[np.flatnonzero(valid & (win == 0))[9], 6] = np.inf              # an infinity in a valid row of window 0
    sim[np.flatnonzero(~valid), 7] = np.nan                             # NaN only in rows that are not valid
    sim[np.flatnonzero(valid & (win == 0))[::2], 8] = 1e308             # a sum that overflows
    pulse = thresholds(sim[:, 9:], obs, win, W)
    want = statement(sim, obs, win, W, 0.925, pulse)
    got = launch(sim, obs, win, W, 0.925, pulse, pad=5)
    hold(got, want, 'planted columns')
    assert np.isnan(got[2]).all()                                       # m == 0
    for w in (0, 1):
        assert np.isnan(got[w, [AC1, RLD, RECESSION], 0]).all() and got[w, FLASHINESS, 0] == 0.0 and got[w, BFI, 0] == 1.0
        assert np.isnan(got[w, [BFI, FLASHINESS], 2]).all() and got[w, MEAN, 2] == 0.0 and got[w, PEAK_ROW, 2] == want[w, PEAK_ROW, 2]
        assert np.isnan(got[w, [BFI, FLASHINESS], 3]).all() and got[w, PEAK, 3] == 0.0
    assert got[0, PEAK, 4] == 1000.0 and got[0, PEAK_ROW, 4] == float(first)        # the first row wins
    first8 = slice(0, PEAK_ROW + 1)                                     # (a column need not have a run of both kinds)
    assert np.isnan(got[1, :, 5]).all() and not np.isnan(got[0, first8, 5]).any()
    assert np.isnan(got[0, :, 6]).all() and not np.isnan(got[1, first8, 6]).any()
    assert np.isnan(got[0, :, 8]).all() and not np.isnan(got[1, first8, 8]).any()
    clean = sim.copy()
    clean[:, 7] = 1.0
    clean[valid, 7] = sim[valid, 7]
    assert not np.isnan(got[:2, first8, 7]).any()
    assert bits_equal(got[:, :, 7], launch(clean, obs, win, W, 0.925, pulse)[:, :, 7])       # nothing changes
    # one strictly rising stretch without gaps: one limb
    one = launch(sim[:, 1:2], None, None, 1, 0.925, None)
    assert one[0, RLD, 0] == 1.0 / (R - 1) and np.isnan(one[0, RECESSION, 0])


def test_two_launches_give_the_same_bits():
    R, n = 1025, 300
    rng, obs, sim = data(11, R, n)
    W, win = window_arrays(rng, R, None)[3]
    pulse = thresholds(sim, obs, win, W)
    first = launch(sim, obs, win, W, 0.925, pulse, pad=1)
    assert bits_equal(first, launch(sim, obs, win, W, 0.925, pulse, pad=1))
    assert bits_equal(first, launch(sim, obs, win, W, 0.925, pulse, pad=70))         # ... whatever the leading dimension


def test_the_observations_as_a_matrix_of_one_column():
    R = 1025
    rng, obs, sim = data(21, R, 1)
    for W, win in window_arrays(rng, R, None):
        pulse = thresholds(sim, obs, win, W)
        column = np.where(np.isnan(obs), -1.0, obs).reshape(R, 1)       # (a missing observation is never read as a flow)
        want = statement(column, obs, win, W, 0.925, pulse)
        hold(launch(obs.reshape(R, 1), obs, win, W, 0.925, pulse), want, 'observations W=%d' % W)


def test_an_error_return_leaves_the_buffer_untouched():
    R, n = 9, 5
    rng, obs, sim = data(3, R, n)
    win = (np.arange(R) % 2).astype(np.int32)
    assert 'alpha' in launch(sim, obs, win, 2, 1.0, None, expect=E_SIZE)
    assert 'n_windows' in launch(sim, obs, None, 2, 0.5, None, expect=E_SIZE)
    from smartpy_amd import engine
    assert 'n_windows' in launch(sim, obs, win, engine.objfn_max_windows() + 1, 0.5, None, expect=E_SIZE)


def test_engine_surface():
    import torch
    from smartpy_amd import engine
    R, n = 501, 130
    rng, obs, sim = data(41, R, n)
    ids = (np.arange(R) % 3 == 0).astype(np.int32) + (np.arange(R) >= 250)       # 0, 1, 2 in stretches; window 3 never
    pulse = thresholds(sim, obs, ids, 4)
    want = statement(sim, obs, ids, 4, 0.5, pulse)
    wide = torch.full((R, n + 63), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :n] = torch.from_numpy(sim).cuda()
    got = engine.signatures(wide[:, :n], torch.from_numpy(obs).cuda(), torch.from_numpy(ids).cuda(), n_windows=4,
                            alpha=0.5, thresholds=pulse)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (4, 12, n) and got[1, 3].is_contiguous()
    hold(got.cpu().numpy(), want, 'engine, strided view')
    assert np.isnan(want[3]).all()
    bare = engine.signatures(sim)                                        # host matrix, nothing else
    hold(bare.cpu().numpy(), statement(sim), 'engine, defaults')
    on_device = engine.signatures(sim, obs, thresholds=torch.from_numpy(pulse[:1]).cuda())
    hold(on_device.cpu().numpy(), statement(sim, obs, None, 1, 0.925, pulse[:1]), 'engine, thresholds on the device')
    empty = engine.signatures(torch.empty((R, 0), dtype=torch.float64, device='cuda'), obs)
    assert tuple(empty.shape) == (1, 12, 0)
    with pytest.raises(engine.SmartEngineError, match='1 of the 501 window ids'):
        bad = torch.from_numpy(ids).cuda()
        bad[17] = 4
        engine.signatures(sim, obs, bad, n_windows=4)


def test_through_the_model(tmp_path):
    from smartpy_amd.montecarlo import LHS
    from smartpy_amd.montecarlo.selection import as_stored, pareto_rows
    from smartpy_amd.windows import evaluation_windows, pulse_thresholds, signatures_header_line
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.sampling.sttngs', '01/01/2007', '31/12/2007', 180)
    np.random.seed(2025)
    n = 130
    lhs = LHS('Catchment', root, 'csv', 'csv', sample_size=n, settings_filename='Catchment.sampling.sttngs')
    lhs.model.extra = EXTRA
    lhs.run()
    obs = np.asarray(lhs.model.nd_flow, dtype=np.float64)
    sim = lhs.model.simulate_ensemble(lhs._sample, save_discharge=True, math_mode=lhs.math_mode).discharge.cpu().numpy().T
    ids, labels = evaluation_windows(lhs.model.timeseries_report[1:], by='hydro_year')
    assert labels == ['2007', '2008']
    res = lhs.hydrological_signatures(windows='hydro_year', write=True)
    pulse = pulse_thresholds(obs, ids, 2)
    assert res.names == NAMES and res.labels == labels and res.alpha == 0.925 and res.device_values.is_cuda
    assert np.array_equal(res.thresholds, pulse) and not np.isnan(pulse).any()
    assert res.values.shape == (2, 12, n) and res.observed.shape == (2, 12)
    want = statement(sim, obs, ids, 2, 0.925, pulse)
    hold(res.values, want, 'hydrological years through the model')
    assert bits_equal(res.values, res.device_values.cpu().numpy())
    column = np.where(np.isnan(obs), -1.0, obs).reshape(-1, 1)
    hold(res.observed[:, :, None], statement(column, obs, ids, 2, 0.925, pulse), 'the observations through the model')
    assert np.array_equal(res.relative_error(), (res.values - res.observed[:, :, None]) / np.abs(res.observed[:, :, None]),
                          equal_nan=True)
    # a column of device_values goes to the Pareto selection as it is
    bfi, flash = res.device_values[0, BFI], res.device_values[0, FLASHINESS]
    assert bfi.is_contiguous() and tuple(bfi.shape) == (n,)
    rows, ranks = pareto_rows(np.stack([res.values[0, BFI], res.values[0, FLASHINESS]], axis=1),
                              [('target', float(res.observed[0, BFI])), ('target', float(res.observed[0, FLASHINESS]))])
    import torch
    on_rows, on_ranks = pareto_rows(torch.stack([bfi, flash], dim=1),
                                    [('target', float(res.observed[0, BFI])), ('target', float(res.observed[0, FLASHINESS]))])
    assert np.array_equal(on_rows.cpu().numpy(), rows) and np.array_equal(on_ranks.cpu().numpy(), ranks) and len(rows) >= 1
    # the file: the rows a sampling database would have kept
    assert res.path == lhs.signatures_file and \
        os.path.normpath(res.path) == os.path.join(root, 'out', 'Catchment', 'Catchment.SMART.lhs.signatures')
    lines = open(res.path).read().split('\n')
    assert len(lines) == n + 2 and lines[-1] == '' and lines[0] + '\n' == signatures_header_line(labels)
    back = np.array([[float(v) for v in line.split(',')] for line in lines[1:-1]], dtype=np.float32)
    assert np.array_equal(back, as_stored(res.values.transpose(2, 0, 1).reshape(n, 24)), equal_nan=True)
    # thresholds of the caller's, another alpha, one window, no file
    mine = np.array([[0.5, 2.0]])
    one = lhs.hydrological_signatures(alpha=0.5, thresholds=mine)
    assert one.path is None and one.labels == ['all'] and one.alpha == 0.5 and np.array_equal(one.thresholds, mine)
    hold(one.values, statement(sim, obs, None, 1, 0.5, mine), 'one window through the model')
