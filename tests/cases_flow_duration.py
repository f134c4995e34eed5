"""The cases of the flow-duration truth tests (tests/test_flow_duration_truth_host.py holds them to its conditions,
tests/test_gpu_flow_duration_truth.py launches them), and the launch the two GPU files of the analysis share.  A plain
module: pytest does not collect it."""
import functools
import zlib

import numpy as np

from cases_objfn import EPS, INVERSE_DECADES, stress
from oracle.analyses.flow_duration import curve_reference, segment_ranks
from oracle.analyses.windows import TRANSFORMS as TRANSFORM_CODES
from support import Guarded, padded, ptr, to_device, workspace

CAPACITY = 16384                        # smart_flow_duration_sort_capacity(): the longest column the sort form takes
METHODS = {'auto': 0, 'sort': 1, 'select': 2}
TRANSFORMS = ('none', 'sqrt', 'log', 'inverse')
SEGMENTS = ((0.0, 1.0), (0.98, 1.0), (0.0, 0.3), (0.3, 0.7))
# R -> (the instance of smart_fdc_sort it runs, N: the last workgroup of that instance's COLS is partial)
INSTANCES = {501: ('1024 x 16', 17), 1025: ('2048 x 8', 15), 2049: ('4096 x 4', 5), 4097: ('8192 x 2', 3),
             16384: ('16384 x 1', 3)}
BIG_TRANSFORMS = ('sqrt', 'inverse')    # R = 16,384 is held to truth under two transforms (its three columns all are)


# ---- the windows -------------------------------------------------------------------------------------------------------
UNEVEN = (0.0, 0.05, 0.15, 0.30, 0.50, 0.62, 0.87, 1.0)     # where the seven windows of 'uneven' begin, as shares of R
EMPTY = 4                                                   # the window of 'uneven' whose observations are all missing


def window_array(R, windows):
    """-> (W, win or None).  'none': no array, one window of every row.  'uneven': seven windows of consecutive rows of
    5, 10, 15, 20, 12, 25 and 13 % of R, every 17th row in no window."""
    if windows == 'none':
        return 1, None
    assert windows == 'uneven', 'windows %r unknown' % (windows,)
    win = np.searchsorted(np.asarray(UNEVEN[1:]) * R, np.arange(R), side='right').astype(np.int32)
    win[16::17] = -1
    return 7, win


# ---- the two families --------------------------------------------------------------------------------------------------
def curves(seed, R, n, transform):
    """-> (sim [R, n], obs [R]): stress(seed, R, n, 0) as it is (under 'inverse': its means from INVERSE_DECADES)"""
    sim, obs, _ = stress(seed, R, n, 0, decades=INVERSE_DECADES if transform == 'inverse' else (-2.0, 4.0))
    return sim, obs


def plateau(seed, R, n, win, W, transform, segment):
    """-> (sim [R, n], obs [R]); 15 % of the observations are missing, a row outside every window holds 1e3 times the
    column's scale.
    A family on which a constant from outside the segment shows: inside the segment of its window a column holds scale
    (1 + rel U(0, 1)), scale = 10^U(-2, 4), rel = 10^U(-6, -3); the ranks below i0 lie at scale 10^U(-4, -1) and the
    ranks from i1 on at scale (2 + U(0, 1)); the rows are shuffled.  The moments about rank 0 of the window have kappa
    of (1 / rel)^2 and more.  The observations are a plateau of their own, 1 + 3e-3 U(0, 1) inside the segment,
    10^U(-3, -1) below and 2 + U(0, 1) above it: a spread of the order of the columns' keeps KGEa = std f(s) / std f(e)
    above SMALL (against observations that span decades a sixth of the columns would fall below it).  Built per window
    and per segment."""
    rng = np.random.default_rng(seed)
    lo, hi = INVERSE_DECADES if transform == 'inverse' else (-2.0, 4.0)
    scale = 10.0 ** rng.uniform(lo, hi, n)
    rel = 10.0 ** rng.uniform(-6.0, -3.0, n)
    obs = np.full(R, np.nan)
    sim = np.tile(1e3 * scale, (R, 1))
    seen = rng.random(R) >= 0.15
    for w in range(W):
        rows = np.flatnonzero(seen if win is None else seen & (win == w))
        m = rows.size
        i0, i1 = segment_ranks(m, segment)
        rows = rng.permutation(rows)
        below, inside, above = rows[:i0], rows[i0:i1], rows[i1:]
        sim[below] = scale * 10.0 ** rng.uniform(-4.0, -1.0, (below.size, n))
        sim[inside] = scale * (1.0 + rel * rng.random((inside.size, n)))
        sim[above] = scale * (2.0 + rng.random((above.size, n)))
        obs[below] = 10.0 ** rng.uniform(-3.0, -1.0, below.size)
        obs[inside] = 1.0 + 3e-3 * rng.random(inside.size)
        obs[above] = 2.0 + rng.random(above.size)
    return sim, obs


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _cases():
    """(R, N, W, windows, transform, segment, family): every R under every transform (R = 16,384 under two) and family,
    once as one window without an array and once as the seven uneven ones.  `curves` walks the four segments so that every
    (R, W) and every (transform, W) meets each of them; `plateau` takes the two with i0 > 0."""
    out = []
    for ri, (R, (_, N)) in enumerate(sorted(INSTANCES.items())):
        for ti, transform in enumerate(TRANSFORMS):
            if R == 16384 and transform not in BIG_TRANSFORMS:
                continue
            for wi, (W, windows) in enumerate(((1, 'none'), (7, 'uneven'))):
                out.append((R, N, W, windows, transform, SEGMENTS[(ri + ti + 2 * wi) % 4], 'curves'))
                # (of seven windows of 501 rows none keeps two ranks of the top 2 %)
                top = (R, W) != (501, 7) and (ti + wi) % 2 == 0
                out.append((R, N, W, windows, transform, SEGMENTS[1 if top else 3], 'plateau'))
    return out


CASES = _cases()
RESEEDED = {}                           # case -> another seed, where the first broke a condition


def case_id(case):
    R, N, W, windows, transform, segment, family = case
    return '%d-%d-W%d-%s-%g_%g-%s' % (R, N, W, transform, segment[0], segment[1], family)


def case_seed(case):
    return RESEEDED.get(case, zlib.crc32(case_id(case).encode()))


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> (sim [R, N], obs [R], win [R] or None, eps); in 'uneven' window EMPTY has no observation"""
    R, N, W, windows, transform, segment, family = case
    _, win = window_array(R, windows)
    if family == 'curves':
        sim, obs = curves(case_seed(case), R, N, transform)
    else:
        sim, obs = plateau(case_seed(case), R, N, win, W, transform, segment)
    if win is not None:
        obs[win == EMPTY] = np.nan
    for a in (sim, obs):
        a.setflags(write=False)
    return sim, obs, win, EPS[transform]


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """-> (want, bnd) [W, N, 7] of the case, computed once and shared"""
    R, N, W, windows, transform, segment, family = case
    sim, obs, win, eps = case_data(case)
    want, bnd = curve_reference(sim, obs, win, W, transform, eps, segment)
    for a in (want, bnd):
        a.setflags(write=False)
    return want, bnd


def launch(sim, probs, obs=None, win=None, W=1, transform='none', eps=0.0, segment=(0.0, 1.0), objfn=False, method='auto',
           pad=0, expect=0):
    """The C entry on a [R, N] host matrix laid out with ld = N + pad (the padding holds NaN) -> (quant [W, K, N], objfn
    [W, N, 7] or None) as numpy.  Both outputs lie support.GUARD doubles inside a buffer of support.SENTINEL with a spare window behind
    them; everything around what the call owns is checked to be as it was."""
    import ctypes
    import torch
    from smartpy_amd import _lib
    L = _lib.lib()
    R, N = sim.shape
    K = len(probs)
    d_sim, ld = padded(sim, pad)
    d_obs, d_win = to_device(obs), to_device(win, np.int32)
    q = np.ascontiguousarray(probs, dtype=np.float64)
    quant = Guarded(W * K * N, tail=K * N)
    own = W * N * 7 if objfn else 0                                     # (not asked for: the whole buffer stays as it was)
    scores = Guarded(own, tail=(W + 1) * N * 7 - own)
    need = L.smart_flow_duration_workspace_bytes(R, W, 1 if objfn else 0)
    work = workspace(need, least=8, fill=0) if objfn else None
    rc = L.smart_flow_duration_hip(N, R, d_sim.data_ptr(), ld, ptr(d_obs), ptr(d_win), W,
                                   q.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), K, quant.ptr(),
                                   TRANSFORM_CODES[transform], float(eps), float(segment[0]), float(segment[1]),
                                   scores.ptr(null=not objfn), ptr(work), need if objfn else 0, METHODS[method],
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, 'returned %d (%s), expected %d' % (rc, L.smart_last_error().decode(), expect)
        assert quant.untouched() and scores.untouched(), 'a refused call wrote to its outputs'
        return L.smart_last_error().decode()
    _lib.check(rc)
    (quant, ok_q), (scores, ok_s) = quant.read(), scores.read()
    assert ok_q and ok_s, 'the call wrote outside what it owns (quantiles intact: %s, scores intact: %s)' % (ok_q, ok_s)
    return quant.reshape(W, K, N), scores.reshape(W, N, 7) if objfn else None
