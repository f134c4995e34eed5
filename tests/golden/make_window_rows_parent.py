"""The four windowed analyses of a stored discharge matrix on the cases of tests/test_gpu_window_rows.py, bit for bit, as the
PARENT commit's library computes them -> tests/golden/window_rows_parent.npz.  Needs an MI355X; run once, with the parent's
library selected:

    bash tools/build_rev_variant.sh <parent rev> parent
    SMART_AMD_LIB=$PWD/tools/variants/libsmart_amd_parent.so python tests/golden/make_window_rows_parent.py [out.npz]

The change the fixture was made for folded four copies of "list the valid rows of window w in row order" (the LDS
compaction of smart_objfn_windows, smart_bootstrap_moments, smart_signatures and the two sort-form kernels of
smart_flow_duration) into one, csrc/smart_window_rows.h, and the walk over that list and the reduction of the partial
moments of the first two with it.  No arithmetic and no order of summation changed: every kernel has to give the parent's
bits.  The cases and how a case is run live here, so that the test runs exactly what the fixture recorded.

Shapes.  All four units look at window[] / obs[] in chunks of 1,024 rows, so R = 1, 2, 1023, 1024, 1025 and 2049 (no
chunk boundary, the boundary exactly, one row past it, two boundaries) at N = 65 (a full wavefront and one live lane); N = 1
and N = 257 at R = 1025 (a smart_signatures workgroup spans 256 samples).  Window arrays: one window; r % 3 (every
sub-chunk of every chunk adds to every list); two blocks, window 1 wholly beyond row 1024; a window whose only rows are 1023
and 1024, one on each side of the boundary (both observed); four blocks with about 10 % of the ids -1.  Observations: about
15 % missing -- and, where R > 1024, once more with every observation of rows 0 .. 1023 missing, so that the first chunk
lists nothing and the first listed row (the shift of the one-pass moments) is found in a later chunk.

Kept per output array: the bits of the sample columns 0, 1, 63 and N - 1, and a sha256 of the whole array -- the row list is
shared by all samples of a workgroup, so a wrong list shows in every column.

AC1 was later re-centred (its one-pass moments about a member of each pair list): the two `signatures` arrays keep the
parent's bits in the eleven other columns only.  `--extend` adds, for those two arrays, the kept-column bits and the
sha256 of the array WITHOUT its AC1 column under the name `<name>|but_ac1`, made by the library of the commit before
that change -- after asserting that this library reproduces the full-array sha256 the fixture already holds -- and
leaves every other key of the fixture as it is:

    SMART_AMD_LIB=$PWD/tools/variants/libsmart_amd_parent.so python tests/golden/make_window_rows_parent.py --extend [out.npz]
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'window_rows_parent.npz')
CHUNK = 1024
SHAPES = [(1, 65), (2, 65), (1023, 65), (1024, 65), (1025, 65), (2049, 65), (1025, 1), (1025, 257)]
WINDOW_KINDS = ('one', 'mod3', 'blocks', 'pair', 'minus')
LOG_EPS = 0.05
PROBS_BOOTSTRAP = (0.05, 0.5, 0.95)
PROBS_CURVE = (0.1, 0.5, 1.0)
SIGNATURE_ARRAYS = ('signatures', 'signatures_thresholds')      # [W, 12, N]
AC1 = 3
BUT_AC1 = '|but_ac1'


def obs_kinds(R):
    return ('some', 'late') if R > CHUNK else ('some',)


def inputs(R, N, window_kind, obs_kind):
    """-> (sim [R, N], obs [R], window ids [R] int32, W)"""
    rng = np.random.default_rng(1000 * R + N)
    obs = np.abs(rng.normal(3.0, 1.5, R))
    obs[rng.random(R) < 0.15] = np.nan
    sim = rng.random((R, N)) * 6 + 0.01
    minus = rng.random(R) < 0.10
    if obs_kind == 'late':
        obs[:CHUNK] = np.nan
    if R > CHUNK:
        obs[CHUNK] = 3.25       # the first row of the second chunk is always observed
    r = np.arange(R)
    if window_kind == 'one':
        win, W = np.zeros(R), 1
    elif window_kind == 'mod3':
        win, W = r % 3, 3
    elif window_kind == 'blocks':
        win, W = r >= CHUNK, 2
    elif window_kind == 'pair':
        win, W = (r == CHUNK - 1) | (r == CHUNK), 2
        obs[CHUNK - 1:CHUNK + 1] = (2.5, 3.5)[:max(0, min(2, R - CHUNK + 1))]
    else:
        win, W = r * 4 // R, 4
        win[minus] = -1
    return sim, obs, np.ascontiguousarray(win, dtype=np.int32), W


def counts(W):
    """five replicates: every window once (the point value's bits), one window left out, and three mixed rows"""
    w = np.arange(W)
    c = np.stack([np.ones(W), np.ones(W), w % 3, np.full(W, 2), w + 1]).astype(np.uint16)
    c[1, W - 1] = 0
    return c


def run_signatures(eng, R, N, window_kind, obs_kind):
    """the two signature launches of a case -> {name: (device array, the axis of it that runs over the samples)}"""
    sim, obs, win, W = inputs(R, N, window_kind, obs_kind)
    return {'signatures': (eng.signatures(sim, obs, win, n_windows=W), 2),
            'signatures_thresholds': (eng.signatures(sim, obs, win, n_windows=W, thresholds=np.tile((1.5, 4.5), (W, 1))), 2)}


def but_ac1(a):
    """[W, 12, N] -> [W, 11, N]: the array without its AC1 column"""
    assert a.shape[1] == 12
    return np.ascontiguousarray(np.delete(a, AC1, axis=1))


def run_case(eng, R, N, window_kind, obs_kind):
    """every entry on one case -> {name: (numpy array, the axis of it that runs over the samples)}"""
    sim, obs, win, W = inputs(R, N, window_kind, obs_kind)
    got = {}
    for transform, eps in (('none', 0.0), ('log', LOG_EPS)):
        got['windows_' + transform] = (eng.objective_functions_windows(sim, obs, win, n_windows=W, transform=transform,
                                                                       eps=eps), 1)
    b = eng.objective_functions_bootstrap(sim, obs, win, counts(W), probs=PROBS_BOOTSTRAP, n_windows=W, replicates=True)
    got.update(bootstrap_point=(b.point, 0), bootstrap_stats=(b.stats, 2), bootstrap_replicates=(b.replicates, 2))
    got.update(run_signatures(eng, R, N, window_kind, obs_kind))
    quant, scores = eng.flow_duration(sim, PROBS_CURVE, obs=obs, windows=win, n_windows=W, transform='sqrt', objfn=True,
                                      method='sort')
    got.update(curve_quant=(quant, 2), curve_objfn=(scores, 1))
    return {k: (np.ascontiguousarray(a.cpu().numpy(), dtype=np.float64), axis) for k, (a, axis) in got.items()}


def columns(N):
    return sorted({0, min(1, N - 1), min(63, N - 1), N - 1})


def kept(a, axis, N):
    """what the fixture holds of an output array -> (the bits of columns(N) as int64, sha256 of shape and bytes)"""
    assert a.shape[axis] == N
    bits = np.ascontiguousarray(np.take(a, columns(N), axis=axis)).view(np.int64)
    return bits, hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()


def key(R, N, window_kind, obs_kind, name):
    return 'R%d|N%d|%s|%s|%s' % (R, N, window_kind, obs_kind, name)


def load_fixture(path=FIXTURE):
    """{key: (bits of the kept columns, flat, sha256 of the whole array)}"""
    z = np.load(path, allow_pickle=False)
    bits, ends = z['bits'], z['ends']
    return {k.decode(): (bits[lo:hi], h.decode())
            for k, h, lo, hi in zip(z['keys'], z['sha256'], np.concatenate([[0], ends[:-1]]), ends)}


def main(path):
    import torch
    from smartpy_amd import _lib, engine
    assert torch.cuda.is_available(), 'the fixture is made on the GPU'
    print('library:', _lib.LIB_PATH)
    keys, hashes, bits = [], [], []
    for R, N in SHAPES:
        for window_kind in WINDOW_KINDS:
            for obs_kind in obs_kinds(R):
                for name, (a, axis) in run_case(engine, R, N, window_kind, obs_kind).items():
                    b, h = kept(a, axis, N)
                    keys.append(key(R, N, window_kind, obs_kind, name))
                    hashes.append(h)
                    bits.append(b.ravel())
    np.savez_compressed(path, keys=np.array(keys, dtype='S'), sha256=np.array(hashes, dtype='S'), bits=np.concatenate(bits),
                        ends=np.cumsum([len(b) for b in bits]))
    print('%d arrays, %d bytes -> %s' % (len(keys), os.path.getsize(path), path))


def extend(path):
    """add the `|but_ac1` entries of the two signature arrays, made by the selected (parent) library, to the fixture"""
    import torch
    from smartpy_amd import _lib, engine
    assert torch.cuda.is_available(), 'the fixture is made on the GPU'
    print('library:', _lib.LIB_PATH)
    z = np.load(FIXTURE, allow_pickle=False)
    old_ends = np.concatenate([[0], z['ends']])
    keys, hashes, bits = [], [], []
    for i, k in enumerate(z['keys']):
        if not k.decode().endswith(BUT_AC1):
            keys.append(k.decode())
            hashes.append(z['sha256'][i].decode())
            bits.append(z['bits'][old_ends[i]:old_ends[i + 1]])
    held = dict(zip(keys, hashes))
    n_old = len(keys)
    for R, N in SHAPES:
        for window_kind in WINDOW_KINDS:
            for obs_kind in obs_kinds(R):
                for name, (a, axis) in run_signatures(engine, R, N, window_kind, obs_kind).items():
                    a = np.ascontiguousarray(a.cpu().numpy(), dtype=np.float64)
                    k = key(R, N, window_kind, obs_kind, name)
                    assert kept(a, axis, N)[1] == held[k], 'this library is not the one the fixture was made by: ' + k
                    b, h = kept(but_ac1(a), axis, N)
                    keys.append(k + BUT_AC1)
                    hashes.append(h)
                    bits.append(b.ravel())
    np.savez_compressed(path, keys=np.array(keys, dtype='S'), sha256=np.array(hashes, dtype='S'), bits=np.concatenate(bits),
                        ends=np.cumsum([len(b) for b in bits]))
    print('%d arrays kept, %d added, %d bytes -> %s' % (n_old, len(keys) - n_old, os.path.getsize(path), path))


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--extend']
    (extend if '--extend' in sys.argv[1:] else main)(args[0] if args else FIXTURE)
