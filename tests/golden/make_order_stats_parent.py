"""The order-statistics entries along the sample axis -- weighted quantiles, ensemble scores, DYNIA, and one bootstrap
case -- on the cases of tests/test_gpu_order_stats.py, bit for bit, as the PARENT commit's library computes them
-> tests/golden/order_stats_parent.npz.  Needs an MI355X; run once, with the parent's library selected:

    bash tools/build_rev_variant.sh <parent rev> parent
    SMART_AMD_LIB=$PWD/tools/variants/libsmart_amd_parent.so python tests/golden/make_order_stats_parent.py [out.npz]

The change the fixture was made for gave smart_quantiles_sort and the ensemble kernels one definition of the bitonic
network in LDS and one of the weight scan (csrc/smart_order_stats.h).  No comparator, no order of summation and no launch
geometry changed: every kernel has to give the parent's bits.  The cases and how a case is run live here, so that the test
runs exactly what the fixture recorded.

Inputs.  R = 3 report steps in a matrix with ld = N + 3 (the padding holds NaN).  Step 0 is random; step 1 is drawn from
seven distinct values, so that ties make the payload permutation of the network matter (the scan sees equal keys in the
network's order, each with its own weight); step 2 has NaN, +-inf and +-0.0 sprinkled in.  Weights: none, random, and
random with a third of them zero.

Sizes, where the shared code changes behaviour: the thread count and the capacity of every (CAP, THREADS) instance and one
past each (QUANTILE_SIZES); the four ways the long stages of the global ensemble form run (no long stage, one lone, one fused
pair, a fused pair and a lone one: GLOBAL_SIZES pad to 4096, 8192, 16384, 32768); the wavefront, the workgroup and both LDS
capacities of smart_dynia_shares (DYNIA_SIZES, the SIZES of tests/test_gpu_dynia.py).

The select form of the quantiles, DYNIA and the bootstrap case (objective_functions_bootstrap, 5 replicates: its quantiles
are the flow-duration sort form, launch_flow_duration, not smart_quantiles_sort) run none of the shared code.  They are
recorded and compared all the same.

Before anything is recorded, check_inputs() verifies on the CPU, with numpy alone, that every case has at least one finite
value per step (of positive weight where there are weights; a finite window sum per step for DYNIA): otherwise a case
would compare only NaN with NaN.

Kept per output array: all its bits as int64, and a sha256 of shape and bytes.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'order_stats_parent.npz')
R = 3
PAD = 3
QUANTILE_SIZES = [1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192]
SORT_CAPACITY = 8192                # smart_quantiles.hip: kSortCapacity; smart_ensemble_scores.hip: kEnsCapacity
SELECT_ONLY = [8193]
GLOBAL_SIZES = [1, 4096, 4097, 8193, 16385]
DYNIA_SIZES = [1, 2, 63, 64, 65, 257, 1000, 2048, 2049, 16384, 16385, 20000]
DYNIA_FRACTIONS = (0.1, 1.0)
DYNIA_SUPPORTS = ('equal', 'linear')
DYNIA_HALF_WIDTH = 1
WEIGHT_KINDS = ('none', 'random', 'zero')
PROBS = {1: (0.5,), 5: (0.05, 0.25, 0.5, 0.75, 1.0), 16: tuple((np.arange(16) + 1) / 16.0)}
SEVEN = (0.125, 0.5, 1.75, 2.0, 3.25, 4.5, 7.0)
SPECIALS = (np.nan, np.inf, -np.inf, 0.0, -0.0)
BOOTSTRAP_SHAPE = (40, 65, 4)       # R, N, windows
BOOTSTRAP_PROBS = (0.05, 0.5, 0.95)

# (entry, N): one group of launches, one test case
GROUPS = ([('quantiles', N) for N in QUANTILE_SIZES + SELECT_ONLY] + [('ensemble_lds', N) for N in QUANTILE_SIZES] +
          [('ensemble_global', N) for N in GLOBAL_SIZES] + [('dynia', N) for N in DYNIA_SIZES] + [('bootstrap', 65)])


def matrix(N):
    """-> sim [R, N + PAD] float64, the padding NaN: the three steps of the docstring"""
    rng = np.random.default_rng(7000 + N)
    sim = np.full((R, N + PAD), np.nan)
    sim[0, :N] = np.exp(rng.normal(0.0, 1.5, N))
    sim[1, :N] = np.asarray(SEVEN)[rng.integers(0, 7, N)]
    sim[2, :N] = rng.normal(0.0, 3.0, N)
    if N >= 2:      # (position 0 stays as it is: a finite value in every step)
        at = 1 + rng.choice(N - 1, size=max(1, (N - 1) // 8), replace=False)
        sim[2, at] = np.asarray(SPECIALS)[np.arange(len(at)) % len(SPECIALS)]
    return sim


def weights(N, kind):
    if kind == 'none':
        return None
    rng = np.random.default_rng(8000 + N)
    w = rng.random(N) + 0.01
    if kind == 'zero':
        w[1 + rng.choice(max(N - 1, 1), size=N // 3, replace=False)] = 0.0     # (position 0 stays live)
    return w


def observations(N):
    """[R], one NaN, its step by N"""
    obs = np.asarray((1.5, 2.0, 0.25))
    obs[N % R] = np.nan
    return obs


def dynia_inputs(N):
    """-> (obs [R], categories [P, N] uint8, bins)"""
    rng = np.random.default_rng(9000 + N)
    P, B = (16, 64) if N in (65, 16385) else (5, 7)
    cat = rng.integers(0, B, size=(P, N)).astype(np.uint8)
    cat[1, ::17] = 255
    return np.asarray((1.5, 2.0, 0.25)), cat, B


def bootstrap_inputs():
    Rb, N, W = BOOTSTRAP_SHAPE
    rng = np.random.default_rng(77)
    obs = np.abs(rng.normal(3.0, 1.5, Rb))
    obs[rng.random(Rb) < 0.15] = np.nan
    sim = rng.random((Rb, N)) * 6 + 0.01
    win = np.ascontiguousarray(np.arange(Rb) * W // Rb, dtype=np.int32)
    w = np.arange(W)
    counts = np.stack([np.ones(W), np.ones(W), w % 3, np.full(W, 2), w + 1]).astype(np.uint16)      # 5 replicates
    counts[1, W - 1] = 0
    return sim, obs, win, W, counts


def check_inputs():
    """numpy alone: every case has at least one finite (and, with weights, live) value per step"""
    for entry, N in GROUPS:
        if entry == 'bootstrap':
            sim, obs, win, W, counts = bootstrap_inputs()
            assert all((np.isfinite(obs) & (win == w)).sum() >= 2 for w in range(W)) and np.isfinite(sim).all()
            continue
        sim = matrix(N)[:, :N]
        assert sim.shape == (R, N) and len({x for x in sim[1]}) <= 7
        if entry == 'dynia':
            obs = dynia_inputs(N)[0]
            E = np.abs(sim - obs[:, None])
            h = DYNIA_HALF_WIDTH
            for r in range(R):
                assert np.isfinite(E[max(0, r - h):r + h + 1].sum(axis=0)).any(), (entry, N, r)
            continue
        for kind in WEIGHT_KINDS:
            w = weights(N, kind)
            live = np.ones(N, dtype=bool) if w is None else w > 0
            assert kind != 'zero' or (~live).sum() == N // 3
            for r in range(R):
                assert (np.isfinite(sim[r]) & live).any(), (entry, N, kind, r)
        if entry != 'quantiles':
            assert np.isnan(observations(N)).sum() == 1


def _device_matrix(N):
    import torch
    return torch.from_numpy(matrix(N)).cuda()[:, :N]      # (a view: the stride from step to step is N + PAD)


def run_group(eng, entry, N):
    """every launch of one group -> {name: numpy array}"""
    got = {}
    if entry == 'bootstrap':
        sim, obs, win, W, counts = bootstrap_inputs()
        b = eng.objective_functions_bootstrap(sim, obs, win, counts, probs=BOOTSTRAP_PROBS, n_windows=W, replicates=True)
        got.update(point=b.point, stats=b.stats, replicates=b.replicates)
    elif entry == 'quantiles':
        sim = _device_matrix(N)
        for method in ('sort', 'select'):
            if method == 'sort' and N > SORT_CAPACITY:
                continue
            for K, probs in PROBS.items():
                for kind in WEIGHT_KINDS:
                    got['%s|K%d|%s' % (method, K, kind)] = eng.weighted_quantiles(sim, probs, weights(N, kind), method=method)
    elif entry in ('ensemble_lds', 'ensemble_global'):
        sim = _device_matrix(N)
        for kind in WEIGHT_KINDS:
            got[kind] = eng.ensemble_scores(sim, observations(N), weights(N, kind), method=entry.split('_')[1])
    else:
        sim = _device_matrix(N)
        obs, cat, B = dynia_inputs(N)
        for support in DYNIA_SUPPORTS:
            for fraction in DYNIA_FRACTIONS:
                d = eng.dynamic_identifiability(sim, obs, cat, B, DYNIA_HALF_WIDTH, fraction=fraction, support=support)
                for name in ('shares', 'cut', 'retained', 'count'):
                    got['%s|%g|%s' % (support, fraction, name)] = getattr(d, name)
    return {k: np.ascontiguousarray(a.cpu().numpy()) for k, a in got.items()}


def kept(a):
    """what the fixture holds of an output array -> (its bits as int64, flat; sha256 of shape, type and bytes)"""
    bits = a.view(np.int64) if a.dtype.itemsize == 8 else a.astype(np.int64)
    return bits.ravel(), hashlib.sha256((repr(a.shape) + str(a.dtype)).encode() + a.tobytes()).hexdigest()


def key(entry, N, name):
    return '%s|N%d|%s' % (entry, N, name)


def load_fixture(path=FIXTURE):
    """{key: (the array's bits as flat int64, sha256 of the whole array)}"""
    z = np.load(path, allow_pickle=False)
    bits, ends = z['bits'], z['ends']
    return {k.decode(): (bits[lo:hi], h.decode())
            for k, h, lo, hi in zip(z['keys'], z['sha256'], np.concatenate([[0], ends[:-1]]), ends)}


def main(path):
    import torch
    from smartpy_amd import _lib, engine
    assert torch.cuda.is_available(), 'the fixture is made on the GPU'
    check_inputs()
    print('library:', _lib.LIB_PATH)
    keys, hashes, bits = [], [], []
    for entry, N in GROUPS:
        for name, a in run_group(engine, entry, N).items():
            b, h = kept(a)
            keys.append(key(entry, N, name))
            hashes.append(h)
            bits.append(b)
    np.savez_compressed(path, keys=np.array(keys, dtype='S'), sha256=np.array(hashes, dtype='S'), bits=np.concatenate(bits),
                        ends=np.cumsum([len(b) for b in bits]))
    print('%d arrays, %d values, %d bytes -> %s' % (len(keys), sum(len(b) for b in bits), os.path.getsize(path), path))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
