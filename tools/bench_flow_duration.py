#!/usr/bin/env python3
"""Time of the flow duration curves (smart_flow_duration: order statistics along time of a stored [R][N] matrix, per
sample and window) -- the sort form with and without the objective functions of the curve and the select form -- beside
two yardsticks measured in the same run on the same matrix: smart_objfn_hip (the cost of reading the matrix once) and
torch.sort(dim=0) + a gather of the K ranks (per window: the window's rows gathered first).  The sort form is timed with
the XCD remap of its block index off and on (SMART_FDC_XCD_REMAP), same box, same run.  HIP events around every launch,
warm-up first, the MEDIAN of the repeated launches; GB/s are matrix bytes (8 * R * N) over that time.  Writes one text
file (default profiles/flow_duration.txt).

    python tools/bench_flow_duration.py [--out FILE] [--sizes 10000,100000] [--reps 5] [--slow-reps 2]
"""
import argparse
import os
import statistics
import sys
from datetime import datetime, timedelta

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smartpy_amd import engine      # noqa: E402
from smartpy_amd.windows import evaluation_windows, non_exceedance      # noqa: E402

R = 3653
EXCEEDANCE = (0.01, 0.05, 0.1, 0.2, 0.5, 0.8, 0.9, 0.95, 0.99)


def torch_curves(sim, obs, ids, n_windows, q):
    """torch.sort along time + a gather of the K ranks -> [W, K, N] (the sorted matrix and its index matrix are
    materialised by torch.sort; nothing pairs the result with the sorted observations)"""
    out = []
    for w in range(n_windows):
        rows = torch.nonzero((ids == w) & ~torch.isnan(obs)).squeeze(1)
        ordered = torch.sort(sim[rows], dim=0).values
        m = rows.numel()
        ranks = torch.tensor([max(1, int(np.ceil(qk * m))) - 1 for qk in q], device=sim.device)
        out.append(ordered[ranks])
    return torch.stack(out)


def timed(fn, reps):
    """warm-up, then `reps` launches each between two HIP events -> (median ms, last result)"""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'flow_duration.txt'))
    ap.add_argument('--sizes', default='10000,100000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--slow-reps', type=int, default=2)
    args = ap.parse_args()
    stamps = [datetime(1990, 10, 1, 9) + timedelta(days=k) for k in range(R)]       # ten hydrological years
    cases = [('one window', np.zeros(R, dtype=np.int32)), ('10 hydro years', evaluation_windows(stamps, by='hydro_year')[0])]
    q = non_exceedance(EXCEEDANCE)
    g = torch.Generator(device='cuda').manual_seed(0)
    rng = np.random.default_rng(0)
    obs_host = np.abs(rng.normal(3.0, 1.5, R))
    obs_host[rng.random(R) < 0.15] = np.nan
    lines = ['flow duration curves of a stored [R = %d][N] fp64 matrix, K = %d probabilities; ms per launch (HIP events, '
             'warm-up, median of %d; select and torch: median of %d); GB/s = 8 * R * N bytes over that time'
             % (R, len(q), args.reps, args.slow_reps),
             'device: %s; 15 %% of the observations missing; remap = SMART_FDC_XCD_REMAP (block index -> XCD-contiguous '
             'sample blocks)' % torch.cuda.get_device_name(),
             '%8s  %-15s %-28s %10s %8s' % ('N', 'case', 'what', 'ms', 'GB/s')]

    def row(n, case, what, ms, note=''):
        lines.append('%8d  %-15s %-28s %10.3f %8.0f%s' % (n, case, what, ms, 8.0 * R * n / 1e6 / ms, note))
        print(lines[-1], flush=True)

    for n in [int(s) for s in args.sizes.split(',')]:
        sim = torch.rand((R, n), dtype=torch.float64, device='cuda', generator=g) * 6 + 0.01
        obs = torch.from_numpy(obs_host).cuda()
        ms, _ = timed(lambda: engine.objective_functions(sim, obs), args.reps)
        row(n, '-', 'smart_objfn_hip (one read)', ms)
        for name, ids_host in cases:
            ids = torch.from_numpy(ids_host).cuda()
            W = int(ids_host.max()) + 1
            results = {}
            for remap in ('0', '1'):
                os.environ['SMART_FDC_XCD_REMAP'] = remap
                ms, got = timed(lambda: engine.flow_duration(sim, q, obs, ids, W, method='sort'), args.reps)
                row(n, name, 'sort, remap %s' % remap, ms)
                results[remap] = got[0]
                ms, got = timed(lambda: engine.flow_duration(sim, q, obs, ids, W, objfn=True, method='sort'), args.reps)
                row(n, name, 'sort + objfn, remap %s' % remap, ms)
            del os.environ['SMART_FDC_XCD_REMAP']
            same = bool((results['0'].view(torch.int64) == results['1'].view(torch.int64)).all())
            ms, picked = timed(lambda: engine.flow_duration(sim, q, obs, ids, W, method='select'), args.slow_reps)
            row(n, name, 'select', ms, '  (bits of the sort form: %s; remap on = off: %s)'
                % (bool((picked[0].view(torch.int64) == results['0'].view(torch.int64)).all()), same))
            ms, ref = timed(lambda: torch_curves(sim, obs, ids, W, q), args.slow_reps)
            row(n, name, 'torch.sort + gather', ms, '  (equal to the sort form: %s)' % bool((ref == results['0']).all()))
            del ref, picked, results, got
            torch.cuda.empty_cache()
        del sim
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
