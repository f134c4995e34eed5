#!/usr/bin/env python3
"""Time of the weighted-quantile kernels (smart_quantiles_sort / smart_quantiles_select: the GLUE prediction bounds)
against the same reduction written with torch on the same device matrix: torch.sort + cumsum + searchsorted, which
materialises a sorted copy and an index matrix.  HIP events around the launches; [N rows] x 3,653 report steps, three
probabilities, likelihood weights.  Writes one text file (default profiles/quantiles_vs_torch.txt).

    python tools/bench_quantiles.py [--out FILE] [--sizes 1000,8192,10000,100000] [--reps 5]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smartpy_amd import engine      # noqa: E402

R = 3653
PROBS = (0.05, 0.5, 0.95)


def torch_baseline(sim, weights, probs):
    """The definition with torch: sort every step's values, accumulate the weights in that order, first position with
    cum >= q * W."""
    values, order = torch.sort(sim, dim=1)
    cum = torch.cumsum(weights[order], dim=1)
    t = cum[:, -1:] * torch.tensor(probs, dtype=torch.float64, device=sim.device)[None, :]
    first = torch.searchsorted(cum, t).clamp_(max=sim.shape[1] - 1)
    return torch.gather(values, 1, first).t()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'quantiles_vs_torch.txt'))
    ap.add_argument('--sizes', default='1000,8192,10000,100000')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    cap = engine.quantiles_sort_capacity()
    g = torch.Generator(device='cuda').manual_seed(0)
    lines = ['weighted quantiles %s of [N] x %d report steps, fp64, likelihood weights; ms per call (HIP events, mean of %d)'
             % (PROBS, R, args.reps),
             'device: %s; sort form up to N = %d, select form beyond' % (torch.cuda.get_device_name(), cap),
             '%8s  %12s  %12s  %12s  %s' % ('N', 'sort [ms]', 'select [ms]', 'torch [ms]', 'verdict')]
    for n in [int(s) for s in args.sizes.split(',')]:
        sim = torch.rand((R, n), dtype=torch.float64, device='cuda', generator=g) * 5
        # weights with exact partial sums, so that the three ways must agree to the bit
        weights = torch.randint(1, 2 ** 20, (n,), device='cuda', generator=g).to(torch.float64) / 1024
        ms, outs = {}, {}
        for form in ('sort', 'select'):
            if form == 'sort' and n > cap:
                continue
            ms[form], outs[form] = timed(lambda: engine.weighted_quantiles(sim, PROBS, weights, method=form), args.reps)
        ms['torch'], outs['torch'] = timed(lambda: torch_baseline(sim, weights, PROBS), args.reps)
        agree = all(torch.equal(outs[f], outs['torch']) for f in outs)
        slower = [f for f in ('sort', 'select') if f in ms and ms[f] >= ms['torch']]
        verdict = ('both forms beat torch' if 'sort' in ms else 'select beats torch') if not slower else \
            'SLOWER THAN TORCH: ' + ', '.join(slower)
        lines.append('%8d  %12s  %12.3f  %12.3f  %s%s' % (n, '%.3f' % ms['sort'] if 'sort' in ms else '-', ms['select'],
                                                          ms['torch'], verdict, '' if agree else '; RESULTS DIFFER'))
        print(lines[-1], flush=True)
        del sim, outs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
