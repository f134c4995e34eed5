#!/usr/bin/env python3
"""Time of the Sobol indices (smart_sobol_indices_hip: point estimates, and point estimates + bootstrap) of a stored
[R][N] matrix in the block-major order of a Saltelli design, beside two yardsticks measured in the same run on the same
matrix: smart_objfn_hip (the cost of reading the matrix once) for the point estimates, and a torch statement of the
bootstrap -- elementwise terms, `sum`, and torch.matmul of counts x terms -- for the bootstrap.  HIP events around every
launch, warm-up first, the MEDIAN of the repeated launches; GB/s are matrix bytes (8 * R * N) over that time, GFLOP/s of the
bootstrap 2 * R * B * n * (2 + 2k) over it.  Writes one text file (default profiles/sobol.txt).

    python tools/bench_sobol.py [--out FILE] [--cases 3653x8192x10x0,3653x8192x10x128,8x100000x10x128] [--reps 5]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smartpy_amd import engine      # noqa: E402


def torch_statement(y, n, k, counts):
    """the definition of include/smart_amd.h in torch: terms [R, n, 2 + 2k], one matmul with the counts [n, B] per row
    batch -> (S1, ST [R, k], S1_std, ST_std [R, k] or None)"""
    R = y.shape[0]
    blocks = y[:, :n * (k + 2)].reshape(R, k + 2, n)
    yA, yB, yAB = blocks[:, 0], blocks[:, 1], blocks[:, 2:]
    mu = (yA.sum(1) + yB.sum(1)) / (2 * n)
    uA, uB = yA - mu[:, None], yB - mu[:, None]
    d = yAB - yA[:, None, :]
    terms = torch.cat([(uA * uA + uB * uB)[:, None], (uA + uB)[:, None], uB[:, None] * d, d * d], dim=1)   # [R, 2 + 2k, n]

    def finish(s):          # s [R, 2 + 2k, X]
        V = s[:, 0] / (2 * n) - (s[:, 1] / (2 * n)) ** 2
        return s[:, 2:2 + k] / (n * V[:, None]), s[:, 2 + k:] / (2 * n * V[:, None])
    S1, ST = finish(terms.sum(2, keepdim=True))
    if counts is None:
        return S1[..., 0], ST[..., 0], None, None
    b1, bt = finish(torch.matmul(terms, counts))        # [R, k, B]
    return S1[..., 0], ST[..., 0], b1.std(dim=2), bt.std(dim=2)


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
                                                  'profiles', 'sobol.txt'))
    ap.add_argument('--cases', default='3653x8192x10x0,3653x8192x10x128,8x100000x10x128')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    g = torch.Generator(device='cuda').manual_seed(0)
    lines = ['Sobol indices of a stored [R][N = n (k + 2)] fp64 matrix; ms per launch (HIP events, warm-up, median of %d); '
             'GB/s = 8 * R * N bytes over that time; GFLOP/s = 2 R B n (2 + 2k) over it' % args.reps,
             'device: %s' % torch.cuda.get_device_name(),
             '%6s %8s %3s %4s  %-34s %10s %8s %9s' % ('R', 'n', 'k', 'B', 'what', 'ms', 'GB/s', 'GFLOP/s')]

    def row(R, n, k, B, what, ms, note=''):
        flops = 2.0 * R * B * n * (2 + 2 * k)
        lines.append('%6d %8d %3d %4d  %-34s %10.3f %8.0f %9.0f%s'
                     % (R, n, k, B, what, ms, 8.0 * R * n * (k + 2) / 1e6 / ms, flops / 1e6 / ms, note))
        print(lines[-1], flush=True)

    for case in args.cases.split(','):
        R, n, k, B = (int(v) for v in case.split('x'))
        N = n * (k + 2)
        y = torch.rand((R, N), dtype=torch.float64, device='cuda', generator=g) * 6 + 0.01
        obs = torch.rand(R, dtype=torch.float64, device='cuda', generator=g) + 1.0
        ms, _ = timed(lambda: engine.objective_functions(y, obs), args.reps)
        row(R, n, k, 0, 'smart_objfn_hip (one read)', ms)
        ms, point = timed(lambda: engine.sobol_indices(y, n, k), args.reps)
        row(R, n, k, 0, 'sobol_indices, point estimates', ms)
        if B:
            counts = torch.from_numpy(engine.sobol_counts(n, B, seed=0).view(np.int16)).cuda()
            ms, both = timed(lambda: engine.sobol_indices(y, n, k, counts=counts), args.reps)
            same = bool((both.S1.view(torch.int64) == point.S1.view(torch.int64)).all())
            row(R, n, k, B, 'sobol_indices, with bootstrap', ms, '  (point estimates the same bits: %s)' % same)
            wide = counts.to(torch.float64)
            try:
                ms, ref = timed(lambda: torch_statement(y, n, k, wide), max(1, args.reps // 2))
                err = float((ref[2] - both.S1_std).abs().max())
                row(R, n, k, B, 'torch: terms + sum + matmul', ms, '  (largest |S1_std - ours| %.1e)' % err)
                del ref
            except torch.OutOfMemoryError:
                lines.append('%6d %8d %3d %4d  torch: terms + sum + matmul: out of memory' % (R, n, k, B))
            del counts, wide, both
        del y, point
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
