#!/usr/bin/env python3
"""Time of the windowed objective functions (smart_objfn_windows: split-sample and low-flow scores of a stored [R][N]
matrix) against (a) smart_objfn_hip on the same matrix -- the cost of one pass over it -- and against a torch statement
of the same sums (per window: gather the window's rows, transform, sum / mean over them on the device).  HIP events
around every launch, warm-up first, the MEDIAN of the repeated launches; GB/s are matrix bytes (8 * R * N) over that
time, whatever share of the rows the windows cover.  Writes one text file (default profiles/objfn_windows.txt).

    python tools/bench_objfn_windows.py [--out FILE] [--sizes 100000,1000000] [--reps 7] [--torch-reps 3]
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
from smartpy_amd.windows import evaluation_windows      # noqa: E402

R = 3653
TRANSFORMS = ('none', 'sqrt', 'log', 'inverse')


def torch_statement(sim, obs, ids, n_windows, transform, eps):
    """The same sums with torch: per window the rows that carry an observation, f of both series, the five moments
    about the observation mean, as masked sum / mean over the report axis -> [W, N, 5] (the finish is arithmetic on
    N numbers and is left out)."""
    f = {'none': lambda x: x, 'sqrt': torch.sqrt, 'log': lambda x: torch.log(x + eps),
         'inverse': lambda x: 1.0 / (x + eps)}[transform]
    out = []
    for w in range(n_windows):
        rows = torch.nonzero((ids == w) & ~torch.isnan(obs)).squeeze(1)
        e = f(obs[rows])
        s = f(sim[rows])
        d = s - e[:, None]
        out.append(torch.stack([d.sum(0), (d * d).sum(0), s.mean(0), s.var(0, unbiased=False),
                                ((e - e.mean())[:, None] * s).sum(0)], dim=1))
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
                                                  'profiles', 'objfn_windows.txt'))
    ap.add_argument('--sizes', default='100000,1000000')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--torch-reps', type=int, default=3)
    args = ap.parse_args()
    stamps = [datetime(1990, 10, 1, 9) + timedelta(days=k) for k in range(R)]       # ten hydrological years
    cases = [('a: one window', np.zeros(R, dtype=np.int32), ('none',))]
    cases.append(('b: 10 hydro years', evaluation_windows(stamps, by='hydro_year')[0], TRANSFORMS))
    cases.append(('c: 4 seasons', evaluation_windows(stamps, by='season')[0], ('none',)))
    g = torch.Generator(device='cuda').manual_seed(0)
    rng = np.random.default_rng(0)
    obs_host = np.abs(rng.normal(3.0, 1.5, R))
    obs_host[rng.random(R) < 0.15] = np.nan
    lines = ['objective functions per window of a stored [R = %d][N] fp64 matrix; ms per launch (HIP events, warm-up, median '
             'of %d; torch: median of %d); GB/s = 8 * R * N bytes over that time' % (R, args.reps, args.torch_reps),
             'device: %s; 15 %% of the observations missing; eps = 0.03 for log and inverse' % torch.cuda.get_device_name(),
             '%9s  %-18s %-8s %10s %8s  %14s %8s  %11s' % ('N', 'case', 'f', 'windows ms', 'GB/s', 'objfn_hip ms', 'GB/s',
                                                          'torch ms')]
    for n in [int(s) for s in args.sizes.split(',')]:
        sim = torch.rand((R, n), dtype=torch.float64, device='cuda', generator=g) * 6 + 0.01
        obs = torch.from_numpy(obs_host).cuda()
        gbytes = 8.0 * R * n / 1e9
        whole_ms, whole = timed(lambda: engine.objective_functions(sim, obs), args.reps)
        for name, ids_host, transforms in cases:
            ids = torch.from_numpy(ids_host).cuda()
            W = int(ids_host.max()) + 1
            for transform in transforms:
                eps = 0.03 if transform in ('log', 'inverse') else 0.0
                ms, got = timed(lambda: engine.objective_functions_windows(sim, obs, ids, n_windows=W,
                                                                           transform=transform, eps=eps), args.reps)
                t_ms, _ = timed(lambda: torch_statement(sim, obs, ids, W, transform, eps), args.torch_reps)
                note = ''
                if name.startswith('a'):
                    worst = float(((got[0] - whole[:, :7]).abs() / whole[:, :7].abs().clamp_(min=1e-12)).max())
                    note = '  (against objfn_hip: max rel %.1e)' % worst
                lines.append('%9d  %-18s %-8s %10.3f %8.0f  %14s %8s  %11.3f%s'
                             % (n, name, transform, ms, gbytes / ms * 1e3,
                                '%.3f' % whole_ms if name.startswith('a') else '-',
                                '%.0f' % (gbytes / whole_ms * 1e3) if name.startswith('a') else '-', t_ms, note))
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
        del sim, whole
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
