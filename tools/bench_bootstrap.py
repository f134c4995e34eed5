#!/usr/bin/env python3
"""Time of the score uncertainty (smart_objfn_bootstrap_hip: per-window moments, B replicates of seven scores, their mean,
standard deviation and three quantiles) of a stored [R, N] discharge matrix, beside two yardsticks measured in the same run
on the same matrix: smart_objfn_hip -- the one-read floor every matrix analysis here is held against -- and a torch
statement of the same contraction: the per-window moments by sums over the rows of every window, `counts.double() @
moments`, the seven formulas, mean and standard deviation over the replicates and the three order statistics by a sort
along them.  The calls are prepared (matrix, observations, window ids, counts, outputs and workspace on the device) and
timed with HIP events around every call, warm-up first, the MEDIAN of the repeated calls; GB/s = the matrix's R * N * 8
bytes over that time.  Mean and standard deviation of the two answers are compared.  Writes one text file (default
profiles/bootstrap.txt).

    python tools/bench_bootstrap.py [--out FILE] [--cases 10000x3653x10x1000,100000x3653x10x1000] [--reps 5] [--torch-reps 3]

A case is N x R x W x B; the W windows are blocks of consecutive report steps (hydrological years), every step observed;
the counts are engine.bootstrap_counts(W, B, seed=0).
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smartpy_amd import _lib, engine      # noqa: E402
from tools.bench_signatures import recessions, timed      # noqa: E402

PROBS = (0.05, 0.5, 0.95)


def torch_statement(sim, obs, bounds, counts):
    """-> (mean [7, N], std [7, N], quantiles [3, 7, N]) of the B replicates: moments per block of rows [lo, hi) about
    the observation mean and the first row, counts @ moments, the formulas of finish_objectives"""
    g, shift = obs.mean(), sim[0]
    ow, mom = [], []
    for lo, hi in bounds:
        e, s = obs[lo:hi], sim[lo:hi]
        d, u, c = s - e[:, None], s - shift, e - g
        ow.append(torch.stack([torch.tensor(float(hi - lo), dtype=torch.float64, device=sim.device), e.sum(), c.sum(),
                               (c * c).sum()]))
        mom.append(torch.stack([d.sum(dim=0), (d * d).sum(dim=0), u.sum(dim=0), (u * u).sum(dim=0),
                                (c[:, None] * u).sum(dim=0)]))
    w = counts.double()
    n, se, s1, s2 = (w @ torch.stack(ow)).t()[:, :, None]
    A, B, C1, C2, C3 = (w @ torch.stack(mom).reshape(len(bounds), -1)).reshape(len(counts), 5, -1).transpose(0, 1)
    see, m1 = s2 - s1 * s1 / n, C1 / n
    var_s, var_e, cov = C2 / n - m1 * m1, see / n, (C3 - s1 * m1) / n
    cc = (cov / torch.sqrt(var_s * var_e)).clamp(-1.0, 1.0)
    alpha, beta = torch.sqrt(var_s / var_e), 1.0 + A / se
    reps = torch.stack([1.0 - B / see, 1.0 - torch.sqrt((cc - 1.0) ** 2 + (alpha - 1.0) ** 2 + (beta - 1.0) ** 2), cc, alpha,
                        beta, 100.0 * (A / se), torch.sqrt(B / n)], dim=1)
    ordered = torch.sort(reps, dim=0).values
    ranks = [max(1, int(-(-q * len(counts) // 1))) - 1 for q in PROBS]
    return reps.mean(dim=0), reps.std(dim=0), ordered[ranks]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'bootstrap.txt'))
    ap.add_argument('--cases', default='10000x3653x10x1000,100000x3653x10x1000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-reps', type=int, default=3)
    args = ap.parse_args()
    L = _lib.lib()
    g = torch.Generator(device='cuda').manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = ['Score uncertainty of a [R, N] fp64 discharge matrix (recessions with random events, every step observed, W '
             'windows of consecutive steps, B bootstrap replicates, quantiles 0.05 / 0.5 / 0.95, no replicates buffer); ms '
             'per call (HIP events, prepared, warm-up, median of %d; torch: of %d); GB/s = R * N * 8 bytes over ms'
             % (args.reps, args.torch_reps),
             'device: %s' % torch.cuda.get_device_name(),
             '%8s %6s %3s %5s  %-52s %10s %9s' % ('N', 'R', 'W', 'B', 'what', 'ms', 'GB/s')]
    matrices = {}

    def row(N, R, W, B, what, ms, note=''):
        lines.append('%8d %6d %3d %5d  %-52s %10.3f %9.0f%s' % (N, R, W, B, what, ms, R * N * 8 / ms / 1e6, note))
        print(lines[-1], flush=True)

    for case in args.cases.split(','):
        N, R, W, B = (int(v) for v in case.split('x'))
        if (N, R) not in matrices:
            matrices.clear()
            torch.cuda.empty_cache()
            matrices[(N, R)] = recessions(N, R, g)
        sim = matrices[(N, R)]
        obs = (sim[:, 0] * (0.7 + 0.6 * torch.rand(R, dtype=torch.float64, device='cuda', generator=g))).contiguous()
        bounds = [(w * R // W, (w + 1) * R // W) for w in range(W)]
        win = torch.empty(R, dtype=torch.int32, device='cuda')
        for w, (lo, hi) in enumerate(bounds):
            win[lo:hi] = w
        host_counts = engine.bootstrap_counts(W, B, seed=0)
        counts = torch.from_numpy(host_counts.view('int16').copy()).cuda()
        wide = torch.from_numpy(host_counts.astype('int64')).cuda()
        q = (ctypes.c_double * len(PROBS))(*PROBS)
        point = torch.empty((N, 7), dtype=torch.float64, device='cuda')
        stats = torch.empty((7, 2 + len(PROBS), N), dtype=torch.float64, device='cuda')
        need = int(L.smart_bootstrap_workspace_bytes(N, W, B, 0))
        work = torch.empty(need, dtype=torch.uint8, device='cuda')
        objfn = torch.empty((N, 8), dtype=torch.float64, device='cuda')

        def bootstrap():
            _lib.check(L.smart_objfn_bootstrap_hip(N, R, sim.data_ptr(), N, obs.data_ptr(), win.data_ptr(), W, 0, 0.0,
                                                   counts.data_ptr(), B, q, len(PROBS), point.data_ptr(), stats.data_ptr(),
                                                   None, work.data_ptr(), need, stream))
            return stats

        def floor():
            _lib.check(L.smart_objfn_hip(N, R, sim.data_ptr(), N, obs.data_ptr(), None, float('nan'), objfn.data_ptr(),
                                         stream))
            return objfn

        ms_f, _ = timed(floor, args.reps)
        row(N, R, W, B, 'smart_objfn_hip (one read of the matrix)', ms_f)
        ms, ours = timed(bootstrap, args.reps)
        row(N, R, W, B, 'smart_objfn_bootstrap_hip (workspace %.0f MiB)' % (need / 2 ** 20), ms,
            '  (%.2f x smart_objfn_hip)' % (ms / ms_f))
        ms_t, (mean, std, quant) = timed(lambda: torch_statement(sim, obs, bounds, wide), args.torch_reps)
        err = max(float(torch.nan_to_num((ours[:, 0] - mean) / mean.abs().clamp_min(1e-12)).abs().max()),
                  float(torch.nan_to_num((ours[:, 1] - std) / std.abs().clamp_min(1e-12)).abs().max()))
        row(N, R, W, B, 'torch: moments, counts @ moments, formulas, sort', ms_t,
            '  (%.2f x smart_objfn_bootstrap_hip; mean and std differ by at most %.1e relative)' % (ms_t / ms, err))
        del mean, std, quant
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
