#!/usr/bin/env python3
"""Time of the hydrological signatures (smart_signatures_hip) of a stored [R, N] discharge matrix, beside two yardsticks
measured in the same run on the same matrix: smart_objfn_hip -- the one-read floor every matrix analysis here is held
against -- and a torch statement of THREE of the twelve columns (flashiness, peak, lag-1 correlation: `diff`, `amax`
and sums over the rows of every window).  The calls are prepared (matrix, observations, window ids, thresholds and
outputs on the device) and timed with HIP events around every launch, warm-up first, the MEDIAN of the repeated launches;
GB/s = the matrix's R * N * 8 bytes over that time.  The three columns of the two answers are compared.  Writes one text
file (default profiles/signatures.txt).

    python tools/bench_signatures.py [--out FILE] [--cases 10000x3653x1,...,100000x3653x10] [--reps 5] [--torch-reps 3]

A case is N x R x W; the W windows are blocks of consecutive report steps (hydrological years), every step observed.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smartpy_amd import _lib      # noqa: E402

FLASHINESS, AC1, PEAK = 2, 3, 6


def recessions(N, R, g):
    """[R, N] on the device: per column s <- k s + event, x = 0.05 + s, k in [0.80, 0.98], events on 15 % of the rows"""
    k = 0.80 + 0.18 * torch.rand(N, dtype=torch.float64, device='cuda', generator=g)
    s = -torch.log(1.0 - torch.rand(N, dtype=torch.float64, device='cuda', generator=g))
    sim = torch.empty((R, N), dtype=torch.float64, device='cuda')
    for r in range(R):
        u = torch.rand((2, N), dtype=torch.float64, device='cuda', generator=g)
        s = k * s + torch.where(u[0] < 0.15, -2.0 * torch.log(1.0 - u[1]), torch.zeros_like(s))
        sim[r] = 0.05 + s
    return sim


def torch_statement(sim, bounds):
    """flashiness, lag-1 correlation and peak of every column per block of rows [lo, hi) -> [W, 3, N]"""
    out = torch.full((len(bounds), 3, sim.shape[1]), float('nan'), dtype=torch.float64, device=sim.device)
    for w, (lo, hi) in enumerate(bounds):
        x = sim[lo:hi]
        out[w, 2] = x.amax(dim=0)
        if hi - lo < 2:
            continue
        a, b = x[:-1], x[1:]
        out[w, 0] = torch.diff(x, dim=0).abs().sum(dim=0) / b.sum(dim=0)
        a, b = a - a.mean(dim=0), b - b.mean(dim=0)
        out[w, 1] = (a * b).sum(dim=0) / torch.sqrt((a * a).sum(dim=0) * (b * b).sum(dim=0))
    return out


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
                                                  'profiles', 'signatures.txt'))
    ap.add_argument('--cases', default='10000x3653x1,10000x3653x10,100000x3653x1,100000x3653x10')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-reps', type=int, default=3)
    args = ap.parse_args()
    L = _lib.lib()
    g = torch.Generator(device='cuda').manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = ['Hydrological signatures of a [R, N] fp64 discharge matrix (recessions with random events, every step observed, W '
             'windows of consecutive steps, alpha 0.925, thresholds 0.5 and 3); ms per call (HIP events, prepared, warm-up, '
             'median of %d; torch: of %d); GB/s = R * N * 8 bytes over ms' % (args.reps, args.torch_reps),
             'device: %s' % torch.cuda.get_device_name(),
             '%8s %6s %3s  %-44s %10s %9s' % ('N', 'R', 'W', 'what', 'ms', 'GB/s')]
    matrices = {}

    def row(N, R, W, what, ms, note=''):
        lines.append('%8d %6d %3d  %-44s %10.3f %9.0f%s' % (N, R, W, what, ms, R * N * 8 / ms / 1e6, note))
        print(lines[-1], flush=True)

    for case in args.cases.split(','):
        N, R, W = (int(v) for v in case.split('x'))
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
        pulse = torch.tensor([[0.5, 3.0]] * W, dtype=torch.float64, device='cuda')
        sig = torch.empty((W, _lib.SIGNATURE_COLS, N), dtype=torch.float64, device='cuda')
        objfn = torch.empty((N, 8), dtype=torch.float64, device='cuda')

        def signatures():
            _lib.check(L.smart_signatures_hip(N, R, sim.data_ptr(), N, obs.data_ptr(), win.data_ptr() if W > 1 else None, W,
                                              0.925, pulse.data_ptr(), sig.data_ptr(), stream))
            return sig

        def floor():
            _lib.check(L.smart_objfn_hip(N, R, sim.data_ptr(), N, obs.data_ptr(), None, float('nan'), objfn.data_ptr(),
                                         stream))
            return objfn

        ms_f, _ = timed(floor, args.reps)
        row(N, R, W, 'smart_objfn_hip (one read of the matrix)', ms_f)
        ms, ours = timed(signatures, args.reps)
        row(N, R, W, 'smart_signatures_hip (twelve columns)', ms, '  (%.2f x smart_objfn_hip)' % (ms / ms_f))
        ms_t, ref = timed(lambda: torch_statement(sim, bounds), args.torch_reps)
        mine = ours[:, [FLASHINESS, AC1, PEAK]]
        same = bool((torch.isnan(mine) == torch.isnan(ref)).all())
        err = float(torch.nan_to_num(mine - ref).abs().max())
        row(N, R, W, 'torch: three columns (diff, amax, sums)', ms_t,
            '  (%.2f x smart_signatures_hip; the same NaN: %s, largest difference %.1e)' % (ms_t / ms, same, err))
        del ref
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
