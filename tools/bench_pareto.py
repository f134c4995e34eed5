#!/usr/bin/env python3
"""Time of the Pareto dominance counts (smart_pareto_counts_hip: keys pass, pair kernel, closing pass) of a score matrix
[N, M], beside a yardstick measured in the same run on the same tensors: a chunked torch statement of the same counts
(keys, then per chunk of candidates the broadcast compares `>=` and `<=` against every row, `all` over the objectives,
`sum` over the challengers).  The call is prepared (scores on the device, workspace allocated) and timed with HIP events
around every launch, warm-up first, the MEDIAN of the repeated launches; ns per pair = that time over E^2 for the E rows
that take part.  The two answers are compared, exactly.  Writes one text file (default profiles/pareto.txt).

    python tools/bench_pareto.py [--out FILE] [--cases 10000x2x1,...,100000x7x0.01] [--reps 5] [--torch-reps 1]

A case is N x M x share of the rows that are eligible.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smartpy_amd import analysis      # noqa: E402

WORDS = ['max', 'min', ('target', 0.5)]
CHUNK_BYTES = 1 << 30       # of one boolean array [chunk, E, M] of the torch statement


def torch_statement(scores, words, eligible):
    """the definition of include/smart_amd.h in torch -> int32 [N]"""
    N, M = scores.shape
    keys = torch.stack([scores[:, m] if w == 'max' else (-scores[:, m] if w == 'min' else -(scores[:, m] - w[1]).abs())
                        for m, w in enumerate(words)], dim=1)
    part = ~torch.isnan(keys).any(dim=1)
    if eligible is not None:
        part &= eligible != 0
    k = keys[part]
    E = k.shape[0]
    counts = torch.empty(E, dtype=torch.int32, device=scores.device)
    step = max(1, CHUNK_BYTES // max(1, E * M))
    for lo in range(0, E, step):
        mine = k[lo:lo + step, None, :]
        ge = (k[None, :, :] >= mine).all(dim=2)
        le = (k[None, :, :] <= mine).all(dim=2)
        counts[lo:lo + step] = (ge & ~le).sum(dim=1)
    out = torch.full((N,), -1, dtype=torch.int32, device=scores.device)
    out[part] = counts
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
                                                  'profiles', 'pareto.txt'))
    ap.add_argument('--cases', default='10000x2x1,10000x7x1,10000x16x1,100000x2x1,100000x7x1,100000x16x1,100000x7x0.01')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-reps', type=int, default=1)
    args = ap.parse_args()
    g = torch.Generator(device='cuda').manual_seed(0)
    lines = ['Pareto dominance counts of a [N, M] fp64 score matrix (normal scores; directions cycle max / min / target 0.5); '
             'ms per call (HIP events, prepared, warm-up, median of %d; torch: of %d); ns per pair = ms over E^2'
             % (args.reps, args.torch_reps),
             'device: %s' % torch.cuda.get_device_name(),
             '%8s %3s %8s %8s  %-34s %10s %10s' % ('N', 'M', 'E', 'front', 'what', 'ms', 'ns/pair')]

    def row(N, M, E, front, what, ms, note=''):
        lines.append('%8d %3d %8d %8d  %-34s %10.3f %10.5f%s' % (N, M, E, front, what, ms, ms * 1e6 / (float(E) * E), note))
        print(lines[-1], flush=True)

    for case in args.cases.split(','):
        N, M, share = case.split('x')
        N, M, share = int(N), int(M), float(share)
        scores = torch.randn((N, M), dtype=torch.float64, device='cuda', generator=g)
        words = [WORDS[m % 3] for m in range(M)]
        eligible = None
        if share < 1.0:
            eligible = (torch.rand(N, device='cuda', generator=g) < share).to(torch.uint8)
        call = analysis._ParetoCall('bench_pareto', scores, words, None, None, eligible)
        ms, ours = timed(lambda: call.counts(call.eligible), args.reps)
        E, front = int((ours >= 0).sum()), int((ours == 0).sum())
        row(N, M, E, front, 'smart_pareto_counts_hip', ms)
        ms_t, ref = timed(lambda: torch_statement(scores, words, eligible), args.torch_reps)
        same = bool((ref == ours).all())
        row(N, M, E, front, 'torch: chunked broadcast compares', ms_t,
            '  (the same integers: %s; %.1f x the time of the kernels)' % (same, ms_t / ms))
        del scores, call, ours, ref
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
