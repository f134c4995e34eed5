#!/usr/bin/env python3
"""Time of the PAWN sensitivity (smart_pawn_ks_hip: per report step the sort of the samples and the Kolmogorov-Smirnov
distances of 10 factors + 3 dummy factors x 10 bins) of a [R, N] matrix of daily steps, beside two yardsticks measured in
the same run on the same matrix: smart_ensemble_scores_hip without weights (the SAME sort of every step and one cheap pass
over it: the cost floor of this design) and a torch statement of the same integers (torch.sort, the categories gathered
through the order, the cumulative one-hot counts of every bin, abs().amax() over the evaluation points), chunked over the
report steps so that its [steps, N, bins] temporaries stay below CHUNK_BYTES each.  The calls are prepared (matrix,
categories, outputs and workspace on the device) and timed with HIP events around every call, warm-up first, the MEDIAN of
the repeated calls.  The torch answer must EQUAL the kernel's, bit for bit.  Writes one text file (default
profiles/pawn.txt).

    python tools/bench_pawn.py [--out FILE] [--sizes 1000,8192,100000] [--reps 5] [--torch-reps 2]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smartpy_amd import _lib, analysis, pawn      # noqa: E402

R, BINS, FACTORS, DUMMIES = 3653, 10, 10, 3
CHUNK_BYTES = 1 << 28       # of one [steps, N, bins] int64 temporary of the torch statement


def torch_statement(y, cat, bins):
    """the definition of include/smart_amd.h in torch (every value finite) -> (ks [R, P, B], the steps of a chunk)"""
    rows, N = y.shape
    P = cat.shape[0]
    index = cat.long()
    every = torch.arange(bins, device=y.device)
    counts = (index[:, :, None] == every).sum(dim=1)                      # [P, B] int64
    at = torch.arange(1, N + 1, device=y.device)[None, :, None]
    ks = torch.empty((rows, P, bins), dtype=torch.float64, device=y.device)
    step = max(1, CHUNK_BYTES // (8 * N * bins))
    for lo in range(0, rows, step):
        hi = min(rows, lo + step)
        v, order = torch.sort(y[lo:hi], dim=1)
        ev = torch.ones_like(v, dtype=torch.bool)
        ev[:, :-1] = v[:, :-1] != v[:, 1:]
        for p in range(P):
            c = torch.cumsum(index[p][order][:, :, None] == every, dim=1)
            d = (at * counts[p] - c * N).abs_()
            num = torch.where(ev[:, :, None], d, torch.zeros((), dtype=torch.int64, device=y.device)).amax(dim=1)
            ks[lo:hi, p] = num.double() / (float(N) * counts[p].double())
    return ks, step


def timed(fn, reps):
    """warm-up, then `reps` calls each between two HIP events -> (median ms, last result)"""
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


def prepared_pawn(L, y, cat, method):
    rows, N = y.shape
    P = cat.shape[0]
    need = int(L.smart_pawn_workspace_bytes(N, rows, method))
    work = torch.empty(max(need, 1), dtype=torch.uint8, device=y.device)
    ks = torch.empty((rows, P, BINS), dtype=torch.float64, device=y.device)
    counts = torch.empty((P, BINS), dtype=torch.int32, device=y.device)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(L.smart_pawn_ks_hip(N, rows, y.data_ptr(), y.stride(0), cat.data_ptr(), P, BINS, ks.data_ptr(),
                                       counts.data_ptr(), method, work.data_ptr(), need, stream))
        return ks
    return call, need


def prepared_sort(L, y):
    rows, N = y.shape
    need = int(L.smart_ensemble_scores_workspace_bytes(N, rows, 0, 0))
    work = torch.empty(max(need, 1), dtype=torch.uint8, device=y.device)
    out = torch.empty((_lib.ENSEMBLE_SCORE_COLS, rows), dtype=torch.float64, device=y.device)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(L.smart_ensemble_scores_hip(N, rows, y.data_ptr(), y.stride(0), None, None, out.data_ptr(), 0,
                                               work.data_ptr(), need, stream))
        return out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'pawn.txt'))
    ap.add_argument('--sizes', default='1000,8192,100000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-reps', type=int, default=2)
    args = ap.parse_args()
    L = _lib.lib()
    g = torch.Generator(device='cuda').manual_seed(0)
    lines = ['PAWN sensitivity (Kolmogorov-Smirnov distances per report step) of [N] x %d daily steps, fp64: %d factors + %d '
             'dummy factors x %d bins; ms per call (HIP events, prepared, warm-up, median of %d; torch: of %d)'
             % (R, FACTORS, DUMMIES, BINS, args.reps, args.torch_reps),
             'device: %s; LDS form up to N = %d, global form beyond (and where named)'
             % (torch.cuda.get_device_name(), analysis.pawn_lds_capacity()),
             '%8s  %-52s %10s  %s' % ('N', 'what', 'ms', 'note')]

    def row(N, what, ms, note=''):
        lines.append('%8d  %-52s %10.3f  %s' % (N, what, ms, note))
        print(lines[-1], flush=True)

    for N in [int(s) for s in args.sizes.split(',')]:
        y = torch.rand((R, N), dtype=torch.float64, device='cuda', generator=g) * 5
        cat = torch.cat([torch.randint(0, BINS, (FACTORS, N), device='cuda', generator=g).to(torch.uint8),
                         torch.from_numpy(pawn.dummy_table(N, BINS, DUMMIES, 0)).cuda()])
        ms_sort, _ = timed(prepared_sort(L, y), args.reps)
        row(N, 'smart_ensemble_scores_hip, no weights (the same sort)', ms_sort)
        lds = N <= analysis.pawn_lds_capacity()
        call, need = prepared_pawn(L, y, cat, 0)
        ms, ks = timed(call, args.reps)
        ours = ks.clone()
        row(N, 'smart_pawn_ks_hip, %s form' % ('LDS' if lds else 'global'), ms,
            '%s%.2f x the shared sort' % ('' if lds else 'workspace %.0f MiB; ' % (need / 2.0 ** 20), ms / ms_sort))
        call, _ = prepared_pawn(L, y, cat[:1].contiguous(), 0)
        ms_one, _ = timed(call, args.reps)
        row(N, 'smart_pawn_ks_hip, ONE factor (its sort, one pass)', ms_one,
            '%.2f x the shared sort; the other %d factors in %d more passes of the walk: %.3f ms'
            % (ms_one / ms_sort, FACTORS + DUMMIES - 1, -(-(FACTORS + DUMMIES) // (64 // BINS)) - 1, ms - ms_one))
        if lds:
            call, need = prepared_pawn(L, y, cat, 2)
            ms_g, ks = timed(call, args.reps)
            row(N, 'smart_pawn_ks_hip, global form', ms_g, 'workspace %.0f MiB; the same bits: %s'
                % (need / 2.0 ** 20, torch.equal(ks.view(torch.int64), ours.view(torch.int64))))
        ms_t, (ref, step) = timed(lambda: torch_statement(y, cat, BINS), args.torch_reps)
        equal = torch.equal(ref.view(torch.int64), ours.view(torch.int64))
        note = '%s; %.2f x the time of smart_pawn_ks_hip' % (
            'one pass over all steps' if step >= R else 'CHUNKED over the steps, %d at a time' % step, ms_t / ms)
        if ms_t < ms:
            note += ' -- THE KERNEL IS SLOWER THAN TORCH'
        row(N, 'torch: sort, gather, one-hot cumsum, abs().amax()', ms_t, '%s; equal to the kernel bit for bit: %s'
            % (note, equal))
        if not equal:
            raise SystemExit('the torch statement and the kernel disagree at N = %d' % N)
        del y, ours, ref, ks
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
