#!/usr/bin/env python3
"""Time of the ensemble verification scores (smart_ensemble_scores_hip: CRPS, spread, both PITs and the mean per report
step, LDS form and global form) of a [R, N] matrix, beside two yardsticks measured in the same run on the same tensors:
the sort form of smart_weighted_quantiles_hip (the same network in LDS, three order statistics out -- up to its capacity)
and a torch statement of the five columns (torch.sort(dim=1), cumsum, a flipped cumsum and the formulas), chunked over the
report steps so that its matrix-sized temporaries stay below CHUNK_BYTES each.  Beyond the LDS capacity the global form
is also timed with four times the workspace the helper entry asks for (more report steps per launch).  The calls are
prepared (matrix, weights, observations and workspace on the device) and timed with HIP events around every launch,
warm-up first, the MEDIAN of the repeated launches.  The answers are compared.  Writes one text file (default profiles/ensemble_scores.txt).

    python tools/bench_ensemble_scores.py [--out FILE] [--sizes 1000,8192,100000] [--reps 5] [--torch-reps 2]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smartpy_amd import _lib, analysis      # noqa: E402

R = 3653
PROBS = (0.05, 0.5, 0.95)
CHUNK_BYTES = 1 << 28       # of one [steps, N] fp64 temporary of the torch statement
AUTO, LDS, GLOBAL = 0, 1, 2


def torch_statement(sim, weights, obs):
    """the five definitions of include/smart_amd.h in torch (finite members, weights > 0) -> [5, R]"""
    rows, N = sim.shape
    out = torch.empty((5, rows), dtype=torch.float64, device=sim.device)
    step = max(1, CHUNK_BYTES // (8 * N))
    for lo in range(0, rows, step):
        x, order = torch.sort(sim[lo:lo + step], dim=1)
        y = obs[lo:lo + step, None]
        w = weights[order] if weights is not None else torch.ones_like(x)
        A = torch.cumsum(w, dim=1)
        B = torch.flip(torch.cumsum(torch.flip(w, (1,)), dim=1), (1,))[:, 1:]      # the suffix sums over j > i
        W = A[:, -1:]
        P, Q = A[:, :-1] / W, B / W
        lower, upper = x[:, :-1], x[:, 1:]
        m = torch.minimum(torch.maximum(y, lower), upper)
        o = out[:, lo:lo + step]
        o[0] = (torch.clamp(x[:, 0] - y[:, 0], min=0) + torch.clamp(y[:, 0] - x[:, -1], min=0)
                + ((m - lower) * P * P + (upper - m) * Q * Q).sum(dim=1))
        o[1] = ((upper - lower) * P * Q).sum(dim=1)
        o[2] = (w * (x < y)).sum(dim=1) / W[:, 0]
        o[3] = (w * (x <= y)).sum(dim=1) / W[:, 0]
        o[4] = (w * x).sum(dim=1) / W[:, 0]
    return out, step


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


def prepared_scores(L, sim, weights, obs, method, times=1):
    """-> a function that launches smart_ensemble_scores_hip on tensors that are all there, and returns its [5, R]; the
    workspace is `times` what smart_ensemble_scores_workspace_bytes asks for (the entry batches by what it is given)"""
    rows, N = sim.shape
    need = times * int(L.smart_ensemble_scores_workspace_bytes(N, rows, 0 if weights is None else 1, method))
    work = torch.empty(need, dtype=torch.uint8, device=sim.device) if need else None
    out = torch.empty((5, rows), dtype=torch.float64, device=sim.device)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(L.smart_ensemble_scores_hip(N, rows, sim.data_ptr(), sim.stride(0), analysis._ptr(weights),
                                               obs.data_ptr(), out.data_ptr(), method, analysis._ptr(work), need, stream))
        return out
    return call, need


def prepared_quantiles(L, sim, weights):
    rows, N = sim.shape
    q = (ctypes.c_double * len(PROBS))(*PROBS)
    out = torch.empty((len(PROBS), rows), dtype=torch.float64, device=sim.device)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(L.smart_weighted_quantiles_hip(N, rows, sim.data_ptr(), sim.stride(0), analysis._ptr(weights), q,
                                                  len(PROBS), out.data_ptr(), _lib.QUANTILES_SORT, stream))
        return out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'ensemble_scores.txt'))
    ap.add_argument('--sizes', default='1000,8192,100000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-reps', type=int, default=2)
    args = ap.parse_args()
    L = _lib.lib()
    cap = analysis.ensemble_scores_lds_capacity()
    qcap = analysis.quantiles_sort_capacity()
    g = torch.Generator(device='cuda').manual_seed(0)
    lines = ['ensemble verification scores (CRPS, SPREAD, PIT_LOW, PIT_HIGH, MEAN) of [N] x %d report steps, fp64; ms per '
             'call (HIP events, prepared, warm-up, median of %d; torch: of %d)' % (R, args.reps, args.torch_reps),
             'device: %s; LDS form up to N = %d, global form beyond (and where named)' % (torch.cuda.get_device_name(), cap),
             '%8s %-10s  %-46s %10s  %s' % ('N', 'weights', 'what', 'ms', 'note')]

    def row(N, weighted, what, ms, note=''):
        lines.append('%8d %-10s  %-46s %10.3f  %s' % (N, 'likelihood' if weighted else 'equal', what, ms, note))
        print(lines[-1], flush=True)

    for N in [int(s) for s in args.sizes.split(',')]:
        sim = torch.rand((R, N), dtype=torch.float64, device='cuda', generator=g) * 5
        obs = torch.rand((R,), dtype=torch.float64, device='cuda', generator=g) * 5
        likelihood = torch.rand((N,), dtype=torch.float64, device='cuda', generator=g) + 0.01
        for weights in (likelihood, None):
            ours = {}
            for name, method in (('LDS form', LDS), ('global form', GLOBAL)):
                if method == LDS and N > cap:
                    continue
                call, need = prepared_scores(L, sim, weights, obs, method)
                ms, out = timed(call, args.reps)
                ours[name] = (ms, out.clone())
                row(N, weights is not None, 'smart_ensemble_scores_hip, ' + name, ms,
                    'workspace %.0f MiB' % (need / 2.0 ** 20) if need else '')
            if N > cap:     # the helper's 256 MiB are fewer steps than the device has compute units: four times as much
                call, need = prepared_scores(L, sim, weights, obs, GLOBAL, times=4)
                ms, out = timed(call, args.reps)
                same = torch.equal(out.view(torch.int64), ours['global form'][1].view(torch.int64))
                row(N, weights is not None, 'smart_ensemble_scores_hip, global form', ms,
                    'workspace %.0f MiB given; the same bits: %s' % (need / 2.0 ** 20, same))
                ours['global form, 4 x the workspace'] = (ms, out.clone())
            best = min(v[0] for v in ours.values())
            if N <= qcap:
                ms_q, _ = timed(prepared_quantiles(L, sim, weights), args.reps)
                row(N, weights is not None, 'smart_weighted_quantiles_hip, sort form, 3 probs', ms_q,
                    'the scores take %.2f x its time' % (best / ms_q))
            else:
                lines.append('%8d %-10s  %-46s %10s  beyond its capacity of %d' % (
                    N, 'likelihood' if weights is not None else 'equal', 'smart_weighted_quantiles_hip, sort form', '-', qcap))
            (ms_t, (ref, step)) = timed(lambda: torch_statement(sim, weights, obs), args.torch_reps)
            worst = max(float(((v[1] - ref).abs() / ref.abs().clamp(min=1e-300)).max()) for v in ours.values())
            if N <= cap:
                against = '%.2f x the time of the LDS form' % (ms_t / ours['LDS form'][0])
            else:
                against = ('%.2f x the time of the global form with the workspace the helper asks for, %.2f x with four times '
                           'as much' % (ms_t / ours['global form'][0], ms_t / ours['global form, 4 x the workspace'][0]))
                if ms_t < ours['global form'][0]:
                    against += ' -- THE GLOBAL FORM IS SLOWER THAN TORCH with the helper\'s workspace'
            row(N, weights is not None, 'torch: sort, cumsum, flipped cumsum, formulas', ms_t,
                '%s; %s; largest relative difference of a column %.1e'
                % ('one pass over all steps' if step >= R else 'CHUNKED over the steps, %d at a time' % step, against, worst))
            del ours, ref
            torch.cuda.empty_cache()
        del sim
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
