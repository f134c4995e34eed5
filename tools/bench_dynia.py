#!/usr/bin/env python3
"""Time of the dynamic identifiability analysis (smart_dynia_hip: moving-window error sums, selection of the best tenth
and the shares of 10 factors x 20 bins per report step) of a [R, N] matrix of daily steps, beside two yardsticks measured
in the same run on the same matrix: smart_objfn_hip (ONE read of the matrix: the floor of anything that looks at every
value) and a torch statement of the same definition (the sliding sum as a difference of cumulative sums along time,
kthvalue over the samples, one scatter_add per factor), chunked over the report steps so that its matrix-sized temporaries
stay below CHUNK_BYTES each.  The calls are prepared (matrix, observations, categories, outputs and workspace on the
device) and timed with HIP events around every call, warm-up first, the MEDIAN of the repeated calls.  The answers are
compared.  Writes one text file (default profiles/dynia.txt).

    python tools/bench_dynia.py [--out FILE] [--sizes 10000,100000] [--reps 5] [--torch-reps 2]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smartpy_amd import _lib, analysis      # noqa: E402

R, H, BINS, FACTORS, FRACTION = 3653, 15, 20, 10, 0.1
CHUNK_BYTES = 1 << 28       # of one [steps, N] fp64 temporary of the torch statement


def torch_statement(sim, obs, cat, h, fraction, bins):
    """the definition of include/smart_amd.h in torch (every window observed enough, every sum finite, linear support with
    S > 0) -> (shares [R, P, B], cut [R], the steps of a chunk)"""
    rows, N = sim.shape
    P = cat.shape[0]
    shares = torch.empty((rows, P, bins), dtype=torch.float64, device=sim.device)
    cut = torch.empty((rows,), dtype=torch.float64, device=sim.device)
    index = cat.long()
    seen = torch.isfinite(obs)
    step = max(1, CHUNK_BYTES // (8 * N) - 2 * h - 1)
    k = max(1, int(math.ceil(fraction * float(N))))
    for lo in range(0, rows, step):
        hi = min(rows, lo + step)
        a, b = max(0, lo - h), min(rows, hi + h)
        d = torch.where(seen[a:b, None], (sim[a:b] - obs[a:b, None]).abs(), torch.zeros((), dtype=torch.float64,
                                                                                      device=sim.device))
        run = torch.cat([torch.zeros((1, N), dtype=torch.float64, device=sim.device), torch.cumsum(d, dim=0)])
        r = torch.arange(lo, hi, device=sim.device)
        first, last = (r - h).clamp(min=0) - a, (r + h).clamp(max=rows - 1) - a + 1
        E = run[last] - run[first]
        c = torch.kthvalue(E, k, dim=1).values
        s = (c[:, None] - E).clamp(min=0.0) * (E <= c[:, None])
        S = s.sum(dim=1)
        for p in range(P):
            acc = torch.zeros((hi - lo, 256), dtype=torch.float64, device=sim.device)
            acc.scatter_add_(1, index[p].expand(hi - lo, N), s)
            shares[lo:hi, p] = acc[:, :bins] / S[:, None]
        cut[lo:hi] = c
    return shares, cut, step


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


def prepared_dynia(L, sim, obs, cat, keep_errors=False):
    rows, N = sim.shape
    P = cat.shape[0]
    need = int(L.smart_dynia_workspace_bytes(N, rows, H, P, BINS))
    work = torch.empty(need, dtype=torch.uint8, device=sim.device)
    shares = torch.empty((rows, P, BINS), dtype=torch.float64, device=sim.device)
    cut = torch.empty((rows,), dtype=torch.float64, device=sim.device)
    retained = torch.empty((rows,), dtype=torch.int32, device=sim.device)
    count = torch.empty((rows,), dtype=torch.int32, device=sim.device)
    err = torch.empty((rows, N), dtype=torch.float64, device=sim.device) if keep_errors else None
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(L.smart_dynia_hip(N, rows, sim.data_ptr(), sim.stride(0), obs.data_ptr(), H, H + 1, FRACTION,
                                     cat.data_ptr(), P, BINS, _lib.DYNIA_SUPPORTS['linear'], shares.data_ptr(),
                                     cut.data_ptr(), retained.data_ptr(), count.data_ptr(), analysis._ptr(err), N,
                                     work.data_ptr(), need, stream))
        return shares, cut
    return call, need


def prepared_objfn(L, sim, obs):
    rows, N = sim.shape
    out = torch.empty((N, 8), dtype=torch.float64, device=sim.device)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(L.smart_objfn_hip(N, rows, sim.data_ptr(), sim.stride(0), obs.data_ptr(), None, float('nan'),
                                     out.data_ptr(), stream))
        return out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'dynia.txt'))
    ap.add_argument('--sizes', default='10000,100000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-reps', type=int, default=2)
    args = ap.parse_args()
    L = _lib.lib()
    g = torch.Generator(device='cuda').manual_seed(0)
    lines = ['dynamic identifiability analysis of [N] x %d daily steps, fp64: half width %d (windows of %d steps), the best '
             '%g retained, linear support, %d factors x %d bins; ms per call (HIP events, prepared, warm-up, median of %d; '
             'torch: of %d)' % (R, H, 2 * H + 1, FRACTION, FACTORS, BINS, args.reps, args.torch_reps),
             'device: %s; the selection keeps a step in LDS up to N = %d' % (torch.cuda.get_device_name(),
                                                                            analysis.dynia_lds_capacity()),
             '%8s  %-44s %10s  %s' % ('N', 'what', 'ms', 'note')]

    def row(N, what, ms, note=''):
        lines.append('%8d  %-44s %10.3f  %s' % (N, what, ms, note))
        print(lines[-1], flush=True)

    for N in [int(s) for s in args.sizes.split(',')]:
        sim = torch.rand((R, N), dtype=torch.float64, device='cuda', generator=g) * 5
        obs = torch.rand((R,), dtype=torch.float64, device='cuda', generator=g) * 5
        cat = torch.randint(0, BINS, (FACTORS, N), device='cuda', generator=g).to(torch.uint8)
        ms_floor, _ = timed(prepared_objfn(L, sim, obs), args.reps)
        row(N, 'smart_objfn_hip (one read of the matrix)', ms_floor, '%.0f GB/s' % (8e-6 * R * N / ms_floor))
        call, need = prepared_dynia(L, sim, obs, cat)
        ms, (shares, cut) = timed(call, args.reps)
        ours = (shares.clone(), cut.clone())
        row(N, 'smart_dynia_hip', ms, 'workspace %.0f MiB; %.1f x the one read' % (need / 2.0 ** 20, ms / ms_floor))
        call, _ = prepared_dynia(L, sim, obs, cat, keep_errors=True)
        ms_err, (shares, cut) = timed(call, args.reps)
        same = torch.equal(shares.view(torch.int64), ours[0].view(torch.int64))
        row(N, 'smart_dynia_hip, err [R, N] kept', ms_err, 'every step in one batch; the same bits: %s' % same)
        ms_t, (ref, ref_cut, step) = timed(lambda: torch_statement(sim, obs, cat, H, FRACTION, BINS), args.torch_reps)
        worst = float((ours[0] - ref).abs().max())
        cuts = float(((ours[1] - ref_cut).abs() / ref_cut).max())
        note = '%s; %.2f x the time of smart_dynia_hip' % (
            'one pass over all steps' if step >= R else 'CHUNKED over the steps, %d at a time' % step, ms_t / ms)
        if ms_t < ms:
            note += ' -- THE KERNELS ARE SLOWER THAN TORCH'
        row(N, 'torch: cumsum differences, kthvalue, scatter_add', ms_t,
            '%s; largest difference of a share %.1e, of a cut %.1e relative' % (note, worst, cuts))
        del sim, ours, ref
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
