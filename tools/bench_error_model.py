#!/usr/bin/env python3
"""Time of the two kernels of the residual error model on a stored [R, N] discharge matrix (3,653 daily steps):
smart_error_model_loglik_hip beside smart_objfn_hip -- the one-read floor every matrix analysis here is held against -- and
beside a torch statement of the definition on the same matrix; smart_error_model_draw_hip (one replicate) beside a torch
statement (torch.randn for the noise, the recurrence as a loop over the steps); and one DE-MCz generation as
montecarlo.DEMCz.run() performs it, with likelihood='gaussian' and with 'ar1', by the wall clock.  The kernel calls are
prepared (everything on the device) and timed with HIP events around every launch, warm-up first, the MEDIAN of the
repeated launches; GB/s = the matrix's R * N * 8 bytes over that time (the draws write as many again).  The two answers of
the likelihood are compared.  Writes one text file (default profiles/error_model.txt).

    python tools/bench_error_model.py [--out FILE] [--sizes 10000,100000] [--reports 3653] [--reps 5] [--chains 10000]
"""
import argparse
import os
import shutil
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from smartpy_amd import _lib, demcz      # noqa: E402
from bench_demcz import EXTRA, SETTINGS, timed, walled      # noqa: E402
from bench_signatures import recessions      # noqa: E402

LN_TWO_PI = 1.8378770664093453


def torch_loglik(sim, obs, theta):
    """the definition of include/smart_amd.h (smart_error_model_loglik_hip) as torch statements on the whole matrix ->
    [3, N]; validity is not looked at"""
    s0, s1, phi = theta[:, 0], theta[:, 1], theta[:, 2]
    seen = ~torch.isnan(obs)
    cont = seen.clone()
    cont[0] = False
    cont[1:] &= seen[:-1]
    start = seen & ~cont
    q = (1.0 - phi) * (1.0 + phi)
    sigma = s0 + s1 * sim
    a = (obs[:, None] - sim) / sigma
    d = a[1:] - phi * a[:-1]
    zero = torch.zeros((), dtype=torch.float64, device=sim.device)
    ssq = torch.where(cont[1:, None], d * d, zero).sum(dim=0) + q * torch.where(start[:, None], a * a, zero).sum(dim=0)
    logsig = torch.where(seen[:, None], torch.log(sigma), zero).sum(dim=0)
    n, S = float(seen.sum()), float(start.sum())
    return torch.stack([((-0.5 * ssq - logsig) + (0.5 * S) * torch.log(q)) - (0.5 * n) * LN_TWO_PI, ssq, logsig])


def torch_draws(sim, theta, out):
    """error realisations on top of the matrix, one replicate: torch.randn, the AR(1) as a loop over the report steps"""
    s0, s1, phi = theta[:, 0], theta[:, 1], theta[:, 2]
    R, N = sim.shape
    eps = torch.randn((R, N), dtype=torch.float64, device=sim.device)
    a = eps[0] / torch.sqrt((1.0 - phi) * (1.0 + phi))
    for t in range(R):
        if t:
            a = phi * a + eps[t]
        out[t] = torch.clamp_min(sim[t] + (s0 + s1 * sim[t]) * a, 0.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'error_model.txt'))
    ap.add_argument('--sizes', default='10000,100000')
    ap.add_argument('--reports', type=int, default=3653)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-reps', type=int, default=3)
    ap.add_argument('--chains', type=int, default=10000, help='chains of the DE-MCz generations (0: leave them out)')
    args = ap.parse_args()
    L = _lib.lib()
    R = args.reports
    g = torch.Generator(device='cuda').manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = ['The residual error model on a [R, N] fp64 discharge matrix (recessions with random events, 10 %% of the steps '
             'without an observation, sigma0 in [0.01, 0.1], sigma1 in [0.05, 0.3], phi in [0, 0.99]); ms per call (HIP '
             'events, prepared, warm-up, median of %d; torch: of %d); GB/s = R * N * 8 bytes over ms'
             % (args.reps, args.torch_reps),
             'device: %s' % torch.cuda.get_device_name(),
             '%8s %6s  %-58s %10s %9s' % ('N', 'R', 'what', 'ms', 'GB/s')]
    print('\n'.join(lines), flush=True)

    def row(N, what, ms, note=''):
        lines.append('%8d %6d  %-58s %10.3f %9.0f%s' % (N, R, what, ms, R * N * 8 / ms / 1e6, note))
        print(lines[-1], flush=True)

    for N in [int(s) for s in args.sizes.split(',')]:
        torch.cuda.empty_cache()
        sim = recessions(N, R, g)
        obs = (sim[:, 0] * (0.7 + 0.6 * torch.rand(R, dtype=torch.float64, device='cuda', generator=g))).contiguous()
        obs[torch.rand(R, dtype=torch.float64, device='cuda', generator=g) < 0.1] = float('nan')
        u = torch.rand((N, 3), dtype=torch.float64, device='cuda', generator=g)
        theta = torch.stack([0.01 + 0.09 * u[:, 0], 0.05 + 0.25 * u[:, 1], 0.99 * u[:, 2]], dim=1).contiguous()
        objfn = torch.empty((N, 8), dtype=torch.float64, device='cuda')
        ll = torch.empty((3, N), dtype=torch.float64, device='cuda')
        drawn = torch.empty((R, N), dtype=torch.float64, device='cuda')

        def floor():
            _lib.check(L.smart_objfn_hip(N, R, sim.data_ptr(), N, obs.data_ptr(), None, float('nan'), objfn.data_ptr(),
                                         stream))

        def loglik():
            _lib.check(L.smart_error_model_loglik_hip(N, R, sim.data_ptr(), N, obs.data_ptr(), theta.data_ptr(), 3,
                                                      ll.data_ptr(), stream))

        def draw():
            _lib.check(L.smart_error_model_draw_hip(N, R, 1, sim.data_ptr(), N, theta.data_ptr(), 3, 0, 0, 1,
                                                    drawn.data_ptr(), N, stream))

        ms_f = timed(floor, args.reps)
        row(N, 'smart_objfn_hip (one read of the matrix)', ms_f)
        ms = timed(loglik, args.reps)
        row(N, 'smart_error_model_loglik_hip', ms, '  (%.2f x smart_objfn_hip)' % (ms / ms_f))
        ref = torch_loglik(sim, obs, theta)
        err = float(((ll - ref).abs() / ref.abs().clamp_min(1.0)).max())
        del ref
        ms_t = timed(lambda: torch_loglik(sim, obs, theta), args.torch_reps)
        row(N, 'torch statement of the likelihood', ms_t,
            '  (%.2f x smart_error_model_loglik_hip; faster: %s; largest relative difference %.1e)'
            % (ms_t / ms, 'the kernel' if ms < ms_t else 'THE TORCH STATEMENT', err))
        ms_d = timed(draw, args.reps)
        row(N, 'smart_error_model_draw_hip (one replicate, truncated)', ms_d, '  (reads R * N * 8 bytes, writes as many)')
        other = torch.empty_like(drawn)
        ms_td = timed(lambda: torch_draws(sim, theta, other), args.torch_reps)
        row(N, 'torch statement of the draws (randn, a loop over the steps)', ms_td,
            '  (%.2f x smart_error_model_draw_hip; faster: %s)'
            % (ms_td / ms_d, 'the kernel' if ms_d < ms_td else 'THE TORCH STATEMENT'))
        del sim, drawn, other
    if args.chains:
        from smartpy_amd import engine
        from smartpy_amd.montecarlo import DEMCz
        root = tempfile.mkdtemp(prefix='smart_error_model_')
        try:
            shutil.copytree(os.path.join(ROOT, 'tests', 'golden', 'data', 'in'), os.path.join(root, 'in'))
            with open(os.path.join(root, 'in', 'Catchment', 'Catchment.bench.sttngs'), 'w') as f:
                f.write(SETTINGS)
            lines.append('One DE-MCz generation of %d chains on the example catchment (ten years of daily steps), as '
                         'montecarlo.DEMCz.run() performs it; wall clock, median of %d' % (args.chains, args.reps))
            walls = {}
            for likelihood in ('gaussian', 'ar1'):
                torch.cuda.empty_cache()
                obj = DEMCz('Catchment', root, 'csv', 'csv', chains=args.chains, generations=10, thin=5, seed=0,
                            likelihood=likelihood, settings_filename='Catchment.bench.sttngs')
                obj.model.extra = EXTRA
                state = obj._new_state(obj.initial_population, 3 + args.reps, engine.default_device())
                scores, payload = obj._launch_chains(state)
                demcz.demcz_step(state, scores=scores, carry_new=payload, append=True, propose=True)

                def generation():
                    sc, pl = obj._launch_chains(state)
                    demcz.demcz_step(state, scores=sc, carry_new=pl, append=True, propose=True)
                walls[likelihood] = walled(generation, args.reps)
                lines.append("%8d  likelihood='%s', %d dimensions: %.3f ms a generation%s"
                             % (args.chains, likelihood, state.n_dims, walls[likelihood],
                                '' if likelihood == 'gaussian' else '  (%.2f x gaussian)' % (walls['ar1'] / walls['gaussian'])))
                print(lines[-1], flush=True)
                del state, obj
        finally:
            shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
