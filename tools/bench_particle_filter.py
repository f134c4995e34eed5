#!/usr/bin/env python3
"""Time of one assimilation window of the particle filter on ten years of daily data (the example catchment of
tests/golden/data, 3,653 steps), per number of particles and window length: the step call (smart_particle_step_hip: weigh,
quantise, decide, resample, move) where it resamples and where it does not, the prepared window launch alone (stored
discharge, final states, started from the particles' states), the same launch prepared each time as run() makes it (the
difference is the engine's per-call preparation), the two quantile calls, the whole window as
montecarlo.ParticleFilter.run() performs it (wall clock: the engine's per-call preparation, launch, copies, quantiles, step),
and a torch statement of the step on the same tensors (sums, exp, cumsum, searchsorted, gathers, rand, clamp -- the same
work, not the same bits).  The calls are timed with HIP events around every call, warm-up first, the MEDIAN of the repeated
calls; the window by the wall clock with a synchronisation at its end.  Writes one text file (default
profiles/particle_filter.txt).

    python tools/bench_particle_filter.py [--out FILE] [--sizes 10000,100000] [--every 1,30] [--reps 5]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smartpy_amd import engine, particle      # noqa: E402
from smartpy_amd.montecarlo import ParticleFilter              # noqa: E402

EXTRA = {'aar': 1200, 'r-o_ratio': 0.45, 'r-o_split': (0.10, 0.15, 0.15, 0.30, 0.30)}
SETTINGS = ('ARGUMENT,VALUE\ncatchment_area_km2,175.46\ngauged_area_km2,175.97\nstart_datetime,01/01/2007 09:00:00\n'
            'end_datetime,31/12/2016 09:00:00\nsimu_timedelta_min,1440\nreport_timedelta_min,1440\nwarm_up_days,365\n'
            'gw_constraint,0.12667\n')


def timed(fn, reps):
    """warm-up, then `reps` calls each between two HIP events -> median ms"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def walled(fn, reps):
    """warm-up, then `reps` calls by the wall clock, the device idle before and after each -> median ms"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def torch_step(s, sim, obs, columns, lo, hi, scale, noise, resample):
    """The same step as torch operations -> (rows, states, logw)"""
    N = s.n_particles
    seen = ~torch.isnan(obs)
    sigma = s.sigma0 + s.sigma1 * obs[seen].abs()
    r = (sim[seen, :N] - obs[seen, None]) / sigma[:, None]
    logw = s.logw - 0.5 * (r * r).sum(dim=0)
    w = torch.exp(logw - logw.max())
    if resample:
        C = torch.cumsum(w, dim=0)
        t = (torch.arange(N, dtype=torch.float64, device=w.device) + torch.rand((), dtype=torch.float64, device=w.device)) \
            * (C[-1] / N)
        parents = torch.searchsorted(C, t).clamp_(max=N - 1)
        logw = torch.zeros_like(logw)
    else:
        parents = torch.arange(N, device=w.device)
    rows = s.rows[parents]
    y = rows[:, columns] + scale * (2.0 * torch.rand((N, len(columns)), dtype=torch.float64, device=w.device) - 1.0)
    y = torch.where(y < lo, 2.0 * lo - y, y)
    y = torch.where(y > hi, 2.0 * hi - y, y)
    inside = ((y >= lo) & (y <= hi)).all(dim=1, keepdim=True)
    rows[:, columns] = torch.where(inside, y, rows[:, columns])
    states = s.states[parents] * (1.0 + noise * (2.0 * torch.rand((N, 12), dtype=torch.float64, device=w.device) - 1.0))
    cap = ((rows[:, s.z_column] / 6.0) / 1e3 * s.area_m2)[:, None]
    states[:, 5:11] = torch.minimum(states[:, 5:11], cap)
    return rows, states, logw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'particle_filter.txt'))
    ap.add_argument('--sizes', default='10000,100000')
    ap.add_argument('--every', default='1,30')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    root = tempfile.mkdtemp(prefix='smart_pf_')
    lines = []

    def row(N, A, what, ms, note=''):
        lines.append('%7d %3d  %-62s %10.3f  %s' % (N, A, what, ms, note))
        print(lines[-1], flush=True)

    try:
        shutil.copytree(os.path.join(ROOT, 'tests', 'golden', 'data', 'in'), os.path.join(root, 'in'))
        with open(os.path.join(root, 'in', 'Catchment', 'Catchment.bench.sttngs'), 'w') as f:
            f.write(SETTINGS)
        for N in [int(s) for s in args.sizes.split(',')]:
            for A in [int(s) for s in args.every.split(',')]:
                obj = ParticleFilter('Catchment', root, 'csv', 'csv', particles=N, assimilate_every=A, sigma=(0.3, 0.1),
                                     tau=0.5, state_noise=0.05, jitter=0.01, seed=0,
                                     settings_filename='Catchment.bench.sttngs')
                obj.model.extra = EXTRA
                axis = obj._axis()
                delta_sec, T, gap, n_warm, R = axis
                if not lines:
                    lines += ['One assimilation window of [N] particles over [A] daily report steps, on %d daily steps, ten '
                              'parameters, fp64; ms (HIP events around each call, prepared, warm-up, median of %d; the window: '
                              'wall clock)' % (T, args.reps),
                              'device: %s' % torch.cuda.get_device_name(),
                              '%7s %3s  %-62s %10s  %s' % ('N', 'A', 'what', 'ms', 'note')]
                    print('\n'.join(lines), flush=True)
                device = engine.default_device()
                model = obj.model
                forcing = model._device_forcing(device)
                obs = model._device_cache[2]
                rows = engine.as_device(obj.initial_population[:, :10], device).clone().contiguous()
                s = particle.ParticleState(rows, torch.zeros((N, 12), dtype=torch.float64, device=device), obj.lo, obj.hi,
                                           obj.columns, float(model.area), sigma=obj.sigma, tau=obj.tau,
                                           state_noise=obj.state_noise, jitter=obj.jitter, seed=0, device=device)
                spin = obj._launch_window(s, forcing, 0, n_warm, axis, None, want_discharge=False)
                s.states.copy_(spin.final_vars[:, 7:])
                r0 = 400                        # a window well inside the record
                w_obs = obs[r0:r0 + A].contiguous()
                out = obj._launch_window(s, forcing, r0 * gap, (r0 + A) * gap, axis, s.states)
                matrix = out.discharge_report_major.clone()
                s.states.copy_(out.final_vars[:, 7:])
                # ---- the step call, on both sides of the decision
                figures = {}
                for tau, word in ((2.0, 'resampled'), (0.0, 'not resampled')):
                    s.tau = tau
                    s.logw.zero_(), s.logw_next.zero_()
                    ms = timed(lambda: particle.particle_step(s, matrix, w_obs), args.reps)
                    figures[word] = ms
                    counts = s.counts.cpu().numpy()
                    row(N, A, 'smart_particle_step_hip, %s' % word, ms,
                        'ess %.0f, distinct parents %d' % (float(s.stats[0]), counts[2]))
                    assert bool(counts[0]) == (tau > 1.0)
                s.tau = obj.tau
                ms_step = figures['resampled']
                # ---- the torch statement on the same tensors
                cols = torch.from_numpy(s.columns.astype('int64')).to(device)
                lo, hi = torch.from_numpy(s.lo).to(device), torch.from_numpy(s.hi).to(device)
                scale, noise = torch.from_numpy(s.scale.copy()).to(device), torch.from_numpy(s.noise.copy()).to(device)
                for resample, word in ((True, 'resampled'), (False, 'not resampled')):
                    ms = timed(lambda: torch_step(s, matrix, w_obs, cols, lo, hi, scale, noise, resample), args.reps)
                    faster = 'the kernels' if figures[word] < ms else 'THE TORCH STATEMENT'
                    row(N, A, 'torch statement of the step, %s' % word, ms,
                        '%.1f x the time of smart_particle_step_hip; faster: %s' % (ms / figures[word], faster))
                # ---- the window launch alone, prepared once
                prep = engine.prepare_ensemble(s.rows.view(N, 10), forcing[r0 * gap:(r0 + A) * gap], float(model.area),
                                               delta_sec, 0, gap, initial=s.states.view(N, 12), math_mode=obj.math_mode,
                                               want_discharge=True, want_final=True, device=device)
                ms_launch = timed(prep.enqueue, args.reps)
                shorter = 'the step is SHORTER than the launch' if ms_step < ms_launch else 'the step is LONGER than the launch'
                row(N, A, 'prepared window launch alone (discharge, final states)', ms_launch, shorter + '; ' + prep.describe())
                # the engine's per-call preparation, measured directly: the launch as run() makes it (prepare, enqueue, read the
                # status word) against the enqueue of the prepared call, both by the wall clock on the same window
                ms_run = walled(lambda: obj._launch_window(s, forcing, r0 * gap, (r0 + A) * gap, axis, s.states), args.reps)
                ms_enqueue = walled(prep.enqueue, args.reps)
                ms_prep = ms_run - ms_enqueue
                row(N, A, 'the window launch as run() makes it (wall), prepared each time', ms_run,
                    'the enqueue of the prepared call alone: %.3f ms (wall); the per-call preparation: %.3f ms'
                    % (ms_enqueue, ms_prep))
                # the two quantile calls of a window: equal weights after a resampling, the step's integers for the analysis
                unit = torch.full((N,), particle.UNIT, dtype=torch.int64, device=device)
                equal, weights = unit.double(), s.q.double()
                ms_fore = timed(lambda: engine.weighted_quantiles(matrix, obj.probs, equal), args.reps)
                row(N, A, 'engine.weighted_quantiles on the window, forecast (equal weights)', ms_fore)
                ms_ana = timed(lambda: engine.weighted_quantiles(matrix, obj.probs, weights), args.reps)
                row(N, A, 'engine.weighted_quantiles on the window, analysis (the step\'s integers)', ms_ana)

                # ---- the whole window as run() performs it
                def window():
                    o = obj._launch_window(s, forcing, r0 * gap, (r0 + A) * gap, axis, s.states)
                    m = o.discharge_report_major
                    s.states.copy_(o.final_vars[:, 7:])
                    engine.weighted_quantiles(m, obj.probs, unit.double())
                    particle.particle_step(s, m, w_obs)
                    w = s.q.double()
                    engine.weighted_quantiles(m, obj.probs, w)
                    torch.where(w > 0.0, m * w, torch.zeros_like(m)).sum(dim=1) / w.sum()
                    s.stats.clone(), s.counts.clone()
                    torch.where(s.counts[0] != 0, unit, s.q)
                ms_window = walled(window, args.reps)
                verdict = 'THE PREPARATION DOMINATES' if ms_prep > 0.5 * ms_window else 'the preparation does not dominate'
                rest = ms_window - ms_run - ms_step - ms_fore - ms_ana
                left = '%.0f %% = %.3f ms' % (100 * rest / ms_window, rest) if rest > 0 else \
                    'not resolved (the calls timed alone add up to more than the window)'
                row(N, A, 'one window as ParticleFilter.run() performs it (wall)', ms_window,
                    'the per-call preparation of the engine %.0f %% = %.3f ms: %s; launch %.0f %%, step %.0f %%, quantiles (timed '
                    'alone) %.0f %%, what is left (copies, the mean, clones): %s'
                    % (100 * ms_prep / ms_window, ms_prep, verdict, 100 * ms_enqueue / ms_window, 100 * ms_step / ms_window,
                       100 * (ms_fore + ms_ana) / ms_window, left))
                del s, prep, obj, out, matrix
                torch.cuda.empty_cache()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
