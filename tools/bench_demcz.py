#!/usr/bin/env python3
"""Time of one DE-MCz generation on ten years of daily data (the example catchment of tests/golden/data, 3,653 steps), per
number of chains: the step call (smart_demcz_step_hip: accept the outstanding proposals, propose the next, with and
without the append to the archive), the prepared model launch alone (objective functions, no stored discharge), the whole
generation as montecarlo.DEMCz.run() performs it (wall clock: launch preparation, launch, payload, step), and a torch
statement of the same step on the same tensors (randint, gather, where, rand().log(), index_copy -- the same moves with
torch's own generator, so the same work but not the same bits).  The calls are timed with HIP events around every call,
warm-up first, the MEDIAN of the repeated calls; the generation by the wall clock with a synchronisation at its end.
Writes one text file (default profiles/demcz.txt).

    python tools/bench_demcz.py [--out FILE] [--sizes 10000,100000] [--reps 5]
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
from smartpy_amd import demcz, engine, structure      # noqa: E402
from smartpy_amd.montecarlo import DEMCz              # noqa: E402

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


def torch_step(s, scores, payload, tables):
    """The same step as a dozen torch operations on the tensors of the state (torch's generator: the same work, other
    bits)"""
    lo, hi, scale, gamma, columns = tables
    N, d, M = s.n_chains, s.n_dims, s.M
    dev = s.x.device
    # accept
    lstar = -((s.n_eff * 0.5) * torch.log(s.n_obs * (scores * scores)))
    u = torch.rand(N, dtype=torch.float64, device=dev)
    take = (s.out == 0) & (u.log() < lstar - s.logp)
    s.x.copy_(torch.where(take[:, None], s.proposal, s.x))
    s.logp.copy_(torch.where(take, lstar, s.logp))
    s.carry.copy_(torch.where(take[:, None], payload, s.carry))
    s.accepted.add_(take.to(torch.int32))
    # propose
    a = torch.randint(0, M, (N,), device=dev)
    b = torch.randint(0, M - 1, (N,), device=dev)
    b = b + (b >= a)
    moved = torch.rand((N, d), device=dev) < s.C / 2.0 ** 32
    none = ~moved.any(dim=1)
    moved = moved | (none[:, None] & (torch.randint(0, d, (N, 1), device=dev) == torch.arange(d, device=dev)[None, :]))
    jump = torch.rand(N, device=dev) < s.J / 2.0 ** 32
    g = torch.where(jump, torch.ones((), dtype=torch.float64, device=dev), gamma[moved.sum(dim=1) - 1])
    eps = scale * (2.0 * torch.rand((N, d), dtype=torch.float64, device=dev) - 1.0)
    y = s.x + (g[:, None] * (s.archive[a] - s.archive[b]) + eps)
    y = torch.where(y < lo, 2.0 * lo - y, y)
    y = torch.where(y > hi, 2.0 * hi - y, y)
    out = (moved & ~((y >= lo) & (y <= hi))).any(dim=1)
    s.proposal.copy_(torch.where(moved, y, s.x))
    s.out.copy_(out.to(torch.uint8))
    s.rows.index_copy_(1, columns, torch.where(out[:, None], s.x, s.proposal))


def prepared_launch(obj, rows):
    """The launch DEMCz makes per generation (smart.SMART.simulate_ensemble's arguments), prepared once"""
    m = obj.model
    device = rows.device
    delta_sec = m.delta_simu.total_seconds()
    T = len(m.timeseries) - 1
    n_warm = structure.warm_up_length(m.warm_up, delta_sec, T) if m.warm_up != 0 else 0
    gap = T // (len(m.timeseries_report) - 1)
    forcing = m._device_forcing(device)
    return engine.prepare_ensemble(rows, forcing, float(m.area), delta_sec, n_warm, gap, extra=m.extra or None,
                                   obs=m._device_cache[2], gw_obs=obj.constraints['gw'], math_mode=obj.math_mode,
                                   want_discharge=False, want_objfn=True, device=device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'demcz.txt'))
    ap.add_argument('--sizes', default='10000,100000')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    root = tempfile.mkdtemp(prefix='smart_demcz_')
    lines = []

    def row(N, what, ms, note=''):
        lines.append('%8d  %-62s %10.3f  %s' % (N, what, ms, note))
        print(lines[-1], flush=True)

    try:
        shutil.copytree(os.path.join(ROOT, 'tests', 'golden', 'data', 'in'), os.path.join(root, 'in'))
        with open(os.path.join(root, 'in', 'Catchment', 'Catchment.bench.sttngs'), 'w') as f:
            f.write(SETTINGS)
        for N in [int(s) for s in args.sizes.split(',')]:
            obj = DEMCz('Catchment', root, 'csv', 'csv', chains=N, generations=10, thin=5, seed=0,
                        settings_filename='Catchment.bench.sttngs')
            obj.model.extra = EXTRA
            steps = len(obj.model.timeseries) - 1
            if not lines:
                lines += ['One DE-MCz generation of [N] chains on %d daily steps (%d observed), ten parameters, fp64; ms '
                          '(HIP events around each call, prepared, warm-up, median of %d; the generation: wall clock)'
                          % (steps, obj.n_obs, args.reps),
                          'device: %s' % torch.cuda.get_device_name(),
                          '%8s  %-62s %10s  %s' % ('N', 'what', 'ms', 'note')]
                print('\n'.join(lines), flush=True)
            device = engine.default_device()
            state = obj._new_state(obj.initial_population, 3 + 4 * (args.reps + 1), device)
            scores, payload = obj._launch_chains(state)
            demcz.demcz_step(state, scores=scores, carry_new=payload, append=True, propose=True)
            scores, payload = obj._launch_chains(state)
            scores, payload = scores.clone(), payload.clone()
            ms_step = timed(lambda: demcz.demcz_step(state, scores=scores, carry_new=payload, propose=True), args.reps)
            row(N, 'smart_demcz_step_hip: accept + propose', ms_step)
            ms_app = timed(lambda: demcz.demcz_step(state, scores=scores, carry_new=payload, append=True, propose=True),
                           args.reps)
            row(N, 'smart_demcz_step_hip: accept + append + propose', ms_app, 'archive rows %d' % state.M)
            table = obj._launch_chains(state)[1][:, :8].contiguous()
            ms_col = timed(lambda: demcz.demcz_step(state, scores=table[:, 6], carry_new=payload, propose=True), args.reps)
            row(N, '... the score read in place at stride 8', ms_col)
            tables = (torch.from_numpy(state.lo).to(device), torch.from_numpy(state.hi).to(device),
                      torch.from_numpy(state.scale).to(device), torch.from_numpy(state.gamma).to(device),
                      torch.from_numpy(state.columns).to(device).long())
            ms_torch = timed(lambda: torch_step(state, scores, payload, tables), args.reps)
            faster = 'the kernels' if ms_step < ms_torch else 'THE TORCH STATEMENT'
            row(N, 'torch statement of the step (randint, gather, where, log)', ms_torch,
                '%.1f x the time of smart_demcz_step_hip; faster: %s' % (ms_torch / ms_step, faster))
            prep = prepared_launch(obj, state.rows)
            ms_launch = timed(prep.enqueue, args.reps)
            row(N, 'prepared model launch alone (objective functions)', ms_launch, prep.describe())
            state = obj._new_state(obj.initial_population, 3 + args.reps, device)
            scores, payload = obj._launch_chains(state)
            demcz.demcz_step(state, scores=scores, carry_new=payload, append=True, propose=True)

            def generation():
                sc, pl = obj._launch_chains(state)
                demcz.demcz_step(state, scores=sc, carry_new=pl, append=True, propose=True)
            ms_gen = walled(generation, args.reps)
            rest = ms_gen - ms_launch - ms_app
            row(N, 'one generation as DEMCz.run() performs it (wall)', ms_gen,
                'launch %.0f %%, step %.0f %%, the rest (the per-call preparation of the engine: classification, plan '
                'read-back, row sort, allocation; the payload) %.0f %%%s'
                % (100 * ms_launch / ms_gen, 100 * ms_app / ms_gen, 100 * rest / ms_gen,
                   ' -- THE PREPARATION DOMINATES' if rest > ms_launch + ms_app else ''))
            del state, prep, obj
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
