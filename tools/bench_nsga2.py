#!/usr/bin/env python3
"""Time of one NSGA-II generation on ten years of daily data (the example catchment of tests/golden/data, 3,653 steps), per
population size and number of objectives: the step call (smart_nsga2_step_hip: rank parents and offspring, keep the N
best, make the next offspring), the prepared model launch alone (objective functions, no stored discharge), the whole
generation as montecarlo.NSGA2.run() performs it (wall clock: launch preparation, launch, payload, step), a torch
statement of the same selection on the same tensors (chunked broadcast dominance, a peel loop with one host read per
front, sort-based crowding, a lexicographic sort, gathers -- the same work, not the same bits), and the step on the chain
input (objective 2 equal to objective 1: one front per distinct value).  The calls are timed with HIP events around every
call, warm-up first, the MEDIAN of the repeated calls; the generation by the wall clock with a synchronisation at its end.
Writes one text file (default profiles/nsga2.txt).

    python tools/bench_nsga2.py [--out FILE] [--sizes 1024,4096,8192] [--objectives 2,3] [--reps 5]
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
from smartpy_amd import engine, nsga2, structure      # noqa: E402
from smartpy_amd.montecarlo import NSGA2              # noqa: E402

EXTRA = {'aar': 1200, 'r-o_ratio': 0.45, 'r-o_split': (0.10, 0.15, 0.15, 0.30, 0.30)}
SETTINGS = ('ARGUMENT,VALUE\ncatchment_area_km2,175.46\ngauged_area_km2,175.97\nstart_datetime,01/01/2007 09:00:00\n'
            'end_datetime,31/12/2016 09:00:00\nsimu_timedelta_min,1440\nreport_timedelta_min,1440\nwarm_up_days,365\n'
            'gw_constraint,0.12667\n')
OBJECTIVES = ['NSE', 'PBias', 'KGE', 'RMSE']
BEYOND = 2 ** 31 - 2


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


def torch_selection(keys, x, carry, N, chunk=2048):
    """The same selection over E candidates as torch operations -> (the survivors' x, keys, carry, ranks; fronts peeled)"""
    E, M = keys.shape
    dev = keys.device
    dom = torch.empty((E, E), dtype=torch.bool, device=dev)                # dom[j][i]: j dominates i
    for j0 in range(0, E, chunk):
        a = keys[j0:j0 + chunk, None, :]
        dom[j0:j0 + chunk] = (a >= keys[None, :, :]).all(dim=2) & ~(a <= keys[None, :, :]).all(dim=2)
    count = dom.sum(dim=0, dtype=torch.int32)
    alive = ~torch.isnan(keys).any(dim=1)
    rank = torch.where(alive, BEYOND, BEYOND + 1).to(torch.int32)
    ranked = fronts = 0
    while ranked < N:
        front = alive & (count == 0)
        n = int(front.sum())                                                # the host read of this front
        if n == 0:
            break
        fronts += 1
        rank[front] = fronts
        alive &= ~front
        count -= dom[front].sum(dim=0, dtype=torch.int32)
        ranked += n
    dist = torch.zeros(E, dtype=torch.float64, device=dev)
    for m in range(M):
        by_key = torch.argsort(keys[:, m], stable=True)
        order = by_key[torch.argsort(rank[by_key], stable=True)]           # by rank, then by key m
        k, r = keys[order, m], rank[order]
        first = torch.ones(E, dtype=torch.bool, device=dev)
        first[1:] = r[1:] != r[:-1]
        last = torch.ones(E, dtype=torch.bool, device=dev)
        last[:-1] = first[1:]
        lowest = torch.full((E + 2,), float('inf'), dtype=torch.float64, device=dev)
        highest = torch.full((E + 2,), float('-inf'), dtype=torch.float64, device=dev)
        slot = torch.clamp(r.long(), max=E + 1)
        lowest.scatter_reduce_(0, slot, k, 'amin')
        highest.scatter_reduce_(0, slot, k, 'amax')
        inner = torch.zeros(E, dtype=torch.float64, device=dev)
        inner[1:-1] = (k[2:] - k[:-2]) / (highest[slot] - lowest[slot])[1:-1]
        term = torch.where(first | last, torch.full_like(inner, float('inf')), inner)
        dist[order] += torch.where(r < BEYOND, term, torch.zeros_like(term))
    order = torch.argsort(-dist, stable=True)
    order = order[torch.argsort(rank[order], stable=True)][:N]             # rank, then distance, then e
    return x[order], keys[order], carry[order], rank[order], fronts


def prepared_launch(obj, rows):
    """The launch NSGA2 makes per generation (smart.SMART.simulate_ensemble's arguments), prepared once"""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nsga2.txt'))
    ap.add_argument('--sizes', default='1024,4096,8192')
    ap.add_argument('--objectives', default='2,3')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    root = tempfile.mkdtemp(prefix='smart_nsga2_')
    lines = []

    def row(N, M, what, ms, note=''):
        lines.append('%6d %2d  %-66s %10.3f  %s' % (N, M, what, ms, note))
        print(lines[-1], flush=True)

    try:
        shutil.copytree(os.path.join(ROOT, 'tests', 'golden', 'data', 'in'), os.path.join(root, 'in'))
        with open(os.path.join(root, 'in', 'Catchment', 'Catchment.bench.sttngs'), 'w') as f:
            f.write(SETTINGS)
        for N in [int(s) for s in args.sizes.split(',')]:
            for M in [int(s) for s in args.objectives.split(',')]:
                obj = NSGA2('Catchment', root, 'csv', 'csv', OBJECTIVES[:M], population=N, generations=10, seed=0,
                            settings_filename='Catchment.bench.sttngs')
                obj.model.extra = EXTRA
                steps = len(obj.model.timeseries) - 1
                if not lines:
                    lines += ['One NSGA-II generation of a population of [N] rows, [M] objectives (%s ...), on %d daily steps, '
                              'ten parameters, fp64; ms (HIP events around each call, prepared, warm-up, median of %d; the '
                              'generation: wall clock)' % (', '.join(OBJECTIVES[:2]), steps, args.reps),
                              'device: %s' % torch.cuda.get_device_name(),
                              '%6s %2s  %-66s %10s  %s' % ('N', 'M', 'what', 'ms', 'note')]
                    print('\n'.join(lines), flush=True)
                device = engine.default_device()
                state = obj._new_state(obj.initial_population, device)
                for g in range(3):          # three generations in: parents and offspring, a population that has moved
                    table, payload, eligible = obj._launch_population(state)
                    nsga2.nsga2_step(state, scores=table, carry_new=payload, vary=True)
                table, payload, _ = obj._launch_population(state)
                table, payload = table.clone(), payload.clone()
                ms_step = timed(lambda: nsga2.nsga2_step(state, scores=table, carry_new=payload, vary=True), args.reps)
                counts = state.counts.cpu().numpy()
                row(N, M, 'smart_nsga2_step_hip: survive + vary', ms_step,
                    'fronts peeled %d, rank 1: %d of %d candidates' % (counts[0], counts[1], 2 * N))
                ms_vary = timed(lambda: nsga2.nsga2_step(state, vary=True), args.reps)
                row(N, M, '... the vary phase alone', ms_vary)
                # the torch statement on the same 2 N candidates: the parents' keys, the offspring's from the table
                cols, code, target = nsga2.directions_of(obj.objectives)
                picked = table[:, torch.from_numpy(cols).long().to(device)]
                fresh = torch.stack([picked[:, m] if code[m] == 0 else (-picked[:, m] if code[m] == 1 else
                                                                        -(picked[:, m] - target[m]).abs())
                                     for m in range(M)], dim=1)
                keys = torch.cat([state.keys, fresh])
                xs = torch.cat([state.x, state.offspring])
                carry = torch.cat([state.carry, payload])
                ms_torch = timed(lambda: torch_selection(keys, xs, carry, N), args.reps)
                fronts = torch_selection(keys, xs, carry, N)[4]
                faster = 'the kernels' if ms_step < ms_torch else 'THE TORCH STATEMENT'
                row(N, M, 'torch statement of the selection (broadcast, peel loop, sorts)', ms_torch,
                    '%d fronts; %.1f x the time of smart_nsga2_step_hip; faster: %s' % (fronts, ms_torch / ms_step, faster))
                prep = prepared_launch(obj, state.rows)
                ms_launch = timed(prep.enqueue, args.reps)
                shorter = 'the step is SHORTER than the launch' if ms_step < ms_launch else 'the step is LONGER than the launch'
                row(N, M, 'prepared model launch alone (objective functions)', ms_launch, shorter + '; ' + prep.describe())

                def generation():
                    tb, pl, el = obj._launch_population(state)
                    nsga2.nsga2_step(state, scores=tb, carry_new=pl, eligible=el, vary=True)
                ms_gen = walled(generation, args.reps)
                rest = ms_gen - ms_launch - ms_step
                row(N, M, 'one generation as NSGA2.run() performs it (wall)', ms_gen,
                    'launch %.0f %%, step %.0f %%, the rest (the per-call preparation of the engine, the payload) %.0f %%'
                    % (100 * ms_launch / ms_gen, 100 * ms_step / ms_gen, 100 * rest / ms_gen))
                # the chain: every objective equal to objective 1, one front per distinct value
                chain = table.clone()
                for m in range(1, M):
                    chain[:, int(cols[m])] = chain[:, int(cols[0])]
                state.direction[:] = 0
                nsga2.nsga2_step(state, scores=chain, carry_new=payload, vary=True)
                ms_chain = timed(lambda: nsga2.nsga2_step(state, scores=chain, carry_new=payload, vary=True), args.reps)
                row(N, M, 'smart_nsga2_step_hip on the chain input (every objective = objective 1)', ms_chain,
                    'fronts peeled %d' % int(state.counts[0]))
                del state, prep, obj, keys, xs, carry
                torch.cuda.empty_cache()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
