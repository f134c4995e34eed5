#!/usr/bin/env python3
"""What a late gauge costs: the bench's headline ensemble (hourly, ten years, a daily report, fused objective functions)
with the observations beginning at report 0, halfway through the record and ten reports before its end.  The reports up
to the first observed one are the ones that may set the constant of the one-pass moments; the interval engine takes them
one interval at a time (interval_loop_obs: no group prefetch) and the every-step kernel outside its stream, so the time
may grow with r1.  Three legs: discharge stored, objective functions only, a report every step.  The variants alternate,
ROUNDS times; one JSON line per leg with every run's mean launch time in ms.

    python tools/bench_late_gauge.py [samples] [launches per run]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                        # noqa: E402
from smartpy_amd import engine                      # noqa: E402
from smartpy_amd.parameters import Parameters       # noqa: E402
from smartpy_amd.sampling import latin_hypercube    # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
LAUNCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ROUNDS = 3
dev = torch.device('cuda')
forcing, rng = bench.synthetic_forcing(0, hourly=True)
gap, W = 24, bench.WARM_DAYS * 24
R = forcing.shape[0] // gap                        # (the warm-up runs over the first W steps of the same forcing)
params = torch.from_numpy(latin_hypercube(N, Parameters().ranges, seed=2718)).to(dev)
d_forcing = torch.from_numpy(forcing).to(dev)
base = np.abs(rng.normal(2.0, 1.0, R)) + 0.01
base[rng.random(R) < 0.12] = np.nan
base[[0, R // 2, R - 10]] = 2.0
FIRST = {'report 0': 0, 'halfway': R // 2, 'ten before the end': R - 10}


def prepared(r1, leg):
    obs = base.copy()
    obs[:r1] = np.nan
    kw = dict(extra=bench.EXTRA, math_mode='fast', device=dev, gw_obs=bench.GW_OBS)
    if leg == 'every':
        return engine.prepare_ensemble(params, d_forcing, bench.AREA, 3600.0, W, 1, obs=np.repeat(obs, gap),
                                       want_discharge=False, **kw)
    return engine.prepare_ensemble(params, d_forcing, bench.AREA, 3600.0, W, gap, obs=obs,
                                   want_discharge=leg == 'stored', **kw)


def mean_ms(prep):
    for _ in range(2):
        prep.launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        prep.launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


for leg in ('stored', 'objectives_only', 'every'):
    preps = {name: prepared(r1, leg) for name, r1 in FIRST.items()}
    runs = {name: [] for name in FIRST}
    for _ in range(ROUNDS):
        for name in FIRST:
            runs[name].append(round(mean_ms(preps[name]), 4))
    print(json.dumps({'leg': leg, 'samples': N, 'reports': R * (gap if leg == 'every' else 1),
                      'kernel': preps['report 0'].describe(), 'first observed report': FIRST, 'ms': runs}), flush=True)
    del preps
