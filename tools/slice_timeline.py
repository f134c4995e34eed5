#!/usr/bin/env python3
"""Where the workgroups of the headline's time-sliced launch are over time: one launch of a -DSMART_SLICE_TIMELINE build.

That build (never the installed library; it is loaded through SMART_AMD_LIB like the other variants) has every sliced
workgroup leave five words behind everything else in the workspace: its ticket, its hardware id (HW_ID, XCC_ID), and the
constant 100 MHz counter (s_memrealtime) when it starts, when its predecessor's hand-over is there, and when it ends.

    python tools/build_variants.py timeline=-DSMART_SLICE_TIMELINE
    SMART_AMD_LIB=tools/variants/libsmart_amd_timeline.so python tools/slice_timeline.py [--samples N] [--no-discharge]
    SMART_SLICE_TAPER=0 SMART_AMD_LIB=... python tools/slice_timeline.py          # the equal cuts, for comparison

Prints: the SIMDs with a running wave over the last 5 % of the launch; the idle SIMD-time of that drain as a share of the
launch; how long slices wait (and how long after their predecessor's end they get going); running waves per SIMD over the
launch.  The stamps cost a few stores per slice, outside the time loop.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
import bench                                                        # noqa: E402
from smartpy_amd import _lib, engine                                # noqa: E402
from smartpy_amd.parameters import Parameters                       # noqa: E402
from smartpy_amd.sampling import latin_hypercube                    # noqa: E402

FIELDS, MAX_SLICES = 5, 64      # kTimelineFields, kTimelineSlices of smart_device.h
TICK_US = 0.01                  # s_memrealtime counts at 100 MHz


def pct(x, qs=(50, 90, 99, 100)):
    return '  '.join('p%d %.2f' % (q, np.percentile(x, q)) for q in qs)


def summarise(rec, n_seg, seg_blocks, out=print):
    """rec: uint64 [seg_blocks * MAX_SLICES, FIELDS], as the launch left it"""
    n = min(n_seg, MAX_SLICES) * seg_blocks
    rec = rec[:n].astype(np.int64)
    ticket, hw, start, woke, end = rec.T
    assert (end > 0).all() and (ticket == np.arange(n)).all(), 'a slice left no record: not a timeline build, or not a sliced launch'
    seg = ticket // seg_blocks
    run = np.where(seg > 0, woke, start)             # first instruction of the slice's own work
    t0, t1 = start.min(), end.max()
    span = float(t1 - t0)
    simd = ((hw >> 32) & 0xf) << 16 | ((hw >> 8) & 0xff) << 8 | ((hw >> 4) & 0x3)      # XCC | SE, SH, CU | SIMD
    keys, simd = np.unique(simd, return_inverse=True)
    n_simd = len(keys)
    out('launch: %d slices x %d blocks, %.3f ms from the first start to the last end, %d SIMDs seen'
        % (n_seg, seg_blocks, span * TICK_US * 1e-3, n_simd))
    length = (end - run) * TICK_US
    for s in sorted(set([0, n_seg // 2, n_seg - 2, n_seg - 1])):
        out('  slice %2d: run time us  %s' % (s, pct(length[seg == s])))

    def busy_at(t):
        on = (run <= t) & (t < end)
        return np.bincount(simd[on], minlength=n_simd)

    out('SIMDs with a running wave over the last 5 %% of the launch (of %d):' % n_simd)
    for frac in np.linspace(0.95, 1.0, 21)[:-1]:
        out('  at %.4f of the launch: %4d' % (frac, int((busy_at(t0 + frac * span) > 0).sum())))
    last_end = np.zeros(n_simd, dtype=np.int64)
    np.maximum.at(last_end, simd, end)
    drain = (t1 - last_end).sum() / (n_simd * span)
    out('idle SIMD-time of the drain (from a SIMD\'s last end to the launch\'s), share of the launch: %.2f %%' % (100 * drain))
    first_run = np.full(n_simd, t1, dtype=np.int64)
    np.minimum.at(first_run, simd, run)
    out('idle SIMD-time of the ramp (from the launch\'s start to a SIMD\'s first running wave), share: %.2f %%'
        % (100 * (first_run - t0).sum() / (n_simd * span)))
    later = seg > 0
    out('wait of a slice for its predecessor, us:  %s' % pct((woke - start)[later] * TICK_US))
    pred_end = end[ticket[later] - seg_blocks]
    polling = start[later] < pred_end               # resident before the predecessor ended: what the poll interval delays
    lag = (woke[later] - pred_end)[polling] * TICK_US
    out('  %d of %d were resident before their predecessor ended; from its end to their first step, us:  %s'
        % (int(polling.sum()), int(later.sum()), pct(lag)))
    out('  the hand-overs of a chain add up to (mean over chains) %.1f us = %.2f %% of the launch'
        % (lag.sum() / seg_blocks, 100 * lag.sum() / seg_blocks / (span * TICK_US)))
    out('running waves per SIMD, sampled at 50 points of the launch\'s first 95 %:')
    counts = np.stack([busy_at(t0 + f * span) for f in np.linspace(0.02, 0.95, 50)])
    out('  mean %.3f;  SIMDs with 0: %.1f %%  1: %.1f %%  2: %.1f %%  3 or more: %.1f %%'
        % (counts.mean(), *(100 * (counts == k).mean() for k in (0, 1, 2)), 100 * (counts >= 3).mean()))
    return {'ms': span * TICK_US * 1e-3, 'drain': drain}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--samples', type=int, default=100000)
    ap.add_argument('--no-discharge', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    forcing, rng = bench.synthetic_forcing(0, hourly=True)
    T, W, gap = forcing.shape[0], bench.WARM_DAYS * 24, 24
    so, _ = bench.load_oracle()
    truth, _ = bench.truth_discharge(so, forcing, 3600.0, T, W, gap, True, so is None)
    obs = bench.synthetic_observations(truth, rng, T // gap)
    params = latin_hypercube(args.samples, Parameters().ranges, seed=2718)
    prep = engine.prepare_ensemble(params, forcing, bench.AREA, 3600.0, W, gap, extra=bench.EXTRA, obs=obs,
                                   gw_obs=bench.GW_OBS, want_discharge=not args.no_discharge, device=dev)
    what = prep.describe()
    print('# %s\n# %s, SMART_SLICE_TAPER=%s' % (what, os.path.basename(_lib.LIB_PATH), os.environ.get('SMART_SLICE_TAPER', 'unset')))
    if ' slices x ' not in what:
        raise SystemExit('not a time-sliced launch')
    n_seg = int(what.split('[')[1].split(' slices')[0])
    seg_blocks = int(what.split(' slices x ')[1].split(' blocks')[0])
    words = seg_blocks * MAX_SLICES * FIELDS
    ws = prep._ws.view(torch.int64)
    assert ws.numel() * 8 == (prep._e.workspace_bytes + 7) // 8 * 8 and ws.numel() > words
    tail = ws[prep._e.workspace_bytes // 8 - words:prep._e.workspace_bytes // 8]
    for _ in range(3):              # (the first launch of a process also sizes the residency cap)
        prep.launch()
    torch.cuda.synchronize()
    tail.zero_()
    prep.launch()
    torch.cuda.synchronize()
    assert prep.status() == 0
    summarise(tail.cpu().numpy().view(np.uint64).reshape(-1, FIELDS), n_seg, seg_blocks)


if __name__ == '__main__':
    main()
