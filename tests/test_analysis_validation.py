"""The refusals of seven matrix-analysis entries of the C ABI (smart_objfn_hip, smart_weighted_quantiles_hip,
smart_objfn_windows_hip, smart_flow_duration_hip, smart_sobol_indices_hip, smart_signatures_hip,
smart_objfn_bootstrap_hip) and of their capacity / workspace entries (the entries that came later hold theirs in their own
host tests):
return code and smart_last_error() text of every refusal branch, as literals.  Validation comes before the device, so
none of these calls needs one, and none dereferences a device pointer (FAKE is never read; the probability lists, which
the host reads, are real arrays).

A row is (entry, what differs from the entry's valid call, return code, text).  Rows that break two rules at once pin the
precedence: which refusal wins.  The pairs were recorded from the library as it stood before the entries moved into a
unit of their own -- those of the signatures and of the bootstrap before the size rules of the entries were folded into
one form; they are the contract both moves had to keep, byte for byte."""
import ctypes

import pytest

from smartpy_amd import _lib

E_NULL, E_SIZE, E_MODE = -1, -2, -7
FAKE = 0x1000                       # a non-NULL address that no refusal path reads
NAN, INF = float('nan'), float('inf')
TWO31 = 2 ** 31

O, Q, W, F, S, G, B = ('smart_objfn_hip', 'smart_weighted_quantiles_hip', 'smart_objfn_windows_hip',
                       'smart_flow_duration_hip', 'smart_sobol_indices_hip', 'smart_signatures_hip',
                       'smart_objfn_bootstrap_hip')


def doubles(*values):
    return (ctypes.c_double * len(values))(*values)


# the valid call of every entry, in the order of its C parameters
VALID = {
    'smart_objfn_hip': dict(n_samples=4, n_reports=3, sim=FAKE, ld=4, obs=FAKE, gw_sim=None, gw_obs=0.0, objfn=FAKE,
                            stream=None),
    'smart_weighted_quantiles_hip': dict(n_samples=4, n_reports=3, sim=FAKE, ld=4, weights=None, probs=(0.5, 1.0),
                                         n_probs=2, out=FAKE, method=0, stream=None),
    'smart_objfn_windows_hip': dict(n_samples=4, n_reports=3, sim=FAKE, ld=4, obs=FAKE, window=FAKE, n_windows=2,
                                    transform=0, eps=0.0, objfn=FAKE, stream=None),
    'smart_flow_duration_hip': dict(n_samples=4, n_reports=3, sim=FAKE, ld=4, obs=FAKE, window=FAKE, n_windows=2,
                                    probs=(0.0, 0.5), n_probs=2, quant=FAKE, transform=0, eps=0.0, seg_lo=0.0, seg_hi=1.0,
                                    objfn=None, workspace=None, workspace_bytes=0, method=0, stream=None),
    'smart_sobol_indices_hip': dict(n_base=8, n_params=2, n_rows=3, y=FAKE, ld=32, s1=FAKE, st=FAKE, moments=FAKE,
                                    counts=None, n_resamples=0, s1_std=None, st_std=None, workspace=None,
                                    workspace_bytes=0, stream=None),
    'smart_signatures_hip': dict(n_samples=4, n_reports=3, sim=FAKE, ld=4, obs=FAKE, window=FAKE, n_windows=2, alpha=0.925,
                                 pulse=FAKE, sig=FAKE, stream=None),
    'smart_objfn_bootstrap_hip': dict(n_samples=4, n_reports=3, sim=FAKE, ld=4, obs=FAKE, window=FAKE, n_windows=2,
                                      transform=0, eps=0.0, counts=FAKE, n_resamples=4, probs=(0.05, 0.5), n_probs=2,
                                      point=FAKE, stats=FAKE, replicates=None, workspace=FAKE, workspace_bytes=1 << 30,
                                      stream=None),
    'smart_flow_duration_workspace_bytes': dict(n_reports=10, n_windows=2, with_objfn=1),
    'smart_sobol_workspace_bytes': dict(n_base=8, n_params=2, n_rows=3, n_resamples=4),
    'smart_bootstrap_workspace_bytes': dict(n_samples=4, n_windows=2, n_resamples=4, with_replicates=0),
    'smart_quantiles_sort_capacity': {}, 'smart_objfn_max_windows': {}, 'smart_flow_duration_sort_capacity': {},
    'smart_sobol_max_resamples': {}, 'smart_sobol_lds_capacity': {}, 'smart_bootstrap_max_windows': {},
    'smart_bootstrap_max_resamples': {},
}
FDC_OBJFN = dict(objfn=FAKE, workspace=FAKE, workspace_bytes=1 << 20)      # the valid call with the curve's scores
SOBOL_BOOT = dict(n_resamples=4, counts=FAKE, s1_std=FAKE, st_std=FAKE)    # ... with the bootstrap


def call(entry, changes):
    """-> (what the entry returned, the text it left; None for the entries that leave none)"""
    args = dict(VALID[entry], **changes)
    assert list(args) == list(VALID[entry]), 'a change names no parameter of %s' % entry
    keep = [doubles(*v) if isinstance(v, tuple) else v for v in args.values()]
    L = _lib.lib()
    rc = getattr(L, entry)(*keep)
    return rc, (L.smart_last_error().decode() if entry.endswith('_hip') else None)


CASES = [
    # ---- smart_objfn_hip
    (O, dict(sim=None), E_NULL, 'smart_objfn_hip: sim, obs and objfn are required'),
    (O, dict(obs=None), E_NULL, 'smart_objfn_hip: sim, obs and objfn are required'),
    (O, dict(objfn=None), E_NULL, 'smart_objfn_hip: sim, obs and objfn are required'),
    (O, dict(n_samples=0), E_SIZE, 'smart_objfn_hip: need n_samples, n_reports >= 1 and ld >= n_samples'),
    (O, dict(n_reports=0), E_SIZE, 'smart_objfn_hip: need n_samples, n_reports >= 1 and ld >= n_samples'),
    (O, dict(ld=3), E_SIZE, 'smart_objfn_hip: need n_samples, n_reports >= 1 and ld >= n_samples'),
    (O, dict(obs=None, n_reports=0), E_NULL, 'smart_objfn_hip: sim, obs and objfn are required'),
    # ---- smart_weighted_quantiles_hip
    (Q, dict(sim=None), E_NULL, 'smart_weighted_quantiles_hip: sim, probs and out are required'),
    (Q, dict(probs=None), E_NULL, 'smart_weighted_quantiles_hip: sim, probs and out are required'),
    (Q, dict(out=None), E_NULL, 'smart_weighted_quantiles_hip: sim, probs and out are required'),
    (Q, dict(n_samples=0), E_SIZE,
     'smart_weighted_quantiles_hip: need n_samples, n_reports, n_probs >= 1 and ld >= n_samples'),
    (Q, dict(n_reports=0), E_SIZE,
     'smart_weighted_quantiles_hip: need n_samples, n_reports, n_probs >= 1 and ld >= n_samples'),
    (Q, dict(n_probs=0), E_SIZE,
     'smart_weighted_quantiles_hip: need n_samples, n_reports, n_probs >= 1 and ld >= n_samples'),
    (Q, dict(ld=3), E_SIZE,
     'smart_weighted_quantiles_hip: need n_samples, n_reports, n_probs >= 1 and ld >= n_samples'),
    (Q, dict(n_reports=TWO31), E_SIZE,
     'smart_weighted_quantiles_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (Q, dict(n_probs=17), E_SIZE, 'smart_weighted_quantiles_hip: 17 probabilities, at most 16 per call'),
    (Q, dict(probs=(0.0, 0.5)), E_SIZE, 'smart_weighted_quantiles_hip: probability 0 is 0, outside (0, 1]'),
    (Q, dict(probs=(0.5, 1.5)), E_SIZE, 'smart_weighted_quantiles_hip: probability 1 is 1.5, outside (0, 1]'),
    (Q, dict(probs=(NAN, 0.5)), E_SIZE, 'smart_weighted_quantiles_hip: probability 0 is nan, outside (0, 1]'),
    (Q, dict(method=3), E_MODE, "smart_weighted_quantiles_hip: method '3' unknown."),
    (Q, dict(method=1, n_samples=8193, ld=8193), E_SIZE,
     'smart_weighted_quantiles_hip: the sort form takes at most 8192 samples, not 8193'),
    (Q, dict(out=None, n_probs=0), E_NULL, 'smart_weighted_quantiles_hip: sim, probs and out are required'),
    (Q, dict(ld=3, n_reports=TWO31), E_SIZE,
     'smart_weighted_quantiles_hip: need n_samples, n_reports, n_probs >= 1 and ld >= n_samples'),
    (Q, dict(n_reports=TWO31, n_probs=17), E_SIZE,
     'smart_weighted_quantiles_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (Q, dict(n_probs=17, probs=(2.0, 0.5)), E_SIZE,
     'smart_weighted_quantiles_hip: 17 probabilities, at most 16 per call'),
    (Q, dict(probs=(0.5, -1.0), method=-1), E_SIZE,
     'smart_weighted_quantiles_hip: probability 1 is -1, outside (0, 1]'),
    (Q, dict(method=3, n_samples=8193, ld=8193), E_MODE, "smart_weighted_quantiles_hip: method '3' unknown."),
    # ---- smart_objfn_windows_hip
    (W, dict(sim=None), E_NULL, 'smart_objfn_windows_hip: sim, obs, window and objfn are required (sim is NULL)'),
    (W, dict(obs=None), E_NULL, 'smart_objfn_windows_hip: sim, obs, window and objfn are required (obs is NULL)'),
    (W, dict(window=None), E_NULL, 'smart_objfn_windows_hip: sim, obs, window and objfn are required (window is NULL)'),
    (W, dict(objfn=None), E_NULL, 'smart_objfn_windows_hip: sim, obs, window and objfn are required (objfn is NULL)'),
    (W, dict(n_samples=0), E_SIZE, 'smart_objfn_windows_hip: need n_samples, n_reports, n_windows >= 1 (got 0, 3, 2)'),
    (W, dict(n_reports=0), E_SIZE, 'smart_objfn_windows_hip: need n_samples, n_reports, n_windows >= 1 (got 4, 0, 2)'),
    (W, dict(n_windows=0), E_SIZE, 'smart_objfn_windows_hip: need n_samples, n_reports, n_windows >= 1 (got 4, 3, 0)'),
    (W, dict(ld=3), E_SIZE, 'smart_objfn_windows_hip: ld 3 is less than n_samples 4'),
    (W, dict(n_reports=TWO31), E_SIZE,
     'smart_objfn_windows_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (W, dict(n_windows=1025), E_SIZE, 'smart_objfn_windows_hip: n_windows 1025, at most 1024 per call'),
    (W, dict(eps=NAN), E_SIZE, 'smart_objfn_windows_hip: eps nan must be finite and >= 0'),
    (W, dict(eps=-1.0), E_SIZE, 'smart_objfn_windows_hip: eps -1 must be finite and >= 0'),
    (W, dict(eps=INF), E_SIZE, 'smart_objfn_windows_hip: eps inf must be finite and >= 0'),
    (W, dict(transform=4), E_MODE, "smart_objfn_windows_hip: transform '4' unknown."),
    (W, dict(transform=-1), E_MODE, "smart_objfn_windows_hip: transform '-1' unknown."),
    (W, dict(obs=None, window=None, ld=3), E_NULL,
     'smart_objfn_windows_hip: sim, obs, window and objfn are required (obs is NULL)'),
    (W, dict(n_windows=0, ld=3), E_SIZE,
     'smart_objfn_windows_hip: need n_samples, n_reports, n_windows >= 1 (got 4, 3, 0)'),
    (W, dict(ld=3, n_reports=TWO31), E_SIZE, 'smart_objfn_windows_hip: ld 3 is less than n_samples 4'),
    (W, dict(n_reports=TWO31, n_windows=1025), E_SIZE,
     'smart_objfn_windows_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (W, dict(n_windows=1025, eps=-1.0), E_SIZE, 'smart_objfn_windows_hip: n_windows 1025, at most 1024 per call'),
    (W, dict(eps=NAN, transform=4), E_SIZE, 'smart_objfn_windows_hip: eps nan must be finite and >= 0'),
    # ---- smart_flow_duration_hip
    (F, dict(sim=None), E_NULL, 'smart_flow_duration_hip: sim, probs and quant are required (sim is NULL)'),
    (F, dict(probs=None), E_NULL, 'smart_flow_duration_hip: sim, probs and quant are required (probs is NULL)'),
    (F, dict(quant=None), E_NULL, 'smart_flow_duration_hip: sim, probs and quant are required (quant is NULL)'),
    (F, dict(FDC_OBJFN, obs=None), E_NULL, 'smart_flow_duration_hip: objfn needs obs (obs is NULL)'),
    (F, dict(n_samples=0), E_SIZE,
     'smart_flow_duration_hip: need n_samples, n_reports, n_windows, n_probs >= 1 (got 0, 3, 2, 2)'),
    (F, dict(n_reports=0), E_SIZE,
     'smart_flow_duration_hip: need n_samples, n_reports, n_windows, n_probs >= 1 (got 4, 0, 2, 2)'),
    (F, dict(n_windows=0), E_SIZE,
     'smart_flow_duration_hip: need n_samples, n_reports, n_windows, n_probs >= 1 (got 4, 3, 0, 2)'),
    (F, dict(n_probs=0), E_SIZE,
     'smart_flow_duration_hip: need n_samples, n_reports, n_windows, n_probs >= 1 (got 4, 3, 2, 0)'),
    (F, dict(ld=3), E_SIZE, 'smart_flow_duration_hip: ld 3 is less than n_samples 4'),
    (F, dict(n_reports=TWO31), E_SIZE,
     'smart_flow_duration_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (F, dict(n_windows=1025), E_SIZE, 'smart_flow_duration_hip: n_windows 1025, at most 1024 per call'),
    (F, dict(window=None), E_SIZE, 'smart_flow_duration_hip: n_windows 2 without a window array (NULL is one window)'),
    (F, dict(n_probs=17), E_SIZE, 'smart_flow_duration_hip: n_probs 17, at most 16 probabilities per call'),
    (F, dict(probs=(-0.1, 0.5)), E_SIZE, 'smart_flow_duration_hip: probability 0 is -0.1, outside [0, 1]'),
    (F, dict(probs=(0.5, 1.5)), E_SIZE, 'smart_flow_duration_hip: probability 1 is 1.5, outside [0, 1]'),
    (F, dict(probs=(0.5, NAN)), E_SIZE, 'smart_flow_duration_hip: probability 1 is nan, outside [0, 1]'),
    (F, dict(eps=NAN), E_SIZE, 'smart_flow_duration_hip: eps nan must be finite and >= 0'),
    (F, dict(eps=-1.0), E_SIZE, 'smart_flow_duration_hip: eps -1 must be finite and >= 0'),
    (F, dict(eps=INF), E_SIZE, 'smart_flow_duration_hip: eps inf must be finite and >= 0'),
    (F, dict(seg_lo=0.5, seg_hi=0.5), E_SIZE,
     'smart_flow_duration_hip: the segment (0.5, 0.5) is not 0 <= seg_lo < seg_hi <= 1'),
    (F, dict(seg_lo=-0.1), E_SIZE, 'smart_flow_duration_hip: the segment (-0.1, 1) is not 0 <= seg_lo < seg_hi <= 1'),
    (F, dict(seg_hi=1.5), E_SIZE, 'smart_flow_duration_hip: the segment (0, 1.5) is not 0 <= seg_lo < seg_hi <= 1'),
    (F, dict(seg_lo=NAN), E_SIZE, 'smart_flow_duration_hip: the segment (nan, 1) is not 0 <= seg_lo < seg_hi <= 1'),
    (F, dict(transform=4), E_MODE, "smart_flow_duration_hip: transform '4' unknown."),
    (F, dict(method=3), E_MODE, "smart_flow_duration_hip: method '3' unknown."),
    (F, dict(FDC_OBJFN, method=2), E_MODE,
     'smart_flow_duration_hip: the select form gives order statistics only (objfn given)'),
    (F, dict(method=1, n_reports=16385), E_SIZE,
     'smart_flow_duration_hip: the sort form takes at most 16384 report steps (the sort capacity), not 16385'),
    (F, dict(FDC_OBJFN, n_reports=16385), E_SIZE,
     'smart_flow_duration_hip: the objective functions of the curve take at most 16384 report steps (the sort '
     'capacity), not 16385'),
    (F, dict(FDC_OBJFN, workspace=None), E_NULL,
     'smart_flow_duration_hip: objfn needs a workspace of 256 bytes (workspace is NULL)'),
    (F, dict(FDC_OBJFN, workspace_bytes=255), E_SIZE, 'smart_flow_duration_hip: workspace_bytes 255, need 256'),
    # (probability 0 is inside the interval here: the later refusal is the one that shows)
    (F, dict(probs=(0.0, 1.0), method=3), E_MODE, "smart_flow_duration_hip: method '3' unknown."),
    (F, dict(quant=None, objfn=FAKE, obs=None), E_NULL,
     'smart_flow_duration_hip: sim, probs and quant are required (quant is NULL)'),
    (F, dict(FDC_OBJFN, obs=None, n_probs=0), E_NULL, 'smart_flow_duration_hip: objfn needs obs (obs is NULL)'),
    (F, dict(n_probs=0, ld=3), E_SIZE,
     'smart_flow_duration_hip: need n_samples, n_reports, n_windows, n_probs >= 1 (got 4, 3, 2, 0)'),
    (F, dict(ld=3, n_reports=TWO31), E_SIZE, 'smart_flow_duration_hip: ld 3 is less than n_samples 4'),
    (F, dict(n_reports=TWO31, n_windows=1025), E_SIZE,
     'smart_flow_duration_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (F, dict(n_windows=1025, window=None), E_SIZE, 'smart_flow_duration_hip: n_windows 1025, at most 1024 per call'),
    (F, dict(window=None, n_probs=17), E_SIZE,
     'smart_flow_duration_hip: n_windows 2 without a window array (NULL is one window)'),
    (F, dict(n_probs=17, probs=(2.0, 0.5)), E_SIZE,
     'smart_flow_duration_hip: n_probs 17, at most 16 probabilities per call'),
    (F, dict(probs=(2.0, 0.5), eps=-1.0), E_SIZE, 'smart_flow_duration_hip: probability 0 is 2, outside [0, 1]'),
    (F, dict(eps=-1.0, seg_hi=1.5), E_SIZE, 'smart_flow_duration_hip: eps -1 must be finite and >= 0'),
    (F, dict(seg_hi=1.5, transform=4), E_SIZE,
     'smart_flow_duration_hip: the segment (0, 1.5) is not 0 <= seg_lo < seg_hi <= 1'),
    (F, dict(transform=4, method=3), E_MODE, "smart_flow_duration_hip: transform '4' unknown."),
    (F, dict(FDC_OBJFN, method=2, n_reports=16385), E_MODE,
     'smart_flow_duration_hip: the select form gives order statistics only (objfn given)'),
    (F, dict(FDC_OBJFN, n_reports=16385, workspace=None), E_SIZE,
     'smart_flow_duration_hip: the objective functions of the curve take at most 16384 report steps (the sort '
     'capacity), not 16385'),
    (F, dict(FDC_OBJFN, workspace=None, workspace_bytes=0), E_NULL,
     'smart_flow_duration_hip: objfn needs a workspace of 256 bytes (workspace is NULL)'),
    # ---- smart_sobol_indices_hip
    (S, dict(y=None), E_NULL, 'smart_sobol_indices_hip: y, s1, st and moments are required (y is NULL)'),
    (S, dict(s1=None), E_NULL, 'smart_sobol_indices_hip: y, s1, st and moments are required (s1 is NULL)'),
    (S, dict(st=None), E_NULL, 'smart_sobol_indices_hip: y, s1, st and moments are required (st is NULL)'),
    (S, dict(moments=None), E_NULL, 'smart_sobol_indices_hip: y, s1, st and moments are required (moments is NULL)'),
    (S, dict(SOBOL_BOOT, counts=None), E_NULL,
     'smart_sobol_indices_hip: n_resamples 4 needs counts, s1_std and st_std (counts is NULL)'),
    (S, dict(SOBOL_BOOT, s1_std=None), E_NULL,
     'smart_sobol_indices_hip: n_resamples 4 needs counts, s1_std and st_std (s1_std is NULL)'),
    (S, dict(SOBOL_BOOT, st_std=None), E_NULL,
     'smart_sobol_indices_hip: n_resamples 4 needs counts, s1_std and st_std (st_std is NULL)'),
    (S, dict(n_base=0), E_SIZE, 'smart_sobol_indices_hip: n_base 0 must be in 1 .. 2^31 - 1'),
    (S, dict(n_base=TWO31), E_SIZE, 'smart_sobol_indices_hip: n_base 2147483648 must be in 1 .. 2^31 - 1'),
    (S, dict(n_params=0), E_SIZE, 'smart_sobol_indices_hip: n_params 0 must be in 1 .. 16'),
    (S, dict(n_params=17), E_SIZE, 'smart_sobol_indices_hip: n_params 17 must be in 1 .. 16'),
    (S, dict(n_rows=0), E_SIZE, 'smart_sobol_indices_hip: n_rows 0 must be in 1 .. 2^31 - 1'),
    (S, dict(n_rows=TWO31), E_SIZE, 'smart_sobol_indices_hip: n_rows 2147483648 must be in 1 .. 2^31 - 1'),
    (S, dict(n_resamples=-1), E_SIZE, 'smart_sobol_indices_hip: n_resamples -1 must be in 0 .. 512'),
    (S, dict(SOBOL_BOOT, n_resamples=513), E_SIZE, 'smart_sobol_indices_hip: n_resamples 513 must be in 0 .. 512'),
    (S, dict(ld=31), E_SIZE, 'smart_sobol_indices_hip: ld 31 is less than n_base * (n_params + 2) = 32'),
    (S, dict(workspace_bytes=-1), E_SIZE, 'smart_sobol_indices_hip: workspace_bytes -1, need 0'),
    (S, dict(workspace=FAKE, workspace_bytes=-1), E_SIZE, 'smart_sobol_indices_hip: workspace_bytes -1, need 0'),
    (S, dict(st=None, n_resamples=4), E_NULL,
     'smart_sobol_indices_hip: y, s1, st and moments are required (st is NULL)'),
    (S, dict(n_resamples=4, n_base=0), E_NULL,
     'smart_sobol_indices_hip: n_resamples 4 needs counts, s1_std and st_std (counts is NULL)'),
    (S, dict(n_base=0, n_params=17), E_SIZE, 'smart_sobol_indices_hip: n_base 0 must be in 1 .. 2^31 - 1'),
    (S, dict(n_params=17, n_rows=0), E_SIZE, 'smart_sobol_indices_hip: n_params 17 must be in 1 .. 16'),
    (S, dict(n_rows=0, n_resamples=-1), E_SIZE, 'smart_sobol_indices_hip: n_rows 0 must be in 1 .. 2^31 - 1'),
    (S, dict(n_resamples=-1, ld=31), E_SIZE, 'smart_sobol_indices_hip: n_resamples -1 must be in 0 .. 512'),
    (S, dict(ld=31, workspace_bytes=-1), E_SIZE,
     'smart_sobol_indices_hip: ld 31 is less than n_base * (n_params + 2) = 32'),
    # ---- smart_signatures_hip
    (G, dict(sim=None), E_NULL, 'smart_signatures_hip: sim and sig are required (sim is NULL)'),
    (G, dict(sig=None), E_NULL, 'smart_signatures_hip: sim and sig are required (sig is NULL)'),
    (G, dict(sim=None, sig=None), E_NULL, 'smart_signatures_hip: sim and sig are required (sim is NULL)'),
    (G, dict(sig=None, n_samples=0), E_NULL, 'smart_signatures_hip: sim and sig are required (sig is NULL)'),
    (G, dict(n_samples=0), E_SIZE, 'smart_signatures_hip: need n_samples, n_reports, n_windows >= 1 (got 0, 3, 2)'),
    (G, dict(n_samples=-2), E_SIZE, 'smart_signatures_hip: need n_samples, n_reports, n_windows >= 1 (got -2, 3, 2)'),
    (G, dict(n_reports=0), E_SIZE, 'smart_signatures_hip: need n_samples, n_reports, n_windows >= 1 (got 4, 0, 2)'),
    (G, dict(n_windows=0), E_SIZE, 'smart_signatures_hip: need n_samples, n_reports, n_windows >= 1 (got 4, 3, 0)'),
    (G, dict(ld=3), E_SIZE, 'smart_signatures_hip: ld 3 is less than n_samples 4'),
    (G, dict(n_reports=TWO31), E_SIZE,
     'smart_signatures_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (G, dict(n_windows=1025), E_SIZE, 'smart_signatures_hip: n_windows 1025, at most 1024 per call'),
    (G, dict(window=None), E_SIZE, 'smart_signatures_hip: n_windows 2 without a window array (NULL is one window)'),
    (G, dict(alpha=0.0), E_SIZE, 'smart_signatures_hip: alpha 0 must lie inside (0, 1)'),
    (G, dict(alpha=1.0), E_SIZE, 'smart_signatures_hip: alpha 1 must lie inside (0, 1)'),
    (G, dict(alpha=NAN), E_SIZE, 'smart_signatures_hip: alpha nan must lie inside (0, 1)'),
    (G, dict(alpha=INF), E_SIZE, 'smart_signatures_hip: alpha inf must lie inside (0, 1)'),
    (G, dict(alpha=-0.5), E_SIZE, 'smart_signatures_hip: alpha -0.5 must lie inside (0, 1)'),
    (G, dict(n_windows=0, ld=3), E_SIZE,
     'smart_signatures_hip: need n_samples, n_reports, n_windows >= 1 (got 4, 3, 0)'),
    (G, dict(ld=3, n_reports=TWO31), E_SIZE, 'smart_signatures_hip: ld 3 is less than n_samples 4'),
    (G, dict(n_reports=TWO31, n_windows=1025), E_SIZE,
     'smart_signatures_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (G, dict(n_windows=1025, window=None), E_SIZE, 'smart_signatures_hip: n_windows 1025, at most 1024 per call'),
    (G, dict(window=None, alpha=2.0), E_SIZE,
     'smart_signatures_hip: n_windows 2 without a window array (NULL is one window)'),
    # ---- smart_objfn_bootstrap_hip (without replicates neither n_probs nor the probabilities are looked at)
    (B, dict(sim=None), E_NULL, 'smart_objfn_bootstrap_hip: sim, obs, window and point are required (sim is NULL)'),
    (B, dict(obs=None), E_NULL, 'smart_objfn_bootstrap_hip: sim, obs, window and point are required (obs is NULL)'),
    (B, dict(window=None), E_NULL,
     'smart_objfn_bootstrap_hip: sim, obs, window and point are required (window is NULL)'),
    (B, dict(point=None), E_NULL, 'smart_objfn_bootstrap_hip: sim, obs, window and point are required (point is NULL)'),
    (B, dict(counts=None), E_NULL,
     'smart_objfn_bootstrap_hip: n_resamples 4 needs counts, probs and stats (counts is NULL)'),
    (B, dict(probs=None), E_NULL,
     'smart_objfn_bootstrap_hip: n_resamples 4 needs counts, probs and stats (probs is NULL)'),
    (B, dict(stats=None), E_NULL,
     'smart_objfn_bootstrap_hip: n_resamples 4 needs counts, probs and stats (stats is NULL)'),
    (B, dict(obs=None, point=None), E_NULL,
     'smart_objfn_bootstrap_hip: sim, obs, window and point are required (obs is NULL)'),
    (B, dict(point=None, counts=None), E_NULL,
     'smart_objfn_bootstrap_hip: sim, obs, window and point are required (point is NULL)'),
    (B, dict(counts=None, stats=None), E_NULL,
     'smart_objfn_bootstrap_hip: n_resamples 4 needs counts, probs and stats (counts is NULL)'),
    (B, dict(stats=None, n_samples=0), E_NULL,
     'smart_objfn_bootstrap_hip: n_resamples 4 needs counts, probs and stats (stats is NULL)'),
    (B, dict(n_samples=0), E_SIZE, 'smart_objfn_bootstrap_hip: n_samples 0 must be in 1 .. 2^31 - 1'),
    (B, dict(n_samples=TWO31, ld=TWO31), E_SIZE,
     'smart_objfn_bootstrap_hip: n_samples 2147483648 must be in 1 .. 2^31 - 1'),
    (B, dict(n_windows=0), E_SIZE, 'smart_objfn_bootstrap_hip: n_windows 0 must be in 1 .. 64'),
    (B, dict(n_windows=65), E_SIZE, 'smart_objfn_bootstrap_hip: n_windows 65 must be in 1 .. 64'),
    (B, dict(n_resamples=-1), E_SIZE, 'smart_objfn_bootstrap_hip: n_resamples -1 must be in 0 .. 4096'),
    (B, dict(n_resamples=4097), E_SIZE, 'smart_objfn_bootstrap_hip: n_resamples 4097 must be in 0 .. 4096'),
    (B, dict(n_reports=0), E_SIZE, 'smart_objfn_bootstrap_hip: need n_reports >= 1 (got 0)'),
    (B, dict(n_reports=-5), E_SIZE, 'smart_objfn_bootstrap_hip: need n_reports >= 1 (got -5)'),
    (B, dict(ld=3), E_SIZE, 'smart_objfn_bootstrap_hip: ld 3 is less than n_samples 4'),
    (B, dict(n_reports=TWO31), E_SIZE,
     'smart_objfn_bootstrap_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (B, dict(n_probs=0), E_SIZE, 'smart_objfn_bootstrap_hip: n_probs 0 must be in 1 .. 16'),
    (B, dict(n_probs=17), E_SIZE, 'smart_objfn_bootstrap_hip: n_probs 17 must be in 1 .. 16'),
    (B, dict(probs=(0.0, 0.5)), E_SIZE, 'smart_objfn_bootstrap_hip: probability 0 is 0, outside (0, 1]'),
    (B, dict(probs=(0.5, 1.5)), E_SIZE, 'smart_objfn_bootstrap_hip: probability 1 is 1.5, outside (0, 1]'),
    (B, dict(probs=(0.5, NAN)), E_SIZE, 'smart_objfn_bootstrap_hip: probability 1 is nan, outside (0, 1]'),
    (B, dict(eps=-1.0), E_SIZE, 'smart_objfn_bootstrap_hip: eps -1 must be finite and >= 0'),
    (B, dict(eps=NAN), E_SIZE, 'smart_objfn_bootstrap_hip: eps nan must be finite and >= 0'),
    (B, dict(eps=INF), E_SIZE, 'smart_objfn_bootstrap_hip: eps inf must be finite and >= 0'),
    (B, dict(transform=4), E_MODE, "smart_objfn_bootstrap_hip: transform '4' unknown."),
    (B, dict(transform=-1), E_MODE, "smart_objfn_bootstrap_hip: transform '-1' unknown."),
    (B, dict(workspace=None), E_NULL,
     'smart_objfn_bootstrap_hip: a workspace of 5376 bytes is needed (workspace is NULL)'),
    (B, dict(workspace_bytes=255), E_SIZE, 'smart_objfn_bootstrap_hip: workspace_bytes 255, need 5376'),
    (B, dict(workspace=None, workspace_bytes=0), E_NULL,
     'smart_objfn_bootstrap_hip: a workspace of 5376 bytes is needed (workspace is NULL)'),
    (B, dict(replicates=FAKE, workspace_bytes=255), E_SIZE,
     'smart_objfn_bootstrap_hip: workspace_bytes 255, need 5376'),
    (B, dict(n_samples=0, n_windows=0), E_SIZE, 'smart_objfn_bootstrap_hip: n_samples 0 must be in 1 .. 2^31 - 1'),
    (B, dict(n_windows=0, n_resamples=-1), E_SIZE, 'smart_objfn_bootstrap_hip: n_windows 0 must be in 1 .. 64'),
    (B, dict(n_resamples=-1, n_reports=0), E_SIZE, 'smart_objfn_bootstrap_hip: n_resamples -1 must be in 0 .. 4096'),
    (B, dict(n_reports=0, ld=3), E_SIZE, 'smart_objfn_bootstrap_hip: need n_reports >= 1 (got 0)'),
    (B, dict(ld=3, n_reports=TWO31), E_SIZE, 'smart_objfn_bootstrap_hip: ld 3 is less than n_samples 4'),
    (B, dict(n_reports=TWO31, n_probs=0), E_SIZE,
     'smart_objfn_bootstrap_hip: n_reports 2147483648 is more than one launch takes (2^31 - 1)'),
    (B, dict(n_probs=17, probs=(2.0, 0.5)), E_SIZE, 'smart_objfn_bootstrap_hip: n_probs 17 must be in 1 .. 16'),
    (B, dict(probs=(2.0, 0.5), eps=-1.0), E_SIZE, 'smart_objfn_bootstrap_hip: probability 0 is 2, outside (0, 1]'),
    (B, dict(eps=-1.0, transform=4), E_SIZE, 'smart_objfn_bootstrap_hip: eps -1 must be finite and >= 0'),
    (B, dict(transform=4, workspace=None), E_MODE, "smart_objfn_bootstrap_hip: transform '4' unknown."),
    (B, dict(n_resamples=0, counts=None, probs=None, stats=None, n_probs=0, eps=-1.0), E_SIZE,
     'smart_objfn_bootstrap_hip: eps -1 must be finite and >= 0'),
    (B, dict(n_resamples=0, n_probs=17, probs=(2.0, 0.5), transform=9), E_MODE,
     "smart_objfn_bootstrap_hip: transform '9' unknown."),
    # ---- the capacity and workspace entries: a size, or SMART_E_SIZE where the sizes are refused
    ('smart_flow_duration_workspace_bytes', {}, 512, None),
    ('smart_flow_duration_workspace_bytes', dict(with_objfn=0), 0, None),
    ('smart_flow_duration_workspace_bytes', dict(n_reports=0), E_SIZE, None),
    ('smart_flow_duration_workspace_bytes', dict(n_reports=TWO31), E_SIZE, None),
    ('smart_flow_duration_workspace_bytes', dict(n_windows=0), E_SIZE, None),
    ('smart_sobol_workspace_bytes', {}, 0, None),
    ('smart_sobol_workspace_bytes', dict(n_base=0), E_SIZE, None),
    ('smart_sobol_workspace_bytes', dict(n_params=17), E_SIZE, None),
    ('smart_sobol_workspace_bytes', dict(n_rows=TWO31), E_SIZE, None),
    ('smart_sobol_workspace_bytes', dict(n_resamples=513), E_SIZE, None),
    ('smart_bootstrap_workspace_bytes', {}, 5376, None),
    ('smart_bootstrap_workspace_bytes', dict(n_samples=0), E_SIZE, None),
    ('smart_bootstrap_workspace_bytes', dict(n_samples=TWO31), E_SIZE, None),
    ('smart_bootstrap_workspace_bytes', dict(n_windows=0), E_SIZE, None),
    ('smart_bootstrap_workspace_bytes', dict(n_windows=65), E_SIZE, None),
    ('smart_bootstrap_workspace_bytes', dict(n_resamples=-1), E_SIZE, None),
    ('smart_bootstrap_workspace_bytes', dict(n_resamples=4097), E_SIZE, None),
    ('smart_bootstrap_workspace_bytes', dict(n_resamples=0), 768, None),
    ('smart_bootstrap_workspace_bytes', dict(with_replicates=1), 5376, None),
    ('smart_bootstrap_max_windows', {}, 64, None),
    ('smart_bootstrap_max_resamples', {}, 4096, None),
    ('smart_quantiles_sort_capacity', {}, 8192, None),
    ('smart_objfn_max_windows', {}, 1024, None),
    ('smart_flow_duration_sort_capacity', {}, 16384, None),
    ('smart_sobol_max_resamples', {}, 512, None),
    ('smart_sobol_lds_capacity', {}, 8192, None),
]


@pytest.mark.parametrize('entry,changes,code,text', CASES,
                         ids=['%s-%s' % (c[0][6:], '+'.join(c[1]) or 'valid') for c in CASES])
def test_refusal(entry, changes, code, text):
    assert call(entry, changes) == (code, text)


def test_every_refusing_entry_has_a_row_that_breaks_two_rules():
    for entry in VALID:
        if entry.endswith('_hip'):
            assert any(c[0] == entry and len(c[1]) >= 2 and c[2] != 0 for c in CASES), entry


def test_a_refusal_leaves_its_own_text_not_the_one_before():
    first = call('smart_objfn_hip', dict(sim=None))
    second = call('smart_sobol_indices_hip', dict(ld=31))
    assert first[1] != second[1] and second[1].startswith('smart_sobol_indices_hip: ld 31 ')
