"""PAWN sensitivity from the sample at hand (Pianosi & Wagener 2015, Environ. Model. Softw. 67; given-data form 2018,
Environ. Model. Softw. 108), host side: what goes into engine.pawn_ks beside identifiability.bin_table -- the dummy
factors that give the noise floor (dummy_table; Khorashadi Zadeh et al. 2017, Environ. Model. Softw. 91) -- and what is
said from the Kolmogorov-Smirnov distances it leaves: the index of every factor per output (pawn_indices), the
two-sample critical value (critical_value), the result class and the `.pawn` writer.  The functions take numpy arrays
and torch tensors of any device alike and answer in kind; nothing here needs a GPU.
"""
import math
import warnings

import numpy as np

from .identifiability import NO_BIN, _is_tensor, bin_table     # noqa: F401  (bin_table: the equal-width bins of a factor)

STATISTICS = ('median', 'mean', 'max')


def dummy_table(n, bins, dummies, seed=0):
    """Dummy factors for engine.pawn_ks -> [dummies, n] uint8.  Every dummy factor is a random partition of the n rows
    into `bins` groups whose sizes differ by at most one (a permutation of the rows from numpy.random.default_rng(seed),
    dealt out in turn): by construction it influences nothing, so its index is what the sample size alone produces --
    the noise floor.  The same seed gives the same table."""
    n, bins, dummies = int(n), int(bins), int(dummies)
    if not 1 <= bins <= 64:
        raise ValueError("bins must be in 1 .. 64, not {}.".format(bins))
    if n < 0 or dummies < 0:
        raise ValueError("n and dummies must be >= 0, not {} and {}.".format(n, dummies))
    rng = np.random.default_rng(seed)
    table = np.empty((dummies, n), dtype=np.uint8)
    for d in range(dummies):
        table[d, rng.permutation(n)] = np.arange(n) % bins
    return table


def default_min_count(n, bins):
    """The rows a bin needs to take part in an index where nothing else is said: max(10, n // (4 bins))."""
    return max(10, int(n) // (4 * int(bins)))


def pawn_indices(ks, counts, statistic='median', min_count=1):
    """ks [R, P, B] and counts [P, B] -> the PAWN index [R, P]: the `statistic` ('median', 'mean' or 'max') of ks over the
    bins of the factor that hold at least `min_count` rows.  The other bins are ignored; NaN where none is left (and where
    ks is NaN: a row of the matrix with a value that is not finite)."""
    if statistic not in STATISTICS:
        raise ValueError("statistic '{}' unknown ({}).".format(statistic, ', '.join(STATISTICS)))
    tensor = _is_tensor(ks)
    if tensor:
        import torch
        device = ks.device
        k = ks.detach().to(torch.float64).cpu().numpy()
        c = counts.detach().cpu().numpy() if _is_tensor(counts) else np.asarray(counts)
    else:
        k, c = np.asarray(ks, dtype=np.float64), np.asarray(counts)
    if k.ndim != 3 or c.shape != k.shape[1:]:
        raise ValueError("ks must be [R, P, B] and counts [P, B], not {} and {}.".format(k.shape, c.shape))
    use = c >= max(1, int(min_count))
    kept = np.where(use[None, :, :], k, np.nan)
    fn = {'median': np.nanmedian, 'mean': np.nanmean, 'max': np.nanmax}[statistic]
    with warnings.catch_warnings():         # (a slice that is all NaN -- no bin left, or a row of NaN -- is NaN, silently)
        warnings.simplefilter('ignore', RuntimeWarning)
        out = fn(kept, axis=2) if kept.shape[2] else np.full(kept.shape[:2], np.nan)
    if tensor:
        return torch.from_numpy(out).to(device)
    return out


def critical_value(n, n_b, alpha=0.05):
    """The two-sample Kolmogorov-Smirnov critical value c(alpha) sqrt((n + n_b) / (n n_b)), c(alpha) =
    sqrt(-ln(alpha / 2) / 2): a distance below it is what two samples of these sizes from ONE distribution show with
    probability 1 - alpha.  n, n_b: numbers or arrays (counts of the bins)."""
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must be in (0, 1), not {}.".format(alpha))
    c = math.sqrt(-math.log(alpha / 2.0) / 2.0)
    n, n_b = np.asarray(n, dtype=np.float64), np.asarray(n_b, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = c * np.sqrt((n + n_b) / (n * n_b))
    return float(out) if out.ndim == 0 else out


def header_line(names):
    """The header of `<catchment>.SMART.<func>.pawn`: DateTime, one index column per parameter, dummy."""
    return ','.join(['DateTime'] + list(names) + ['dummy']) + '\n'


def write_file(path, stamps, names, index, dummy):
    """header_line, then one line per output: its stamp (or label), '%.6e' of the index of every parameter and of the
    dummy."""
    from .montecarlo.selection import write_text_table
    R = len(stamps)
    table = np.concatenate([np.asarray(index)[:R, :len(names)], np.asarray(dummy)[:R, None]], axis=1)
    write_text_table(path, header_line(names)[:-1], table, '%.6e', '\n', labels=stamps)


class PawnSensitivity(object):
    """What MonteCarlo.pawn_sensitivity returns.  `datetime` (the R report stamps, or the R labels of the outputs) and
    `names` (the P parameters); numpy: `ks` [R, P + D, B] float64 and `counts` [P + D, B] int32 as the launch left them
    (the D dummy factors behind the parameters), `index` [R, P] (pawn_indices with `statistic` and `min_count`), `dummy`
    [R] (the largest index among the dummy factors; NaN without any), `influential` [R, P] = index > dummy (False where
    either is NaN); `categories` [P + D, N] uint8, the bins the distances were taken on (or None); `statistic`, `min_count`,
    `bins`, `dummies` as used; `device_ks` (the tensor where it was computed, or
    None) and `file` (the path written, or None)."""

    def __init__(self, stamps, names, ks, counts, statistic='median', min_count=1, categories=None, device_ks=None,
                 file=None):
        self.datetime, self.names = stamps, list(names)
        self.ks = np.asarray(ks, dtype=np.float64)
        self.counts = np.asarray(counts, dtype=np.int32)
        self.statistic, self.min_count = statistic, int(min_count)
        P = len(self.names)
        self.bins, self.dummies = self.ks.shape[2], self.ks.shape[1] - P
        every = pawn_indices(self.ks, self.counts, statistic, self.min_count)
        self.index = every[:, :P]
        if self.dummies > 0:
            tail = every[:, P:]
            none = np.isnan(tail).all(axis=1)
            self.dummy = np.where(none, np.nan, np.max(np.where(np.isnan(tail), -np.inf, tail), axis=1))
        else:
            self.dummy = np.full(self.ks.shape[0], np.nan)
        with np.errstate(invalid='ignore'):
            self.influential = self.index > self.dummy[:, None]
        self.categories, self.device_ks, self.file = categories, device_ks, file
