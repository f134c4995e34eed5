"""Dynamic identifiability analysis (DYNIA, Wagener et al. 2003, Hydrol. Process. 17), host side: what goes into
engine.dynamic_identifiability -- the bin of every sample on every parameter (bin_table) -- and what is said from the
shares it leaves: per report step and parameter the confidence limits of the retained rows' distribution over the
parameter's range (confidence_limits) and the information content 1 - width / range (information_content).  A narrow
band means the data of that period constrain the parameter.  The functions take numpy arrays and torch tensors of any
device alike and answer in kind; nothing here needs a GPU.
"""
import numpy as np

NO_BIN = 255        # the category of a row that takes no part in a factor (include/smart_amd.h: smart_dynia_hip)


def _is_tensor(x):
    return type(x).__module__.startswith('torch')


def _ranges(ranges, names=None):
    """dict name -> (lo, hi) (with `names` for the order), or [P, 2] -> numpy [P, 2] float64"""
    if isinstance(ranges, dict):
        ranges = [ranges[name] for name in (names if names is not None else ranges)]
    out = np.asarray(ranges, dtype=np.float64)
    if out.ndim != 2 or out.shape[1] != 2:
        raise ValueError("ranges must be (lo, hi) per factor, shape (P, 2), not {}.".format(out.shape))
    return out


def bin_table(sample, ranges, bins):
    """The category table of engine.dynamic_identifiability -> [P, N] uint8.  sample: [N, P], a row per sample and a
    column per factor; ranges: (lo, hi) per factor; bins: 1 .. 64 equal-width bins over [lo, hi].  The bin of x is
    min(bins - 1, floor((x - lo) / (hi - lo) * bins)): x == lo is bin 0, x == hi the last bin.  255 for a NaN and for a
    value outside the range."""
    bins = int(bins)
    if not 1 <= bins <= 64:
        raise ValueError("bins must be in 1 .. 64, not {}.".format(bins))
    rng = _ranges(ranges)
    if not np.all(rng[:, 1] > rng[:, 0]):
        raise ValueError("every range needs lo < hi.")
    if len(sample.shape) != 2 or sample.shape[1] != rng.shape[0]:
        raise ValueError("sample must be [N, {}] (a column per factor), not {}.".format(rng.shape[0], tuple(sample.shape)))
    if _is_tensor(sample):
        import torch
        x = sample.to(torch.float64).t()
        lo = torch.as_tensor(rng[:, 0:1], device=x.device)
        hi = torch.as_tensor(rng[:, 1:2], device=x.device)
        inside = (x >= lo) & (x <= hi)          # (False for a NaN)
        b = torch.floor((x - lo) / (hi - lo) * bins).clamp(0, bins - 1)
        b = torch.where(inside, b, torch.full_like(b, float(NO_BIN)))
        return b.to(torch.uint8).contiguous()
    x = np.asarray(sample, dtype=np.float64).T
    lo, hi = rng[:, 0:1], rng[:, 1:2]
    inside = (x >= lo) & (x <= hi)
    with np.errstate(invalid='ignore', divide='ignore'):
        b = np.clip(np.floor((x - lo) / (hi - lo) * bins), 0, bins - 1)
    return np.ascontiguousarray(np.where(inside, b, float(NO_BIN)).astype(np.uint8))


def confidence_limits(shares, ranges, level=0.9):
    """shares [R, P, B] -> [R, P, 2]: the (1 - level) / 2 and (1 + level) / 2 quantiles of every factor's distribution
    over its range.  The shares of a factor are renormalised to sum to one (rows of category 255 leave them short of it),
    summed up over the bins, and the quantile is interpolated linearly inside the bin where the cumulative share first
    reaches it.  NaN stays NaN (a step that was not assessed), and a factor without any share is NaN."""
    level = float(level)
    if not 0.0 < level <= 1.0:
        raise ValueError("level must be in (0, 1], not {}.".format(level))
    rng = _ranges(ranges)
    if len(shares.shape) != 3 or shares.shape[1] != rng.shape[0]:
        raise ValueError("shares must be [R, {}, B], not {}.".format(rng.shape[0], tuple(shares.shape)))
    tensor = _is_tensor(shares)
    if tensor:
        import torch
        s = shares.to(torch.float64)
        lo = torch.as_tensor(rng[:, 0], device=s.device)[None, :]
        width = torch.as_tensor(rng[:, 1] - rng[:, 0], device=s.device)[None, :]
        p = s / s.sum(-1, keepdim=True)
        cum = torch.cumsum(p, -1)
        before = torch.cat([torch.zeros_like(cum[..., :1]), cum[..., :-1]], -1)
    else:
        s = np.asarray(shares, dtype=np.float64)
        lo, width = rng[None, :, 0], (rng[:, 1] - rng[:, 0])[None, :]
        with np.errstate(invalid='ignore', divide='ignore'):
            p = s / s.sum(-1, keepdims=True)
        cum = np.cumsum(p, -1)
        before = np.concatenate([np.zeros_like(cum[..., :1]), cum[..., :-1]], -1)
    B = s.shape[-1]
    sides = []
    for q in ((1.0 - level) / 2.0, (1.0 + level) / 2.0):
        reached = (cum >= q) & (cum > 0.0)              # (False for a NaN; q == 0 is reached where the mass begins)
        if tensor:
            reached[..., -1] |= ~torch.isnan(cum[..., -1])      # the last bin, where rounding leaves the sum short of q
            b = torch.argmax(reached.to(torch.uint8), -1, keepdim=True)
            take = lambda a: torch.take_along_dim(a, b, -1)[..., 0]     # noqa: E731
            frac = ((q - take(before)) / take(p)).clamp(0.0, 1.0)
            frac = torch.where(reached.any(-1), frac, torch.full_like(frac, float('nan')))
            sides.append(lo + (b[..., 0].to(torch.float64) + frac) / B * width)
        else:
            reached[..., -1] |= ~np.isnan(cum[..., -1])
            b = np.argmax(reached, -1)[..., None]
            take = lambda a: np.take_along_axis(a, b, -1)[..., 0]       # noqa: E731
            with np.errstate(invalid='ignore', divide='ignore'):
                frac = np.clip((q - take(before)) / take(p), 0.0, 1.0)
            frac = np.where(reached.any(-1), frac, np.nan)
            sides.append(lo + (b[..., 0] + frac) / B * width)
    if tensor:
        import torch
        return torch.stack(sides, -1)
    return np.stack(sides, -1)


def information_content(limits, ranges):
    """limits [R, P, 2] -> [R, P]: 1 - (hi - lo) / (range_hi - range_lo).  1 = the retained rows sit on one value, 0 =
    they spread over the whole range; NaN where the limits are."""
    rng = _ranges(ranges)
    width = rng[:, 1] - rng[:, 0]
    if _is_tensor(limits):
        import torch
        width = torch.as_tensor(width, device=limits.device)
    return 1.0 - (limits[..., 1] - limits[..., 0]) / width[None, :]


def header_line(names):
    """The header of `<catchment>.SMART.<func>.dynia`: DateTime, then IC@<name>,LO@<name>,HI@<name> per parameter."""
    return ','.join(['DateTime'] + ['{}@{}'.format(col, name) for name in names for col in ('IC', 'LO', 'HI')]) + '\n'


def write_file(path, stamps, names, information, limits):
    """header_line, then one line per report step: its stamp and '%.6e' of IC, LO, HI per parameter."""
    from .montecarlo.selection import write_text_table
    R, P = len(stamps), len(names)
    table = np.concatenate([np.asarray(information)[:R, :P, None], np.asarray(limits)[:R, :P]], axis=2).reshape(R, 3 * P)
    write_text_table(path, header_line(names)[:-1], table, '%.6e', '\n', labels=stamps)


class DynamicIdentifiability(object):
    """What MonteCarlo.dynamic_identifiability returns.  `datetime` (the R report stamps), `names` (the P parameters) and
    `ranges` ([P, 2]); numpy float64: `shares` [R, P, B], `limits` [R, P, 2] and `information` [R, P] (confidence_limits
    and information_content at `level`), `cut` [R] (the window's SUM of absolute errors at the cut) and `mean_error` [R]
    (cut / count, the mean absolute error at the cut), `mean_errors` [R, N] (errors / count) where the sums were kept, else
    None; int32: `retained` [R] and `count` [R]; `half_width`, `fraction`, `support`, `min_valid`, `level` as used;
    `device_shares` (the [R, P, B] tensor where it was computed, or None) and `file` (the path written, or None)."""

    def __init__(self, stamps, names, ranges, shares, cut, retained, count, level=0.9, errors=None, half_width=None,
                 fraction=None, support=None, min_valid=None, device_shares=None, file=None):
        self.datetime, self.names = stamps, list(names)
        self.ranges = _ranges(ranges, self.names)
        self.shares = np.asarray(shares, dtype=np.float64)
        self.cut = np.asarray(cut, dtype=np.float64)
        self.retained, self.count = np.asarray(retained, dtype=np.int32), np.asarray(count, dtype=np.int32)
        self.level, self.half_width, self.fraction = float(level), half_width, fraction
        self.support, self.min_valid = support, min_valid
        self.limits = confidence_limits(self.shares, self.ranges, self.level)
        self.information = information_content(self.limits, self.ranges)
        with np.errstate(invalid='ignore', divide='ignore'):
            self.mean_error = self.cut / self.count
            self.mean_errors = None if errors is None else np.asarray(errors, dtype=np.float64) / self.count[:, None]
        self.device_shares, self.file = device_shares, file
