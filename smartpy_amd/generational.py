"""What the bindings of the generational samplers share (demcz.py: DE-MCz, nsga2.py: NSGA-II): N rows that move in lockstep,
one ensemble launch per generation and one C entry around it that proposes the next rows by a differential-evolution move
inside a box (csrc/smart_de_move.h).  Here: the rule that turns a probability into the threshold a 32-bit word is compared
with, the part of a state both samplers keep (BoxState: the device, the population, the box, the seed, the launch matrix),
how the entries are told about the launch matrix and the payload, and the writer of the diagnostics files.  A refusal
carries the sampler's own name (`who`), as the two modules word theirs."""
import math

import numpy as np

from ._lib import SmartEngineError

TWO32 = 1 << 32


def threshold(who, name, p):
    """-> floor(p 2^32): what a 32-bit word is compared with"""
    if not 0.0 <= float(p) <= 1.0:
        raise SmartEngineError(-2, "{}: {} {} must be in [0, 1].".format(who, name, p))
    return int(math.floor(float(p) * TWO32))


class BoxState(object):
    """The part of a state both samplers keep: device, lo, hi, scale = b_star (hi - lo), seed (64 bits), columns (int32:
    the d columns of the launch matrix that the step writes) and rows [N, ld] (the launch matrix).  A state's constructor
    calls _place, states the size rules of its own, and calls _set_box."""

    def _place(self, who, rows_word, x, device):
        """sets `device` -> x as a contiguous [N, d] tensor of the state's own on it"""
        import torch
        from .engine import as_device, default_device
        self.device = torch.device(device) if device is not None else (
            x.device if isinstance(x, torch.Tensor) and x.is_cuda else default_device())
        population = as_device(x, self.device).clone().contiguous()
        if population.dim() != 2:
            raise SmartEngineError(-2, "{}: the population must be [{}, dimensions], not {}."
                                   .format(who, rows_word, tuple(population.shape)))
        return population

    def _set_box(self, who, population, lo, hi, b_star, seed, columns, ld, rows, fill):
        """rows: a launch matrix of the caller's, or None for one of ld columns filled with `fill` (NaN: columns that
        nobody reads) that holds the population in `columns`"""
        import torch
        N, d = population.shape
        self.lo = np.ascontiguousarray(np.asarray(lo, dtype=np.float64).reshape(-1))
        self.hi = np.ascontiguousarray(np.asarray(hi, dtype=np.float64).reshape(-1))
        if self.lo.shape != (d,) or self.hi.shape != (d,):
            raise SmartEngineError(-2, "{}: lo and hi must hold {} values.".format(who, d))
        self.scale = np.ascontiguousarray(float(b_star) * (self.hi - self.lo))
        self.seed = int(seed) & (2 ** 64 - 1)
        self.columns = np.ascontiguousarray(np.arange(d) if columns is None else columns, dtype=np.int32)
        if rows is None:
            ld = d if ld is None else int(ld)
            rows = torch.full((N, ld), float(fill), dtype=torch.float64, device=self.device)
            if ld >= d and int(self.columns.max()) < ld:
                rows[:, torch.from_numpy(self.columns.astype(np.int64)).to(self.device)] = population
        self.rows = rows

    @property
    def ld(self):
        """the stride of the launch matrix's rows, as the entries take it"""
        return self.rows.stride(0) if self.rows.dim() == 2 and self.rows.shape[0] > 1 else self.rows.shape[-1]


def check_carry_new(who, carry_new, n_rows, n_carry):
    """carry_new: None, or the payload of the rows just launched as the entries read it"""
    import torch
    if carry_new is not None and not (isinstance(carry_new, torch.Tensor) and carry_new.is_cuda
                                      and carry_new.dtype == torch.float64
                                      and tuple(carry_new.shape) == (n_rows, n_carry) and carry_new.is_contiguous()):
        raise SmartEngineError(-2, "{}: carry_new must be a contiguous float64 device tensor [{}, {}]."
                               .format(who, n_rows, n_carry))


def write_diagnostics(path, header, integers, diagnostics):
    """header (a line), then one line per row of diagnostics [rows, columns of the header]: the first `integers` columns
    as integers, the others '%.6e'."""
    width = header.count(',') + 1
    with open(path, 'w', newline='', encoding='utf8') as f:
        f.write(header)
        for row in np.asarray(diagnostics, dtype=np.float64).reshape(-1, width):
            f.write(','.join(['%d' % int(v) for v in row[:integers]] + ['%.6e' % v for v in row[integers:]]) + '\n')
