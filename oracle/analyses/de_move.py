"""The differential-evolution move the generational samplers share (csrc/smart_de_move.h), in numpy: what the statements of
DE-MCz (demcz.py) and NSGA-II (nsga2.py) both call, and what the two kernels are held to BIT FOR BIT.  TEST INFRASTRUCTURE
ONLY.  The draw layout is that of include/smart_amd.h: counter (row, generation, 2 + j, 0) belongs to dimension j -- word 0
against the crossover threshold, words 1 and 2 the jitter."""
import numpy as np

from oracle.philox import philox4x32, u53


def mulhi(w, n):
    return (w * np.uint64(n)) >> np.uint64(32)


def crossover(c, g, key, d, C, fallback):
    """rows c (uint64) of generation g -> (W: the draws of the d dimensions, for move(); moved [n, d] bool: the dimensions
    whose word 0 is below C, the fallback dimension of a row where none was drawn; the number of rows that took it)"""
    W = [philox4x32((c, g, 2 + j, 0), key) for j in range(d)]
    moved = np.stack([W[j][0] < np.uint64(C) for j in range(d)], axis=1)
    none = ~moved.any(axis=1)
    moved[none, fallback[none]] = True
    return W, moved, int(none.sum())


def move(W, moved, scale, lo, hi, base, a, b, weight):
    """base + (weight (a - b) + jitter) in the dimensions of `moved`, each operation rounded once, reflected once at lo,
    then once at hi -> (the moved rows, out [n] bool: a moved dimension is still outside the box)"""
    d = base.shape[1]
    eps = np.stack([scale[j] * (2.0 * u53(W[j][1], W[j][2]) - 1.0) for j in range(d)], axis=1)
    lo, hi = lo[None, :], hi[None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        t = a - b
        t = weight * t
        t = t + eps
        y = base + t
        y = np.where(y < lo, 2.0 * lo - y, y)
        y = np.where(y > hi, 2.0 * hi - y, y)
        inside = (y >= lo) & (y <= hi)
    return np.where(moved, y, base), (moved & ~inside).any(axis=1)


def launch_rows(out, base, moved_rows):
    """what goes into the launch matrix: the base row where the move left the box (a row the model can run)"""
    return np.where(out[:, None], base, moved_rows)
