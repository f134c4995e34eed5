"""NSGA-II: the numpy statement of include/smart_amd.h (smart_nsga2_step_hip), which the kernels are held to BIT FOR BIT.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

from oracle.analyses.de_move import crossover, launch_rows, move, mulhi
from oracle.philox import philox4x32

MAX, MIN, TARGET = 0, 1, 2
RANK_BEYOND, RANK_OUT = 2 ** 31 - 2, 2 ** 31 - 1


class Population(object):
    """The state of the statement, in numpy: what nsga2.Nsga2State keeps on the device.  objectives: [(column, direction)]
    with a direction MAX, MIN or (TARGET, value)."""

    def __init__(self, x, lo, hi, objectives, seed=0, f=0.5, cr=0.9, b_star=1e-6, n_carry=0, columns=None, ld=None,
                 fill=np.nan):
        self.offspring = np.array(x, dtype=np.float64)
        N, d = self.offspring.shape
        self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        self.scale = float(b_star) * (self.hi - self.lo)
        self.f, self.C = float(f), int(math.floor(float(cr) * 2.0 ** 32))
        self.key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        self.columns = np.arange(d) if columns is None else np.asarray(columns)
        self.score_columns = [int(col) for col, _ in objectives]
        self.direction = [w[0] if isinstance(w, tuple) else w for _, w in objectives]
        self.target = [float(w[1]) if isinstance(w, tuple) else 0.0 for _, w in objectives]
        M = len(objectives)
        self.x = np.zeros((N, d))
        self.keys = np.full((N, M), np.nan)
        self.carry = np.zeros((N, n_carry))
        self.part = np.zeros(N, dtype=np.uint8)
        self.rank = np.full(N, RANK_OUT, dtype=np.int32)
        self.crowding = np.zeros(N)
        self.origin = np.arange(N, dtype=np.int32)
        self.counts = np.zeros(2, dtype=np.int32)
        self.out = np.zeros(N, dtype=np.uint8)
        self.rows = np.full((N, d if ld is None else ld), fill)
        self.rows[:, self.columns] = self.offspring
        self.parents, self.g = False, 1
        self.fallbacks = 0              # how often the fallback dimension was taken


def keys_of(scores, score_columns, direction, target):
    """key[c][m] of the selected columns of a score matrix: x, -x or -|x - target|"""
    scores = np.asarray(scores, dtype=np.float64)
    keys = np.empty((scores.shape[0], len(score_columns)))
    for m, (col, word, value) in enumerate(zip(score_columns, direction, target)):
        x = scores[:, col]
        keys[:, m] = x if word == MAX else (-x if word == MIN else -np.abs(x - value))
    return keys


def dominance(keys):
    """dom[j][i]: candidate j dominates candidate i -- all keys >= and not all <=, IEEE compares (a NaN key makes every
    compare false: a candidate that takes no part holds NaN keys)"""
    with np.errstate(invalid='ignore'):
        ge = np.ones((len(keys), len(keys)), dtype=bool)
        le = np.ones((len(keys), len(keys)), dtype=bool)
        for m in range(keys.shape[1]):
            ge &= keys[:, None, m] >= keys[None, :, m]
            le &= keys[:, None, m] <= keys[None, :, m]
    return ge & ~le


def ranks_of(keys, part, N):
    """-> (rank [E] int32, the number of fronts peeled): fronts are peeled until at least N candidates are ranked or none
    that takes part is left"""
    dom = dominance(keys)
    count = dom.sum(axis=0)
    rank = np.where(part, RANK_BEYOND, RANK_OUT).astype(np.int32)
    ranked = fronts = 0
    while ranked < N:
        front = (rank == RANK_BEYOND) & (count == 0)
        if not front.any():
            break
        fronts += 1
        rank[front] = fronts
        ranked += int(front.sum())
        count = count - dom[front].sum(axis=0)
    return rank, fronts


def crowding_of(keys, rank):
    """The value-based crowding distance of every candidate of a peeled front, 0.0 for the others"""
    E, M = keys.shape
    dist = np.zeros(E)
    for r in np.unique(rank[rank < RANK_BEYOND]):
        members = np.nonzero(rank == r)[0]
        k = keys[members]                                   # [F, M]
        other = ~np.eye(len(members), dtype=bool)           # [i][j]: j != i
        total = np.zeros(len(members))
        for m in range(M):
            v = k[:, m]
            lowest, highest = v.min(), v.max()
            up = np.where(other & (v[None, :] >= v[:, None]), v[None, :], np.inf).min(axis=1)
            down = np.where(other & (v[None, :] <= v[:, None]), v[None, :], -np.inf).max(axis=1)
            with np.errstate(invalid='ignore', divide='ignore'):
                t = up - down
                t = t / (highest - lowest)
                inner = total + t
            total = np.where((v == lowest) | (v == highest), np.inf, inner)
        dist[members] = total
    return dist


def positions_of(rank, dist):
    """pos(e) = the number of candidates that precede e in (rank ascending, distance descending, e ascending)"""
    order = np.lexsort((np.arange(len(rank)), -dist, rank))
    pos = np.empty(len(rank), dtype=np.int64)
    pos[order] = np.arange(len(rank))
    return pos


def nsga2_statement(s, scores=None, carry_new=None, eligible=None, vary=True):
    """One call of smart_nsga2_step_hip, as include/smart_amd.h words it, on a Population object"""
    N, d = s.offspring.shape
    if scores is not None:
        scores = np.asarray(scores, dtype=np.float64)
        selected = scores[:, s.score_columns]
        takes = (s.out == 0) & ~np.isnan(selected).any(axis=1)
        if eligible is not None:
            takes &= np.asarray(eligible) != 0
        fresh = keys_of(scores, s.score_columns, s.direction, s.target)
        fresh[~takes] = np.nan
        payload = np.zeros((N, 0)) if s.carry.shape[1] == 0 else np.asarray(carry_new, dtype=np.float64)
        if s.parents:
            x = np.concatenate([s.x, s.offspring])
            keys = np.concatenate([s.keys, fresh])
            carry = np.concatenate([s.carry, payload])
            part = np.concatenate([s.part != 0, takes])
        else:
            x, keys, carry, part = s.offspring.copy(), fresh, payload.copy(), takes
        rank, fronts = ranks_of(keys, part, N)
        dist = crowding_of(keys, rank)
        pos = positions_of(rank, dist)
        survivors = np.nonzero(pos < N)[0]
        to = pos[survivors]
        s.x, s.keys, s.carry = np.empty((N, d)), np.empty((N, keys.shape[1])), np.empty((N, carry.shape[1]))
        s.part, s.rank, s.crowding = np.empty(N, dtype=np.uint8), np.empty(N, dtype=np.int32), np.empty(N)
        s.origin = np.empty(N, dtype=np.int32)
        s.x[to], s.keys[to], s.carry[to] = x[survivors], keys[survivors], carry[survivors]
        s.part[to], s.rank[to], s.crowding[to], s.origin[to] = part[survivors], rank[survivors], dist[survivors], survivors
        s.counts = np.array([fronts, int((rank == 1).sum())], dtype=np.int32)
        s.parents = True
        s.last = dict(rank=rank, dist=dist, pos=pos, keys=keys, part=part)     # (for the tests that look at all E candidates)
    if vary:
        assert s.parents, 'the vary phase needs a population'
        c = np.arange(N, dtype=np.uint64)
        r = philox4x32((c, s.g, 0, 0), s.key)
        a = mulhi(r[0], N)
        b = mulhi(r[1], N - 1)
        b = b + (b >= a).astype(np.uint64)
        t = np.minimum(a, b).astype(np.int64)
        p1 = mulhi(r[2], N)
        p2 = mulhi(r[3], N - 1)
        p2 = p2 + (p2 >= p1).astype(np.uint64)
        fallback = mulhi(philox4x32((c, s.g, 1, 0), s.key)[0], d).astype(np.int64)
        W, crossed, fallbacks = crossover(c, s.g, s.key, d, s.C, fallback)
        s.fallbacks += fallbacks
        base = s.x[t]
        s.offspring, out = move(W, crossed, s.scale, s.lo, s.hi, base, s.x[p1.astype(np.int64)], s.x[p2.astype(np.int64)],
                                s.f)
        s.out = out.astype(np.uint8)
        s.rows[:, s.columns] = launch_rows(out, base, s.offspring)
        s.g += 1
