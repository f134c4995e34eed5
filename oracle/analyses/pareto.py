"""Pareto selection: the numpy statement of the dominance counts and ranks.  TEST INFRASTRUCTURE ONLY.

The statement.  key = x for 'max', -x for 'min', -|x - value| for ('target', value), in float64 exactly as written.  A row
takes part iff it is eligible and none of its SELECTED scores is a NaN.  Row j dominates row i iff both take part, every
key of j is >= that of i and at least one is > (all >= and not all <=): brute force over all pairs, chunked over the
candidates so that no array passes about 256 MB.  dominated_by = the number of dominating rows, -1 where the row does not
take part.  Ranks by peeling: rank r = the rows with count 0 once the ranks below r are left out; 0 = not ranked within
max_rank; -1 = not taking part."""
import numpy as np

CHUNK_BYTES = 256 * 2 ** 20


def pareto_keys(scores, directions, targets=None, columns=None):
    """-> float64 [N, M]; NaN exactly where the selected score is a NaN"""
    scores = np.asarray(scores, dtype=np.float64)
    if scores.ndim == 1:
        scores = scores[:, None]
    M = len(directions)
    columns = list(range(M)) if columns is None else list(columns)
    keys = np.empty((scores.shape[0], M), dtype=np.float64)
    for m, (word, col) in enumerate(zip(directions, columns)):
        x = scores[:, col]
        value = None
        if isinstance(word, tuple):
            word, value = word
        elif word == 'target':
            value = targets[m]
        if word == 'max':
            keys[:, m] = x
        elif word == 'min':
            keys[:, m] = -x
        else:
            assert word == 'target', 'direction %r unknown' % (word,)
            keys[:, m] = -np.abs(x - np.float64(value))
    return keys


def dominance_counts(keys):
    """brute force over all pairs of the rows of keys [E, M] (no NaN) -> int64 [E]"""
    E, M = keys.shape
    out = np.zeros(E, dtype=np.int64)
    step = max(1, CHUNK_BYTES // max(1, E * M))
    for lo in range(0, E, step):
        mine = keys[lo:lo + step, None, :]
        with np.errstate(invalid='ignore'):
            ge = (keys[None, :, :] >= mine).all(axis=2)
            le = (keys[None, :, :] <= mine).all(axis=2)
        out[lo:lo + step] = (ge & ~le).sum(axis=1)
    return out


def pareto_statement(scores, directions, targets=None, columns=None, eligible=None):
    keys = pareto_keys(scores, directions, targets, columns)
    part = ~np.isnan(keys).any(axis=1)
    if eligible is not None:
        part &= np.asarray(eligible) != 0
    out = np.full(keys.shape[0], -1, dtype=np.int32)
    out[part] = dominance_counts(keys[part])
    return out


def pareto_rank_statement(scores, directions, targets=None, columns=None, eligible=None, max_rank=1):
    keys = pareto_keys(scores, directions, targets, columns)
    part = ~np.isnan(keys).any(axis=1)
    if eligible is not None:
        part &= np.asarray(eligible) != 0
    ranks = np.where(part, 0, -1).astype(np.int32)
    left, rank = part.copy(), 0
    while left.any() and (max_rank is None or rank < max_rank):
        rank += 1
        idx = np.nonzero(left)[0]
        front = idx[dominance_counts(keys[idx]) == 0]
        ranks[front] = rank
        left[front] = False
    return ranks
