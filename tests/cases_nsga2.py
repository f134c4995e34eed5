"""The cases of the NSGA-II tests that more than one file runs: the loop of montecarlo.NSGA2 on the numpy statement
(oracle/analyses/nsga2.py), and the two-point convergence problem of tests/test_nsga2_host.py and
profiles/nsga2_statement.txt.  A plain module: pytest does not collect it."""
import numpy as np

from oracle.analyses.nsga2 import MAX, Population, nsga2_statement

POINT_A = np.array([0.2, 0.3, 0.7, 0.6, 0.25, 0.8])
POINT_B = np.array([0.8, 0.6, 0.2, 0.4, 0.75, 0.3])
CONVERGENCE = dict(N=128, d=6, generations=60, seeds=range(6))


def two_point_scores(x):
    """Two objectives to maximise: the negated squared distances to POINT_A and POINT_B.  The Pareto set is the segment
    between the two points."""
    return np.stack([-((x - POINT_A) ** 2).sum(axis=1), -((x - POINT_B) ** 2).sum(axis=1)], axis=1)


def segment_figures(x):
    """-> (the mean distance of the rows of x to the segment A B, the largest gap between neighbouring projections along
    it, how far the outermost projections are from its two ends -- the larger of the two); projections in [0, 1]"""
    ab = POINT_B - POINT_A
    t = np.clip((x - POINT_A) @ ab / (ab @ ab), 0.0, 1.0)
    foot = POINT_A + t[:, None] * ab
    along = np.sort(t)
    return (float(np.sqrt(((x - foot) ** 2).sum(axis=1)).mean()), float(np.diff(along).max()),
            float(max(along[0], 1.0 - along[-1])))


def convergence_run(seed):
    """The statement on the two-point problem from a uniform population of the seed -> (figures before, figures after,
    the best key per objective after every survive phase [generations + 1, 2])"""
    N, d, G = CONVERGENCE['N'], CONVERGENCE['d'], CONVERGENCE['generations']
    x0 = np.random.default_rng(seed).uniform(0.0, 1.0, size=(N, d))
    s = Population(x0, [0.0] * d, [1.0] * d, [(0, MAX), (1, MAX)], seed=seed)
    kept = []
    run_statement(s, two_point_scores, G, keep=kept)
    best = np.stack([np.nanmax(keys, axis=0) for keys, _ in kept])
    return segment_figures(x0), segment_figures(s.x), best


def run_statement(s, score_function, generations, keep=None):
    """The loop of montecarlo.NSGA2 on a Population object and a score function of the test's (launch rows -> score
    matrix).  keep: a list that takes (keys, x) of the population after every survive phase."""
    for g in range(0, generations + 1):
        nsga2_statement(s, scores=score_function(s.rows[:, s.columns]), vary=g < generations)
        if keep is not None:
            keep.append((s.keys.copy(), s.x.copy()))
