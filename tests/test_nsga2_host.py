"""NSGA-II, host side: the numpy statement of include/smart_amd.h (smart_nsga2_step_hip) that tests/test_gpu_nsga2.py holds
the kernels to BIT FOR BIT, against a brute-force reading of the definition in Python loops (peeling by sets, crowding by
sorting) and against the textbook's sorted-neighbour crowding distance; that the statement converges on a problem whose
Pareto set is known (six seeds, thresholds from profiles/nsga2_statement.txt); every refusal of the C entry, as literals,
the workspace query at the size limits and the refusals of montecarlo.NSGA2.  Nothing here needs a device."""
import bisect
import ctypes
import os
import re

import numpy as np
import pytest

import cases_nsga2 as cases
import oracle.analyses.nsga2 as st
from oracle.analyses.nsga2 import MAX, MIN, TARGET, RANK_BEYOND, RANK_OUT, Population, nsga2_statement
from smartpy_amd import _lib, nsga2
from support import E_MODE, E_NO_DEVICE, E_NULL, E_SIZE, FAKE, example_root, refusal, same_bits, settings_file

INF = float('inf')


# ---- a brute-force reading of the definition --------------------------------------------------------------------------------
def brute(keys, part, N):
    """-> (rank, distance, pos, fronts) of E candidates, by Python loops over include/smart_amd.h's words"""
    E, M = len(keys), len(keys[0])

    def dominates(j, i):
        if not (part[j] and part[i]):
            return False
        return all(keys[j][m] >= keys[i][m] for m in range(M)) and not all(keys[j][m] <= keys[i][m] for m in range(M))

    left = {e for e in range(E) if part[e]}
    rank = [RANK_BEYOND if part[e] else RANK_OUT for e in range(E)]
    fronts, ranked = [], 0
    while ranked < N and left:
        front = {i for i in left if not any(dominates(j, i) for j in left)}
        fronts.append(sorted(front))
        for i in front:
            rank[i] = len(fronts)
        left -= front
        ranked += len(front)
    dist = [0.0] * E
    for front in fronts:
        for i in front:
            total = 0.0
            for m in range(M):
                values = [keys[j][m] for j in front]
                others = sorted(keys[j][m] for j in front if j != i)
                v = keys[i][m]
                if v == min(values) or v == max(values):
                    total = INF
                    continue
                up = others[bisect.bisect_left(others, v)]             # the smallest >= v
                down = others[bisect.bisect_right(others, v) - 1]      # the largest <= v
                total = total + (up - down) / (max(values) - min(values))
            dist[i] = total
    order = sorted(range(E), key=lambda e: (rank[e], -dist[e], e))
    pos = [0] * E
    for place, e in enumerate(order):
        pos[e] = place
    return rank, dist, pos, len(fronts)


def textbook_crowding(keys, front):
    """Deb's distance of the members of one front whose keys hold no ties: per objective the members sorted, the two ends
    infinite, an inner member the difference of its two neighbours over the range -- summed from 0.0 in objective order"""
    total = {i: 0.0 for i in front}
    for m in range(len(keys[0])):
        ordered = sorted(front, key=lambda i: keys[i][m])
        width = keys[ordered[-1]][m] - keys[ordered[0]][m]
        for at, i in enumerate(ordered):
            if at == 0 or at == len(ordered) - 1:
                total[i] = INF
            else:
                total[i] = total[i] + (keys[ordered[at + 1]][m] - keys[ordered[at - 1]][m]) / width
    return total


def of_statement(keys, part, N):
    keys, part = np.asarray(keys, dtype=np.float64), np.asarray(part, dtype=bool)
    keys = np.where(part[:, None], keys, np.nan)            # (a candidate that takes no part holds NaN keys)
    rank, fronts = st.ranks_of(keys, part, N)
    dist = st.crowding_of(keys, rank)
    return rank, dist, st.positions_of(rank, dist), fronts


def agree(keys, part, N):
    rank, dist, pos, fronts = of_statement(keys, part, N)
    b_rank, b_dist, b_pos, b_fronts = brute([list(map(float, k)) for k in keys], list(part), N)
    assert rank.tolist() == b_rank and fronts == b_fronts
    assert same_bits(dist, np.array(b_dist, dtype=np.float64))
    assert pos.tolist() == b_pos and sorted(b_pos) == list(range(len(keys)))
    return rank, dist, pos


TINY = [(E, M, N, seed) for seed, (E, M, N) in enumerate([(24, 2, 12), (24, 3, 12), (24, 4, 12), (8, 2, 4), (7, 2, 7),
                                                          (23, 3, 23), (16, 2, 3), (5, 4, 4)])]


@pytest.mark.parametrize('E,M,N,seed', TINY)
def test_the_statement_is_the_brute_force_reading_without_ties(E, M, N, seed):
    rng = np.random.default_rng(100 + seed)
    keys = rng.normal(size=(E, M))
    part = np.ones(E, dtype=bool)
    part[rng.random(E) < 0.15] = False
    rank, dist, _ = agree(keys, part, N)
    # on keys without ties the distance of every peeled front is the textbook's, to the bit
    for r in range(1, int(rank[rank < RANK_BEYOND].max()) + 1):
        front = np.nonzero(rank == r)[0].tolist()
        want = textbook_crowding(keys.tolist(), front)
        assert same_bits(dist[front], np.array([want[i] for i in front]))
    assert (dist[rank >= RANK_BEYOND] == 0.0).all()


@pytest.mark.parametrize('E,M,N,seed', TINY)
def test_the_statement_is_the_brute_force_reading_with_ties(E, M, N, seed):
    rng = np.random.default_rng(200 + seed)
    keys = rng.integers(0, 4, size=(E, M)).astype(np.float64)
    keys[keys == 0.0] *= rng.choice([1.0, -1.0], size=int((keys == 0.0).sum()))      # -0.0 equals +0.0
    part = rng.random(E) >= 0.15
    agree(keys, part, N)


def test_fronts_by_hand():
    # duplicated extremes, a duplicate in the interior, and equal rows that do not dominate each other
    keys = [[0.0, 4.0], [0.0, 4.0], [1.0, 3.0], [1.0, 3.0], [2.0, 2.5], [4.0, 0.0],      # front 1
            [0.5, 2.0],                                                                  # front 2, alone
            [0.0, 1.0], [0.25, 0.5]]                                                     # front 3, two members
    rank, dist, pos = agree(keys, [True] * 9, 9)
    assert rank.tolist() == [1, 1, 1, 1, 1, 1, 2, 3, 3]
    assert dist[[0, 1, 5, 6, 7, 8]].tolist() == [INF] * 6                                # every duplicate of an extreme
    assert dist[2] == dist[3] == (1.0 - 1.0) / 4.0 + (3.0 - 3.0) / 4.0 == 0.0            # U = L = the duplicate
    assert dist[4] == (4.0 - 1.0) / 4.0 + (3.0 - 0.0) / 4.0
    assert pos.tolist() == [0, 1, 4, 5, 3, 2, 6, 7, 8]                                   # ties cut by e alone
    # peeling stops with the front that reaches N: the rest lies beyond, with distance 0
    rank, dist, pos = agree(keys, [True] * 9, 5)
    assert rank.tolist() == [1] * 6 + [RANK_BEYOND] * 3 and dist[6:].tolist() == [0.0] * 3
    # a candidate that takes no part ranks last, whatever its keys were
    rank, dist, pos = agree(keys, [False] + [True] * 8, 9)
    assert rank[0] == RANK_OUT and pos[0] == 8 and dist[0] == 0.0 and dist[1] == INF
    # nobody takes part
    rank, dist, pos = agree(keys, [False] * 9, 4)
    assert rank.tolist() == [RANK_OUT] * 9 and pos.tolist() == list(range(9))


def test_a_step_by_hand():
    # four rows, one dimension, two objectives x and -x on [0, 4]: every row is on the front, the ends are infinite
    s = Population([[1.0], [3.0], [2.0], [0.5]], [0.0], [4.0], [(0, MAX), (2, MIN)], seed=5, n_carry=1, b_star=0.0)
    scores = np.array([[1.0, np.nan, 1.0], [3.0, np.nan, 3.0], [2.0, np.nan, 2.0], [0.5, np.nan, 0.5]])
    nsga2_statement(s, scores=scores, carry_new=np.array([[10.0], [30.0], [20.0], [5.0]]))
    assert s.parents and s.g == 2 and s.counts.tolist() == [1, 4]
    # (the two ends first, by e; then the larger distance)
    assert s.origin.tolist() == [1, 3, 2, 0] and s.x[:, 0].tolist() == [3.0, 0.5, 2.0, 1.0]
    assert s.crowding.tolist() == [INF, INF, (3.0 - 1.0) / 2.5 + (3.0 - 1.0) / 2.5, (2.0 - 0.5) / 2.5 + (2.0 - 0.5) / 2.5]
    assert s.carry[:, 0].tolist() == [30.0, 5.0, 20.0, 10.0] and s.keys.tolist() == [[3.0, -3.0], [0.5, -0.5], [2.0, -2.0],
                                                                                     [1.0, -1.0]]
    assert s.part.tolist() == [1, 1, 1, 1] and s.rank.tolist() == [1, 1, 1, 1]
    # the offspring: a base row of the population plus f times a difference, reflected once; the launch rows follow
    for c in range(4):
        y = s.offspring[c, 0]
        assert 0.0 <= y <= 4.0 and not s.out[c] and s.rows[c, 0] == y
        assert any(y == v for base in s.x[:, 0] for a in s.x[:, 0] for b in s.x[:, 0]
                   for v in [base + 0.5 * (a - b)] + [2 * 0.0 - (base + 0.5 * (a - b)), 2 * 4.0 - (base + 0.5 * (a - b))])
    # the second call ranks eight candidates: NaN scores, an `out` flag and eligible = 0 keep an offspring out
    s.out[:] = [0, 1, 0, 0]
    scores = np.array([[9.0, 0.0, 9.0], [9.5, 0.0, 9.5], [np.nan, 0.0, 1.0], [0.1, 0.0, 0.1]])
    nsga2_statement(s, scores=scores, carry_new=np.zeros((4, 1)), eligible=np.array([1, 1, 1, 0]), vary=False)
    assert s.last['part'].tolist() == [True] * 4 + [True, False, False, False]
    assert np.isnan(s.last['keys'][5:]).all() and s.last['rank'][5:].tolist() == [RANK_OUT] * 3
    # five candidates on one front: the ends 0.5 (parent 1) and 9.0 (offspring 0 = candidate 4), then 3.0, 2.0; 1.0 is cut
    assert s.origin.tolist() == [1, 4, 0, 2] and s.g == 2 and s.x[:, 0].tolist()[0::2] == [0.5, 3.0]
    # a TARGET key
    assert st.keys_of(np.array([[1.0], [3.5]]), [0], [TARGET], [3.0]).tolist() == [[-2.0], [-0.5]]


# ---- the statement converges ---------------------------------------------------------------------------------------------
#: profiles/nsga2_statement.txt: the worst of the six seeds times two (tools/profile_nsga2_statement.py writes the file)
DISTANCE, GAP, ENDS = 0.066714, 0.060031, 0.019552


def test_the_thresholds_are_the_recorded_ones():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                             'nsga2_statement.txt')).read()
    recorded = re.search(r'thresholds \(worst x 2\):\s+distance (\S+)\s+gap (\S+)\s+ends (\S+)', text)
    assert recorded and [float(v) for v in recorded.groups()] == [DISTANCE, GAP, ENDS]


@pytest.mark.parametrize('seed', list(cases.CONVERGENCE['seeds']))
def test_the_statement_converges_on_the_segment(seed):
    """Two objectives, the negated squared distances to two points of the unit box, d = 6, N = 128, 60 generations: the
    population ends on the segment between the points, spread along it, both ends reached."""
    before, after, best = cases.convergence_run(seed)
    print('seed %d: distance %.6f -> %.6f, gap %.6f -> %.6f, ends %.6f' % (seed, before[0], after[0], before[1], after[1],
                                                                            after[2]))
    assert before[0] > 0.5
    assert after[0] <= DISTANCE
    assert after[1] <= GAP
    assert after[2] <= ENDS
    assert best.shape == (61, 2) and (np.diff(best, axis=0) >= 0.0).all()      # the best key of an objective never falls


def test_hypervolume_2d():
    assert nsga2.hypervolume_2d([[1.0, 3.0], [2.0, 2.0], [3.0, 1.0], [1.5, 1.5], [np.nan, 9.0], [-1.0, 9.0]], (0.0, 0.0)) == 6.0
    assert nsga2.hypervolume_2d([[2.0, 2.0]], (0.0, 1.0)) == 2.0 and nsga2.hypervolume_2d(np.zeros((0, 2)), (0.0, 0.0)) == 0.0
    assert nsga2.hypervolume_2d([[1.0, 1.0]], (1.0, 0.0)) == 0.0


def test_the_diagnostics_file(tmp_path):
    assert nsga2.diagnostics_header(['NSE', 'PBias']) == 'generation,front_size,best_NSE,best_PBias\n'
    path = str(tmp_path / 'Catchment.SMART.nsga2.diagnostics')
    nsga2.write_diagnostics(path, ['NSE', 'PBias'], np.array([[0.0, 7.0, 0.25, -1.5], [5.0, 31.0, 0.5, -0.125]]))
    assert open(path).read().split('\n') == ['generation,front_size,best_NSE,best_PBias', '0,7,2.500000e-01,-1.500000e+00',
                                             '5,31,5.000000e-01,-1.250000e-01', '']


# ---- the refusals of the C entry ------------------------------------------------------------------------------------------
TWO32 = 2 ** 32
K_ = 'smart_nsga2_step_hip'
W_ = 'smart_nsga2_workspace_bytes'
_LO = (ctypes.c_double * 16)(*([0.0] * 16))
_HI = (ctypes.c_double * 16)(*([1.0] * 16))
_COLS = (ctypes.c_int32 * 16)(*range(16))
_SC = (ctypes.c_int32 * 4)(0, 5, 6, 7)
_DIR = (ctypes.c_int32 * 4)(MAX, TARGET, MIN, MAX)
_TGT = (ctypes.c_double * 4)(0.0, 0.0, 0.0, 0.0)


def _addr(a):
    return ctypes.addressof(a)


def workspace_bytes(N):
    """the layout of smart_nsga2.hip, in Python"""
    part = lambda b: (b + 255) // 256 * 256         # noqa: E731
    W = (2 * N + 63) // 64
    Eld = 64 * W
    return (part(8) + part((N + 8) * 4) + part(2 * W * 8) + part(Eld * 32) + part(Eld) + 2 * part(Eld * 4) + part(Eld * 8)
            + part(max(W, 16) * Eld * 8))


VALID = dict(n_rows=8, n_dims=3, n_objectives=2, n_carry=2, seed=1, generation=2, parents=1, pop_x=FAKE, pop_keys=FAKE,
             pop_carry=FAKE, pop_part=FAKE, next_x=FAKE, next_keys=FAKE, next_carry=FAKE, next_part=FAKE, rank=FAKE,
             crowding=FAKE, origin=FAKE, counts=FAKE, offspring=FAKE, out=FAKE, scores=FAKE, ld_scores=8,
             score_columns=_addr(_SC), direction=_addr(_DIR), target=_addr(_TGT), eligible=None, carry_new=FAKE,
             workspace=FAKE, workspace_bytes=workspace_bytes(8), vary=1, lo=_addr(_LO), hi=_addr(_HI), scale=_addr(_LO),
             f=0.5, cr_threshold=TWO32, rows=FAKE, ld=10, columns=_addr(_COLS), stream=None)
SURVIVE = K_ + (': the survive phase needs next_x, next_keys, next_part, rank, crowding, origin, counts, score_columns and '
                'direction (%s is NULL)')
VARY = K_ + ': the vary phase needs lo, hi, scale, rows and columns (%s is NULL)'
_BAD_LO = (ctypes.c_double * 16)(*([0.0, 2.0] + [0.0] * 14))
_NAN_HI = (ctypes.c_double * 16)(*([1.0, 1.0, float('nan')] + [1.0] * 13))
_TWICE = (ctypes.c_int32 * 16)(*([4, 2, 4] + list(range(3, 16))))
_FAR = (ctypes.c_int32 * 16)(*([0, 10, 2] + list(range(3, 16))))
_NEG = (ctypes.c_int32 * 16)(*([-1, 1, 2] + list(range(3, 16))))
_SC_FAR = (ctypes.c_int32 * 4)(0, 8, 6, 7)
_SC_NEG = (ctypes.c_int32 * 4)(-1, 5, 6, 7)
_SC_TWICE = (ctypes.c_int32 * 4)(5, 5, 6, 7)
_DIR_BAD = (ctypes.c_int32 * 4)(MAX, 3, MIN, MAX)
_TGT_NAN = (ctypes.c_double * 4)(0.0, float('nan'), 0.0, 0.0)

CASES = [
    (dict(offspring=None), E_NULL, K_ + ': offspring and out are required (offspring is NULL)'),
    (dict(out=None), E_NULL, K_ + ': offspring and out are required (out is NULL)'),
    (dict(out=None, n_rows=0), E_NULL, K_ + ': offspring and out are required (out is NULL)'),       # pointers before sizes
    (dict(n_rows=3), E_SIZE, K_ + ': n_rows 3 must be in 4 .. 8192'),
    (dict(n_rows=8193), E_SIZE, K_ + ': n_rows 8193 must be in 4 .. 8192'),
    (dict(n_rows=3, n_dims=0), E_SIZE, K_ + ': n_rows 3 must be in 4 .. 8192'),                     # the first one wins
    (dict(n_dims=0), E_SIZE, K_ + ': n_dims 0 must be in 1 .. 16'),
    (dict(n_dims=17), E_SIZE, K_ + ': n_dims 17 must be in 1 .. 16'),
    (dict(n_objectives=1), E_SIZE, K_ + ': n_objectives 1 must be in 2 .. 4'),
    (dict(n_objectives=5), E_SIZE, K_ + ': n_objectives 5 must be in 2 .. 4'),
    (dict(n_carry=-1), E_SIZE, K_ + ': n_carry -1 must be in 0 .. 16'),
    (dict(n_carry=17), E_SIZE, K_ + ': n_carry 17 must be in 0 .. 16'),
    (dict(generation=0), E_SIZE, K_ + ': generation 0 must be in 1 .. 4294967295'),
    (dict(generation=TWO32), E_SIZE, K_ + ': generation 4294967296 must be in 1 .. 4294967295'),
    (dict(generation=0, direction=_addr(_DIR_BAD)), E_SIZE, K_ + ': generation 0 must be in 1 .. 4294967295'),
    (dict(scores=None, vary=0), E_NULL, K_ + ': neither phase is asked for (scores is NULL and vary is 0)'),
    # ---- the survive phase
    (dict(next_x=None), E_NULL, SURVIVE % 'next_x'),
    (dict(next_keys=None), E_NULL, SURVIVE % 'next_keys'),
    (dict(next_part=None), E_NULL, SURVIVE % 'next_part'),
    (dict(rank=None), E_NULL, SURVIVE % 'rank'),
    (dict(crowding=None), E_NULL, SURVIVE % 'crowding'),
    (dict(origin=None), E_NULL, SURVIVE % 'origin'),
    (dict(counts=None), E_NULL, SURVIVE % 'counts'),
    (dict(score_columns=None), E_NULL, SURVIVE % 'score_columns'),
    (dict(direction=None), E_NULL, SURVIVE % 'direction'),
    (dict(direction=None, rank=None), E_NULL, SURVIVE % 'rank'),
    (dict(pop_x=None), E_NULL, K_ + ': parents need pop_x, pop_keys and pop_part (pop_x is NULL)'),
    (dict(pop_keys=None), E_NULL, K_ + ': parents need pop_x, pop_keys and pop_part (pop_keys is NULL)'),
    (dict(pop_part=None), E_NULL, K_ + ': parents need pop_x, pop_keys and pop_part (pop_part is NULL)'),
    (dict(next_carry=None), E_NULL, K_ + ': n_carry 2 needs next_carry and carry_new (next_carry is NULL)'),
    (dict(carry_new=None), E_NULL, K_ + ': n_carry 2 needs next_carry and carry_new (carry_new is NULL)'),
    (dict(pop_carry=None), E_NULL, K_ + ': parents with n_carry 2 needs pop_carry (pop_carry is NULL)'),
    (dict(ld_scores=0), E_SIZE, K_ + ': ld_scores 0 must be in 1 .. 2^31 - 1'),
    (dict(score_columns=_addr(_SC_FAR)), E_SIZE, K_ + ': score column 8 of objective 1 is outside 0 .. ld_scores - 1 = 7'),
    (dict(score_columns=_addr(_SC_NEG)), E_SIZE, K_ + ': score column -1 of objective 0 is outside 0 .. ld_scores - 1 = 7'),
    (dict(ld_scores=5), E_SIZE, K_ + ': score column 5 of objective 1 is outside 0 .. ld_scores - 1 = 4'),
    (dict(score_columns=_addr(_SC_TWICE)), E_SIZE, K_ + ': score column 5 is named twice (objectives 0 and 1)'),
    (dict(direction=_addr(_DIR_BAD)), E_MODE, K_ + ": direction '3' of objective 1 unknown."),
    (dict(direction=_addr(_DIR_BAD), workspace=None), E_MODE, K_ + ": direction '3' of objective 1 unknown."),
    (dict(target=None), E_NULL, K_ + ': objective 1 is a TARGET (target is NULL)'),
    (dict(target=_addr(_TGT_NAN)), E_SIZE, K_ + ': target nan of objective 1 must be finite'),
    (dict(workspace=None), E_NULL, K_ + ': a workspace of %d bytes is needed (workspace is NULL)' % workspace_bytes(8)),
    (dict(workspace_bytes=workspace_bytes(8) - 1), E_SIZE,
     K_ + ': workspace_bytes %d, need %d' % (workspace_bytes(8) - 1, workspace_bytes(8))),
    (dict(n_rows=64), E_SIZE, K_ + ': workspace_bytes %d, need %d' % (workspace_bytes(8), workspace_bytes(64))),
    # ---- the vary phase
    (dict(lo=None), E_NULL, VARY % 'lo'),
    (dict(hi=None), E_NULL, VARY % 'hi'),
    (dict(scale=None), E_NULL, VARY % 'scale'),
    (dict(rows=None), E_NULL, VARY % 'rows'),
    (dict(columns=None), E_NULL, VARY % 'columns'),
    (dict(scores=None, parents=0), E_NULL,
     K_ + ': the vary phase needs a population: the survive phase, or parents (scores is NULL)'),
    (dict(scores=None, pop_x=None), E_NULL, K_ + ': the vary phase without the survive phase reads pop_x (pop_x is NULL)'),
    (dict(f=float('nan')), E_SIZE, K_ + ': f nan must be finite'),
    (dict(f=float('inf')), E_SIZE, K_ + ': f inf must be finite'),
    (dict(cr_threshold=-1), E_SIZE, K_ + ': cr_threshold -1 must be in 0 .. 4294967296'),
    (dict(cr_threshold=TWO32 + 1), E_SIZE, K_ + ': cr_threshold 4294967297 must be in 0 .. 4294967296'),
    (dict(ld=2), E_SIZE, K_ + ': ld 2 is less than n_dims 3'),
    (dict(columns=_addr(_FAR)), E_SIZE, K_ + ': columns[1] 10 must be in 0 .. 9'),
    (dict(columns=_addr(_NEG)), E_SIZE, K_ + ': columns[0] -1 must be in 0 .. 9'),
    (dict(columns=_addr(_TWICE)), E_SIZE, K_ + ': columns[0] and columns[2] name the same column 4'),
    (dict(lo=_addr(_BAD_LO)), E_SIZE, K_ + ': lo[1] 2 and hi[1] 1: need finite lo <= hi'),
    (dict(hi=_addr(_NAN_HI)), E_SIZE, K_ + ': lo[2] 0 and hi[2] nan: need finite lo <= hi'),
    (dict(workspace=None, lo=None), E_NULL,
     K_ + ': a workspace of %d bytes is needed (workspace is NULL)' % workspace_bytes(8)),   # survive before vary
]


def _case_id(i, changes):
    return '%02d-' % i + '-'.join(changes)


@pytest.mark.parametrize('changes,code,text', CASES, ids=[_case_id(i, c[0]) for i, c in enumerate(CASES)])
def test_refusals(changes, code, text):
    assert refusal({K_: VALID}, K_, changes) == (code, text)


def test_a_well_formed_call_gets_as_far_as_the_device():
    L = _lib.lib()
    if L.smart_device_count() == 0:
        # ... and no further: there is no CPU fallback
        for changes in (dict(), dict(vary=0), dict(vary=0, lo=None, hi=None, scale=None, rows=None, columns=None),
                        dict(scores=None), dict(scores=None, next_x=None, next_keys=None, next_part=None, rank=None,
                                                crowding=None, origin=None, counts=None, score_columns=None,
                                                direction=None, workspace=None, workspace_bytes=0),
                        dict(parents=0, pop_x=None, pop_keys=None, pop_carry=None, pop_part=None),
                        dict(n_carry=0, pop_carry=None, next_carry=None, carry_new=None),
                        dict(n_rows=4, n_dims=1, n_objectives=4), dict(n_dims=16, ld=16, n_carry=16),
                        dict(n_rows=8192, workspace_bytes=workspace_bytes(8192), generation=TWO32 - 1),
                        dict(cr_threshold=0, f=0.0), dict(eligible=FAKE), dict(workspace_bytes=workspace_bytes(8) + 1)):
            rc, text = refusal({K_: VALID}, K_, changes)
            assert rc == E_NO_DEVICE and 'device' in text, changes
    else:
        # with a device the refusals leave the error text as they set it, and the entry is run for real by
        # tests/test_gpu_nsga2.py
        assert refusal({K_: VALID}, K_, dict(offspring=None))[0] == E_NULL


def test_the_workspace_query():
    L = _lib.lib()
    for N in (4, 5, 32, 33, 64, 1030, 8192):
        for M in (2, 3, 4):
            assert L.smart_nsga2_workspace_bytes(N, M) == workspace_bytes(N), (N, M)
    assert 0 < workspace_bytes(8192) - (32 << 20) < 1 << 20          # the bit matrix is 32 MiB of it, the rest below 1 MiB
    for N, M in ((3, 2), (0, 2), (-1, 2), (8193, 2), (4, 1), (4, 5), (8192, 0)):
        assert L.smart_nsga2_workspace_bytes(N, M) == E_SIZE, (N, M)


def test_the_new_names_are_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'smart_amd.h')).read()
    assert K_ in _lib.SYMBOLS and W_ in _lib.SYMBOLS and getattr(_lib.lib(), K_) is not None
    assert _lib.SYMBOLS[K_][0] is ctypes.c_int and len(_lib.SYMBOLS[K_][1]) == len(VALID) == 40
    assert _lib.SYMBOLS[W_] == (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32])
    declared = re.search(r'^int %s\(([^;]*)\);' % K_, header, re.M)
    names = re.findall(r'(\w+)\s*(?:,|$)', declared.group(1).replace('\n', ' '))
    assert names == list(VALID)                      # the dictionary above is the entry's argument list, in its order
    for macro, value in (('SMART_NSGA2_MAX_ROWS', 8192), ('SMART_NSGA2_MAX_DIMS', 16), ('SMART_NSGA2_MAX_OBJECTIVES', 4),
                         ('SMART_NSGA2_MAX_CARRY', 16), ('SMART_NSGA2_RANK_BEYOND', RANK_BEYOND),
                         ('SMART_NSGA2_RANK_OUT', RANK_OUT)):
        assert re.search(r'^#define %s %d$' % (macro, value), header, re.M), macro
    assert (_lib.NSGA2_MAX_ROWS, _lib.NSGA2_MAX_DIMS, _lib.NSGA2_MAX_OBJECTIVES, _lib.NSGA2_MAX_CARRY) == (8192, 16, 4, 16)
    assert (_lib.NSGA2_RANK_BEYOND, _lib.NSGA2_RANK_OUT) == (RANK_BEYOND, RANK_OUT) and _lib.lib().smart_abi_version() == 7
    assert _lib.PARETO_DIRECTIONS == {'max': MAX, 'min': MIN, 'target': TARGET}
    from smartpy_amd import build
    assert build.UNITS['smart_nsga2.hip'] == ['-ffp-contract=off']
    from smartpy_amd import montecarlo
    assert 'NSGA2' in montecarlo.__all__
    assert 'pow' in nsga2.__doc__ and 'pow' in montecarlo.NSGA2.__doc__      # why there is no SBX: said where users read


# ---- the refusals of the binding and of montecarlo.NSGA2 --------------------------------------------------------------------
def test_the_words_of_the_binding():
    assert nsga2.cr_threshold(1.0) == TWO32 and nsga2.cr_threshold(0.0) == 0 and nsga2.cr_threshold(0.9) == int(0.9 * TWO32)
    with pytest.raises(_lib.SmartEngineError, match=r'cr 1.5 must be in \[0, 1\]'):
        nsga2.cr_threshold(1.5)
    cols, code, target = nsga2.directions_of([(0, 'max'), (5, ('target', 0.0)), (6, 'min')])
    assert (cols.tolist(), code.tolist(), target.tolist()) == ([0, 5, 6], [MAX, TARGET, MIN], [0.0, 0.0, 0.0])
    for bad, code in (([(0, 'max')], -2), ([(m, 'max') for m in range(5)], -2), ([(0, 'max'), (0, 'min')], -2),
                      ([(0, 'up'), (1, 'min')], -7), ([(0, 'target'), (1, 'min')], -7), ([(0, ('max', 1.0)), (1, 'min')], -7)):
        with pytest.raises(_lib.SmartEngineError) as err:
            nsga2.directions_of(bad)
        assert err.value.code == code, bad


def test_the_constructor_refuses(tmp_path):
    from smartpy_amd.montecarlo import NSGA2
    from smartpy_amd.montecarlo.montecarlo import MonteCarlo
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.nsga2.sttngs', '01/01/2007', '31/12/2007', 90, simu_minutes=1440)

    def make(objectives=('NSE', 'PBias'), **kw):
        return NSGA2('Catchment', root, 'csv', 'csv', objectives, settings_filename='Catchment.nsga2.sttngs', **kw)
    for kw, code, words in ((dict(objectives=['NSE']), -2, '1 objectives, between 2 and 4'),
                            (dict(objectives=['NSE', 'KGE', 'KGEc', 'RMSE', 'PBias']), -2, '5 objectives, between 2 and 4'),
                            (dict(objectives=['NSE', 'nse']), -7, r"\['nse'\] are not among"),
                            (dict(objectives={'NSE': 'max', 'Bias': 'min'}), -7, r"\['Bias'\] are not among"),
                            (dict(population=3), -2, 'a population of 3 rows, between 4 and 8192'),
                            (dict(population=8193), -2, 'a population of 8193 rows, between 4 and 8192'),
                            (dict(vary=['T'] * 17), -2, '17 dimensions, at most 16'),
                            (dict(generations=0), -2, 'need generations >= 1'),
                            (dict(cr=1.5), -2, 'cr 1.5 must be in'),
                            (dict(objectives={'NSE': 'up', 'PBias': 'min'}), -7, "direction 'up' unknown")):
        with pytest.raises(_lib.SmartEngineError, match=words) as err:
            make(**kw)
        assert err.value.code == code, kw
    with pytest.raises(Exception, match='`vary` must name at least one of'):
        make(vary=['T', 'T'])
    with pytest.raises(Exception, match='are unknown or also vary'):
        make(vary=['T'], fixed={'T': 1.0})
    obj = make(population=8, generations=2, vary=['T', 'SK'], fixed={'C': 0.5}, seed=3)
    assert isinstance(obj, MonteCarlo) and obj.db_file.endswith('Catchment.SMART.nsga2')
    assert obj.diagnostics_file.endswith('Catchment.SMART.nsga2.diagnostics')
    assert obj.objectives == [(0, 'max'), (5, ('target', 0.0))] and obj._sample.shape == (8, 10)
    names = obj.param_names
    assert (obj._sample[:, names.index('C')] == 0.5).all() and len(set(obj._sample[:, names.index('T')])) == 8
    assert obj.columns == [names.index('T'), names.index('SK')] and obj.front_index is None
