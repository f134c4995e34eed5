"""NSGA-II on the device: smart_nsga2_step_hip against the numpy statement of oracle/analyses/nsga2.py BIT FOR BIT -- the
population (parameters, keys, payload, flags), ranks, crowding distances, origins, the two counters, offspring, `out` flags
and launch rows after every one of 40 generations, inside buffers with guards; stress inputs (massive ties, a chain of
fronts, one front cut by crowding alone, candidates that take no part, the first call); the rank-1 set against
engine.pareto_counts; the same bits from two copies of a state; and montecarlo.NSGA2 end to end on the example catchment.

The test plays the score function: it copies the launch rows to the host, evaluates distances to anchor points in numpy
and uploads a score table as wide as the engine's; the statement gets the same numbers.  No operation of the step is
rounded otherwise than numpy rounds it, so there is no margin to watch."""

import numpy as np
import pytest

import oracle.analyses.nsga2 as st
from oracle.analyses.nsga2 import MAX, MIN, TARGET, RANK_BEYOND, RANK_OUT, Population, nsga2_statement
from support import EXTRA, GATE, Guarded, example_root, same_bits, settings_file

pytestmark = pytest.mark.gpu

GUARD = 32
SENTINEL = {'float64': -7.0, 'int32': -7, 'uint8': 0xA5}
SHARED = ('rank', 'crowding', 'origin', 'counts', 'offspring', 'out', 'rows')
BUFFERED = ('x', 'keys', 'carry', 'part')
WORDS = {MAX: 'max', MIN: 'min'}
LD_SCORES = 8
SCORE_COLUMNS = [6, 1, 4, 3]


def into_guards(state):
    """Every array of the state moved into the middle of a buffer of its own with GUARD sentinels on either side -> the
    buffers"""
    buffers = []
    for owner, names in [(state, SHARED)] + [(b, BUFFERED) for b in state.buffers]:
        for name in names:
            t = getattr(owner, name)
            dtype = str(t.dtype).split('.')[-1]
            g = Guarded(t.numel(), dtype=dtype, guard=GUARD, sentinel=SENTINEL[dtype])
            inner = g.inner().view(t.shape)
            inner.copy_(t)
            setattr(owner, name, inner)
            buffers.append(g)
    return buffers


def objectives_of(M, kinds):
    """[(column, direction)] of the statement and of the device state, from kinds like ('max', 'min', 'target')"""
    of_statement, of_device = [], []
    for m in range(M):
        col, kind = SCORE_COLUMNS[m], kinds[m % len(kinds)]
        of_statement.append((col, MAX if kind == 'max' else (MIN if kind == 'min' else (TARGET, 0.25))))
        of_device.append((col, kind if kind != 'target' else ('target', 0.25)))
    return of_statement, of_device


def anchors(lo, hi, M, kinds):
    """A score function of the test's own: objective m is the squared distance, in units of the box, to an anchor point --
    negated where it is to be maximised, plain where it is to be minimised, its square root where it aims at a target"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    d = len(lo)
    points = np.random.default_rng(77).uniform(0.15, 0.85, size=(M, d))

    def table(x):
        u = (x - lo[None, :]) / (hi - lo)[None, :]
        scores = np.full((len(x), LD_SCORES), np.nan)
        for m in range(M):
            kind = kinds[m % len(kinds)]
            r2 = ((u - points[m][None, :]) ** 2).sum(axis=1)
            scores[:, SCORE_COLUMNS[m]] = -r2 if kind == 'max' else (r2 if kind == 'min' else np.sqrt(r2))
        return scores
    return table


def payload_of(x, n_carry):
    return np.ascontiguousarray(x.sum(axis=1)[:, None] * np.arange(1.0, n_carry + 1.0)[None, :])


def make_pair(N, d, M, seed, kinds=('max', 'min', 'target'), cr=0.9, f=0.5, b_star=1e-6, n_carry=3, columns=None, ld=None,
              width=None, lo=None, hi=None):
    """The statement's Population and the device's Nsga2State from one initial population"""
    import torch
    from smartpy_amd import nsga2
    rng = np.random.default_rng(1000 + seed)
    lo = np.linspace(-1.0, 2.0, d) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = lo + np.linspace(1.0, 30.0, d) if hi is None else np.asarray(hi, dtype=np.float64)
    x0 = rng.uniform(lo, hi, size=(N, d))
    of_statement, of_device = objectives_of(M, kinds)
    common = dict(seed=seed, f=f, cr=cr, b_star=b_star, n_carry=n_carry, columns=columns)
    s = Population(x0, lo, hi, of_statement, ld=ld, fill=np.nan, **common)
    if width is not None:           # a launch matrix `width` wide inside ld columns: fixed columns 0.5, NaN in the padding
        s.rows[:, :width] = 0.5
        s.rows[:, s.columns] = x0
    rows = torch.from_numpy(s.rows.copy()).cuda()
    t = nsga2.Nsga2State(x0, lo, hi, of_device, rows=rows, **common)
    return s, t


def compare(s, t, where=''):
    for name in SHARED + BUFFERED:
        got = getattr(t, name).cpu().numpy()
        want = getattr(s, name)
        assert same_bits(got, want.astype(got.dtype) if name in ('out', 'part') else want), (name, where)
    assert (s.g, s.parents) == (t.g, t.parents), where


def spoil(scores, g, M):
    """NaN among the selected scores of generation g, and rows that are not eligible: offspring that take no part"""
    scores = scores.copy()
    n = len(scores)
    scores[(np.arange(n) + g) % 11 == 3, SCORE_COLUMNS[g % M]] = np.nan
    eligible = ((np.arange(n) + 2 * g) % 13 != 5).astype(np.uint8)
    return scores, eligible


def device_step(t, scores, carry_new, eligible=None, vary=True):
    import torch
    from smartpy_amd import nsga2
    nsga2.nsga2_step(t, scores=None if scores is None else torch.from_numpy(np.ascontiguousarray(scores)).cuda(),
                     carry_new=None if carry_new is None else torch.from_numpy(carry_new).cuda(),
                     eligible=None if eligible is None else torch.from_numpy(eligible).cuda(), vary=vary)


def run_both(s, t, table, generations, spoiled=True, tables=None):
    """The loop of montecarlo.NSGA2 on the statement and on the device, each fed from its own launch rows, compared after
    every generation -> (the `out` offspring seen, the fronts peeled per call).  tables: the score table of a generation
    from (launch rows, g), where the test plays another function than `table`."""
    n_carry, M = s.carry.shape[1], len(s.score_columns)
    outs, fronts, idle = 0, [], run_both.idle
    del idle[:]
    for g in range(0, generations + 1):
        launched_s = s.rows[:, s.columns]
        launched_t = t.rows.cpu().numpy()[:, s.columns]
        sc_s, sc_t = (table(launched_s), table(launched_t)) if tables is None else (tables(launched_s, g), tables(launched_t, g))
        el = None
        if spoiled and g > 0:
            (sc_s, el), (sc_t, _) = spoil(sc_s, g, M), spoil(sc_t, g, M)
        vary = g < generations
        nsga2_statement(s, scores=sc_s, carry_new=payload_of(launched_s, n_carry), eligible=el, vary=vary)
        device_step(t, sc_t, payload_of(launched_t, n_carry), eligible=el, vary=vary)
        compare(s, t, where='generation %d' % g)
        outs += int(s.out.sum()) if vary else 0
        fronts.append(int(s.counts[0]))
        idle.append(int((s.part == 0).sum()))
    return outs, fronts


run_both.idle = []      # after a run: the rows of the population that take no part, per generation


CASES = {
    # name: (N, d, M, seed, extra arguments of make_pair)
    'one-wavefront-two-mask-words': (64, 3, 2, 1, dict()),
    'ragged-third-word-d1': (65, 1, 2, 2, dict(kinds=('max', 'max'))),
    'several-workgroups-m3': (300, 10, 3, 3, dict(columns=[7, 2, 5, 0, 1, 3, 4, 6, 8, 9], ld=13, width=10, n_carry=9)),
    'ragged-slices-d16-m4': (1030, 16, 4, 4, dict(n_carry=16, cr=0.2)),
    'smallest-population': (4, 2, 2, 5, dict(n_carry=0)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_the_step_is_the_statement_bit_for_bit(name):
    N, d, M, seed, extra = CASES[name]
    s, t = make_pair(N, d, M, seed, **extra)
    buffers = into_guards(t)
    kinds = extra.get('kinds', ('max', 'min', 'target'))
    outs, fronts = run_both(s, t, anchors(s.lo, s.hi, M, kinds), generations=40)
    compare(s, t)
    assert all(b.intact() for b in buffers)
    assert (s.g, t.current) == (41, 1) and min(fronts) >= 1
    assert (s.rank[:-1] <= s.rank[1:]).all()                      # the population lies in tournament order
    same_rank = s.rank[:-1] == s.rank[1:]
    assert (s.crowding[:-1][same_rank] >= s.crowding[1:][same_rank]).all()
    if name == 'ragged-slices-d16-m4':
        assert s.fallbacks > 0                                      # CR 0.2: no dimension drawn, the fallback dimension taken
    if name == 'several-workgroups-m3':                             # the other columns as the caller left them
        rows = t.rows.cpu().numpy()
        assert np.isnan(rows[:, 10:]).all() and rows.shape == (300, 13)
    if N >= 64:                                                     # the population has moved towards the front
        assert int(s.counts[1]) > N // 4


# ---- stress inputs -----------------------------------------------------------------------------------------------------------
def five_integers(launched, g):
    rng = np.random.default_rng(500 + g)
    scores = np.full((len(launched), LD_SCORES), np.nan)
    scores[:, SCORE_COLUMNS[0]] = rng.integers(0, 5, len(launched))
    scores[:, SCORE_COLUMNS[1]] = rng.integers(0, 5, len(launched))
    return scores


def chain(launched, g):
    scores = np.full((len(launched), LD_SCORES), np.nan)
    scores[:, SCORE_COLUMNS[0]] = launched[:, 0] + 0.001 * g
    scores[:, SCORE_COLUMNS[1]] = scores[:, SCORE_COLUMNS[0]]
    return scores


def one_front(launched, g):
    scores = chain(launched, g)
    scores[:, SCORE_COLUMNS[1]] = -scores[:, SCORE_COLUMNS[0]]
    return scores


@pytest.mark.parametrize('N', [64, 300])
@pytest.mark.parametrize('what', ['five-integers', 'chain', 'one-front', 'few-take-part'])
def test_stress_inputs(what, N):
    d, generations = 2, 6
    if what == 'few-take-part':
        # a box as narrow as the jitter: `out` occurs; NaN scores and rows that are not eligible on top of it
        s, t = make_pair(N, d, 2, 20, kinds=('max', 'max'), lo=[0.0, 0.0], hi=[1.0, 1.0], b_star=2.0)
    else:
        s, t = make_pair(N, d, 2, 21, kinds=('max', 'max'))
    buffers = into_guards(t)

    def quarter(launched, g):
        # three quarters of the first rows and a quarter of every later generation's have a NaN score
        scores = one_front(launched, g)
        i = np.arange(len(scores))
        scores[(i % 4 != 0) if g == 0 else ((i + g) % 4 == 0), SCORE_COLUMNS[g % 2]] = np.nan
        return scores
    tables = {'five-integers': five_integers, 'chain': chain, 'one-front': one_front, 'few-take-part': quarter}[what]
    outs, fronts = run_both(s, t, None, generations, spoiled=what == 'few-take-part', tables=tables)
    assert all(b.intact() for b in buffers)
    if what == 'five-integers':     # at most 25 different rows: duplicates everywhere, the cut is made by e alone
        assert len(np.unique(s.keys, axis=0)) <= 25 and np.isinf(s.crowding).sum() > 2
    if what == 'chain':             # one front per distinct value: N fronts, far beyond the first batch of 16 passes
        assert fronts[0] == N and min(fronts[1:]) > 16 and s.rank[0] == 1 and s.rank[-1] > 16
    if what == 'one-front':         # every candidate on front 1, the N survivors chosen by crowding
        assert fronts == [1] * (generations + 1) and s.counts.tolist() == [1, 2 * N]
        assert (s.rank == 1).all() and np.isinf(s.crowding[:2]).all() and np.isinf(s.crowding).sum() < N // 4
    if what == 'few-take-part':
        # fewer than N of the 2 N candidates of the second call took part: rows that take no part filled the population
        assert outs > 0 and run_both.idle[0] > N // 2 and run_both.idle[1] > 0
        assert (s.rank[s.part == 0] == RANK_OUT).all() and np.isnan(s.keys[s.part == 0]).all()
        assert (s.rank[s.part != 0] < RANK_BEYOND).all()


@pytest.mark.parametrize('N', [64, 300])
def test_the_first_call(N):
    """No parents: the N launched rows are the candidates, all of them enter the population -- ranked, or beyond"""
    s, t = make_pair(N, 3, 3, 30)
    buffers = into_guards(t)
    table = anchors(s.lo, s.hi, 3, ('max', 'min', 'target'))(s.rows[:, s.columns])
    table[5, SCORE_COLUMNS[1]] = np.nan
    eligible = np.ones(N, dtype=np.uint8)
    eligible[7] = 0
    nsga2_statement(s, scores=table, carry_new=payload_of(s.offspring, 3), eligible=eligible, vary=False)
    device_step(t, table, payload_of(s.offspring, 3), eligible=eligible, vary=False)
    compare(s, t)
    assert all(b.intact() for b in buffers)
    assert sorted(s.origin.tolist()) == list(range(N)) and s.origin[-2:].tolist() == [5, 7]
    assert s.rank[-2:].tolist() == [RANK_OUT] * 2 and (s.rank[:-2] < RANK_BEYOND).all() and t.g == 1 and t.parents


# ---- the rank-1 set against the Pareto kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize('N,M', [(64, 2), (300, 3), (1030, 4)])
def test_rank_one_is_what_pareto_counts_leaves_undominated(N, M):
    import torch
    from smartpy_amd import engine
    s, t = make_pair(N, 4, M, 40)
    table = anchors(s.lo, s.hi, M, ('max', 'min', 'target'))
    run_both(s, t, table, generations=3)
    # the 2 N candidates of one more call: the parents' keys as they lie, the offspring's from their scores
    launched = t.rows.cpu().numpy()[:, s.columns]
    scores, eligible = spoil(table(launched), 4, M)
    parents, parents_part, out = t.keys.clone(), t.part.clone(), t.out.cpu().numpy()
    device_step(t, scores, payload_of(launched, 3), eligible=eligible, vary=False)
    fresh = st.keys_of(scores, s.score_columns, s.direction, s.target)
    keys = torch.cat([parents, torch.from_numpy(fresh).cuda()])
    takes = torch.cat([parents_part, torch.from_numpy(((out == 0) & (eligible != 0)).astype(np.uint8)).cuda()])
    counts = engine.pareto_counts(keys, ['max'] * M, eligible=takes).cpu().numpy()
    undominated = np.nonzero(counts == 0)[0]
    rank, origin = t.rank.cpu().numpy(), t.origin.cpu().numpy()
    assert int(t.counts[1]) == len(undominated) > 0
    if len(undominated) <= N:
        assert sorted(origin[rank == 1].tolist()) == undominated.tolist()
    else:
        assert (rank == 1).all() and np.isin(origin, undominated).all()
    assert (counts[origin[rank == RANK_OUT]] == -1).all()


# ---- determinism -------------------------------------------------------------------------------------------------------------
def test_the_same_call_on_two_copies_gives_the_same_bits():
    results = []
    for _ in range(2):
        s, t = make_pair(300, 5, 3, 50)
        table = anchors(s.lo, s.hi, 3, ('max', 'min', 'target'))
        for g in range(0, 6):
            launched = t.rows.cpu().numpy()[:, s.columns]
            scores, eligible = spoil(table(launched), g, 3)
            device_step(t, scores, payload_of(launched, 3), eligible=eligible, vary=True)
        results.append({name: getattr(t, name).cpu().numpy() for name in SHARED + BUFFERED})
    for name in SHARED + BUFFERED:
        assert same_bits(results[0][name], results[1][name]), name
    # ... and another seed gives other offspring
    _, other = make_pair(300, 5, 3, 51)
    assert not same_bits(other.offspring.cpu().numpy(), results[0]['offspring'])


# ---- montecarlo.NSGA2 end to end ---------------------------------------------------------------------------------------------
def _calibration(root, **kw):
    from smartpy_amd.montecarlo import NSGA2
    args = dict(population=128, generations=5, seed=3, thin=2, settings_filename='Catchment.nsga2.sttngs')
    args.update(kw)
    obj = NSGA2('Catchment', root, 'csv', 'csv', ['NSE', 'PBias'], **args)
    obj.model.extra = EXTRA
    return obj


@pytest.mark.parametrize('gw_constraint', [False, True])
def test_nsga2_end_to_end(tmp_path, gw_constraint):
    import torch
    from smartpy_amd import engine
    from smartpy_amd.montecarlo import Pareto
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.nsga2.sttngs', '01/01/2007', '31/12/2009', 180, simu_minutes=1440)
    a = _calibration(root, gw_constraint=gw_constraint)
    a.run(write=True)
    N = 128
    # ---- the files
    db = open(a.db_file, 'rb').read()
    assert a.db_file.endswith('Catchment.SMART.nsga2') and len(db.split(b'\n')) == N + 2
    lines = open(a.diagnostics_file).read().split('\n')
    assert lines[0] == 'generation,front_size,best_NSE,best_PBias' and len(lines) == 4 + 2
    assert a.diagnostics[:, 0].tolist() == [0.0, 2.0, 4.0, 5.0] and a.diagnostics.shape == (4, 4)
    assert (np.diff(a.diagnostics[:, 2:], axis=0) >= 0.0).all()             # the best keys never fall
    # ---- shapes, and the tournament order of the population
    assert a._sample.shape == (N, 10) and a.obj_fns.shape == (N, 8) and tuple(a.device_obj_fns.shape) == (N, 8)
    assert a.rank.shape == a.crowding.shape == (N,) and (a.rank[:-1] <= a.rank[1:]).all()
    assert a.front_index.tolist() == list(range(len(a.front_index)))
    assert len(a.front_index) == min(a.diagnostics[-1, 1], N) > 0        # (front_size counts parents and offspring)
    ranges = a.model.parameters.ranges
    for j, p in enumerate(a.param_names):
        assert (a._sample[:, j] >= ranges[p][0]).all() and (a._sample[:, j] <= ranges[p][1]).all(), p
    # ---- a fresh launch of the final rows gives the objective functions they carried
    out = a.model.simulate_ensemble(a.device_sample, objective_functions=True, gw_constraint=a.constraints['gw'],
                                    save_discharge=False, math_mode=a.math_mode)
    fresh = torch.cat([out.objfn[:N], out.gw[:N].unsqueeze(1)], dim=1).cpu().numpy()
    carried = a.state.carry.cpu().numpy()
    close = (np.abs(fresh - carried) <= GATE * np.maximum(1.0, np.abs(carried))) | (np.isnan(fresh) & np.isnan(carried))
    assert close.all(), np.nanmax(np.abs(fresh - carried))
    assert same_bits(carried[:, :8], a.obj_fns) and same_bits(carried[:, 8], a.gw_contributions)
    # ---- the keys are the carried objective functions: NSE, and -|PBias|
    keys = a.keys.cpu().numpy()
    takes = a.state.part.cpu().numpy() != 0
    assert same_bits(keys[takes], np.stack([carried[takes, 0], -np.abs(carried[takes, 5] - 0.0)], axis=1))
    if gw_constraint:
        assert (takes == (carried[:, 7] > 0.0)).all()
    else:
        assert takes.all()
    # ---- the front is what the Pareto kernel leaves undominated in the final population
    counts = engine.pareto_counts(a.device_obj_fns, ['max', ('target', 0.0)], columns=[0, 5],
                                  eligible=torch.from_numpy(takes.astype(np.uint8)).cuda()).cpu().numpy()
    assert np.nonzero(counts == 0)[0].tolist() == a.front_index.tolist()
    assert (a.rank[counts == -1] == RANK_OUT).all()
    # ---- the second stages take the object as they take an LHS run
    if not gw_constraint:
        front = Pareto('Catchment', root, 'csv', 'csv', ['NSE', 'PBias'], settings_filename='Catchment.nsga2.sttngs',
                       sampling=a)
        assert np.asarray(front.pareto_index).tolist() == a.front_index.tolist()
