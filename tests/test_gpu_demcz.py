"""DE-MCz on the device: smart_demcz_step_hip against the numpy statement of oracle/analyses/demcz.py BIT FOR BIT -- chain
states, log-densities, payload, acceptance counts, `out` flags, proposals, launch rows and the whole archive after 40
generations, on both sides of every switch, inside buffers with guards; the score kinds that take a logarithm or a
quotient on the device; the same bits from one seed however the call is cut (phases, parts of the chains); and
montecarlo.DEMCz end to end on the example catchment.

The test plays the density: it copies the launch rows to the host, evaluates a quadratic form in numpy and uploads the
scores; the statement gets the same numbers.  The one device operation that is not correctly rounded by definition is
log(u), so every comparison first asserts that the statement's smallest decision margin is far above what a last-bit
difference of a logarithm can move."""

import numpy as np
import pytest

from oracle.analyses.demcz import Chains, demcz_statement, log_density, LOGP, RMSE, RMSE_SIGMA
from support import EXTRA, Guarded, example_root, same_bits, settings_file

pytestmark = pytest.mark.gpu

GUARD = 32
SENTINEL = {'float64': -7.0, 'int32': -7, 'uint8': 0xA5}
ARRAYS = ('x', 'logp', 'carry', 'accepted', 'proposal', 'out', 'archive', 'archive_logp', 'archive_carry', 'rows')
MARGIN = 1e-12


def into_guards(state):
    """Every array of the state moved into the middle of a buffer of its own with GUARD sentinels on either side -> the
    buffers, by name."""
    buffers = {}
    for name in ARRAYS:
        t = getattr(state, name)
        dtype = str(t.dtype).split('.')[-1]
        buffers[name] = Guarded(t.numel(), dtype=dtype, guard=GUARD, sentinel=SENTINEL[dtype])
        inner = buffers[name].inner().view(t.shape)
        inner.copy_(t)
        setattr(state, name, inner)
    return buffers


def quadratic(lo, hi, width=0.2):
    """A log-density of the test's own: a Gaussian around the middle of the box, `width` of its extent wide"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    centre, w = 0.5 * (lo + hi), width * (hi - lo)

    def density(x):
        r = (x - centre[None, :]) / w[None, :]
        return -0.5 * (r * r).sum(axis=1)
    return density


def payload_of(x, n_carry):
    return np.ascontiguousarray(x.sum(axis=1)[:, None] * np.arange(1.0, n_carry + 1.0)[None, :])


def make_pair(N, d, seed, cr, p_jump, b_star=1e-6, n_carry=3, columns=None, ld=None, width=None, prefill=0, snapshots=11,
              lo=None, hi=None, **score):
    """The statement's Chains and the device's DemczState from one initial population, the archive filled exactly"""
    import torch
    from smartpy_amd import demcz
    rng = np.random.default_rng(1000 + seed)
    lo = np.linspace(-1.0, 2.0, d) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = lo + np.linspace(1.0, 30.0, d) if hi is None else np.asarray(hi, dtype=np.float64)
    x0 = rng.uniform(lo, hi, size=(N, d))
    capacity = prefill + snapshots * N
    common = dict(seed=seed, cr=cr, p_jump=p_jump, b_star=b_star, n_carry=n_carry, columns=columns)
    s = Chains(x0, lo, hi, capacity, ld=ld, fill=np.nan, score_kind=score.get('score_kind', LOGP),
               n_obs=score.get('n_obs', 0), n_eff=score.get('n_eff', 0.0), sigma=score.get('sigma', 0.0), **common)
    if width is not None:           # a launch matrix `width` wide inside ld columns: fixed columns 0.5, NaN in the padding
        s.rows[:, :width] = 0.5
        s.rows[:, s.columns] = x0
    rows = torch.from_numpy(s.rows.copy()).cuda()
    t = demcz.DemczState(x0, lo, hi, capacity, rows=rows, score_kind=score.get('score_kind', LOGP),
                         n_obs=score.get('n_obs', 0), n_eff=score.get('n_eff', 0.0), sigma=score.get('sigma', 0.0), **common)
    if prefill:
        seeds = rng.uniform(lo, hi, size=(prefill, d))
        s.archive[:prefill] = seeds
        s.archive_logp[:prefill] = -1.0
        t.archive[:prefill] = torch.from_numpy(seeds).cuda()
        t.archive_logp[:prefill] = -1.0
        s.M = t.M = prefill
    return s, t


def compare(s, t, what=ARRAYS):
    for name in what:
        got = getattr(t, name).cpu().numpy()
        want = getattr(s, name)
        assert same_bits(got, want.astype(got.dtype) if name == 'out' else want), name
    assert (s.M, s.g) == (t.M, t.g)


def spoil(scores, g):
    """NaN and -inf among the scores of generation g: proposals that are rejected whatever u is"""
    scores = scores.copy()
    n = len(scores)
    scores[(np.arange(n) + g) % 11 == 3] = np.nan
    scores[(np.arange(n) + g) % 13 == 5] = -np.inf
    return scores


def device_step(t, scores, carry_new, **kw):
    import torch
    from smartpy_amd import demcz
    demcz.demcz_step(t, scores=None if scores is None else torch.from_numpy(scores).cuda(),
                     carry_new=None if carry_new is None else torch.from_numpy(carry_new).cuda(), **kw)


def run_both(s, t, density, generations=40, thin=4, spoiled=True):
    """The loop of montecarlo.DEMCz on the statement and on the device, each fed from its own launch rows -> the smallest
    relative decision margin of the statement, the `out` proposals seen"""
    n_carry = s.carry.shape[1]
    smallest, outs = np.inf, 0
    for g in range(0, generations + 1):
        launched_s = s.rows[:, s.columns]
        launched_t = t.rows.cpu().numpy()[:, s.columns]
        sc_s, sc_t = density(launched_s), density(launched_t)
        if spoiled and g > 0:
            sc_s, sc_t = spoil(sc_s, g), spoil(sc_t, g)
        kw = dict(append=g % thin == 0, propose=g < generations)
        dec = demcz_statement(s, scores=sc_s, carry_new=payload_of(launched_s, n_carry), **kw)
        device_step(t, sc_t, payload_of(launched_t, n_carry), **kw)
        smallest = min(smallest, dec.smallest)
        outs += int(s.out.sum()) if kw['propose'] else 0
    return smallest, outs


CASES = {
    # name: (N, d, seed, cr, p_jump, extra arguments of make_pair)
    'one-chain': (1, 3, 1, 0.9, 0.1, dict(prefill=3)),
    'below-a-wave-d1': (63, 1, 2, 1.0, 0.0, dict()),
    'a-wave-scattered-columns': (64, 3, 3, 0.9, 0.1, dict(columns=[7, 2, 5], ld=13, width=10)),
    'above-a-wave-d16-fallback': (65, 16, 4, 0.1, 0.1, dict(n_carry=16)),
    'two-blocks-d10-all-jumps': (257, 10, 5, 0.9, 1.0, dict(n_carry=9)),
    'cr-one': (64, 3, 6, 1.0, 0.1, dict(n_carry=0)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_the_step_is_the_statement_bit_for_bit(name):
    N, d, seed, cr, p_jump, extra = CASES[name]
    s, t = make_pair(N, d, seed, cr, p_jump, **extra)
    buffers = into_guards(t)
    smallest, _ = run_both(s, t, quadratic(s.lo, s.hi))
    assert smallest > MARGIN, 'a decision of this seed hangs on the last bits of log(u): take another seed'
    compare(s, t)
    assert all(b.intact() for b in buffers.values())
    assert s.M == len(s.archive) == t.capacity              # the appends filled the capacity exactly
    assert (s.accepted < 40).all() and (N == 1 or s.accepted.sum() > 0)      # (NaN and -inf scores were rejected)
    if name == 'above-a-wave-d16-fallback':
        assert s.fallbacks > 0                              # CR 0.1: no dimension drawn, the fallback dimension taken
    if name == 'cr-one':
        assert s.fallbacks == 0
    if name == 'two-blocks-d10-all-jumps':
        assert s.jumps == 40 * N
    if name == 'below-a-wave-d1':
        assert s.jumps == 0
    if name == 'a-wave-scattered-columns':                  # the other columns as the caller left them, NaN in the padding
        rows = t.rows.cpu().numpy()
        assert (rows[:, [0, 1, 3, 4, 6, 8, 9]] == 0.5).all() and np.isnan(rows[:, 10:]).all()


def test_a_box_as_narrow_as_the_archive_makes_out_proposals():
    """d = 1 on a box that the population fills: gamma (z_a - z_b) reaches beyond a whole width, the second reflection
    cannot bring it back, the proposal is `out` -- and its row of the launch matrix holds the chain's current state"""
    s, t = make_pair(65, 1, 7, 1.0, 0.0, lo=[0.0], hi=[1.0], n_carry=2, snapshots=4)
    buffers = into_guards(t)
    seen = 0
    out = np.zeros(65, dtype=bool)
    for g in range(0, 13):
        launched_s, launched_t = s.rows[:, s.columns], t.rows.cpu().numpy()[:, s.columns]
        before, offered = t.x.cpu().numpy().copy(), t.proposal.cpu().numpy().copy()
        # a score that rises by far more than -log(u) can be: every proposal inside the box is accepted (the chains keep
        # filling the box), and an `out` proposal is rejected whatever its score says
        scores = np.full(65, 1.0e6 * g)
        kw = dict(append=g % 4 == 0, propose=True)
        demcz_statement(s, scores=scores, carry_new=payload_of(launched_s, 2), **kw)
        device_step(t, scores, payload_of(launched_t, 2), **kw)
        after = t.x.cpu().numpy()
        if g > 0:
            assert same_bits(after[out], before[out]) and same_bits(after[~out], offered[~out])
        out = t.out.cpu().numpy().astype(bool)
        rows, proposal = t.rows.cpu().numpy(), t.proposal.cpu().numpy()
        assert same_bits(rows[out], after[out]) and same_bits(rows[~out], proposal[~out])
        assert ((proposal[out] < 0.0) | (proposal[out] > 1.0)).all()
        assert ((proposal[~out] >= 0.0) & (proposal[~out] <= 1.0)).all()
        seen += int(out.sum())
    assert seen > 0
    compare(s, t)
    assert s.M == len(s.archive) and all(b.intact() for b in buffers.values())


def test_nan_and_minus_infinity_reject_and_plus_infinity_accepts():
    s2, t2 = make_pair(130, 4, 8, 0.9, 0.1, snapshots=2)
    density = quadratic(s2.lo, s2.hi)
    for state_step in (lambda **kw: demcz_statement(s2, **kw),
                       lambda **kw: device_step(t2, kw.pop('scores'), kw.pop('carry_new'), **kw)):
        state_step(scores=density(s2.x), carry_new=payload_of(s2.x, 3), append=True, propose=True)
    compare(s2, t2)
    x, accepted, logp = t2.x.cpu().numpy().copy(), t2.accepted.cpu().numpy().copy(), t2.logp.cpu().numpy().copy()
    for bad in (np.nan, -np.inf):
        device_step(t2, np.full(130, bad), payload_of(x, 3) + 1.0, propose=False)
        assert same_bits(t2.x.cpu().numpy(), x) and same_bits(t2.accepted.cpu().numpy(), accepted)
        assert same_bits(t2.logp.cpu().numpy(), logp) and same_bits(t2.carry.cpu().numpy(), payload_of(x, 3))
    device_step(t2, np.full(130, np.inf), payload_of(x, 3) + 1.0, propose=False)
    inside = ~t2.out.cpu().numpy().astype(bool)
    assert inside.sum() > 100
    assert same_bits(t2.x.cpu().numpy()[inside], t2.proposal.cpu().numpy()[inside])
    assert (t2.accepted.cpu().numpy() == accepted + inside).all()
    assert (t2.logp.cpu().numpy()[inside] == np.inf).all()
    assert same_bits(t2.carry.cpu().numpy()[inside], (payload_of(x, 3) + 1.0)[inside])


def step_in_pieces(t, scores, carry_new, append, propose, parts):
    """One generation as calls of one phase each, over parts of the chains: every accept phase first (the archive is
    complete before anyone draws from it), then every propose phase"""
    N = t.n_chains
    for part in parts:
        device_step(t, scores, carry_new, append=append, propose=False, chains=part)
    if append:
        t.M += N
    if propose:
        for part in parts:
            device_step(t, None, None, propose=True, chains=part)
        t.g += 1


def test_same_seed_same_bits_however_the_call_is_cut():
    """One seed twice: identical bits.  Accept-only and propose-only calls, and calls over halves (and uneven thirds) of
    the chains, give the bits of the combined call over all of them: the draws are counter-based."""
    N, d = 131, 5
    cuts = {'combined': None, 'again': None, 'phases': [(0, N)], 'halves': [(0, 66), (66, 65)],
            'thirds': [(0, 1), (1, 64), (65, 66)]}
    results = {}
    for how, parts in cuts.items():
        _, t = make_pair(N, d, 9, 0.5, 0.2, snapshots=6)
        density = quadratic(t.lo, t.hi)
        for g in range(0, 11):
            launched = t.rows.cpu().numpy()
            kw = dict(append=g % 2 == 0, propose=g < 10)
            scores = spoil(density(launched), g) if g else density(launched)
            if parts is None:
                device_step(t, scores, payload_of(launched, 3), **kw)
            else:
                step_in_pieces(t, scores, payload_of(launched, 3), kw['append'], kw['propose'], parts)
        assert t.M == t.capacity and t.g == 11
        results[how] = {name: getattr(t, name).cpu().numpy() for name in ARRAYS}
    assert results['combined']['accepted'].sum() > 0
    for how in ('again', 'phases', 'halves', 'thirds'):
        for name in ARRAYS:
            assert same_bits(results[how][name], results['combined'][name]), (how, name)
    # ... and another seed gives other bits
    _, other = make_pair(N, d, 10, 0.5, 0.2, snapshots=6)
    _, t = make_pair(N, d, 9, 0.5, 0.2, snapshots=6)
    other.x.copy_(t.x)
    other.rows.copy_(t.rows)
    for state in (t, other):
        device_step(state, quadratic(t.lo, t.hi)(t.x.cpu().numpy()), payload_of(t.x.cpu().numpy(), 3), append=True)
    assert not same_bits(other.proposal.cpu().numpy(), t.proposal.cpu().numpy())


@pytest.mark.parametrize('kind', [RMSE, RMSE_SIGMA])
def test_the_score_kinds_that_compute_on_the_device(kind):
    """The score is an RMSE, read at stride 8 from a table like the engine's: l within 1e-14 relative of the numpy
    formula, every decision the statement's wherever the statement's margin exceeds 1e-9 (1 + |delta|) -- and the
    inputs chosen here leave no decision out."""
    import torch
    from smartpy_amd import demcz
    N, d, G = 257, 3, 20
    score = dict(score_kind=kind, n_obs=1000, n_eff=400.0, sigma=0.05 if kind == RMSE_SIGMA else 0.0)
    s, t = make_pair(N, d, 11, 0.9, 0.1, snapshots=G + 1, **score)
    t.score_kind = {RMSE: 'rmse', RMSE_SIGMA: 'rmse_sigma'}[kind]
    centre, w = 0.5 * (s.lo + s.hi), 0.5 * (s.hi - s.lo)

    def rmse(x):            # an error that grows away from the middle of the box
        return 0.3 + np.sqrt((((x - centre) / w) ** 2).mean(axis=1))

    decided = left_out = outs = 0
    for g in range(0, G + 1):
        outs += int(s.out.sum())
        launched_s, launched_t = s.rows[:, s.columns], t.rows.cpu().numpy()[:, s.columns]
        assert same_bits(launched_s, launched_t)
        table = np.full((N, 8), np.nan)
        table[:, 6] = rmse(launched_t)
        on_device = torch.from_numpy(table).cuda()
        before = t.accepted.cpu().numpy().copy()
        kw = dict(append=True, propose=g < G)
        dec = demcz_statement(s, scores=table[:, 6], carry_new=payload_of(launched_s, 3), **kw)
        demcz.demcz_step(t, scores=on_device[:, 6], carry_new=torch.from_numpy(payload_of(launched_t, 3)).cuda(), **kw)
        took = (t.accepted.cpu().numpy() - before).astype(bool)
        if g > 0:
            with np.errstate(invalid='ignore'):
                sure = dec.finite & (dec.margin > 1e-9 * (1.0 + np.abs(dec.delta)))
            decided += int(dec.finite.sum())
            left_out += int((dec.finite & ~sure).sum())
            assert (took[sure] == dec.take[sure]).all()
            assert (took == dec.take).all()          # (none was left out: the trajectories stay together)
        logp = t.logp.cpu().numpy()
        assert np.allclose(logp, s.logp, rtol=1e-14, atol=0.0)
        assert same_bits(t.x.cpu().numpy(), s.x)
    assert decided + outs == G * N and outs < N and left_out == 0
    assert np.allclose(t.logp.cpu().numpy(), log_density(rmse(t.x.cpu().numpy()), kind, 1000, 400.0, score['sigma']),
                       rtol=1e-14, atol=0.0)
    assert np.allclose(t.archive_logp.cpu().numpy(), s.archive_logp, rtol=1e-14, atol=0.0)
    compare(s, t, what=('x', 'carry', 'accepted', 'proposal', 'out', 'archive', 'archive_carry', 'rows'))
    assert 0 < s.accepted.sum() < G * N


# ---- montecarlo.DEMCz end to end --------------------------------------------------------------------------------------
def _sampler(root, **kw):
    from smartpy_amd.montecarlo import DEMCz
    args = dict(chains=256, generations=60, thin=5, seed=3, settings_filename='Catchment.demcz.sttngs')
    args.update(kw)
    obj = DEMCz('Catchment', root, 'csv', 'csv', **args)
    obj.model.extra = EXTRA
    return obj


def test_demcz_end_to_end(tmp_path):
    import torch
    from smartpy_amd.montecarlo import GLUE
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.demcz.sttngs', '01/01/2007', '31/12/2009', 180, simu_minutes=1440)
    runs = []
    for _ in range(2):
        obj = _sampler(root)
        obj.run(write=True)
        runs.append((obj, open(obj.db_file, 'rb').read(), open(obj.diagnostics_file).read()))
    (a, db_a, diag_a), (b, db_b, diag_b) = runs
    # ---- one seed, the same bits
    assert db_a == db_b and diag_a == diag_b and a.db_file.endswith('Catchment.SMART.demcz')
    assert same_bits(a._sample, b._sample) and same_bits(a.rhat, b.rhat) and same_bits(a.obj_fns, b.obj_fns)
    assert same_bits(a.log_density.cpu().numpy(), b.log_density.cpu().numpy())
    assert a.acceptance_rate == b.acceptance_rate and same_bits(a.diagnostics, b.diagnostics)
    # ---- shapes: 13 snapshots of 256 chains, the first six dropped
    S, N, first = 13, 256, 6
    n = (S - first) * N
    assert a._sample.shape == (n, 10) and a.obj_fns.shape == (n, 8) and tuple(a.device_obj_fns.shape) == (n, 8)
    assert tuple(a.log_density.shape) == (n,) and a.rhat.shape == (10,) and a.diagnostics.shape == (S, 12)
    assert a.posterior.burn_in == first and tuple(a.posterior.history.shape) == (S, N, 10) and a.vary == a.param_names
    assert a.diagnostics[:, 0].tolist() == [5.0 * k for k in range(S)] and np.isnan(a.diagnostics[0, 1])
    assert 0.0 < a.acceptance_rate < 1.0 and a.diagnostics[-1, 1] == a.acceptance_rate
    assert np.isfinite(a.rhat).all() and same_bits(a.diagnostics[-1, 2:], a.rhat)
    lines = diag_a.split('\n')
    assert lines[0] == 'generation,acceptance_rate,' + ','.join('Rhat_' + p for p in a.param_names) and len(lines) == S + 2
    assert len(db_a.split(b'\n')) == n + 2                  # the header, a line per posterior row
    # ---- every posterior row inside the ranges
    ranges = a.model.parameters.ranges
    for j, p in enumerate(a.param_names):
        assert (a._sample[:, j] >= ranges[p][0]).all() and (a._sample[:, j] <= ranges[p][1]).all(), p
    # ---- a fresh launch of the posterior rows gives the objective functions the chains carried, and their l
    out = a.model.simulate_ensemble(a.device_sample, objective_functions=True, gw_constraint=a.constraints['gw'],
                                    save_discharge=False, math_mode=a.math_mode)
    fresh = torch.cat([out.objfn[:n], out.gw[:n].unsqueeze(1)], dim=1).cpu().numpy()
    carried = a.posterior.carry.cpu().numpy()
    close = (np.abs(fresh - carried) <= 1e-9 * np.maximum(1.0, np.abs(carried))) | (np.isnan(fresh) & np.isnan(carried))
    assert close.all(), np.nanmax(np.abs(fresh - carried))
    assert same_bits(carried[:, :8], a.obj_fns) and same_bits(carried[:, 8], a.gw_contributions)
    ell = a.log_density_of(fresh[:, 6])
    got = a.log_density.cpu().numpy()
    assert np.isfinite(got).all() and (np.abs(ell - got) <= 1e-9 * np.maximum(1.0, np.abs(got))).all()
    # ---- the chains move uphill from the Latin hypercube
    history = a.posterior.history_log_density
    assert float(history[-1].median()) > float(history[0].median())
    # ---- the second stages and the analyses take the object as they take an LHS run
    glue = GLUE('Catchment', root, 'csv', 'csv', conditioning={'NSE': ('min', (float(np.median(a.obj_fns[:, 0])),))},
                settings_filename='Catchment.demcz.sttngs', sampling=a)
    assert 0 < glue._sample.shape[0] <= n
    res = a.pawn_sensitivity(of='objective_functions')
    assert res.index.shape == (8, 10)


def test_demcz_accepted_counts_are_the_changes_of_the_archive(tmp_path):
    """thin = 1: every generation is a snapshot, so the proposals accepted are the state changes between consecutive
    snapshots; with a part of the parameters fixed and the groundwater constraint as a prior."""
    root = example_root(tmp_path)
    settings_file(root, 'Catchment.demcz.sttngs', '01/01/2007', '31/12/2007', 90, simu_minutes=1440)
    vary = ['T', 'SK', 'FK', 'GK']
    obj = _sampler(root, chains=64, generations=12, thin=1, burn_in=0.0, vary=vary, fixed={'C': 0.5}, gw_prior=True, seed=4)
    obj.run()
    history = obj.posterior.history
    assert tuple(history.shape) == (13, 64, 4) and obj.posterior.names == vary and obj._sample.shape == (13 * 64, 10)
    changes = (history[1:] != history[:-1]).any(dim=2)
    assert int(changes.sum()) == int(obj.posterior.accepted.sum()) > 0
    assert (changes.sum(dim=0).cpu().numpy() == obj.posterior.accepted).all()
    assert obj.acceptance_rate == obj.posterior.accepted.sum() / (64.0 * 12.0)
    names = obj.param_names
    assert (obj._sample[:, names.index('C')] == 0.5).all()
    for p in names:
        if p not in vary and p != 'C':
            lo, hi = obj.model.parameters.ranges[p]
            assert (obj._sample[:, names.index(p)] == 0.5 * (lo + hi)).all()
    # a row that fails the groundwater constraint has the log-density -inf, and no chain moves onto one
    flag = obj.posterior.carry[:, 7].cpu().numpy()
    ell = obj.log_density.cpu().numpy()
    assert np.isin(flag, (0.0, 1.0)).all() and (ell[flag == 0.0] == -np.inf).all() and np.isfinite(ell[flag == 1.0]).all()
    moved_onto = changes.cpu().numpy().reshape(-1)
    assert (flag[64:][moved_onto] == 1.0).all()
