"""The compiled code AROUND the interval engine's asm loops -- the walk over the report intervals, the scalar tests on the
forcing, the loads of the observations, the report -- on shapes small enough to run in a blink and built to take every
branch of it (tests/golden/make_interval_glue_parent.py has the cases and says why).  Needs an MI355X.

Every launch is held to two things:
  (a) the oracle, at the gates tests/test_gpu_parity.py uses for the same quantities: 1e-9 relative on the discharge,
      1e-10 on the groundwater ratio, 1e-9 on the objective functions with the constraint flag equal, 1e-8 on the
      final state vector; with no valid observation at all the reference raises, and the scores must not be finite;
  (b) the bits of tests/golden/interval_glue_parent.npz, made by the library of the commit BEFORE that code was
      rewritten: the rewrite changed no arithmetic, so smart_fast_intervals / _exits / _states, smart_fast_runs /
      _exits and smart_fast_intervals_raw have to reproduce every bit, whole or in time slices -- except, where report 0
      carries no observation, the three scores whose moments are taken about a constant (the comment at (b)).
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

from support import bits_equal, rel, eng      # noqa: F401 (eng is a fixture)
from oracle import smart_oracle as so
from oracle import objfn_oracle
from oracle.analyses.objfn import bounds, first_observed

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_interval_glue_parent',
                                               os.path.join(HERE, 'golden', 'make_interval_glue_parent.py'))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

REL_FAST = 1e-9


@pytest.fixture(scope='module')
def parent():
    return cases.load_fixture()


@functools.lru_cache(maxsize=None)
def oracle(n, days, warm_days, forcing_kind, report):
    """(discharge [n, R], gw [n], final [n, 19]) of the reference-exact oracle: once per set-up, shared by the launches"""
    f = cases.forcing(forcing_kind, days)
    code = so.REPORT_RAW if report == 'raw' else so.REPORT_SUMMARY
    out = so.run_batch(cases.AREA, 3600.0, f.shape[0], warm_days * 24, f[:, 0].copy(), f[:, 1].copy(),
                       cases.parameters(n), cases.EXTRA, code, cases.GAP, want_final=True)
    for a in out:
        a.setflags(write=False)
    return out


def test_the_forcing_takes_every_branch():
    """what the cases claim about their forcing, from the numbers: per block of 64 lanes the wet / dry split of every day"""
    f = cases.DAILY
    assert ((f[:, 0] == 0) & (f[:, 1] > 0)).sum() >= 1 and ((f[:, 0] == 0) & (f[:, 1] == 0)).sum() >= 1
    for n in sorted({s[0] for s in cases.SETUPS}):
        T = cases.parameters(n)[:, 0]
        pad = np.concatenate([T, np.full((-n) % 64, T[-1])]).reshape(-1, 64)
        assert n % 64 in (1, 2)                                     # one or two live lanes in the last block
        ex = f[None, None, :, 0] * pad[:, :, None] - f[None, None, :, 1]        # [block, lane, day]
        rainy = f[:, 0] > 0
        all_wet, all_dry = (ex >= 0).all(1), (ex < 0).all(1)
        mixed = ~all_wet & ~all_dry
        assert (all_wet[:, rainy].sum(1) >= 2).all() and (all_dry[:, rainy].sum(1) >= 2).all()
        assert (mixed[:n // 64].sum(1) >= 2).all()                  # full blocks: at least two days of mixed sign
        if n % 64 == 2:
            assert mixed[-1].sum() >= 1                             # ... and one between the last block's two lanes


@pytest.mark.parametrize('obs_kind', cases.OBS_KINDS)
@pytest.mark.parametrize('n, days, warm_days', cases.SETUPS)
def test_every_mode_against_the_oracle_and_the_parent_commits_bits(eng, parent, n, days, warm_days, obs_kind):
    obs = cases.observations(obs_kind, days)
    for mode in cases.MODES:
        name, forcing_kind, report, final, slices, exits, with_obs, store = mode
        got, what = cases.run_mode(eng, mode, n, days, warm_days, obs_kind)
        tag = '%s N=%d T=%d W=%d %s: %s' % (name, n, days * 24, warm_days * 24, obs_kind, what)
        assert cases.kernel_of(name) in what, tag
        if slices != 0:     # (the slices the launch was asked for, as far as the library cuts a run of this length)
            n_slices = cases.slices_run(slices, days, warm_days)
            assert ('[%d slices' % n_slices in what) == (n_slices > 1) and ('slices' in what) == (n_slices > 1), tag
        # (a) the oracle
        dis, gw, fin = oracle(n, days, warm_days, forcing_kind, report)
        if store:
            assert got['discharge'].shape == dis.shape == (n, days), tag
            assert rel(got['discharge'], dis) < REL_FAST, tag
        assert rel(got['gw'], gw) < 1e-10, tag
        if final:
            assert rel(got['final_vars'][:, 7:], fin[:, 7:], floor=1e-290) <= 1e-8, tag
            assert rel(got['final_vars'][:, :7], fin[:, :7], floor=1e-290) <= 1e-8, tag
        if with_obs and obs_kind == 'all_nan':
            with pytest.raises(ZeroDivisionError):          # the reference, inside spotpy's pbias (montecarlo.py:202)
                objfn_oracle.objective_matrix(dis[:1], obs, gw[:1], cases.GW_OBS)
            assert not np.isfinite(got['objfn'][:, :2]).any(), tag
        elif with_obs:
            want = objfn_oracle.objective_matrix(dis, obs, gw, cases.GW_OBS)
            assert rel(got['objfn'][:, :7], want[:, :7]) < 1e-9, tag
            assert np.array_equal(got['objfn'][:, 7], want[:, 7]), tag
        # (b) the parent commit's bits -- but for KGE, KGEc and KGEa where report 0 carries no observation: the constant of
        # their moments is now the sample's value at the first OBSERVED report, where that library took report 0.  There
        # both values lie within their own bound of the same exact scores of the same discharge (its bits are the
        # parent's), so they differ by no more than the two bounds together (oracle/analyses/objfn.py: bounds about
        # row r1 and about row 0); NSE, KGEb, PBias, RMSE and the constraint flag, sums that hold no constant, keep the bits
        moved = with_obs and obs_kind != 'all_nan' and bool(np.isnan(obs[0]))
        for field, a in got.items():
            was = parent[cases.key(name, n, days, warm_days, obs_kind, field)]
            if field == 'objfn' and moved:
                stored = got if store else cases.run_mode(eng, mode[:-1] + (True,), n, days, warm_days, obs_kind)[0]
                sim = np.ascontiguousarray(stored['discharge'].T)
                slack = bounds(sim, obs, first_observed(obs)) + bounds(sim, obs, 0)
                assert np.isfinite(slack[:, 1:4]).all(), (tag, field)          # (an infinite bound would hold nothing)
                assert bits_equal(a[:, [0, 4, 5, 6, 7]], was[:, [0, 4, 5, 6, 7]]), (tag, field)
                assert np.all(np.abs(a[:, 1:4] - was[:, 1:4]) <= slack[:, 1:4]), (tag, field)
                continue
            assert bits_equal(a, was), (tag, field)
