"""DE-MCz posterior sampling, host side: Philox4x32-10 against the known answers of Random123; the numpy statement of
include/smart_amd.h (smart_demcz_step_hip) that tests/test_gpu_demcz.py holds the kernels to BIT FOR BIT, and that it
samples what it should (a correlated Gaussian: mean, variance, R-hat, acceptance rate, six seeds); every refusal of the C
entry, as literals; gelman_rubin against numpy; the diagnostics file.  Nothing here needs a device."""
import ctypes
import math

import numpy as np
import pytest

from oracle.analyses.demcz import (LOGP, RMSE, RMSE_SIGMA, Chains, demcz_statement, log_density, mulhi, run_statement)
from oracle.philox import philox4x32, u53
from smartpy_amd import _lib, demcz
from support import E_MODE, E_NO_DEVICE, E_NULL, E_SIZE, FAKE, refusal


def test_philox_known_answers():
    def words(counter, key):
        return ' '.join('%08x' % int(w) for w in philox4x32(counter, key))
    ones = 0xFFFFFFFF
    assert words((0, 0, 0, 0), (0, 0)) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    assert words((ones,) * 4, (ones, ones)) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    assert words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        'd16cfe09 94fdcceb 5001e420 24126ea1'
    # arrays of counters give what the counters give one by one
    got = philox4x32((np.arange(5), 7, 1, 0), (3, 9))
    for i in range(5):
        assert [int(w[i]) for w in got] == [int(w) for w in philox4x32((i, 7, 1, 0), (3, 9))]
    assert u53(np.uint64(ones), np.uint64(ones)) == 1.0 - 2.0 ** -53 and u53(np.uint64(31), np.uint64(63)) == 0.0
    assert int(mulhi(np.uint64(ones), 10)) == 9 and int(mulhi(np.uint64(0), 10)) == 0


def test_the_statement_by_hand():
    # two chains, one dimension, CR = 1, no jump, no jitter: the proposal is x + gamma (z_a - z_b), reflected once
    s = Chains([[1.0], [3.0]], [0.0], [4.0], capacity=4, seed=5, cr=1.0, p_jump=0.0, b_star=0.0, n_carry=1)
    demcz_statement(s, scores=np.array([-1.0, -2.0]), carry_new=np.array([[10.0], [20.0]]), append=True)
    assert (s.M, s.g) == (2, 2) and s.logp.tolist() == [-1.0, -2.0] and s.accepted.tolist() == [0, 0]
    assert s.archive[:2].tolist() == [[1.0], [3.0]] and s.archive_carry[:2].tolist() == [[10.0], [20.0]]
    g1 = 2.38 / math.sqrt(2.0)
    for i, x in enumerate((1.0, 3.0)):              # with two archive rows a != b: the difference is +-2
        y = s.proposal[i, 0]
        want = [x + g1 * 2.0, x - g1 * 2.0]
        want = [2 * 0.0 - v if v < 0.0 else (2 * 4.0 - v if v > 4.0 else v) for v in want]
        assert y in want and not s.out[i] and s.rows[i, 0] == y
    # a score of +inf is accepted whatever u is, NaN and -inf are not, and an accepted chain takes proposal and payload
    before = s.x.copy()
    dec = demcz_statement(s, scores=np.array([np.inf, np.nan]), carry_new=np.array([[11.0], [21.0]]), propose=False)
    assert dec.take.tolist() == [True, False] and s.accepted.tolist() == [1, 0] and s.g == 2
    assert s.x[0, 0] == s.proposal[0, 0] and s.x[1, 0] == before[1, 0] and s.carry.tolist() == [[11.0], [20.0]]
    assert s.logp.tolist() == [np.inf, -2.0] and dec.smallest == np.inf
    s.logp[:] = [-1.0, -2.0]
    dec = demcz_statement(s, scores=np.array([-np.inf, -np.inf]), carry_new=s.carry, propose=False)
    assert not dec.take.any()
    # the score kinds
    assert log_density(2.0, RMSE, 100, 50.0, 0.0) == -(25.0 * np.log(400.0))
    assert log_density(2.0, RMSE_SIGMA, 0, 50.0, 0.5) == -(50.0 * 4.0) / 0.5
    assert log_density(np.inf, RMSE, 100, 50.0, 0.0) == -np.inf and np.isnan(log_density(np.nan, RMSE, 100, 50.0, 0.0))
    assert demcz.gamma_table(3).tolist() == [2.38 / math.sqrt(2.0), 2.38 / math.sqrt(4.0), 2.38 / math.sqrt(6.0)]
    assert demcz.thresholds(0.1, 1.0) == (int(0.1 * 2 ** 32), 2 ** 32) and demcz.thresholds(0.0, 0.0) == (0, 0)


# ---- the statement samples what it should ---------------------------------------------------------------------------
MU = np.array([1.0, -2.0, 0.5])
SD = np.array([1.0, 0.5, 2.0])
SIGMA = (0.6 + 0.4 * np.eye(3)) * np.outer(SD, SD)
PRECISION = np.linalg.inv(SIGMA)


def gaussian(x):
    r = x - MU
    return -0.5 * np.einsum('ni,ij,nj->n', r, PRECISION, r)


@pytest.mark.parametrize('seed', range(6))
def test_the_statement_samples_the_target(seed):
    """N(mu, Sigma), d = 3, all correlations 0.6, on the box [-10, 10]^3: 64 chains, 3,000 generations, thin 10, CR 1,
    p_jump 0.1, b* 1e-6; over the states of the second half.  Conditions, not measurements."""
    N, G = 64, 3000
    x0 = np.random.default_rng(seed).uniform(-10.0, 10.0, size=(N, 3))
    s = Chains(x0, [-10.0] * 3, [10.0] * 3, capacity=(1 + G // 10) * N, seed=seed, cr=1.0, p_jump=0.1, b_star=1e-6)
    states = []
    run_statement(s, gaussian, G, 10, keep=states)
    assert s.M == len(s.archive)
    half = np.stack(states[G // 2:])                                   # [1500, 64, 3]
    chain_means = half.mean(axis=0)
    se = chain_means.std(axis=0, ddof=1) / math.sqrt(N)
    z = (chain_means.mean(axis=0) - MU) / se
    ratio = half.reshape(-1, 3).var(axis=0, ddof=1) / np.diag(SIGMA)
    rhat = demcz.gelman_rubin(np.stack(states))
    rate = s.accepted.sum() / float(N * G)
    print('seed %d: z %s variance ratio %s rhat %s acceptance %.3f' % (seed, z, ratio, rhat, rate))
    assert (np.abs(z) <= 4.0).all()
    assert (np.abs(ratio - 1.0) <= 0.1).all()
    assert (rhat < 1.01).all()
    assert 0.15 <= rate <= 0.45


# ---- gelman_rubin ---------------------------------------------------------------------------------------------------------
def test_gelman_rubin_against_numpy():
    import torch
    rng = np.random.default_rng(3)
    for S, N, d in ((40, 8, 3), (41, 5, 1), (4, 2, 2)):
        h = rng.normal(size=(S, N, d)) + rng.normal(size=(1, N, d)) * 0.3
        half = h[S // 2:]
        n = half.shape[0]
        W = half.var(axis=0, ddof=1).mean(axis=0)
        B_n = half.mean(axis=0).var(axis=0, ddof=1)
        want = np.sqrt(((n - 1) / n * W + B_n) / W)
        got = demcz.gelman_rubin(h)
        assert isinstance(got, np.ndarray) and got.shape == (d,) and np.allclose(got, want, rtol=1e-12, atol=0)
        on_tensor = demcz.gelman_rubin(torch.from_numpy(h))
        assert isinstance(on_tensor, torch.Tensor) and np.array_equal(on_tensor.numpy(), got)
    assert np.isnan(demcz.gelman_rubin(np.zeros((2, 4, 3)))).all()            # one snapshot in the second half
    assert np.isnan(demcz.gelman_rubin(np.zeros((8, 1, 3)))).all()            # one chain
    same = np.broadcast_to(rng.normal(size=(10, 1, 2)), (10, 6, 2))           # every chain alike: B = 0
    assert np.allclose(demcz.gelman_rubin(same), math.sqrt(4.0 / 5.0))
    with pytest.raises(ValueError, match=r'history must be \[snapshots, chains, dimensions\]'):
        demcz.gelman_rubin(np.zeros((4, 3)))


# ---- side files -----------------------------------------------------------------------------------------------------------
def test_the_diagnostics_file(tmp_path):
    names = ['T', 'SK']
    assert demcz.diagnostics_header(names) == 'generation,acceptance_rate,Rhat_T,Rhat_SK\n'
    table = np.array([[0.0, np.nan, np.nan, np.nan], [10.0, 0.25, 1.5, 1.25], [20.0, 0.3125, 1.0625, 1.001]])
    path = str(tmp_path / 'Catchment.SMART.demcz.diagnostics')
    demcz.write_diagnostics(path, names, table)
    assert open(path).read().split('\n') == [
        'generation,acceptance_rate,Rhat_T,Rhat_SK', '0,nan,nan,nan', '10,2.500000e-01,1.500000e+00,1.250000e+00',
        '20,3.125000e-01,1.062500e+00,1.001000e+00', '']
    back = np.genfromtxt(path, delimiter=',', skip_header=1)
    assert np.array_equal(back, table, equal_nan=True)
    post = demcz.PosteriorSample(names, None, None, None, None, None, [3, 4], [1.0, 1.1], 0.25, table, 1)
    assert post.names == names and post.rhat.tolist() == [1.0, 1.1] and post.acceptance_rate == 0.25
    assert post.accepted.tolist() == [3, 4] and post.burn_in == 1 and post.file is None and post.diagnostics.shape == (3, 4)
    from smartpy_amd.montecarlo import DEMCz
    from smartpy_amd.montecarlo.montecarlo import MonteCarlo
    assert issubclass(DEMCz, MonteCarlo) and isinstance(DEMCz.diagnostics_file, property)


# ---- the refusals of the C entry ------------------------------------------------------------------------------------------
TWO31, TWO32 = 2 ** 31, 2 ** 32
K_ = 'smart_demcz_step_hip'
_LO = (ctypes.c_double * 16)(*([0.0] * 16))
_HI = (ctypes.c_double * 16)(*([1.0] * 16))
_COLS = (ctypes.c_int32 * 16)(*range(16))


def _addr(a):
    return ctypes.addressof(a)


VALID = dict(n_chains=8, chain_offset=0, n_dims=3, seed=1, generation=2, archive_size=8, capacity=24, x=FAKE, logp=FAKE,
             carry=FAKE, accepted=FAKE, proposal=FAKE, out=FAKE, score=FAKE, score_stride=1, score_kind=LOGP, n_obs=0,
             n_eff=0.0, sigma=0.0, carry_new=FAKE, n_carry=2, append=1, archive=FAKE, archive_logp=FAKE, archive_carry=FAKE,
             propose=1, lo=_addr(_LO), hi=_addr(_HI), scale=_addr(_LO), gamma=_addr(_HI), jump_threshold=100,
             cr_threshold=TWO32, rows=FAKE, ld=10, columns=_addr(_COLS), stream=None)
REQUIRED = K_ + ': x, logp, proposal, out and archive are required (%s is NULL)'
PROPOSE = K_ + ': the propose phase needs lo, hi, scale, gamma, rows and columns (%s is NULL)'
_BAD_LO = (ctypes.c_double * 16)(*([0.0, 2.0] + [0.0] * 14))
_NAN_HI = (ctypes.c_double * 16)(*([1.0, 1.0, float('nan')] + [1.0] * 13))
_TWICE = (ctypes.c_int32 * 16)(*([4, 2, 4] + list(range(3, 16))))
_FAR = (ctypes.c_int32 * 16)(*([0, 10, 2] + list(range(3, 16))))
_NEG = (ctypes.c_int32 * 16)(*([-1, 1, 2] + list(range(3, 16))))

CASES = [
    (dict(x=None), E_NULL, REQUIRED % 'x'),
    (dict(logp=None), E_NULL, REQUIRED % 'logp'),
    (dict(proposal=None), E_NULL, REQUIRED % 'proposal'),
    (dict(out=None), E_NULL, REQUIRED % 'out'),
    (dict(archive=None), E_NULL, REQUIRED % 'archive'),
    (dict(out=None, logp=None), E_NULL, REQUIRED % 'logp'),                         # the first in the list is named
    (dict(x=None, n_chains=0), E_NULL, REQUIRED % 'x'),                             # pointers before sizes
    (dict(n_chains=0), E_SIZE, K_ + ': need n_chains >= 1 (got 0)'),
    (dict(n_chains=-4, n_dims=0), E_SIZE, K_ + ': need n_chains >= 1 (got -4)'),
    (dict(chain_offset=-1), E_SIZE, K_ + ': chain_offset -1 must be in 0 .. 4294967295'),
    (dict(chain_offset=TWO32), E_SIZE, K_ + ': chain_offset 4294967296 must be in 0 .. 4294967295'),
    (dict(chain_offset=TWO32 - 8, n_chains=9), E_SIZE,
     K_ + ": chains 4294967288 .. 4294967296: a chain's number stays below 2^32"),
    (dict(n_dims=0), E_SIZE, K_ + ': n_dims 0 must be in 1 .. 16'),
    (dict(n_dims=17), E_SIZE, K_ + ': n_dims 17 must be in 1 .. 16'),
    (dict(n_dims=17, generation=0), E_SIZE, K_ + ': n_dims 17 must be in 1 .. 16'),
    (dict(generation=0), E_SIZE, K_ + ': generation 0 must be in 1 .. 4294967295'),
    (dict(generation=TWO32), E_SIZE, K_ + ': generation 4294967296 must be in 1 .. 4294967295'),
    (dict(capacity=0), E_SIZE, K_ + ': capacity 0 must be in 1 .. 2^31 - 1'),
    (dict(capacity=TWO31), E_SIZE, K_ + ': capacity 2147483648 must be in 1 .. 2^31 - 1'),
    (dict(archive_size=-1), E_SIZE, K_ + ': archive_size -1 must be in 0 .. 24 (the capacity)'),
    (dict(archive_size=25), E_SIZE, K_ + ': archive_size 25 must be in 0 .. 24 (the capacity)'),
    (dict(n_carry=-1), E_SIZE, K_ + ': n_carry -1 must be in 0 .. 16'),
    (dict(n_carry=17), E_SIZE, K_ + ': n_carry 17 must be in 0 .. 16'),
    (dict(n_carry=17, score_kind=3), E_SIZE, K_ + ': n_carry 17 must be in 0 .. 16'),      # sizes before the mode
    (dict(score=None, propose=0, append=0), E_NULL, K_ + ': neither phase is asked for (score is NULL and propose is 0)'),
    # ---- the accept phase
    (dict(score_kind=3), E_MODE, K_ + ": score_kind '3' unknown."),
    (dict(score_kind=-1), E_MODE, K_ + ": score_kind '-1' unknown."),
    (dict(score_kind=3, accepted=None), E_MODE, K_ + ": score_kind '3' unknown."),
    (dict(score_stride=0), E_SIZE, K_ + ': score_stride 0 must be in 1 .. 2^31 - 1'),
    (dict(score_kind=RMSE, n_eff=5.0), E_SIZE, K_ + ': n_obs 0 must be in 1 .. 2^31 - 1'),
    (dict(score_kind=RMSE, n_obs=100), E_SIZE, K_ + ': n_eff 0 must be finite and > 0'),
    (dict(score_kind=RMSE, n_obs=100, n_eff=float('inf')), E_SIZE, K_ + ': n_eff inf must be finite and > 0'),
    (dict(score_kind=RMSE_SIGMA, n_eff=float('nan')), E_SIZE, K_ + ': n_eff nan must be finite and > 0'),
    (dict(score_kind=RMSE_SIGMA, n_eff=5.0), E_SIZE, K_ + ': sigma 0 must be finite and > 0'),
    (dict(score_kind=RMSE_SIGMA, n_eff=5.0, sigma=-1.0), E_SIZE, K_ + ': sigma -1 must be finite and > 0'),
    (dict(accepted=None), E_NULL, K_ + ': the accept phase needs accepted (accepted is NULL)'),
    (dict(carry=None), E_NULL, K_ + ': n_carry 2 needs carry and carry_new (carry is NULL)'),
    (dict(carry_new=None), E_NULL, K_ + ': n_carry 2 needs carry and carry_new (carry_new is NULL)'),
    (dict(archive_logp=None), E_NULL, K_ + ': append needs archive_logp (archive_logp is NULL)'),
    (dict(archive_carry=None), E_NULL, K_ + ': append with n_carry 2 needs archive_carry (archive_carry is NULL)'),
    (dict(archive_size=17), E_SIZE, K_ + ': append of archive rows 17 .. 24 passes the capacity 24'),
    (dict(chain_offset=9), E_SIZE, K_ + ': append of archive rows 17 .. 24 passes the capacity 24'),
    (dict(archive_size=24, propose=0), E_SIZE, K_ + ': append of archive rows 24 .. 31 passes the capacity 24'),
    (dict(score=None), E_NULL, K_ + ': append needs the accept phase (score is NULL)'),
    # ---- the propose phase
    (dict(lo=None), E_NULL, PROPOSE % 'lo'),
    (dict(hi=None), E_NULL, PROPOSE % 'hi'),
    (dict(scale=None), E_NULL, PROPOSE % 'scale'),
    (dict(gamma=None), E_NULL, PROPOSE % 'gamma'),
    (dict(rows=None), E_NULL, PROPOSE % 'rows'),
    (dict(columns=None), E_NULL, PROPOSE % 'columns'),
    (dict(score=None, append=0, archive_size=1), E_SIZE,
     K_ + ': the propose phase draws two rows of the archive: its size is 1, need at least 2'),
    (dict(score=None, append=0, archive_size=0), E_SIZE,
     K_ + ': the propose phase draws two rows of the archive: its size is 0, need at least 2'),
    (dict(append=0, archive_size=1), E_SIZE,
     K_ + ': the propose phase draws two rows of the archive: its size is 1, need at least 2'),
    (dict(n_chains=1, archive_size=0, n_carry=0), E_SIZE,
     K_ + ': the propose phase draws two rows of the archive: its size is 1, need at least 2'),
    (dict(jump_threshold=-1), E_SIZE, K_ + ': jump_threshold -1 must be in 0 .. 4294967296'),
    (dict(jump_threshold=TWO32 + 1), E_SIZE, K_ + ': jump_threshold 4294967297 must be in 0 .. 4294967296'),
    (dict(cr_threshold=TWO32 + 1), E_SIZE, K_ + ': cr_threshold 4294967297 must be in 0 .. 4294967296'),
    (dict(ld=2), E_SIZE, K_ + ': ld 2 is less than n_dims 3'),
    (dict(columns=_addr(_FAR)), E_SIZE, K_ + ': columns[1] 10 must be in 0 .. 9'),
    (dict(columns=_addr(_NEG)), E_SIZE, K_ + ': columns[0] -1 must be in 0 .. 9'),
    (dict(columns=_addr(_TWICE)), E_SIZE, K_ + ': columns[0] and columns[2] name the same column 4'),
    (dict(lo=_addr(_BAD_LO)), E_SIZE, K_ + ': lo[1] 2 and hi[1] 1: need finite lo <= hi'),
    (dict(hi=_addr(_NAN_HI)), E_SIZE, K_ + ': lo[2] 0 and hi[2] nan: need finite lo <= hi'),
]


def _case_id(i, changes):
    return '%02d-' % i + '-'.join('%s=%s' % (k, 'table' if k in ('lo', 'hi', 'columns') and v else v)
                                  for k, v in changes.items())


@pytest.mark.parametrize('changes,code,text', CASES, ids=[_case_id(i, c[0]) for i, c in enumerate(CASES)])
def test_refusals(changes, code, text):
    assert refusal({K_: VALID}, K_, changes) == (code, text)


def test_a_well_formed_call_gets_as_far_as_the_device():
    L = _lib.lib()
    if L.smart_device_count() == 0:
        # ... and no further: there is no CPU fallback
        for changes in (dict(), dict(propose=0), dict(score=None, append=0), dict(archive_size=16),
                        dict(n_dims=16, ld=16, n_carry=16), dict(n_dims=1, n_carry=0, carry=None, carry_new=None,
                                                                  archive_carry=None),
                        dict(generation=1, archive_size=0), dict(chain_offset=8, capacity=32),
                        dict(score_kind=RMSE, n_obs=3000, n_eff=3000.0, score_stride=8),
                        dict(score_kind=RMSE_SIGMA, n_eff=10.0, sigma=0.5),
                        dict(jump_threshold=0, cr_threshold=0), dict(jump_threshold=TWO32),
                        dict(generation=TWO32 - 1, chain_offset=TWO32 - 8, append=0, capacity=TWO31 - 1)):
            rc, text = refusal({K_: VALID}, K_, changes)
            assert rc == E_NO_DEVICE and 'device' in text, changes
    else:
        # with a device the refusals leave the error text as they set it, and the entry is run for real by
        # tests/test_gpu_demcz.py
        assert refusal({K_: VALID}, K_, dict(x=None))[0] == E_NULL


def test_the_new_name_is_bound():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'smart_amd.h')).read()
    assert K_ in _lib.SYMBOLS and getattr(_lib.lib(), K_) is not None
    assert _lib.SYMBOLS[K_][0] is ctypes.c_int and len(_lib.SYMBOLS[K_][1]) == len(VALID) == 36
    declared = re.search(r'^int %s\(([^;]*)\);' % K_, header, re.M)
    assert declared and declared.group(1).count(',') + 1 == 36
    names = re.findall(r'(\w+)\s*(?:,|$)', declared.group(1).replace('\n', ' '))
    assert names == list(VALID)                      # the dictionary above is the entry's argument list, in its order
    for macro, value in (('SMART_DEMCZ_MAX_DIMS', 16), ('SMART_DEMCZ_MAX_CARRY', 16), ('SMART_DEMCZ_SCORE_LOGP', 0),
                         ('SMART_DEMCZ_SCORE_RMSE', 1), ('SMART_DEMCZ_SCORE_RMSE_SIGMA', 2)):
        assert re.search(r'^#define %s %d$' % (macro, value), header, re.M), macro
    assert _lib.DEMCZ_SCORES == {'logp': LOGP, 'rmse': RMSE, 'rmse_sigma': RMSE_SIGMA}
    assert (_lib.DEMCZ_MAX_DIMS, _lib.DEMCZ_MAX_CARRY) == (16, 16) and _lib.lib().smart_abi_version() == 7
    from smartpy_amd import build
    assert build.UNITS['smart_demcz.hip'] == ['-ffp-contract=off']
    from smartpy_amd import montecarlo
    assert 'DEMCz' in montecarlo.__all__
    with pytest.raises(_lib.SmartEngineError, match=r'p_jump 1.5 must be in \[0, 1\]') as err:
        demcz.thresholds(1.5, 0.5)
    assert err.value.code == -2
