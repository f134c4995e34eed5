"""The particle filter's assimilation step as a numpy statement (the definition of include/smart_amd.h:
smart_particle_step_hip), and the case tables the host and the GPU tests share.  TEST INFRASTRUCTURE ONLY:
a plain module, pytest does not collect it.  Every floating-point operation below is a numpy operation on float64 --
rounded once, in the order written; from the quantisation on everything is uint64."""
import numpy as np

from oracle.analyses import de_move
from oracle.philox import philox4x32, u53

UNIT = 1 << 22
STATES, FIRST_LAYER = 12, 5
DEGENERATE, NO_OBS = 1, 2
U64 = np.uint64


def key_of(seed):
    return (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


# ---- weigh and quantise ------------------------------------------------------------------------------------------------
def weigh(sim, obs, logw, sigma0, sigma1):
    """sim [Rw, N], obs [Rw] -> logw' [N]"""
    s = np.zeros(sim.shape[1])
    bad = np.zeros(sim.shape[1], dtype=bool)
    with np.errstate(all='ignore'):
        for t in range(sim.shape[0]):
            if np.isnan(obs[t]):
                continue
            sigma = sigma0 + sigma1 * np.abs(obs[t])
            bad |= ~np.isfinite(sim[t])
            r = (sim[t] - obs[t]) / sigma
            s = s + r * r
        post = logw + (-0.5 * s)
    return np.where(bad, -np.inf, post)


def quantise(logw):
    """-> (q uint64 [N], m: the largest finite log-weight or -inf); all 0 where none is finite"""
    finite = np.isfinite(logw)
    if not finite.any():
        return np.zeros(len(logw), dtype=U64), -np.inf
    m = logw[finite].max()
    with np.errstate(all='ignore'):
        e = np.exp(np.where(finite, logw, m) - m)
    return np.where(finite, np.rint(float(UNIT) * e), 0.0).astype(U64), m


# ---- decide and resample -----------------------------------------------------------------------------------------------
def effective_size(q):
    """-> (ess, Q, S2) from the integers: Python integers for the sums, one double operation each for the quotient"""
    Q, S2 = int(q.astype(object).sum()), int((q.astype(object) ** 2).sum())
    with np.errstate(all='ignore'):
        ess = np.float64(Q) * np.float64(Q)
        ess = ess / np.float64(S2)
    return ess, Q, S2


def comb_offset(seed, k, Q, offset=-1):
    """rho = min(offset >= 0 ? offset : floor(fl(u Q)), Q - 1)"""
    if offset < 0:
        w = philox4x32((0xFFFFFFFF, k, 0, 0), key_of(seed))
        offset = int(np.floor(u53(w[0], w[1]) * np.float64(Q)))
    return min(int(offset), Q - 1)


def parents_of(q, rho):
    """a_j = #{i : N C_i <= j Q + rho} in uint64 (every product below 2^60)"""
    N = len(q)
    C = np.cumsum(q.astype(U64), dtype=U64)
    t = np.arange(N, dtype=U64) * C[-1] + U64(rho)
    return np.searchsorted(U64(N) * C, t, side='right').astype(np.int64)


# ---- move --------------------------------------------------------------------------------------------------------------
def move(rows, states, parents, k, seed, columns, lo, hi, scale, noise, z_column, area):
    """-> (rows' [N, ld] with the varying columns of the children, the others as `rows` has them; states' [N, 12])"""
    N, d = len(parents), len(columns)
    key, j = key_of(seed), np.arange(N, dtype=U64)
    base = rows[parents][:, columns]
    W = [philox4x32((j, k, 2 + c, 0), key) for c in range(d)]
    moved = np.broadcast_to(np.asarray(scale) != 0.0, (N, d))
    y, out = de_move.move(W, moved, np.asarray(scale, dtype=np.float64), np.asarray(lo, dtype=np.float64),
                          np.asarray(hi, dtype=np.float64), base, base, base, 0.0)
    new = rows.copy()
    new[:, columns] = de_move.launch_rows(out, base, y)
    Z = new[:, z_column] if z_column in list(columns) else rows[parents, z_column]
    cap = Z / 6.0
    cap = cap / 1e3
    cap = cap * area
    x = states[parents]
    x_new = np.empty_like(x)
    with np.errstate(all='ignore'):
        for s in range(STATES):
            w = philox4x32((j, k, 18 + s // 2, 0), key)
            f = 2.0 * (u53(w[0], w[1]) if s % 2 == 0 else u53(w[2], w[3]))
            f = f - 1.0
            f = noise[s] * f
            f = 1.0 + f
            v = x[:, s] * f
            if FIRST_LAYER <= s < FIRST_LAYER + 6:
                v = np.where(v > cap, cap, v)
            x_new[:, s] = v
    return new, x_new


# ---- the step ----------------------------------------------------------------------------------------------------------
class Step(object):
    """what a step leaves: logw_post, q, ess, Q, S2, resampled, rho, flags, parents, distinct, rows, states, logw,
    evidence, m, m_prior, Q_prior"""


def step(rows, states, logw, k, seed, columns, lo, hi, scale, noise, z_column, area, tau, sim=None, obs=None,
         sigma=(1.0, 0.0), q_in=None, q_device=None, offset=-1):
    """One assimilation step.  q_in: integers that stand in for the weighing.  q_device: the integers a device made of
    THIS window -- the weighing runs (logw_post, m) but everything downstream uses them, as the GPU tests ask."""
    o = Step()
    N = len(logw)
    o.flags = 0
    if q_in is not None:
        o.logw_post, o.q = logw.copy(), np.asarray(q_in).astype(U64)
        o.m = o.m_prior = o.evidence = np.nan
        o.Q_prior = 0
    else:
        o.logw_post = weigh(sim, obs, logw, sigma[0], sigma[1])
        o.q, o.m = quantise(o.logw_post)
        q0, o.m_prior = quantise(logw)
        o.Q_prior = int(q0.astype(object).sum())
        if np.isnan(obs).all():
            o.flags |= NO_OBS
        if not np.isfinite(o.m):
            o.q = np.full(N, UNIT, dtype=U64)
        if q_device is not None:
            o.q = np.asarray(q_device).astype(U64)
    o.ess, o.Q, o.S2 = effective_size(o.q)
    if (o.Q == 0) if q_in is not None else not np.isfinite(o.m):
        o.flags |= DEGENERATE
    if q_in is None:
        with np.errstate(all='ignore'):
            o.evidence = (o.m + np.log(np.float64(o.Q) / float(UNIT))) - (o.m_prior + np.log(np.float64(o.Q_prior) / float(UNIT)))
    o.resampled = bool(o.flags == 0 and o.ess < np.float64(tau) * np.float64(N))
    o.rho = comb_offset(seed, k, o.Q, offset) if o.resampled else 0
    o.parents = parents_of(o.q, o.rho) if o.resampled else np.arange(N, dtype=np.int64)
    o.distinct = len(np.unique(o.parents))
    o.rows, o.states = move(rows, states, o.parents, k, seed, columns, lo, hi, scale, noise, z_column, area)
    o.logw = np.zeros(N) if o.resampled or (o.flags & DEGENERATE) else o.logw_post.copy()
    return o


# ---- case tables -------------------------------------------------------------------------------------------------------
RESAMPLING_SIZES = (1, 2, 63, 64, 65, 257, 1000)
STEP_SIZES = (1, 63, 64, 65, 256, 257, 1000, 4099)
LARGEST = 1 << 19


def weight_patterns(N, seed):
    """name -> integers q [N] (uint64, at least one above 0): what the resampling is asked to do"""
    rng = np.random.default_rng(seed)
    spread = np.rint(UNIT * np.exp(-rng.exponential(3.0, N))).astype(U64)
    spread[rng.integers(0, N)] = UNIT
    zeros = spread.copy()
    zeros[rng.random(N) < 0.5] = 0
    zeros[rng.integers(0, N)] = UNIT
    heavy = np.zeros(N, dtype=U64)
    heavy[rng.integers(0, N)] = UNIT
    nearly = np.ones(N, dtype=U64)
    nearly[N // 2] = UNIT
    return {'spread': spread, 'zeros': zeros, 'one heavy': heavy, 'one heavy among ones': nearly,
            'equal': np.full(N, UNIT, dtype=U64)}


def particles(N, seed, ld=12, d=4, z_varies=True):
    """rows [N, ld], states [N, 12], a box and scales for a launch matrix whose column 5 is Z: (rows, states, columns, lo,
    hi).  The varying columns are 5 (Z), 0, 7 and 2 in that order (d of them; without z_varies 0, 7, 2, 4)."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(1.0, 2.0, (N, ld))
    rows[:, 5] = rng.uniform(15.0, 150.0, N)
    columns = ([5, 0, 7, 2] if z_varies else [0, 7, 2, 4])[:d]
    lo = np.array([15.0 if c == 5 else 1.0 for c in columns])
    hi = np.array([150.0 if c == 5 else 2.0 for c in columns])
    states = rng.uniform(0.0, 50.0, (N, STATES))
    return rows, states, columns, lo, hi


AREA = 1.0e6        # with Z in 15 .. 150 a layer holds 2,500 .. 25,000: the states above are never clamped ...
NOISE = np.array([0.05, 0.0, 0.1, 0.05, 0.2, 0.05, 0.05, 0.3, 0.05, 0.05, 0.05, 0.9])
