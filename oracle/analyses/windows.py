"""Split-sample objective functions: the numpy statement of smart_objfn_windows_hip.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import objfn_oracle

TRANSFORMS = {'none': 0, 'sqrt': 1, 'log': 2, 'inverse': 3}


def transformed(name, x, eps):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all='ignore'):
        return {'none': lambda: x + 0.0, 'sqrt': lambda: np.sqrt(x), 'log': lambda: np.log(x + eps),
                'inverse': lambda: 1.0 / (x + eps)}[name]()


def statement(sim, obs, win, n_windows, transform='none', eps=0.0):
    """sim [R, n], obs [R] (NaN = missing), win [R] -> [n_windows, n, 7]."""
    out = np.full((n_windows, sim.shape[1], 7), np.nan)
    for w in range(n_windows):
        rows = (win == w) & ~np.isnan(obs)
        e = transformed(transform, obs[rows], eps)
        if rows.sum() < 2 or not np.isfinite(e).all():
            continue
        for n in range(sim.shape[1]):
            s = transformed(transform, sim[rows, n], eps)
            if np.isfinite(s).all():
                with np.errstate(all='ignore'):
                    out[w, n] = objfn_oracle.objective_functions(s, e)[:7]
    return out
