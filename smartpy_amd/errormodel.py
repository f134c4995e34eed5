"""The residual error model, host side: a standard deviation linear in the simulated flow, sigma_t = sigma0 + sigma1
sim_t, and standardised residuals that follow a first-order autoregression with coefficient phi (Schoups & Vrugt 2010,
Water Resour. Res. 46; Evin et al. 2014, Water Resour. Res. 50) -- the names of its three parameters, their default prior
ranges, how an `error_model=` argument is read, the result objects of MonteCarlo.residual_likelihood and
MonteCarlo.predictive_bounds, and the writers of their side files.  numpy only, nothing hot: the two kernels are behind
engine.residual_log_likelihood and engine.predictive_draws (include/smart_amd.h: smart_error_model_loglik_hip).
"""
import numpy as np

from ._lib import SmartEngineError, ERROR_MODEL_ROWS

PARAMETER_NAMES = ['sigma0', 'sigma1', 'phi']            # the columns of error_parameters, in order
LIKELIHOOD_NAMES = list(ERROR_MODEL_ROWS)                # the rows of engine.residual_log_likelihood, in order


def default_ranges(obs):
    """The prior ranges of the three parameters from the mean m of the observed flows: sigma0 in [1e-4 m, m], sigma1 in
    [0, 1], phi in [0, 0.99]."""
    flow = np.asarray(obs, dtype=np.float64)
    flow = flow[~np.isnan(flow)]
    if flow.size == 0:
        raise SmartEngineError(-2, "errormodel: no observed flow to take the default range of sigma0 from.")
    m = float(flow.mean())
    return {'sigma0': (1e-4 * m, m), 'sigma1': (0.0, 1.0), 'phi': (0.0, 0.99)}


def resolve(error_model, obs):
    """error_model: None, or a dict name -> (lo, hi) (the parameter is sampled) or a number (it is fixed); a name that is
    missing takes its default range -> (sampled: the names that are sampled, in the order of PARAMETER_NAMES; ranges: name
    -> (lo, hi) of those; fixed: name -> value of the others)."""
    given = dict(error_model or {})
    unknown = [p for p in given if p not in PARAMETER_NAMES]
    if unknown:
        raise SmartEngineError(-2, "errormodel: the error parameter(s) {} are not among {}."
                               .format(unknown, PARAMETER_NAMES))
    defaults = default_ranges(obs) if any(p not in given for p in PARAMETER_NAMES) else {}
    sampled, ranges, fixed = [], {}, {}
    for p in PARAMETER_NAMES:
        v = given.get(p, defaults.get(p))
        if np.ndim(v) == 0:
            fixed[p] = float(v)
            if not np.isfinite(fixed[p]):
                raise SmartEngineError(-2, "errormodel: the fixed {} {} must be finite.".format(p, v))
        else:
            if len(v) != 2:
                raise SmartEngineError(-2, "errormodel: {} takes a (lo, hi) range or a number, not {}.".format(p, v))
            lo, hi = float(v[0]), float(v[1])
            if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
                raise SmartEngineError(-2, "errormodel: the range of {} ({}, {}) needs finite lo <= hi.".format(p, lo, hi))
            sampled.append(p)
            ranges[p] = (lo, hi)
    lo_phi, hi_phi = ranges.get('phi', (fixed.get('phi'),) * 2)
    if not (-1.0 < lo_phi and hi_phi < 1.0):
        raise SmartEngineError(-2, "errormodel: phi must stay inside (-1, 1), not ({}, {}).".format(lo_phi, hi_phi))
    for p in ('sigma0', 'sigma1'):
        if ranges.get(p, (fixed.get(p),))[0] < 0.0:
            raise SmartEngineError(-2, "errormodel: {} must not be negative.".format(p))
    return sampled, ranges, fixed


def parameter_table(error_parameters, n):
    """error_parameters of a call on the host: [n, 3], or one triple for all n rows -> [n, 3] float64"""
    table = np.asarray(error_parameters, dtype=np.float64)
    if table.shape == (len(PARAMETER_NAMES),):
        table = np.tile(table, (n, 1))
    if table.shape != (n, len(PARAMETER_NAMES)):
        raise SmartEngineError(-2, "errormodel: error_parameters must be [{}, 3] (sigma0, sigma1, phi) or one triple, not "
                                   "shape {}.".format(n, table.shape))
    return np.ascontiguousarray(table)


class ResidualLikelihood(object):
    """What MonteCarlo.residual_likelihood returns, per row of the sample: `error_parameters` (numpy [N, 3]),
    `log_likelihood`, `ssq`, `logsig` (numpy [N]; -inf / NaN / NaN for an invalid row), `device` (the [3, N] tensor they
    came from, or None) and `file` (the path written, or None)."""

    def __init__(self, error_parameters, values, device=None, file=None):
        values = np.asarray(values, dtype=np.float64)
        self.error_parameters = error_parameters
        self.log_likelihood, self.ssq, self.logsig = values[0], values[1], values[2]
        self.device, self.file = device, file


class PredictiveBounds(object):
    """What MonteCarlo.predictive_bounds returns: `quantiles` (the K probabilities), `bounds` (numpy [K, R]: the weighted
    quantiles of the TOTAL predictive distribution -- `replicates` error realisations on top of every row's simulation),
    `parametric` ([K, R]: the same quantiles of the simulations alone), `containment` and `parametric_containment` (the
    share of the observations inside [bounds[0], bounds[-1]]; NaN without observations), `datetime` (the R report stamps),
    `replicates`, `seed`, `truncate`, `verification` (verification.EnsembleVerification of the draws, or None) and `file`."""

    def __init__(self, quantiles, bounds, parametric, containment, parametric_containment, stamps, replicates, seed,
                 truncate, verification=None, file=None):
        self.quantiles, self.bounds, self.parametric = quantiles, bounds, parametric
        self.containment, self.parametric_containment = containment, parametric_containment
        self.datetime, self.replicates, self.seed, self.truncate = stamps, replicates, seed, truncate
        self.verification, self.file = verification, file


def write_likelihood_file(path, error_parameters, values):
    """`<catchment>.SMART.<func>.errormodel`: header sigma0,sigma1,phi,LOGLIK,SSQ,LOGSIG, one line per row of the sample in
    the sample's order, '%.6e'."""
    from .montecarlo.selection import write_text_table
    table = np.concatenate([np.asarray(error_parameters, dtype=np.float64), np.asarray(values, dtype=np.float64).T], axis=1)
    write_text_table(path, ','.join(PARAMETER_NAMES + LIKELIHOOD_NAMES), table, '%.6e', '\r\n')


def write_predictive_file(path, stamps, quantiles, bounds, parametric):
    """`<catchment>.SMART.<func>.predictive`: header DateTime,q<p>,...,param_q<p>,...; one line per report step with the
    dates and the '%e' of the modelled flow file."""
    from .montecarlo.selection import write_text_table
    header = ','.join(['DateTime'] + ['q%g' % p for p in quantiles] + ['param_q%g' % p for p in quantiles])
    write_text_table(path, header, np.concatenate([np.asarray(bounds).T, np.asarray(parametric).T], axis=1), '%e', '\r\n',
                     labels=stamps)
