"""Monte-Carlo workflows on the GPU engine (counterpart of smartpy/montecarlo): LHS, GLUE, Best, Total, the Sobol
sensitivity analysis on a Saltelli design, the Pareto selection over several objective functions, DE-MCz posterior
sampling, multi-objective calibration by NSGA-II, and the particle filter of the model states."""
from .lhs import LHS
from .glue import GLUE
from .best import Best
from .total import Total
from .sobol import Sobol
from .pareto import Pareto
from .demcz import DEMCz
from .nsga2 import NSGA2
from .particle import ParticleFilter

__all__ = ['LHS', 'GLUE', 'Best', 'Total', 'Sobol', 'Pareto', 'DEMCz', 'NSGA2', 'ParticleFilter']
