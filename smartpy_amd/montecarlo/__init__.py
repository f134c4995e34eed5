"""Monte-Carlo workflows on the GPU engine (counterpart of smartpy/montecarlo): LHS, GLUE, Best, Total, the Sobol
sensitivity analysis on a Saltelli design, the Pareto selection over several objective functions, and DE-MCz posterior
sampling."""
from .lhs import LHS
from .glue import GLUE
from .best import Best
from .total import Total
from .sobol import Sobol
from .pareto import Pareto
from .demcz import DEMCz

__all__ = ['LHS', 'GLUE', 'Best', 'Total', 'Sobol', 'Pareto', 'DEMCz']
