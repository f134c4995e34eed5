"""Monte-Carlo workflows on the GPU engine (counterpart of smartpy/montecarlo): LHS, GLUE, Best, Total, and the Sobol
sensitivity analysis on a Saltelli design."""
from .lhs import LHS
from .glue import GLUE
from .best import Best
from .total import Total
from .sobol import Sobol

__all__ = ['LHS', 'GLUE', 'Best', 'Total', 'Sobol']
