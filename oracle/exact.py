"""What the exact-arithmetic truths share: the unit roundoff and how relative errors compose.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

U = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -20    # the magnitudes inside `bounds` are themselves float64 sums (docstring of bounds)


def gamma(k):
    return k * U / (1.0 - k * U)


def mul(a, b):
    """relative errors of two factors -> of their product"""
    return a + b + a * b


def div(a, b):
    return np.where(b < 1.0, (a + b) / np.maximum(1.0 - b, 1e-300), np.inf)


def sqrt(a):
    """relative error a of x -> of sqrt x (the lower side is the larger one)"""
    return np.where(a < 1.0, 1.0 - np.sqrt(np.maximum(1.0 - a, 0.0)), np.inf)
