"""CPU statements of the matrix analyses.  TEST INFRASTRUCTURE ONLY.

One module per analysis: the numpy definition the kernels are held to and, where the analysis has them, its exact truth,
the bounds derived for the kernel's form, an emulation of its order of additions, and the seeded inputs that its host test
and its GPU test share.  They import numpy, fractions, math and other oracle modules only.
"""
