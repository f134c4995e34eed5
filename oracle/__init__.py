"""Parity oracle for the SMART hot path.  TEST INFRASTRUCTURE ONLY.

CPU restatements of the reference algorithm (ThibHlln/smartpy v0.2.2) used as the checker by tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg.  The product package (smartpy_amd) must never
import anything from here.

smart_oracle the model, lhs_oracle the samplers, objfn_oracle the objective functions as the reference calls them;
analyses/ one module per matrix analysis (objfn, quantiles, windows, flow_duration, signatures, sobol, bootstrap, pareto,
ensemble_scores, dynia, pawn, demcz, error_model): its definition and, where it has them, exact truth, bounds, emulation;
exact what those truths share (U, SLACK, gamma, mul, div, sqrt); philox Philox4x32-10 and the 53-bit uniform.
"""
