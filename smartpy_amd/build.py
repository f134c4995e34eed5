"""Build libsmart_amd.so (HIP, gfx950) in-tree with hipcc.  `python -m smartpy_amd.build [--force]`.

hipcc cross-compiles for gfx950 without a GPU.  The shared object stays next to the sources
(smartpy_amd/csrc/libsmart_amd.so) so that it travels with the tree; it is git-ignored.
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(CSRC, 'libsmart_amd.so')
ARCH = 'gfx950'

# translation unit -> extra flags.  The literal kernels must round every operation separately.
UNITS = {
    'smart_literal.hip': ['-ffp-contract=off'],
    # the literal model inside the fast kernel opts out of contraction per function (pragma); no NaN ever enters the
    # arithmetic (missing observations are tested on their bit pattern), which spares the sNaN-quieting
    # `v_max_f64 x, x, x` hipcc otherwise puts in front of fmin / fmax (-1.2 % kernel time, A/B measured)
    'smart_fast_intervals.hip': ['-ffp-contract=fast-honor-pragmas', '-fno-honor-nans'],
    'smart_fast_runs.hip': ['-ffp-contract=fast-honor-pragmas', '-fno-honor-nans'],
    'smart_fast_steps.hip': ['-ffp-contract=fast-honor-pragmas', '-fno-honor-nans'],
    'smart_fast_reports.hip': ['-ffp-contract=fast-honor-pragmas', '-fno-honor-nans'],
    # ... except where the literal model lives inside the fast mode (the ill-conditioned rows and rows with NaN or
    # infinite parameters): NaNs honoured -- what a NaN does in the reference's compares is part of what it reproduces
    'smart_fast_guarded.hip': ['-ffp-contract=fast-honor-pragmas'],
    # the ensemble's weighted quantiles per report step (GLUE prediction bounds): default flags, NaNs honoured -- a
    # NaN value has a place in the order (above +inf)
    'smart_quantiles.hip': [],
    # the objective functions per window of report steps, on transformed flows: default flags, NaNs honoured -- a NaN
    # or an infinity that a transform makes has to reach the sums (it is how the kernel finds it)
    'smart_objfn_windows.hip': [],
    # flow duration curves (order statistics along time, per sample): default flags, NaNs honoured -- a NaN value has a
    # place in the order, and a non-finite transformed flow has to reach the sums
    'smart_flow_duration.hip': [],
    # hydrological signatures (a recurrence along time, per sample): default flags, NaNs honoured -- a value that is not
    # finite has to reach the one sum that finds it
    'smart_signatures.hip': [],
    # Sobol sensitivity indices of a Saltelli design (point estimates and bootstrap): default flags, NaNs honoured -- a
    # value that is not finite has to reach the one sum that finds it
    'smart_sobol.hip': [],
    # block bootstrap and jackknife of the objective functions (per-window moments, counts x moments per replicate):
    # default flags, NaNs honoured -- a value that is not finite has to reach the sums of its window, and a NaN replicate
    # the mean and the standard deviation
    'smart_bootstrap.hip': [],
    # Pareto selection over the scores of the analyses (dominance counts): default flags, NaNs honoured -- the keys are
    # compared as IEEE says
    'smart_pareto.hip': [],
    # ensemble verification per report step (CRPS, spread, PIT, mean across the samples): default flags, NaNs honoured --
    # a live member that is not finite is found by its key, and a missing observation by its bits
    'smart_ensemble_scores.hip': [],
    # dynamic identifiability analysis (moving-window error sums along time, selection and shares across the samples):
    # default flags, NaNs honoured -- a value that is not finite has to reach the window sums it lies in, and is found
    # there by its key
    'smart_dynia.hip': [],
    # PAWN sensitivity (Kolmogorov-Smirnov distances across the samples, per row of a matrix): default flags, NaNs
    # honoured -- a value that is not finite is found by its key, and the integers held in doubles are exact either way
    'smart_pawn.hip': [],
    # the step of the DE-MCz sampler (proposal, crossover, reflection, Metropolis decision, archive): every operation of
    # the proposal rounded once -- the numpy statement of the tests is held to it bit for bit
    'smart_demcz.hip': ['-ffp-contract=off'],
    # the step of the NSGA-II sampler (dominance bit matrix, peeled fronts, crowding distance, truncation, differential
    # variation): every operation of the distance and of the offspring rounded once -- the numpy statement of the tests is
    # held to it bit for bit; NaNs honoured -- a NaN key loses every compare, which is how a row that takes no part is kept out
    'smart_nsga2.hip': ['-ffp-contract=off'],
    # the step of the particle filter (window likelihood, integer weights, systematic resampling, jitter and state noise):
    # every operation of the weights and of the move rounded once -- the numpy statement of the tests is held to it bit for
    # bit; NaNs honoured -- a missing observation and a particle that is not finite are found by their compares
    'smart_particle.hip': ['-ffp-contract=off'],
    # the residual error model (the AR(1) log-likelihood of a stored matrix, error realisations on top of it): every
    # operation rounded once, as the numpy statement of the tests rounds it; NaNs honoured -- a NaN at a step without an
    # observation is selected away, one at an observed step makes the sample invalid
    'smart_error_model.hip': ['-ffp-contract=off'],
    'smart_capi.hip': [],
    # the C entries of the matrix analyses, and smart_objfn_matrix: the flags smart_capi.hip had it compiled with
    'smart_analysis_capi.hip': [],
    'smart_hostio.cpp': ['-pthread'],      # host only: the sampling-database writer
}
COMMON = ['-O3', '-fPIC', '-std=c++17', '--offload-arch=' + ARCH, '-fno-gpu-rdc', '-Wall']
# every header of csrc and the public one: a new header cannot be forgotten
DEPS = sorted(f for f in os.listdir(CSRC) if f.endswith('.h')) + [os.path.join('..', '..', 'include', 'smart_amd.h')]


def hipcc():
    exe = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(exe):
        raise RuntimeError('hipcc not found: the HIP extension cannot be built')
    return exe


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def build(force=False, verbose=False, extra_flags=(), lib_path=LIB):
    cc = hipcc()
    deps = [os.path.join(CSRC, d) for d in DEPS] + [os.path.abspath(__file__)]
    objs, jobs = [], []
    suffix = '' if lib_path == LIB else '.' + os.path.basename(lib_path)
    for unit, flags in UNITS.items():
        src = os.path.join(CSRC, unit)
        obj = os.path.join(CSRC, os.path.splitext(unit)[0] + suffix + '.o')
        if force or _stale(obj, [src] + deps):
            jobs.append([cc] + COMMON + flags + list(extra_flags) + ['-c', src, '-o', obj])
        objs.append(obj)
    if jobs:        # the translation units are independent: compile them side by side
        if verbose:
            for cmd in jobs:
                print(' '.join(cmd))
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as pool:
            list(pool.map(subprocess.check_call, jobs))
    from . import isa_lint
    relink = force or _stale(lib_path, objs)
    if relink or isa_lint.record_state(lib_path) != 'this-build':
        # linked (or, for a library without a record of its own -- copied here, or its record lost -- copied) under a name
        # of this process's own, looked at, stamped with the verdict on its pair blocks, then renamed onto the library: a
        # process that loads it meanwhile sees the old file or the new one, never half of one
        tmp = '%s.%d.tmp' % (lib_path, os.getpid())
        try:
            if relink:
                cmd = [cc, '-shared', '-fPIC', '-pthread', '--offload-arch=' + ARCH, '-o', tmp] + objs
                if verbose:
                    print(' '.join(cmd))
                subprocess.check_call(cmd)
            else:
                shutil.copy(lib_path, tmp)
            isa_lint.lint_and_record(tmp, record_for=lib_path, stamp=True, check=lambda path: lint(path, verbose))
            os.replace(tmp, lib_path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return lib_path


class BuildLintError(RuntimeError):
    pass


def lint(path, verbose=False):
    """smartpy_amd.isa_lint on a freshly linked library, BEFORE it is put in place: the pair blocks where the code words
    point, the hand-over sequences, the DPP distances of the row form.  A hand-over or a row chain that fails refuses
    the library (BuildLintError: those have no other form to fall back to); pair blocks that fail are recorded, and the
    library will run its threaded chunks (smartpy_amd._lib)."""
    from . import isa_lint
    report = isa_lint.check_library(path)
    report['library'] = os.path.basename(LIB)
    if verbose or report['problems']:
        print('isa_lint: %s' % ('; '.join(report['problems']) if report['problems'] else
                                'pair blocks, hand-over and row chains of the linked library are in order'))
    if report['handover'] is False or report['rows'] is False:
        raise BuildLintError('smartpy_amd.build: the linked library fails the code lints and is not installed: '
                             + '; '.join(report['problems']))
    return report


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
