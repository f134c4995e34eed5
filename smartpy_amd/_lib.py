"""ctypes binding of libsmart_amd.so (the C ABI of include/smart_amd.h).

The library is the product: there is no CPU fallback.  If the shared object is missing (not built) or
cannot be loaded, importing the engine fails loudly with instructions, and every compute entry point
returns SMART_E_NO_DEVICE when no HIP device is visible.
"""
import contextlib
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMART_AMD_LIB selects another build of the same ABI (kernel tuning experiments: tools/ab_variants.sh)
LIB_PATH = os.environ.get('SMART_AMD_LIB') or os.path.join(_HERE, 'csrc', 'libsmart_amd.so')

REPORT_SUMMARY, REPORT_RAW = 1, 2
MATH_LITERAL, MATH_FAST = 0, 1
ABI_VERSION = 7
PLAN_VALID = 0x100
PLAN_CLASS_BITS = {0: 0x01, 1: 0x02, 2: 0x04, 3: 0x08}     # regular, stiff, guard, ill-conditioned
PLAN_FORCING_PIECEWISE, PLAN_FORCING_VARYING, PLAN_FORCING_RUNS = 0x10, 0x20, 0x80
PLAN_ROWS_ORDERED = 0x40
PLAN_ILLCOND_BLOCKS_SHIFT, PLAN_ILLCOND_BLOCKS_MAX = 12, 0x7ffff    # ABI 7: class-3 blocks counted by the plan
LITERAL_FORM_AUTO, LITERAL_FORM_ROWS, LITERAL_FORM_LANES = 0, 1, 2
STATUS_SLICE_TIMEOUT, STATUS_STALE_PLAN, STATUS_NONFINITE_FORCING = 0x1, 0x2, 0x4
QUANTILES_AUTO, QUANTILES_SORT, QUANTILES_SELECT = 0, 1, 2
QUANTILES_MAX_PROBS = 16
TRANSFORMS = {'none': 0, 'sqrt': 1, 'log': 2, 'inverse': 3}     # SMART_TRANSFORM_*
OBJFN_WINDOW_COLS = 7
FDC_METHODS = {'auto': 0, 'sort': 1, 'select': 2}              # SMART_FDC_*
SIGNATURE_NAMES = ['MEAN', 'BFI', 'FLASHINESS', 'AC1', 'RLD', 'RECESSION', 'PEAK', 'PEAK_ROW', 'HIGH_COUNT',
                   'HIGH_DURATION', 'LOW_COUNT', 'LOW_DURATION']     # SMART_SIG_*, in column order
SIGNATURE_COLS = len(SIGNATURE_NAMES)
BOOT_MEAN, BOOT_STD = 0, 1                                       # SMART_BOOT_*: the rows of stats in front of the quantiles
SOBOL_MAX_PARAMS = 16
PARETO_MAX_OBJECTIVES = 16
PARETO_DIRECTIONS = {'max': 0, 'min': 1, 'target': 2}           # SMART_PARETO_*
ENSEMBLE_SCORE_NAMES = ['CRPS', 'SPREAD', 'PIT_LOW', 'PIT_HIGH', 'MEAN']     # SMART_ENS_*, in column order
ENSEMBLE_SCORE_COLS = len(ENSEMBLE_SCORE_NAMES)
ENSEMBLE_METHODS = {'auto': 0, 'lds': 1, 'global': 2}           # SMART_ENS_*
DYNIA_MAX_FACTORS, DYNIA_MAX_BINS = 16, 64
DYNIA_SUPPORTS = {'equal': 0, 'linear': 1}                      # SMART_DYNIA_*
PAWN_MAX_FACTORS, PAWN_MAX_BINS = 16, 64
PAWN_METHODS = {'auto': 0, 'lds': 1, 'global': 2}               # SMART_PAWN_*
DEMCZ_MAX_DIMS, DEMCZ_MAX_CARRY = 16, 16
DEMCZ_SCORES = {'logp': 0, 'rmse': 1, 'rmse_sigma': 2}          # SMART_DEMCZ_SCORE_*
NSGA2_MAX_ROWS, NSGA2_MAX_DIMS, NSGA2_MAX_OBJECTIVES, NSGA2_MAX_CARRY = 8192, 16, 4, 16
NSGA2_RANK_BEYOND, NSGA2_RANK_OUT = 2 ** 31 - 2, 2 ** 31 - 1     # SMART_NSGA2_RANK_*
PARTICLE_MAX_PARTICLES, PARTICLE_MAX_DIMS, PARTICLE_STATES, PARTICLE_FIRST_LAYER = 2 ** 19, 16, 12, 5
PARTICLE_WEIGH, PARTICLE_RESAMPLE, PARTICLE_MOVE = 1, 2, 4        # SMART_PARTICLE_*: the phase mask
PARTICLE_FLAG_DEGENERATE, PARTICLE_FLAG_NO_OBS = 1, 2
PARTICLE_STATS = ['ESS', 'EVIDENCE', 'MAX', 'MAX_PRIOR']        # SMART_PARTICLE_*, the doubles of the header in order
PARTICLE_COUNTS = ['RESAMPLED', 'Q', 'DISTINCT', 'FLAGS', 'OFFSET', 'S2', 'Q_PRIOR']     # ... and its integers
ERROR_MODEL_SEGMENT = 64                                       # SMART_ERROR_MODEL_SEGMENT
ERROR_MODEL_ROWS = ['LOGLIK', 'SSQ', 'LOGSIG']                  # SMART_ERROR_MODEL_*, in row order

_dp = ctypes.c_void_p   # device or host address, passed as an integer


class SmartEnsemble(ctypes.Structure):
    """struct SmartEnsemble of include/smart_amd.h (field for field)."""
    _fields_ = [
        ('n_catchments', ctypes.c_int64), ('n_samples', ctypes.c_int64), ('n_steps', ctypes.c_int64),
        ('n_warm', ctypes.c_int64), ('report_gap', ctypes.c_int64),
        ('report_type', ctypes.c_int32), ('math_mode', ctypes.c_int32), ('delta_sec', ctypes.c_double),
        ('area_m2', _dp), ('forcing', _dp), ('params', _dp), ('params_catchment_stride', ctypes.c_int64),
        ('extra', _dp), ('initial', _dp), ('obs', _dp), ('gw_obs', _dp),
        ('discharge', _dp), ('discharge_ld', ctypes.c_int64), ('gw', _dp), ('objfn', _dp),
        ('final_vars', _dp), ('workspace', _dp), ('workspace_bytes', ctypes.c_int64), ('stream', _dp),
        ('time_slices', ctypes.c_int32), ('plan', ctypes.c_int32),
        ('literal_form', ctypes.c_int32), ('reserved0', ctypes.c_int32),
    ]


# every symbol include/smart_amd.h declares: (restype, argtypes)
SYMBOLS = {
    'smart_n_reports': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]),
    'smart_run_ensemble_hip': (ctypes.c_int, [ctypes.POINTER(SmartEnsemble)]),
    'smart_check_ensemble': (ctypes.c_int, [ctypes.POINTER(SmartEnsemble)]),
    'smart_workspace_bytes': (ctypes.c_int64, [ctypes.POINTER(SmartEnsemble)]),
    'smart_plan_ensemble': (ctypes.c_int, [ctypes.POINTER(SmartEnsemble), ctypes.POINTER(ctypes.c_int32)]),
    'smart_launch_status': (ctypes.c_int, [ctypes.POINTER(SmartEnsemble), ctypes.POINTER(ctypes.c_int32)]),
    'smart_describe_launch': (ctypes.c_int, [ctypes.POINTER(SmartEnsemble), ctypes.c_char_p, ctypes.c_int64]),
    'smart_allsteps_hip': (ctypes.c_int, [ctypes.c_double, ctypes.c_double, ctypes.c_int64, _dp, _dp, _dp, _dp,
                                          ctypes.c_int32, ctypes.c_int64, _dp, _dp, _dp]),
    'smart_hook_counters': (ctypes.c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.c_int64]),
    'smart_onestep_hip': (ctypes.c_int, [ctypes.c_int64, _dp, _dp]),
    'smart_river_step_hip': (ctypes.c_int, [ctypes.c_int64, _dp, _dp]),
    'smart_objfn_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp, _dp,
                                       ctypes.c_double, _dp, _dp]),
    'smart_weighted_quantiles_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp,
                                                    ctypes.POINTER(ctypes.c_double), ctypes.c_int32, _dp,
                                                    ctypes.c_int32, _dp]),
    'smart_quantiles_sort_capacity': (ctypes.c_int64, []),
    'smart_objfn_windows_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp, _dp,
                                               ctypes.c_int32, ctypes.c_int32, ctypes.c_double, _dp, _dp]),
    'smart_objfn_max_windows': (ctypes.c_int32, []),
    'smart_flow_duration_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp, _dp,
                                               ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.c_int32, _dp,
                                               ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double, _dp,
                                               _dp, ctypes.c_int64, ctypes.c_int32, _dp]),
    'smart_flow_duration_workspace_bytes': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    'smart_flow_duration_sort_capacity': (ctypes.c_int64, []),
    'smart_signatures_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp, _dp, ctypes.c_int32,
                                            ctypes.c_double, _dp, _dp, _dp]),
    'smart_signature_cols': (ctypes.c_int32, []),
    'smart_sobol_indices_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, _dp, ctypes.c_int64, _dp,
                                               _dp, _dp, _dp, ctypes.c_int32, _dp, _dp, _dp, ctypes.c_int64, _dp]),
    'smart_sobol_workspace_bytes': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]),
    'smart_sobol_max_resamples': (ctypes.c_int32, []),
    'smart_sobol_lds_capacity': (ctypes.c_int64, []),
    'smart_objfn_bootstrap_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp, _dp,
                                                 ctypes.c_int32, ctypes.c_int32, ctypes.c_double, _dp, ctypes.c_int32,
                                                 ctypes.POINTER(ctypes.c_double), ctypes.c_int32, _dp, _dp, _dp, _dp,
                                                 ctypes.c_int64, _dp]),
    'smart_bootstrap_workspace_bytes': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    'smart_bootstrap_max_windows': (ctypes.c_int32, []),
    'smart_bootstrap_max_resamples': (ctypes.c_int32, []),
    'smart_pareto_counts_hip': (ctypes.c_int, [ctypes.c_int64, _dp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                                               ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
                                               ctypes.c_int32, _dp, _dp, _dp, ctypes.c_int64, _dp]),
    'smart_pareto_workspace_bytes': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    'smart_pareto_max_objectives': (ctypes.c_int, []),
    'smart_ensemble_scores_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp, _dp, _dp,
                                                 ctypes.c_int32, _dp, ctypes.c_int64, _dp]),
    'smart_ensemble_scores_workspace_bytes': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                                               ctypes.c_int32]),
    'smart_ensemble_scores_lds_capacity': (ctypes.c_int64, []),
    'smart_dynia_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_double, _dp, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_int32, _dp, _dp, _dp, _dp, _dp, ctypes.c_int64, _dp, ctypes.c_int64, _dp]),
    'smart_dynia_workspace_bytes': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                                     ctypes.c_int32]),
    'smart_dynia_max_half_width': (ctypes.c_int32, []),
    'smart_dynia_lds_capacity': (ctypes.c_int64, []),
    'smart_pawn_ks_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp, ctypes.c_int32,
                                         ctypes.c_int32, _dp, _dp, ctypes.c_int32, _dp, ctypes.c_int64, _dp]),
    'smart_pawn_workspace_bytes': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]),
    'smart_pawn_lds_capacity': (ctypes.c_int64, []),
    'smart_demcz_step_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp,
                                            _dp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_double,
                                            ctypes.c_double, _dp, ctypes.c_int32, ctypes.c_int32, _dp, _dp, _dp,
                                            ctypes.c_int32, _dp, _dp, _dp, _dp, ctypes.c_int64, ctypes.c_int64, _dp,
                                            ctypes.c_int64, _dp, _dp]),
    'smart_nsga2_step_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                            ctypes.c_int64, ctypes.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                            _dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp,
                                            ctypes.c_int64, ctypes.c_int32, _dp, _dp, _dp, ctypes.c_double,
                                            ctypes.c_int64, _dp, ctypes.c_int64, _dp, _dp]),
    'smart_nsga2_workspace_bytes': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    'smart_particle_step_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32,
                                               ctypes.c_int64, _dp, ctypes.c_int64, _dp, ctypes.c_double, ctypes.c_double,
                                               ctypes.c_double, _dp, ctypes.c_int64, _dp, _dp, ctypes.c_int64, _dp,
                                               ctypes.c_int32, ctypes.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                               _dp, _dp, _dp, _dp, _dp, ctypes.c_int64, _dp]),
    'smart_particle_workspace_bytes': (ctypes.c_int64, [ctypes.c_int64]),
    'smart_error_model_loglik_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp, _dp,
                                                    ctypes.c_int64, _dp, _dp]),
    'smart_error_model_draw_hip': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int64, _dp,
                                                  ctypes.c_int64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, _dp,
                                                  ctypes.c_int64, _dp]),
    'smart_db_append_rows': (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_int32]),
    'smart_db_parse_rows': (ctypes.c_int64, [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_float), ctypes.c_int64, ctypes.c_int32]),
    'smart_row_class': (ctypes.c_int, [_dp, ctypes.c_double, _dp, ctypes.c_double]),
    'smart_device_count': (ctypes.c_int, []),
    'smart_abi_version': (ctypes.c_int, []),
    'smart_build_info': (ctypes.c_char_p, []),
    'smart_last_error': (ctypes.c_char_p, []),
}

_lib = None


class SmartEngineError(Exception):
    """Raised when the C ABI reports an error (the reference raises plain Exception at the same places)."""

    def __init__(self, code, message):
        Exception.__init__(self, message)
        self.code = code


def _apply_lint_verdict():
    """The streaming step loops jump through byte offsets that another kernel wrote (smart_fast_arms.h: pair blocks); the
    offsets are right for a library whose code smartpy_amd.isa_lint has looked at -- smartpy_amd.build does that for
    every library it links and leaves the outcome next to it.  A library without that record, or with one written for
    another file (rebuilt elsewhere, by another hipcc), or whose blocks failed the lint, runs the THREADED CHUNKS instead
    (SMART_PAIR_BLOCKS=0: the same arithmetic, bit for bit, without computed jumps) and says so; never wrong code
    words.  A library whose hand-over or row chains failed the lint is refused.  SMART_PAIR_BLOCKS set by the caller
    stands (A/B builds: tools/variants)."""
    import warnings
    from . import isa_lint
    report = None
    if isa_lint.record_state(LIB_PATH) != 'this-build' and os.path.exists(isa_lint.OBJDUMP):
        # no record, or one for another file (a library that travelled without it, or was rebuilt by something else): look
        # at the code now (~6 s) and leave the record for the next load.  ONE process of a job does it -- the others wait
        # at the lock and read what it wrote
        with contextlib.ExitStack() as held:
            try:
                import fcntl
                fcntl.flock(held.enter_context(open(LIB_PATH + '.lint.lock', 'w')), fcntl.LOCK_EX)
            except (ImportError, OSError):
                pass            # (a read-only tree: every process looks for itself)
            if isa_lint.record_state(LIB_PATH) != 'this-build':
                report = isa_lint.lint_and_record(LIB_PATH)
    # (the report in hand rather than the record: in a read-only tree none was written)
    ok, pairs, reason = isa_lint.verdict_of(report, report['sha256']) if report else isa_lint.verdict_for(LIB_PATH)
    if not ok:
        raise ImportError("smartpy_amd: %s failed the code lints of smartpy_amd.isa_lint (%s); rebuild it with "
                          "`python -m smartpy_amd.build --force`" % (LIB_PATH, reason))
    if 'SMART_PAIR_BLOCKS' in os.environ:
        return                  # (the caller's word stands: A/B builds, tools/variants)
    if not pairs:
        os.environ['SMART_PAIR_BLOCKS'] = '0'
        warnings.warn("smartpy_amd: %s; the step loops run their threaded chunks instead of the pair blocks "
                      "(SMART_PAIR_BLOCKS=0).  `python -m smartpy_amd.build --force` builds and checks the library."
                      % reason)
    elif isa_lint.library_stamp(LIB_PATH) != 'pairs-ok':
        # the code has been looked at (just now, or by the record's writer) but the file carries no stamp of it -- a
        # library that smartpy_amd.build did not link: the library by itself would run the threaded chunks (smart_capi.hip:
        # pair_blocks_wanted); this process has the lint's word for the pair blocks
        os.environ['SMART_PAIR_BLOCKS'] = '1'


def lib():
    """Load libsmart_amd.so once.  No fallback of any kind."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "smartpy_amd: the HIP extension %s has not been built.  Run `python -m smartpy_amd.build` "
                "(needs hipcc; cross-compiles for gfx950 without a GPU).  There is no CPU fallback." % LIB_PATH)
        # torch first: its wheel brings a HIP runtime of its own, and the one that is loaded first is the one that
        # owns the device.  Loaded the other way round (this library, then torch: __graft_entry__.build() followed by
        # smoke() in ONE process did that) the library's own runtime reports "no ROCm-capable device".
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _apply_lint_verdict()
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)       # AttributeError here = the header and the library disagree
            fn.restype = res
            fn.argtypes = args
        if L.smart_abi_version() != ABI_VERSION:
            raise ImportError("smartpy_amd: ABI version mismatch between smartpy_amd/_lib.py and %s" % LIB_PATH)
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SmartEngineError(rc, lib().smart_last_error().decode('utf8', 'replace') or 'error %d' % rc)
