"""Host side of the ensemble engine: torch tensors in, one HIP launch through the C ABI, torch tensors out.

PyTorch is plumbing here (device memory, streams, torch.distributed); all arithmetic of the hot path is in
smartpy_amd/csrc/*.hip behind include/smart_amd.h.  Nothing in this module computes model steps on the CPU
and nothing imports the test oracle.
"""
import collections
import ctypes
import math
import threading
import warnings
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import SmartEngineError, REPORT_SUMMARY, REPORT_RAW, MATH_LITERAL, MATH_FAST  # noqa: F401

OBJ_FN_NAMES = ['NSE', 'KGE', 'KGEc', 'KGEa', 'KGEb', 'PBias', 'RMSE', 'GW']   # montecarlo.py:71-74
VARIABLES = ['Q_aeva', 'Q_ove', 'Q_dra', 'Q_int', 'Q_sgw', 'Q_dgw', 'Q_out',
             'V_ove', 'V_dra', 'V_int', 'V_sgw', 'V_dgw',
             'V_ly1', 'V_ly2', 'V_ly3', 'V_ly4', 'V_ly5', 'V_ly6', 'V_river']  # structure.py:78-82

_REPORT = {'summary': REPORT_SUMMARY, 'raw': REPORT_RAW}
_MATH = {'literal': MATH_LITERAL, 'fast': MATH_FAST}
_LITERAL_FORMS = {'auto': _lib.LITERAL_FORM_AUTO, 'rows': _lib.LITERAL_FORM_ROWS, 'lanes': _lib.LITERAL_FORM_LANES}


def report_code(report):
    """structure.py:65-70."""
    try:
        return _REPORT[report]
    except KeyError:
        raise Exception("Reporting type '{}' unknown.".format(report))


def default_device():
    if not torch.cuda.is_available():
        raise SmartEngineError(-6, "smartpy_amd needs a HIP device (torch.cuda.is_available() is False); "
                                   "there is no CPU fallback")
    return torch.device('cuda', torch.cuda.current_device())


#: bytes this module has copied from the host to a device since it was imported (as_device and SingleRun): what the
#: tests hold "a repeated simulate() uploads its ten parameters and nothing else" against
h2d_bytes = 0


def as_device(x, device, shape=None):
    """numpy / list / tensor -> contiguous fp64 tensor on device."""
    global h2d_bytes
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
    if not x.is_cuda and torch.device(device).type == 'cuda':
        h2d_bytes += x.numel() * 8
    x = x.to(device=device, dtype=torch.float64).contiguous()
    if shape is not None:
        x = x.reshape(shape)
    return x


def extra_vector(extra):
    """{'aar', 'r-o_ratio', 'r-o_split'} -> the 7 doubles of include/smart_amd.h (structure.py:100-112)."""
    if not extra:
        return None
    return [float(extra['aar']), float(extra['r-o_ratio'])] + [float(v) for v in extra['r-o_split']]


def _per_catchment(x, device, C, tail=()):
    """An input with a catchment axis, on the device: a scalar (tail == ()) or an array of shape `tail` that the
    catchments share -> contiguous [C, *tail]; an array that has one entry per catchment -> reshaped to [C, *tail]."""
    if x is None:
        return None
    if not tail:
        return as_device(np.full(C, x, dtype=np.float64) if np.ndim(x) == 0 else x, device, (C,))
    x = as_device(x, device)
    if x.numel() == math.prod(tail):
        return x.reshape((1,) + tail).expand((C,) + tail).contiguous()
    return x.reshape((C,) + tail)


class EnsembleResult(object):
    """Outputs of one launch.  discharge is a [C, N, R] *view* of the sample-minor buffer the kernel writes."""

    def __init__(self, discharge_rn, gw, objfn, final_vars, n_samples, squeeze):
        self._dis = discharge_rn        # [C, R, ld] or None
        self._n = n_samples
        self._squeeze = squeeze
        self.gw = gw[0] if squeeze else gw
        self.objfn = None if objfn is None else (objfn[0] if squeeze else objfn)
        self.final_vars = None if final_vars is None else (final_vars[0] if squeeze else final_vars)

    @property
    def discharge_report_major(self):
        """[C, R, N] (or [R, N]) exactly as stored: row r holds every sample's discharge of report step r."""
        if self._dis is None:
            return None
        d = self._dis[:, :, :self._n]
        return d[0] if self._squeeze else d

    @property
    def discharge(self):
        """[C, N, R] (or [N, R]): discharge[n] is what SMART.simulate(row n)[0] returns (smart.py:208)."""
        d = self.discharge_report_major
        return None if d is None else d.transpose(-1, -2)


def n_reports(n_steps, gap, report_type):
    return int(_lib.lib().smart_n_reports(n_steps, gap, report_type))


def variant_classes(params, delta_sec, initial=None, area=None):
    """Which arithmetic variant of the fast kernels each row of params [N, 10] needs at a step of delta_sec seconds --
    the rules of wave_class() in csrc/smart_fast_model.h: 0 regular, 1 stiff (some k*3600 < dt: clamps / river rule
    reachable), 2 guarded (S outside [0, 0.5], C < 0 or Z <= 0), 3 ill-conditioned (dt / (RK*3600) > 2, the river:
    literal arithmetic).  Class 3 as well, for the literal arithmetic to decide what comes of it: a row with a NaN or an
    infinite parameter, or a share or a residence time that is none (D or H outside [0, 1], T < 0, a k <= 0); and, when
    initial ([C, N, 12] or [N, 12] states) is given with area (the catchments' areas, scalar or [C]), a row whose
    initial states hold a NaN, an infinity, a negative volume, or soil so far above its capacity that
    S * sum(levels) / Z starts beyond 0.5 or H * sum(levels) / Z beyond 1 (in any catchment).  -> int64 [N]"""
    k = params[:, 6:10] * 3600.0
    cls = torch.zeros(params.shape[0], dtype=torch.int64, device=params.device)
    cls[~(k >= delta_sec).all(dim=1)] = 1
    cls[~((params[:, 4] >= 0.0) & (params[:, 4] <= 0.5) & (params[:, 1] >= 0.0) & (params[:, 5] > 0.0))] = 2
    cls[~(k[:, 3] >= 0.5 * delta_sec)] = 3
    cls[~torch.isfinite(params).all(dim=1)] = 3
    # shares that are none (D or H outside [0, 1], a negative T): negative inflows, the reference's clamps -- literal too
    cls[~((params[:, 3] >= 0.0) & (params[:, 3] <= 1.0) & (params[:, 2] >= 0.0) & (params[:, 2] <= 1.0) &
          (params[:, 0] >= 0.0))] = 3
    cls[~(params[:, 6:10] > 0.0).all(dim=1)] = 3      # ... and residence times that are none (k <= 0)
    cls[~(params[:, 5] > 0.0)] = 3                    # ... and a soil without capacity (Z <= 0: quotients by it)
    cls[~(params[:, 0] >= 0.2) | ~(params[:, 5] <= 1.0e3)] = 3   # ... and a discharge orders below the rain's
    cls[~(params[:, 5] >= 1.0)] = 3                   # ... and a soil of less than a millimetre
    if initial is not None:
        st = initial.reshape(-1, params.shape[0], 12)
        ar = torch.as_tensor(area, dtype=torch.float64, device=params.device).reshape(-1, 1)
        bad = (~torch.isfinite(st) | (st < 0.0)).any(dim=2)                  # (-0.0 is a zero like any other)
        lay = torch.zeros_like(st[:, :, 5])         # summed in wave_class()'s order: 0.0 + ly1 + ... + ly6, left to right
        for i in range(5, 11):
            lay = lay + st[:, :, i]
        fill = (lay / ar * 1e3) / params[:, 5].unsqueeze(0)                    # tot / Z of the first step
        s_init = params[:, 4].unsqueeze(0) * fill
        h_init = params[:, 2].unsqueeze(0) * fill     # the overland share of the first rainy step's excess: beyond one it
        bad = bad | ~(s_init <= 0.5) | ~(h_init <= 1.0)     # leaves the filling a negative excess (wave_class has the story)
        cls[bad.any(dim=0)] = 3
    return cls


def _variant_grouping(params, delta_sec, sort_rows=False, initial=None, area=None):
    """A wavefront runs ONE variant for its 64 lanes, the most general one any of its rows needs.  To keep a row's
    arithmetic (and cost) independent of its neighbours, rows are grouped by variant before the launch, each group
    padded to whole wavefronts with copies of its last row.  Returns (gather [N_run], inverse [N]) or None when the
    matrix needs no reordering (one variant only -- always the case for hourly steps with the default ranges).
    params, delta_sec, initial and area are those of variant_classes(), which decides the variants.

    sort_rows: within a variant, order the rows so that the 64 samples of a wavefront behave alike -- by T (the
    rainfall correction factor) in 64 bins, then by S * Z.  Wet or dry is decided by the sign of rain * T - peva, so a
    wavefront whose rows have nearly the same T takes one side of that branch together on (almost) every step
    instead of executing both; and how far the rain excess of a step gets down the soil column depends on the deficit
    the leaks have left in the top layers, which goes with S * Z -- rows alike in it let the wave-uniform early exits
    of the filling cascade fire.  -2.5 % launch time at 1e5 samples, -5 % at 125,000, -8 % at 1e6
    (tools/debug/sort_rows.py).  Only asked for when no discharge matrix is stored -- its columns would have to be
    permuted back, which costs more than the launch gains; the per-sample results are permuted back on the way out."""
    cls = variant_classes(params, delta_sec, initial, area)
    mixed = int(cls.min()) != int(cls.max())
    if not mixed and not sort_rows:
        return None
    pieces = []
    for c in range(4):
        idx = torch.nonzero(cls == c)[:, 0] if mixed else (torch.arange(params.shape[0], device=params.device)
                                                            if c == int(cls[0]) else cls[:0])
        if idx.numel():
            if sort_rows:
                t, sz = params[idx, 0], params[idx, 4] * params[idx, 5]
                span = lambda v: (v - v.min()) / torch.clamp(v.max() - v.min(), min=1e-300)     # noqa: E731
                idx = idx[torch.argsort(torch.clamp((span(t) * 64).floor(), max=63) * 2.0 + span(sz), stable=True)]
            pad = (-idx.numel()) % 64 if mixed else 0
            pieces.append(torch.cat([idx, idx[-1:].expand(pad)]) if pad else idx)
    gather = torch.cat(pieces)
    inverse = torch.empty(params.shape[0], dtype=torch.int64, device=params.device)
    inverse[gather] = torch.arange(gather.numel(), device=params.device)    # duplicates hold identical results
    return gather, inverse


_MemoEntry = collections.namedtuple('_MemoEntry', 'refs versions key value')


class _Memo(object):
    """One prepare_ensemble() call's handle on what has been worked out about its (params, forcing) pair: the variant
    grouping of the rows and the launch plan (which kernels the rows and the forcing need, smart_plan_ensemble).  What
    is remembered is tied to the tensor OBJECTS the caller passed (weak references), their in-place version counters at
    the time and the key (everything else the two depend on), never to addresses: a fresh tensor that happens to reuse
    a freed address starts from nothing.  Nothing is remembered (`applies` is False) outside fast mode, with initial
    states (the rows' classes depend on them as well) or when an input was converted on the way in (anything but a
    tensor on the device: a fresh object is classified afresh); lookup(), store() and forget() then do nothing, as they
    do once one of the tensors is gone.  One list of entries for the process, at most SIZE, guarded by a lock (the C
    side is thread-aware as well: DeviceCtx::mu)."""
    _entries = []
    _lock = threading.Lock()
    SIZE = 8

    def __init__(self, inputs, key, device, initial=None, fast=True):
        on = [t for t in inputs if isinstance(t, torch.Tensor) and t.device.type == device.type]
        self.applies = fast and initial is None and len(on) == len(inputs)
        self.refs, self.key = [weakref.ref(t) for t in on], key
        self.refresh()

    def refresh(self):
        """Take the version counters again (None: the tensor is gone): what is stored next describes the tensors as
        they are now."""
        self.versions = tuple(None if r() is None else r()._version for r in self.refs)

    def _is_about(self, ent):
        return (self.applies and ent.key == self.key and len(ent.refs) == len(self.refs)
                and all(r() is not None and r() is mine() for r, mine in zip(ent.refs, self.refs)))

    def lookup(self):
        """The value stored last for these objects at these versions under this key, or None.  Entries whose tensors
        have died are dropped on the way."""
        with self._lock:
            self._entries[:] = [ent for ent in self._entries if all(r() is not None for r in ent.refs)]
            hits = [ent.value for ent in self._entries if self._is_about(ent) and ent.versions == self.versions]
        return hits[-1] if hits else None

    def store(self, value):
        if self.applies and None not in self.versions:
            with self._lock:
                self._entries.append(_MemoEntry(self.refs, self.versions, self.key, value))
                del self._entries[:-self.SIZE]

    def forget(self):
        """Drop what is remembered about these tensors: it turned out stale without a version bump (a write through
        ctypes, a foreign kernel, `.data`), and would be handed out again to the next prepare_ensemble()."""
        with self._lock:
            self._entries[:] = [ent for ent in self._entries if not self._is_about(ent)]


def _compose_plan(planned, keep=0, row_class=None):
    """The plan word of a launch from what smart_plan_ensemble answered: that the rows were ordered is carried over
    from `keep`, the word being replaced.  With row_class, the plan of a call of ONE row of that class instead: valid,
    the kinds of forcing that `planned` (the plan in force) names, the kernel of that class and no other."""
    if row_class is not None:
        forcing = _lib.PLAN_FORCING_PIECEWISE | _lib.PLAN_FORCING_VARYING | _lib.PLAN_FORCING_RUNS
        return _lib.PLAN_VALID | (planned & forcing) | _lib.PLAN_CLASS_BITS[row_class]
    return planned | (keep & _lib.PLAN_ROWS_ORDERED)


class PreparedEnsemble(object):
    """One ensemble call, made ready: inputs on the device, output buffers, the workspace and the launch plan, all
    owned here -- launch() only enqueues the kernels (no allocation, no synchronisation), so a caller that repeats the
    call (a benchmark, a HIP-graph capture, a calibration loop over observation sets) pays for the set-up once.
    Build one with prepare_ensemble()."""

    repeated = False    # did the last verify() have to repeat the launch?

    def __init__(self, e, device, n_samples, squeeze, outputs, workspace, grouping, caller_out, keep, memo):
        self._e = e                     # the filled SmartEnsemble struct; it points into everything below
        self.device, self.n_samples, self._squeeze = device, n_samples, squeeze
        self._dis, self._gw, self._objfn, self._fin = outputs       # [C, R, ld] or None, [C, N_run], [C, N_run, 8], ...
        self._ws = workspace            # the library's scratch (None: the call needs none)
        self._grouping = grouping       # None, or (gather [N_run], inverse [N]): the rows run in another order
        self._caller_out = caller_out   # the caller's discharge buffer, when the rows had to be permuted behind it
        self._keep = keep               # the inputs on the device: alive for as long as the struct points at them
        self._memo = memo               # the _Memo of the caller's (params, forcing)

    @property
    def has_status(self):
        """Does a launch leave a status word for status() and verify()?  (The fast kernels do, in the workspace.)"""
        return self._ws is not None and self._e.math_mode == MATH_FAST

    def enqueue(self):
        """The kernels onto torch's current stream of the device, nothing else: no result object is built, nothing is
        permuted or copied (launch() = enqueue() + result())."""
        with torch.cuda.device(self.device):
            self._e.stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(_lib.lib().smart_run_ensemble_hip(ctypes.byref(self._e)))

    def launch(self):
        """Enqueue on torch's current stream of the device.  Returns the EnsembleResult (views of this object's
        buffers: the next launch() overwrites them)."""
        self.enqueue()
        return self._result()

    def result(self):
        """The EnsembleResult of the last enqueue(): rows back in the caller's order (one permutation of the outputs
        when the rows were grouped; the stored discharge matrix included)."""
        return self._result()

    def status(self):
        """SMART_STATUS_* bits of the last launch (synchronises with the stream)."""
        word = ctypes.c_int32(0)
        with torch.cuda.device(self.device):
            self._e.stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(_lib.lib().smart_launch_status(ctypes.byref(self._e), ctypes.byref(word)))
        return int(word.value)

    def describe(self):
        """The kernels launch() enqueues on this device, as text (smart_describe_launch)."""
        buf = ctypes.create_string_buffer(512)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().smart_describe_launch(ctypes.byref(self._e), buf, len(buf)))
        return buf.value.decode()

    def verify(self):
        """Read the status word of the last launch and repair what it reports: a time slice that gave up waiting for
        its predecessor (never seen on an idle GPU; possible when the queue is preempted) -> the launch is repeated
        unsliced; a plan that no longer matches the inputs -> re-planned and repeated.  Raises if the second launch
        is not clean either.  Returns the result to use."""
        word = self.status()
        self.repeated = word != 0
        if word == 0:
            return self._result()
        warnings.warn("smartpy_amd: launch status %#x (%s); repeating the launch %s" % (
            word, ' + '.join(n for b, n in ((_lib.STATUS_SLICE_TIMEOUT, 'a time slice timed out'),
                                            (_lib.STATUS_STALE_PLAN, 'stale plan'),
                                            (_lib.STATUS_NONFINITE_FORCING, 'a NaN or an infinity in the forcing'))
                             if word & b),
            'in literal arithmetic' if word & _lib.STATUS_NONFINITE_FORCING else (
                'without time slices' if word & _lib.STATUS_SLICE_TIMEOUT else 'with a fresh plan')))
        if word & _lib.STATUS_NONFINITE_FORCING:
            # what the reference's branches make of a NaN only the literal kernel reproduces (forcing that came from the
            # host never gets here: prepare_ensemble looked at it)
            self._e.math_mode = MATH_LITERAL
        if word & _lib.STATUS_SLICE_TIMEOUT:
            self._e.time_slices = 1
        if word & _lib.STATUS_STALE_PLAN:
            self._memo.forget()      # what was remembered about these tensors is what went stale
            self._memo.refresh()
            self._plan()
            self._memo.store((self._grouping, int(self._e.plan)))
        self.enqueue()
        word = self.status()
        if word != 0:
            raise SmartEngineError(-6, "smartpy_amd: the repeated launch reports status %#x as well" % word)
        return self._result()

    def _plan(self, ordered=0):
        """Ask the library which kernels the rows and the forcing need (smart_plan_ensemble: synchronises) and make
        that the plan of the launches to come; that the rows were ordered stays on record across a re-plan."""
        keep, word = self._e.plan | ordered, ctypes.c_int32(0)
        self._e.plan = 0
        with torch.cuda.device(self.device):
            self._e.stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(_lib.lib().smart_plan_ensemble(ctypes.byref(self._e), ctypes.byref(word)))
        self._e.plan = _compose_plan(int(word.value), keep)

    def aim_at(self, row_class):
        """A call of ONE row: the plan names the kernel of that row's class and no other (the forcing stays as planned)."""
        self._e.plan = _compose_plan(self._e.plan, row_class=row_class)

    def _result(self):
        dis, gw, objfn, fin = self._dis, self._gw, self._objfn, self._fin
        if self._grouping is not None:        # back to the caller's row order
            inverse = self._grouping[1]
            gw = gw[:, inverse]
            objfn = None if objfn is None else objfn[:, inverse]
            fin = None if fin is None else fin[:, inverse]
            if dis is not None:
                if self._caller_out is not None:
                    self._caller_out[:, :, :self.n_samples].copy_(torch.index_select(dis, 2, inverse))
                    dis = self._caller_out
                else:
                    dis = torch.index_select(dis, 2, inverse)
        return EnsembleResult(dis, gw, objfn, fin, self.n_samples, self._squeeze)


def _normalise_inputs(params, forcing, report, math_mode, device):
    """Step 1 of prepare_ensemble(): both inputs on the device, the forcing as [C, T, 2], report type and math mode as codes."""
    device = torch.device(device) if device is not None else (
        params.device if isinstance(params, torch.Tensor) and params.is_cuda else default_device())
    forcing_in = forcing
    params = as_device(params, device)
    forcing = as_device(forcing, device)
    squeeze = forcing.dim() == 2
    if squeeze:
        forcing = forcing.unsqueeze(0)
    if forcing.shape[2] != 2:
        raise Exception("forcing must be [T, 2] or [C, T, 2] (rain, peva)")
    if params.dim() != 2 and params.shape[0] != forcing.shape[0]:
        raise Exception("params [C, N, 10] must have one block per catchment")
    if params.shape[-1] != 10:
        raise Exception("params must have 10 columns (T, C, H, D, S, Z, SK, FK, GK, RK)")
    pstride = 0 if params.dim() == 2 else params.shape[1] * 10
    rtype = report_code(report)
    try:
        mmode = _MATH[math_mode]
    except KeyError:
        raise Exception("math mode '{}' unknown.".format(math_mode))
    # A NaN or an infinity in the forcing (a gap someone filled with 'nan'): the reference's branches see it -- a NaN
    # excess is "not wet", the evaporation cascade then empties all six layers (structure.py:359, :409-419) -- and only
    # the literal kernel takes those decisions; the fast kernels are compiled for numbers.  Forcing that arrives from
    # the host is looked at here; a caller who keeps it on the device says math_mode='literal' for such data.
    if mmode == MATH_FAST and not (isinstance(forcing_in, torch.Tensor) and forcing_in.is_cuda):
        if not bool(np.isfinite(np.asarray(forcing_in, dtype=np.float64)).all()):
            mmode = MATH_LITERAL
    return device, params, forcing, squeeze, pstride, rtype, mmode


def _allocate_outputs(C, R, N, device, want_discharge, want_objfn, want_final, discharge_out):
    """Step 3: (discharge [C, R, ld >= N] or None, gw [C, N], objfn [C, N, 8] or None, final_vars [C, N, 19] or None)."""
    dis = discharge_out
    if dis is not None:
        assert dis.is_contiguous() and dis.dtype == torch.float64 and dis.shape[:2] == (C, R) and dis.shape[2] >= N
    elif want_discharge:
        dis = torch.empty((C, R, N), dtype=torch.float64, device=device)
    return (dis, torch.empty((C, N), dtype=torch.float64, device=device),
            torch.empty((C, N, 8), dtype=torch.float64, device=device) if want_objfn else None,
            torch.empty((C, N, 19), dtype=torch.float64, device=device) if want_final else None)


def _fill_struct(inputs, outputs, pstride, n_warm, report_gap, rtype, mmode, delta_sec, time_slices, literal_form):
    """Step 4: the SmartEnsemble of include/smart_amd.h, pointing at the inputs (area, forcing, params, extra, initial,
    obs, gw_obs) and the outputs of step 3."""
    def ptr(t):
        return None if t is None else t.data_ptr()

    forcing, params, dis = inputs[1], inputs[2], outputs[0]
    e = _lib.SmartEnsemble()
    e.n_catchments, e.n_samples, e.n_steps, e.n_warm = forcing.shape[0], params.shape[-2], forcing.shape[1], int(n_warm)
    e.report_gap, e.report_type, e.math_mode, e.delta_sec = int(report_gap), rtype, mmode, float(delta_sec)
    e.area_m2, e.forcing, e.params, e.extra, e.initial, e.obs, e.gw_obs = [ptr(t) for t in inputs]
    e.discharge, e.gw, e.objfn, e.final_vars = [ptr(t) for t in outputs]
    e.discharge_ld = params.shape[-2] if dis is None else dis.shape[2]
    e.params_catchment_stride, e.time_slices = pstride, int(time_slices)
    try:
        e.literal_form = _LITERAL_FORMS[literal_form]
    except KeyError:
        raise Exception("literal_form '{}' unknown ('auto', 'rows' or 'lanes').".format(literal_form))
    return e


def _size_workspace(e, device):
    """Step 5: the caller of the C ABI owns every buffer, the library's scratch included (header, observation statistics,
    slice hand-over); with it in place the library checks the whole struct."""
    with torch.cuda.device(device):
        n_ws = int(_lib.lib().smart_workspace_bytes(ctypes.byref(e)))
    ws = torch.empty((n_ws + 7) // 8, dtype=torch.float64, device=device) if n_ws > 0 else None
    e.workspace, e.workspace_bytes = (None if ws is None else ws.data_ptr()), n_ws
    _lib.check(_lib.lib().smart_check_ensemble(ctypes.byref(e)))
    return ws


def prepare_ensemble(params, forcing, area_m2, delta_sec, n_warm, report_gap, report='summary', extra=None,
                     initial=None, obs=None, gw_obs=None, math_mode='fast', want_discharge=True, want_objfn=None,
                     want_final=False, device=None, discharge_out=None, group_variants=True, time_slices=0,
                     literal_form='auto'):
    """Everything of run_ensemble() short of the launch: see PreparedEnsemble.  Arguments as run_ensemble()."""
    _lib.lib()      # (a library that cannot be loaded is reported before anything else)
    inputs_in = (params, forcing)
    device, params, forcing, squeeze, pstride, rtype, mmode = _normalise_inputs(params, forcing, report, math_mode, device)
    C, T, N = forcing.shape[0], forcing.shape[1], params.shape[-2]
    R = n_reports(T, report_gap, rtype)
    area = _per_catchment(area_m2, device, C)
    extra = _per_catchment(extra_vector(extra) if isinstance(extra, dict) else extra, device, C, (7,))
    initial = _per_catchment(initial, device, C, (N, 12))
    if want_objfn is None:
        want_objfn = obs is not None
    if want_objfn and obs is None:
        raise Exception("objective functions need observations")
    obs = _per_catchment(obs, device, C, (R,))
    gw_obs = _per_catchment(gw_obs, device, C)

    sort_rows = not want_discharge and discharge_out is None
    memo = _Memo(inputs_in, (float(delta_sec), int(report_gap), rtype, C, N, T, bool(group_variants), sort_rows),
                 device, initial, mmode == MATH_FAST)
    known = memo.lookup()               # (grouping, plan) of an earlier call with these very tensors, or None
    grouping, caller_out = None, None
    if group_variants and mmode == MATH_FAST and pstride == 0 and N > 64:     # one shared matrix, more than a wavefront
        grouping = known[0] if known else _variant_grouping(params, float(delta_sec), sort_rows, initial, area)
    if grouping is not None:            # the rows run in that order
        params = params[grouping[0]].contiguous()
        initial = None if initial is None else initial[:, grouping[0]].contiguous()
    if grouping is not None and discharge_out is not None:
        caller_out, discharge_out, want_discharge = discharge_out, None, True     # permuted into it by result()
    outputs = _allocate_outputs(C, R, params.shape[-2], device, want_discharge, want_objfn, want_final, discharge_out)
    inputs = (area, forcing, params, extra, initial, obs, gw_obs)
    e = _fill_struct(inputs, outputs, pstride, n_warm, report_gap, rtype, mmode, delta_sec, time_slices, literal_form)
    p = PreparedEnsemble(e, device, N, squeeze, outputs, _size_workspace(e, device), grouping, caller_out, inputs, memo)
    if p.has_status:
        if known:
            e.plan = known[1]
        elif not torch.cuda.is_current_stream_capturing():
            # (planning synchronises: inside a graph capture the plan stays 0 and every kernel the call could need runs)
            p._plan(_lib.PLAN_ROWS_ORDERED if (sort_rows and grouping is not None) else 0)
            memo.store((grouping, int(e.plan)))
    return p


def run_ensemble(params, forcing, area_m2, delta_sec, n_warm, report_gap, report='summary', extra=None,
                 initial=None, obs=None, gw_obs=None, math_mode='fast', want_discharge=True, want_objfn=None,
                 want_final=False, device=None, discharge_out=None, group_variants=True, time_slices=0, verify=True,
                 literal_form='auto'):
    """One launch of the whole ensemble: the batched form of the spotpy loop over MonteCarlo.simulation /
    objectivefunction (montecarlo.py:153-154,179-209).

    params   [N, 10] or [C, N, 10]    forcing [T, 2] or [C, T, 2] (rain, peva per step)
    area_m2  scalar or [C]            extra   dict / 7-vector / [C, 7] / None
    initial  [N, 12] / [C, N, 12]     obs     [R] or [C, R], NaN = missing    gw_obs scalar / [C] / None

    verify: read the launch's status word afterwards (synchronises with the stream) and repeat the launch if a time
    slice timed out; skipped while the stream is being captured into a HIP graph.  Callers that pipeline launches
    use prepare_ensemble() / launch() and call verify() when they synchronise anyway.

    literal_form: how the rows that need the reference's own operation order (class 3: dt / RK > 2 -- a tenth of a daily
    ensemble -- or a parameter that is none) are laid over the wavefronts: 'rows' (one sample per DPP row, the latency
    form), 'lanes' (one per lane, the throughput form) or 'auto' (from the number of such blocks the plan counted).
    The same bits either way.
    """
    p = prepare_ensemble(params, forcing, area_m2, delta_sec, n_warm, report_gap, report=report, extra=extra,
                         initial=initial, obs=obs, gw_obs=gw_obs, math_mode=math_mode,
                         want_discharge=want_discharge, want_objfn=want_objfn, want_final=want_final, device=device,
                         discharge_out=discharge_out, group_variants=group_variants, time_slices=time_slices,
                         literal_form=literal_form)
    p.enqueue()
    # (verify() builds the result once: after the status word has been read)
    out = p.verify() if verify and p.has_status and not torch.cuda.is_current_stream_capturing() else p.result()
    out._prepared = p       # the result's tensors live in the prepared call's buffers
    return out


class SingleRun(object):
    """ONE parameter set at a time over a fixed forcing series -- SMART.simulate() (smart.py:154-210), the call a
    calibration loop written against the reference's per-sample protocol makes thousands of times
    (montecarlo.py:179-186) -- made ready once: the forcing on the device, a [1, 10] parameter buffer, the outputs, the
    workspace and what smart_plan_ensemble found out about the forcing all live here.  run(params) then copies 80
    bytes to the device, enqueues the one kernel the row's class needs, and brings [R] + 1 doubles back; nothing is
    allocated, the forcing is not touched, no planning kernel runs."""

    def __init__(self, forcing, area_m2, delta_sec, n_warm, report_gap, report='summary', extra=None, device=None,
                 math_mode='fast'):
        self.device = torch.device(device) if device is not None else default_device()
        self.delta_sec = float(delta_sec)
        self.params = torch.zeros((1, 10), dtype=torch.float64, device=self.device)
        self._host = torch.zeros((1, 10), dtype=torch.float64).pin_memory() if self.device.type == 'cuda' \
            else torch.zeros((1, 10), dtype=torch.float64)
        self.forcing = forcing if isinstance(forcing, torch.Tensor) and forcing.is_cuda else as_device(forcing, self.device)
        self._args = (area_m2, delta_sec, n_warm, report_gap)
        self._kw = dict(report=report, extra=extra, math_mode=math_mode, device=self.device)
        self._prep = None

    def run(self, params):
        """params: the ten values (T, C, H, D, S, Z, SK, FK, GK, RK).  -> (discharge ndarray [R], gw float)."""
        global h2d_bytes
        row = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(1, 10))
        self._host.copy_(torch.from_numpy(row))
        self.params.copy_(self._host, non_blocking=True)        # the 80 bytes of this call
        h2d_bytes += 80
        if self._prep is None:
            # the first call plans: which kinds of forcing the series holds comes back once and stays in the plan
            self._prep = prepare_ensemble(self.params, self.forcing, *self._args, **self._kw)
        p = self._prep
        if p.has_status:
            # the row's class on the host (ten numbers, the rules of wave_class): the plan names its kernel and no other
            p.aim_at(int(_lib.lib().smart_row_class(row.ctypes.data, self.delta_sec, None, 0.0)))
        p.enqueue()
        out = p.verify() if p.has_status else p.result()
        return np.ascontiguousarray(out.discharge.cpu().numpy()[0]), float(out.gw.cpu().numpy()[0])


# the analyses of a stored discharge matrix live in analysis.py; every name of them is a name of this module as well
from .analysis import (objective_functions, quantiles_sort_capacity, weighted_quantiles,  # noqa: E402,F401
                       objfn_max_windows, objective_functions_windows, flow_duration_sort_capacity, flow_duration,
                       SIGNATURE_NAMES, signatures,
                       sobol_max_resamples, sobol_lds_capacity, sobol_counts, SobolResult, sobol_indices,
                       bootstrap_max_windows, bootstrap_max_resamples, bootstrap_counts, jackknife_counts,
                       BootstrapResult, objective_functions_bootstrap,
                       pareto_max_objectives, pareto_counts, pareto_ranks,
                       ENSEMBLE_SCORE_NAMES, ensemble_scores_lds_capacity, ensemble_scores,
                       dynia_max_half_width, dynia_lds_capacity, DyniaResult, dynamic_identifiability,
                       pawn_lds_capacity, PawnResult, pawn_ks,
                       ERROR_MODEL_ROWS, residual_log_likelihood, predictive_draws)


def allsteps(area_m2, delta_sec, length_simu, nd_rain, nd_peva, nd_parameters, nd_initial, report_type, report_gap):
    """smartcpp.allsteps: same arguments and results as run_all_steps (structure.py:149-152,197); host arrays."""
    L = _lib.lib()
    rain = np.ascontiguousarray(nd_rain, dtype=np.float64)
    peva = np.ascontiguousarray(nd_peva, dtype=np.float64)
    par = np.ascontiguousarray(nd_parameters, dtype=np.float64)
    ini = np.ascontiguousarray(nd_initial, dtype=np.float64)
    length_simu, report_gap = int(length_simu), int(report_gap)
    if len(rain) < length_simu or len(peva) < length_simu or len(par) != 10 or len(ini) != 19:
        raise Exception("allsteps: inconsistent argument sizes")
    if report_type == REPORT_SUMMARY and report_gap > 0 and length_simu % report_gap:
        raise ValueError("cannot reshape array of size {} into shape ({})".format(length_simu, report_gap))
    R = n_reports(length_simu, report_gap, report_type)
    dis = np.empty(max(R, 0), dtype=np.float64)
    gw = ctypes.c_double(math.nan)
    fin = np.empty(19, dtype=np.float64)
    _lib.check(L.smart_allsteps_hip(float(area_m2), float(delta_sec), length_simu, rain.ctypes.data, peva.ctypes.data,
                                    par.ctypes.data, ini.ctypes.data, int(report_type), report_gap, dis.ctypes.data,
                                    ctypes.addressof(gw), fin.ctypes.data))
    return dis, gw.value, fin


def hook_counters():
    """{calls, allocations, forcing_bytes_uploaded, fast_calls, plans} of the smartcpp.allsteps stand-in since the library
    was loaded (smart_hook_counters)."""
    c = (ctypes.c_int64 * 5)()
    _lib.check(_lib.lib().smart_hook_counters(c, 5))
    return dict(zip(('calls', 'allocations', 'forcing_bytes_uploaded', 'fast_calls', 'plans'), (int(v) for v in c)))


def onestep(*args):
    """smartcpp.onestep: the 26 positional floats of run_one_step (structure.py:200-206) -> 19 floats."""
    if len(args) != 26:
        raise TypeError("onestep() takes exactly 26 positional arguments ({} given)".format(len(args)))
    return onestep_batch(np.asarray(args, dtype=np.float64).reshape(1, 26))[0]


def onestep_batch(inputs):
    """[n, 26] -> [n, 19]: n independent single steps in one launch."""
    L = _lib.lib()
    x = np.ascontiguousarray(inputs, dtype=np.float64)
    out = np.empty((x.shape[0], 19), dtype=np.float64)
    _lib.check(L.smart_onestep_hip(x.shape[0], x.ctypes.data, out.ctypes.data))
    return out


def river_step_batch(inputs):
    """[n, 4] (time_gap_sec, r_in_q_riv, r_p_rk [h], r_s_v_riv) -> [n, 2] (r_out_q_riv, r_s_v_riv): n independent
    calls of run_one_step_river (structure.py:461-503) in one launch."""
    L = _lib.lib()
    x = np.ascontiguousarray(inputs, dtype=np.float64)
    out = np.empty((x.shape[0], 2), dtype=np.float64)
    _lib.check(L.smart_river_step_hip(x.shape[0], x.ctypes.data, out.ctypes.data))
    return out
