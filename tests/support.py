"""What the test files share, each written once: the comparisons ("equal" has one meaning per name), the example
catchment, the seeded inputs of the windowed analyses, the margins a module records and prints, and the device plumbing of
the C-entry tests.  A plain module: pytest does not collect it, and it imports torch and smartpy_amd inside the functions
that need them.  Its checks return a bool for the test to assert on (pytest rewrites `assert` only in test modules)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

EXTRA = {'aar': 1200, 'r-o_ratio': 0.45, 'r-o_split': (0.10, 0.15, 0.15, 0.30, 0.30)}
SENTINEL = -7.0         # what an output buffer holds before a call
GUARD = 64              # elements of SENTINEL on either side of a guarded output
#: the 'min' threshold on the sampling run's NSE in the GLUE tests (256 rows from np.random.seed(2024) on the example
#: catchment): between 10 and 200 of the rows pass
NSE_MIN = 0.2
GATE = 1e-9             # the relative gate the analysis tests of the suite hold a kernel's results to
SMALL = 1e-6            # a finite |truth| below this is left out of relative comparisons
E_NULL, E_SIZE, E_NO_DEVICE, E_MODE = -1, -2, -6, -7
FAKE = 0x1000           # a non-NULL address that no refusal path reads


# ---- comparisons -------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    """both cast to float64 (an int or float32 array against its float64 value passes), then shape and bit patterns"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_bits(a, b):
    """shape, dtype and bytes: no cast, so float32 is not float64 and int32 is not int64"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def tensors_same_bits(a, b):
    """two lists of float64 device tensors (None for an output that was not asked for), pairwise bit for bit"""
    import torch
    return all((x is None and y is None) or torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def same(a, b):
    """`==` everywhere (so -0.0 is 0.0), NaN where NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same_values(a, b, any_nan=False):
    """bit-equal, a zero against a zero of either sign included; with any_nan, NaN against NaN of any payload"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    ok = (a.view(np.int64) == b.view(np.int64)) | ((a == 0.0) & (b == 0.0))
    if any_nan:
        ok |= np.isnan(a) & np.isnan(b)
    return bool(np.all(ok))


def rel(a, b, floor=0.0):
    """max |a - b| / max(|a|, |b|); magnitudes that are not above `floor` count as equal (subnormal reservoir volumes that
    have been draining for ten years carry no relative precision).  Symmetric, and a NaN is not an error here:
    rel_to_want is the one that minds them."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    m = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(m > floor, np.abs(a - b) / m, 0.0)
    return float(np.max(r)) if r.size else 0.0


def rel_to_want(got, want, floor=1e-12):
    """max |got - want| / max(|want|, floor); a NaN on one side only counts as infinitely far.  Unlike rel: relative to
    `want` alone, |want| floored instead of small values skipped, shapes and the pattern of NaN part of the verdict."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return float('inf')
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), floor)))


def excess(got, want, rtol, top=None, top_frac=1e-13, tiny=1e-40, empty_ok=False):
    """Largest |got - want| / (rtol * |want| + top_frac * top + tiny); <= 1 is within the tolerance, and the call sites
    ask for a fraction of it (their EXCESS_GATE).  `top` is the largest magnitude of
    the row (default: of `want` along its last axis): a value that has drained to 1e-9 of its row's peak carries the
    absolute rounding of the states it came from, not nine digits of its own.  `tiny`: a catchment that never held
    water carries storages of 1e-59 m3, whose last digits the river's 95 % rule flips on rounding noise -- zero, to any
    hydrologist, in any of the units compared here (m3, m3/s, mm).  The shapes have to be equal and `want` has to hold
    something; with empty_ok, shapes that broadcast pass and nothing to compare is a margin of 0."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    if empty_ok:
        if want.size == 0:
            return 0.0
    elif got.shape != want.shape or not want.size:
        raise AssertionError('excess(): got of shape %s against want of shape %s' % (got.shape, want.shape))
    if top is None:
        top = np.abs(want).max(axis=-1, keepdims=True) if want.ndim > 1 else np.abs(want).max()
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.abs(got - want) / (rtol * np.abs(want) + top_frac * top + tiny)
    return float(np.nanmax(np.where(np.abs(got - want) == 0, 0.0, r)))


# ---- margins -----------------------------------------------------------------------------------------------------------
class Margins(dict):
    """key -> (the largest margin of this run, where it was seen).  A module keeps one, notes into it as it compares, and
    its autouse fixture publishes the table it makes of it when the module is done."""

    def note(self, key, margin, where=''):
        if margin > self.get(key, (-1.0, ''))[0]:
            self[key] = (margin, where)

    def excess(self, *args, **kw):
        """excess(...), noted under the CALLER's function and line: one key per comparison of the test file"""
        worst = excess(*args, **kw)
        frame = sys._getframe(1)
        self.note('%s:%d' % (frame.f_code.co_name, frame.f_lineno), worst)
        return worst

    @staticmethod
    def publish(text, directory=None, name=None):
        """print the text, and write it (newline-terminated) to directory/name where the directory exists"""
        print('\n' + text)
        if directory and os.path.isdir(directory):
            with open(os.path.join(directory, name), 'w') as fh:
                fh.write(text if text.endswith('\n') else text + '\n')


def margins_dir():
    return os.environ.get('SMART_MARGINS_DIR')


def hold(margins, path, what, got, want, bnd):
    """scores against their exact truth and the bound derived for them: the pattern of NaN and of infinities equal, every
    finite entry within its bound; the largest used fraction is noted in `margins` under `path`.  (Plain asserts with
    their own messages: this module is not rewritten by pytest.)"""
    assert got.shape == want.shape == bnd.shape, what
    finite = np.isfinite(want)
    with np.errstate(all='ignore'):
        used = np.where(finite & np.isfinite(got), np.abs(got - want) / bnd, np.where(finite, np.inf, 0.0))
    worst = float(np.max(used)) if used.size else 0.0
    where = np.unravel_index(int(np.argmax(used)), used.shape) if used.size else ()
    print('%s: %s: %.3g of the bound at %s' % (path, what, worst, where))
    margins.note(path, worst, what)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: %s: the pattern of NaN' % (path, what)
    assert np.array_equal(got[~finite & ~np.isnan(want)], want[~finite & ~np.isnan(want)]), '%s: %s: infinities' % (path, what)
    assert np.array_equal(np.isfinite(got), finite), '%s: %s: the pattern of infinities' % (path, what)
    assert worst <= 1.0, '%s: %s: %.3g times the bound at %s' % (path, what, worst, where)


# ---- the example catchment ---------------------------------------------------------------------------------------------
def example_root(tmp_path):
    """a copy of the example catchment's input files (tests/golden/data/in) under tmp_path -> the root to run from"""
    root = os.path.join(str(tmp_path), 'data')
    shutil.copytree(os.path.join(GOLDEN, 'data', 'in'), os.path.join(root, 'in'))
    return root


def settings_file(root, name, start, end, warm, simu_minutes=60):
    """in/Catchment/<name>: a .sttngs file from `start` to `end` (dd/mm/yyyy, 09:00), daily reports, hourly steps or
    (simu_minutes=1440) daily ones"""
    with open(os.path.join(root, 'in', 'Catchment', name), 'w') as f:
        f.write('ARGUMENT,VALUE\ncatchment_area_km2,175.46\ngauged_area_km2,175.97\nstart_datetime,%s 09:00:00\n'
                'end_datetime,%s 09:00:00\nsimu_timedelta_min,%d\nreport_timedelta_min,1440\nwarm_up_days,%d\n'
                'gw_constraint,0.12667\n' % (start, end, simu_minutes, warm))


def golden_script(name):
    """tests/golden/<name>.py as a module: the script that made a fixture holds the cases, and the test runs them"""
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


# ---- seeded inputs of the windowed matrix analyses ---------------------------------------------------------------------
def data(seed, R, n, obs_plus):
    """(rng, obs [R] with 15 % missing, sim [R, n]) of one seed; the observations are |normal(3, 1.5)| + obs_plus.  (The
    signatures and the bootstrap draw theirs from cases_signatures.data: a hydrograph, not noise.)"""
    rng = np.random.default_rng(seed)
    obs = np.abs(rng.normal(3.0, 1.5, R)) + obs_plus           # (+ 0.0 leaves every bit of a magnitude as it is)
    obs[rng.random(R) < 0.15] = np.nan
    sim = rng.random((R, n)) * 6 + 0.01
    return rng, obs, sim


def window_arrays(rng, R, whole):
    """[(W, window of every row)] for W = 1, 2, 7 and 16, the last with 10 % of the rows in no window.  `whole` is how
    the single window is given: 'zeros' (an array of zeros) or None (no array at all)."""
    sixteen = (np.arange(R) * 16 // R).astype(np.int32)
    sixteen[rng.random(R) < 0.10] = -1
    return [(1, {'zeros': np.zeros(R, dtype=np.int32), None: None}[whole]), (2, (np.arange(R) >= R // 2).astype(np.int32)),
            (7, (np.arange(R) % 7).astype(np.int32)), (16, sixteen)]


def columns(rng, n, draws):
    """the first and the last of n columns and `draws` random ones, sorted, each once"""
    return np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, draws)]))


# ---- the C entries without a device: the refusal tables ----------------------------------------------------------------
def binding():
    """-> (smartpy_amd._lib, the loaded library)"""
    from smartpy_amd import _lib
    return _lib, _lib.lib()


def refusal(valid, entry, changes):
    """valid[entry] (name -> value of a call that breaks no rule) with `changes` -> (what the entry returned, the text it
    left; None for the entries that leave none).  A tuple becomes an array of doubles."""
    import ctypes
    args = dict(valid[entry], **changes)
    assert list(args) == list(valid[entry]), 'a change names no parameter of %s' % entry
    keep = [(ctypes.c_double * len(v))(*v) if isinstance(v, tuple) else v for v in args.values()]
    L = binding()[1]
    rc = getattr(L, entry)(*keep)
    return rc, (L.smart_last_error().decode() if entry.endswith('_hip') else None)


# ---- device plumbing of the C-entry tests ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def eng():
    """the engine module, on a machine with a GPU (a fixture: a test module imports it by name to have it)"""
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from smartpy_amd import engine
    return engine


def padded(matrix, pad, junk=np.nan):
    """[R, N] host matrix -> (device tensor [R, N + pad] whose padding holds `junk`, ld = N + pad)"""
    import torch
    matrix = np.asarray(matrix, dtype=np.float64)
    R, N = matrix.shape
    host = np.full((R, N + pad), junk)
    host[:, :N] = matrix
    return torch.from_numpy(host).cuda(), N + pad


def to_device(a, dtype=np.float64):
    """None, or the array as a contiguous device tensor of `dtype`"""
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def filled(shape, dtype='float64', sentinel=SENTINEL):
    """a device tensor of SENTINEL: an output with spare rows that the test expects as they were after the call"""
    import torch
    return torch.full(shape, sentinel, dtype=getattr(torch, dtype), device='cuda')


def workspace(need, least=0, fill=None):
    """`need` bytes on the device (at least `least`; None for none at all), as they come or filled with one byte"""
    import torch
    size = max(int(need), least)
    if not size:
        return None
    return torch.empty(size, dtype=torch.uint8, device='cuda') if fill is None else filled((size,), 'uint8', fill)


class Guarded:
    """`own` elements for a call to write, `tail` more behind them that it must not (a spare row, a spare window), and
    `guard` elements on either side, all holding `sentinel` before the call."""

    def __init__(self, own, tail=0, dtype='float64', guard=GUARD, sentinel=SENTINEL):
        self.own, self.guard, self.sentinel = own, guard, sentinel
        self.flat = filled((2 * guard + max(own + tail, 1),), dtype, sentinel)

    def ptr(self, null=False):
        """the address of the first element the call owns (None with `null`: an output the call is not given)"""
        return None if null else self.flat.data_ptr() + self.guard * self.flat.element_size()

    def inner(self):
        """the owned elements, on the device"""
        return self.flat[self.guard:self.guard + self.own]

    def untouched(self):
        return bool((self.flat == self.sentinel).all())

    def read(self, own=None):
        """-> (the owned elements as numpy -- the first `own` of them, should the call have been given less --, whether
        everything around them is as it was)"""
        own = self.own if own is None else own
        host = self.flat.cpu().numpy()
        intact = np.all(host[:self.guard] == self.sentinel) and np.all(host[self.guard + own:] == self.sentinel)
        return host[self.guard:self.guard + own], bool(intact)

    def intact(self):
        return self.read()[1]


def build_c_example(tmp_path):
    """examples/ensemble_from_c.c with plain gcc (C, not C++): the header is C, the only link dependencies are the
    library and the HIP runtime."""
    exe = str(tmp_path / 'ensemble_from_c')
    csrc = os.path.join(ROOT, 'smartpy_amd', 'csrc')
    subprocess.check_call(['gcc', '-O2', '-Wall', '-Werror', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include',
                           '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'examples', 'ensemble_from_c.c'),
                           '-L', csrc, '-lsmart_amd', '-L/opt/rocm/lib', '-lamdhip64', '-lm',
                           '-Wl,-rpath,' + csrc, '-Wl,-rpath,/opt/rocm/lib', '-o', exe])
    return exe
