"""tools/kernel_hashes.py on the built library: every kernel is listed -- the fast kernels and the ones of the matrix
analyses alike -- and a library held against itself reads "same" line by line, with exit status 0."""
import os
import subprocess
import sys

from conftest import ROOT
from smartpy_amd import build

TOOL = os.path.join(ROOT, 'tools', 'kernel_hashes.py')


def test_a_library_against_itself_is_the_same_kernel_by_kernel():
    run = subprocess.run([sys.executable, TOOL, '--against', build.LIB, build.LIB], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split('\n')
    assert lines[0].split() == ['kernel', 'parent', 'new', 'verdict']
    rows, last = lines[1:-1], lines[-1]
    assert len(rows) >= 40 and all(row.endswith('  same') for row in rows), run.stdout
    assert last == '# %d kernels and device functions the same, 0 not' % len(rows)
    for row in rows:        # name, then instructions and hash twice over
        cells = row[:-len('same')].split()
        assert cells[-4:-2] == cells[-2:] and int(cells[-2]) > 0 and len(cells[-1]) == 12, row
    names = ' '.join(rows)
    for kernel in ('smart_objfn_matrix', 'smart_fdc_sort', 'smart_quantiles_select', 'smart_objfn_windows',
                   'smart_sobol_bootstrap', 'smart_fast_intervals', 'smart_ensemble_literal'):
        assert 'smart::%s' % kernel in names, kernel


def test_a_kernel_that_differs_is_missing_or_is_new_fails_the_comparison():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        import kernel_hashes
    finally:
        sys.path.pop(0)
    parent = {'smart::a': (10, 'a' * 12), 'smart::b<1, 2>': (20, 'b' * 12), 'smart::gone': (5, 'c' * 12)}
    new = {'smart::a': (10, 'a' * 12), 'smart::b<1, 2>': (20, 'd' * 12), 'smart::fresh': (7, 'e' * 12)}
    lines, bad = kernel_hashes.compare(parent, new)
    assert bad == 3 and [line.split()[-1] for line in lines[1:-1]] == ['same', 'DIFFERENT', 'NEW', 'library']
    assert kernel_hashes.compare(parent, parent)[1] == 0
    assert kernel_hashes.short_name('void smart::f<(smart::E)1, 4>(long, smart::P) [clone .kd]') == 'smart::f<(smart::E)1, 4>'
    assert kernel_hashes.short_name('smart::g(smart::KArgs, double const*)') == 'smart::g'
