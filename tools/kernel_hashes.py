#!/usr/bin/env python3
"""A hash of the instruction stream of every kernel (and every device function that was not inlined) of a built library:
an edit that is meant to leave the kernels' code alone shows here whether it did.

    python tools/kernel_hashes.py [LIB.so]                       one line per kernel: instructions, hash
    python tools/kernel_hashes.py --against OTHER.so [LIB.so]    OTHER (the parent's build) beside LIB: parent / new / verdict
                                                                 per kernel; exit status 1 unless every line reads "same"

LIB defaults to the library of this tree.  The hash is the sha256 (12 hex digits) of "mnemonic operands" of every
instruction in llvm-objdump's order: registers, immediates and relative branch distances count, addresses do not, so a
kernel may move to another translation unit.  Kernels are matched by their demangled name WITHOUT the parameter list
(`smart::smart_fdc_sort<1024, 16>`): renaming a parameter's struct is no difference."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smartpy_amd.isa_lint import OBJDUMP, parse      # noqa: E402

LIB = os.path.join(ROOT, 'smartpy_amd', 'csrc', 'libsmart_amd.so')


def short_name(demangled):
    """`void smart::f<(smart::E)1, 4>(long, smart::P) [clone]` -> `smart::f<(smart::E)1, 4>`"""
    depth = 0
    for i, ch in enumerate(demangled):
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            demangled = demangled[:i]
            break
    return re.sub(r'^void ', '', demangled)      # (an instance of a template is printed with its return type)


def _run(*args):
    return subprocess.run([OBJDUMP] + list(args), check=True, capture_output=True, text=True).stdout


def kernel_hashes(lib):
    """{name without parameters: (instructions, hash)} over the gfx950 code objects bundled in `lib`"""
    found = {}
    tmp = tempfile.mkdtemp(prefix='smart_hashes_')
    try:
        copy = os.path.join(tmp, os.path.basename(lib))
        shutil.copy(lib, copy)
        _run('--offloading', copy)      # (writes the code objects next to its input)
        for f in sorted(os.listdir(tmp)):
            if 'gfx950' not in f:
                continue
            path = os.path.join(tmp, f)
            names = {int(m.group(1), 16): short_name(m.group(2)) for m in
                     re.finditer(r'^([0-9a-f]+) \S+\s+F \.text\t[0-9a-f]+ (?:\.\w+ )?(.*)$', _run('-t', '-C', path), re.M)}
            for m in re.finditer(r'^([0-9a-f]+) <([^>]+)>:\n(.*?)(?=^\S|\Z)', _run('-d', path), re.M | re.S):
                start = int(m.group(1), 16)
                ins = [x for x in parse(start, m.group(3)) if x['op'] != 's_code_end']
                text = '\n'.join(x['op'] + ' ' + x['args'] for x in ins)
                found.setdefault(names.get(start, m.group(2)), []).append(
                    (len(ins), hashlib.sha256(text.encode()).hexdigest()[:12]))
    finally:
        shutil.rmtree(tmp)
    # a file-local device function may exist once per code object under one name: numbered in the order of their hashes
    return {k + (' #%d' % (i + 1) if len(v) > 1 else ''): x for k, v in found.items() for i, x in enumerate(sorted(v))}


def compare(parent, new):
    """-> (lines of the table, number of kernels that are not the same)"""
    width = max(len(k) for k in list(parent) + list(new))
    cell = lambda v: '%7d %s' % v if v else '%7s %-12s' % ('-', '-')      # noqa: E731
    lines = ['%-*s  %20s  %20s  verdict' % (width, 'kernel', 'parent', 'new')]
    bad = 0
    for k in sorted(set(parent) | set(new)):
        a, b = parent.get(k), new.get(k)
        verdict = 'same' if a == b else ('DIFFERENT' if a and b else ('MISSING in the new library' if a else 'NEW'))
        bad += verdict != 'same'
        lines.append('%-*s  %s  %s  %s' % (width, k, cell(a), cell(b), verdict))
    lines.append('# %d kernels and device functions the same, %d not' % (len(lines) - 1 - bad, bad))
    return lines, bad


def main(argv):
    args = list(argv)
    other = None
    if '--against' in args:
        i = args.index('--against')
        other = args[i + 1]
        del args[i:i + 2]
    lib = args[0] if args else LIB
    new = kernel_hashes(lib)
    if other is None:
        for k in sorted(new):
            print('%-60s %6d instructions  %s' % (k, new[k][0], new[k][1]))
        return 0
    lines, bad = compare(kernel_hashes(other), new)
    print('\n'.join(lines))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
