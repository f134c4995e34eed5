"""The cuts of a time-sliced launch (smartpy_amd/csrc/smart_slice_cuts.h), on the CPU: a stand-alone program that includes
nothing of the project but that header, built by the host compiler with the address and undefined-behaviour sanitizers,
walks every (n_all, n_seg) below and checks the properties the kernels and the host rely on."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, 'smartpy_amd', 'csrc')

PROGRAM = r'''
#include "smart_slice_cuts.h"
#include <cstdio>
#include <vector>

using namespace smart;

// the header's promise: usable in constant expressions, and the headline's own cuts
static_assert(slice_cut(4018, 0, 24, 1) == 0 && slice_cut(4018, 24, 24, 1) == 4018, "ends of the axis");
static_assert(slice_cut(4018, 7, 24, 0) == 4018L * 7 / 24, "equal cuts");
static_assert(slice_taper_applies(4018, 24), "the headline is tapered");

static long bad = 0;
static void fail(const char *what, long n_all, long n_seg, long k)
{
    if (++bad <= 20)
        std::printf("FAIL %s: n_all %ld n_seg %ld slice %ld\n", what, n_all, n_seg, k);
}

static long applied = 0, fell_back = 0;

static void check(long n_all, long n_seg)
{
    std::vector<long> eq(n_seg + 1), tp(n_seg + 1); // (a heap block per case: an index past n_seg is the sanitizer's)
    for (long k = 0; k <= n_seg; ++k) {
        eq[k] = slice_cut(n_all, k, n_seg, 0);
        tp[k] = slice_cut(n_all, k, n_seg, 1);
        if (eq[k] != n_all * k / n_seg)
            fail("taper 0 is not n_all * k / n_seg", n_all, n_seg, k);
    }
    bool same = true, short_slice = false;
    for (long k = 0; k <= n_seg; ++k)
        same = same && eq[k] == tp[k];
    for (const std::vector<long> *c : {&eq, &tp}) {
        if ((*c)[0] != 0)
            fail("cut(0) != 0", n_all, n_seg, 0);
        if ((*c)[n_seg] != n_all)
            fail("cut(n_seg) != n_all", n_all, n_seg, n_seg);
        for (long k = 0; k < n_seg; ++k)
            if ((*c)[k + 1] <= (*c)[k])
                fail("cuts do not increase", n_all, n_seg, k);
    }
    for (long k = 0; k < n_seg; ++k)
        short_slice = short_slice || tp[k + 1] - tp[k] < 4;
    if (short_slice && !same)
        fail("a tapered slice under 4 intervals", n_all, n_seg, -1);
    if (n_seg < 8 && !same)
        fail("tapered with fewer than 8 slices", n_all, n_seg, -1);
    if (same != !slice_taper_applies(n_all, n_seg))
        fail("slice_taper_applies and the cuts disagree", n_all, n_seg, -1);
    if (same) {
        ++fell_back;
        return;
    }
    ++applied;
    const long m = n_seg / 4 < 6 ? n_seg / 4 : 6;
    for (long k = n_seg - m; k + 1 < n_seg; ++k)
        if (tp[k + 2] - tp[k + 1] > tp[k + 1] - tp[k])
            fail("the tail grows", n_all, n_seg, k + 1);
    if (2 * (tp[n_seg] - tp[n_seg - 1]) > tp[1] - tp[0])
        fail("the last slice is over half the first", n_all, n_seg, n_seg - 1);
    for (long k = 0; k < n_seg; ++k) // what the kernels call must be what slice_cut says
        if (slice_cut_tapered(n_all, k, n_seg) != tp[k])
            fail("slice_cut_tapered differs", n_all, n_seg, k);
}

int main()
{
    for (long n_seg = 2; n_seg <= 48; ++n_seg) {
        for (long n_all = 64; n_all <= 5000; ++n_all)
            check(n_all, n_seg);
        for (long n_all = 15 * n_seg; n_all <= 17 * n_seg; ++n_all)
            if (n_all >= n_seg)
                check(n_all, n_seg);
    }
    check(4018, 24);
    if (!slice_taper_applies(4018, 24))
        fail("the headline is not tapered", 4018, 24, -1);
    // the headline's last slice: 48 / 19897 of the axis, nine or ten intervals
    const long tail = 4018 - slice_cut(4018, 23, 24, 1);
    if (tail < 9 || tail > 10)
        fail("the headline's last slice", 4018, 24, tail);
    std::printf("applied %ld fell back %ld failures %ld\n", applied, fell_back, bad);
    return bad ? 1 : applied == 0 ? 2 : 0;
}
'''


def test_slice_cut_properties(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    src, exe = tmp_path / 'slice_cuts.cpp', tmp_path / 'slice_cuts'
    src.write_text(PROGRAM)
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I', HEADER_DIR, str(src), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' failures 0' in run.stdout
