"""The host's decision whether the backward raster may address its pixel planes with 32-bit byte offsets (sr_common.h:
plane_offsets_fit32, taken in sr_raster.hip: make_args for every call and carried to the launchers in RasterArgs::plane_off32), at its
boundaries.  The kernel holds one base per (image, tensor), so the offsets span the tensor's nch + 1 planes of 4 IS^2 bytes; they fit
while that span stays below 2^32 bytes.  Beyond it the launchers take the instantiation with 64-bit per-lane addresses.

The library exports no entry point for this (the exported names are fixed), so the test compiles the function itself, host side only,
into a small program and runs it: nothing is allocated and no device is opened.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'lasr_amd', 'csrc')

MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include "sr_common.h"
int main(int argc, char** argv)
{
    for (int i = 1; i + 1 < argc; i += 2) {
        const int nch = atoi(argv[i]), IS = atoi(argv[i + 1]);
        printf("%d %d %llu %d\n", nch, IS, lasr::plane_offset_span(nch, IS), lasr::plane_offsets_fit32(nch, IS));
    }
    return 0;
}
'''

# (channels, image side): around every boundary, small sides, and the largest side the entry points accept (32767)
CASES = [(3, 0), (3, 1), (3, 256), (3, 11585), (3, 11586), (3, 16383), (3, 16384), (3, 32767),
         (6, 1), (6, 256), (6, 12385), (6, 12386), (6, 32767),
         (9, 1), (9, 256), (9, 10362), (9, 10363), (9, 32767)]


def expected(nch, IS):
    span = (nch + 1) * IS * IS * 4
    return span, int(span < 2 ** 32)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    hipcc = shutil.which(os.environ.get('HIPCC', 'hipcc')) or '/opt/rocm/bin/hipcc'
    d = tmp_path_factory.mktemp('plane_range')
    src, exe = os.path.join(str(d), 'main.cpp'), os.path.join(str(d), 'plane_range')
    with open(src, 'w') as f:
        f.write(MAIN)
    subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O0', '-I', CSRC, '-o', exe, src], check=True, timeout=120)
    return exe


def test_boundaries_are_where_the_arithmetic_puts_them():
    # the largest side whose span is below 2^32, per channel count, from the rule itself; 3 x 11586: the span passes 2^31
    for nch, side in ((3, 16383), (6, 12385), (9, 10362)):
        assert expected(nch, side)[1] == 1 and expected(nch, side + 1)[1] == 0
    assert expected(3, 11585)[0] < 2 ** 31 <= expected(3, 11586)[0]


def test_host_predicate_at_its_boundaries(program):
    args = [str(v) for case in CASES for v in case]
    out = subprocess.run([program] + args, check=True, capture_output=True, text=True, timeout=60).stdout.split('\n')
    rows = [tuple(int(v) for v in line.split()) for line in out if line.strip()]
    assert len(rows) == len(CASES)
    for (nch, IS), row in zip(CASES, rows):
        assert row == (nch, IS) + expected(nch, IS), row


def test_the_plan_takes_the_decision_and_the_launcher_follows_it():
    raster = open(os.path.join(CSRC, 'sr_raster.hip')).read()
    make_args = raster[raster.index('static RasterArgs make_args('):raster.index('// records, pixel rects and group rects')]
    assert re.search(r'A\.plane_off32\s*=\s*plane_offsets_fit32\(c\.nch,\s*c\.IS\);', make_args)
    fast = open(os.path.join(CSRC, 'sr_backward_fast.hip')).read()
    for nch in (3, 6, 9):
        assert re.search(r'if \(A\.plane_off32\) LASR_LAUNCH_BWD\(%d, false\); else LASR_LAUNCH_BWD\(%d, true\);' % (nch, nch), fast)
    backward = raster[raster.index('ProfScope ps(K_SR_BACKWARD'):]
    assert re.search(r'else if \(A\.plane_off32\)\s*hipLaunchKernelGGL\(\(sr_backward_kernel<false, 3>\)', backward)
    assert 'sr_backward_kernel<false, 3, true>' in backward
