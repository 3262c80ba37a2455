"""
The format kernels' own source (koala_amd/csrc/kns_format.hip) run on the CPU as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer: every index, every 16-byte load's and store's alignment, the peeled heads and tails, the funnel shift at every
byte offset and both codecs in both directions, without a GPU.  tests/format_emulation/shim.inc stands in for HIP, driver.inc holds the
cases (frame matrices B = 3, T F in {128, 256, 768}; packet matrices of max_samples 1, 80 and 701 with counts 0, 1, max_samples and odd
ones in between; base pointers 1 and 15 bytes, 2 bytes, 4 and 12 bytes in) and the codecs restated.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'format_emulation')


def translation_unit():
    header = open(os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_kernels.h')).read()
    kernels = open(os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_format.hip')).read().replace('#include "kns_kernels.h"', '')
    kernels = kernels[:kernels.index('template <int Fmt>\nstatic void launch_format(')] + '}\n'
    section = header[header.index('enum SampleFormat {'):header.index('// fmt: kFmtF32, kFmtUlaw or kFmtAlaw')]
    return (open(os.path.join(SRC, 'shim.inc')).read() + 'namespace kns {\n' + section + '}\n' + kernels +
            open(os.path.join(SRC, 'driver.inc')).read())


@pytest.fixture(scope='module')
def emulator(tmp_path_factory):
    gxx = shutil.which('g++')
    if not gxx:
        pytest.skip('needs g++')
    # the sanitizer runtimes are looked for BEFORE the build, so that every failure of the build itself is a failure of the test
    for runtime in ('libasan.so', 'libubsan.so'):
        found = subprocess.run([gxx, '-print-file-name=' + runtime], capture_output=True, text=True, timeout=60).stdout.strip()
        if not os.path.isabs(found):  # (g++ echoes the bare name back when it has no such file)
            pytest.skip('g++ has no %s' % runtime)
    d = tmp_path_factory.mktemp('format_emulation')
    (d / 'emu.cpp').write_text(translation_unit())
    exe = str(d / 'emu')
    build = subprocess.run([gxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', str(d / 'emu.cpp'),
                            '-o', exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_kernels_convert_exactly_and_touch_nothing_else(emulator):
    # the environment stays as it is; a library preloaded into it may come before the sanitizer runtime, which is all the order check is about
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:verify_asan_link_order=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([emulator], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    # 3 formats x 2 directions x 3 x 2 base offsets x (3 frame matrices + 3 packet matrices)
    assert 'format kernels ok: 216 cases' in run.stdout, run.stdout[-2000:]
