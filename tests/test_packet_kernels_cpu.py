"""
The packet kernels' own source (koala_amd/csrc/kns_packet.hip) run on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer: every
index, every 16-byte store's alignment and the whole rebuffering logic, without a GPU.  tests/packet_emulation/shim.inc stands in for HIP
(256 threads and a barrier per workgroup), driver.inc for the engine's call sequence around a delay-only frame call.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'packet_emulation')


def translation_unit():
    header = open(os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_kernels.h')).read()
    kernels = open(os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_packet.hip')).read().replace('#include "kns_kernels.h"', '')
    kernels = kernels[:kernels.index('void launch_packet_in(')] + '}\n'
    structs = (header[header.index('struct PacketArgs {'):header.index('void launch_packet_in')] +
               header[header.index('struct PacketStateArgs {'):header.index('void launch_packet_reset')])
    return (open(os.path.join(SRC, 'shim.inc')).read() + 'namespace kns {\n' + structs + '}\n' + kernels +
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
    d = tmp_path_factory.mktemp('packet_emulation')
    (d / 'emu.cpp').write_text(translation_unit())
    exe = str(d / 'emu')
    build = subprocess.run([gxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', str(d / 'emu.cpp'),
                            '-o', exe, '-lpthread'], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


# frame length, the inner engine's max_frames = ceil(max_samples / F), max_samples
@pytest.mark.parametrize('F,max_frames,max_samples', [(256, 2, 320), (768, 2, 960), (128, 1, 80), (512, 2, 640), (256, 1, 1),
                                                      (256, 3, 701)])
def test_kernels_rebuffer_exactly_and_touch_nothing_else(emulator, F, max_frames, max_samples):
    # the environment stays as it is; a library preloaded into it may come before the sanitizer runtime, which is all the order check is about
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:verify_asan_link_order=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([emulator, str(F), str(max_frames), str(max_samples)], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count('samples ok') == 5
