"""
The packet kernels' own source (koala_amd/csrc/kns_packet.hip) run on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer: every
index, every 16-byte store's alignment and the whole rebuffering logic, without a GPU.  tests/packet_emulation/shim.inc stands in for HIP
(256 threads and a barrier per workgroup), driver.inc for the engine's call sequence around a delay-only frame call.
"""
import os

import pytest

import sanitized_build
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
    return sanitized_build.build_translation_unit(translation_unit(), tmp_path_factory.mktemp('packet_emulation'))


# frame length, the inner engine's max_frames = ceil(max_samples / F), max_samples
@pytest.mark.parametrize('F,max_frames,max_samples', [(256, 2, 320), (768, 2, 960), (128, 1, 80), (512, 2, 640), (256, 1, 1),
                                                      (256, 3, 701)])
def test_kernels_rebuffer_exactly_and_touch_nothing_else(emulator, F, max_frames, max_samples):
    run = sanitized_build.run(emulator, F, max_frames, max_samples)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count('samples ok') == 5
