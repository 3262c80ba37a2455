"""
The format kernels' own source (koala_amd/csrc/kns_format.hip) run on the CPU as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer: every index, every 16-byte load's and store's alignment, the peeled heads and tails, the funnel shift at every
byte offset and both codecs in both directions, without a GPU.  tests/format_emulation/shim.inc stands in for HIP, driver.inc holds the
cases (frame matrices B = 3, T F in {128, 256, 768}; packet matrices of max_samples 1, 80 and 701 with counts 0, 1, max_samples and odd
ones in between; base pointers 1 and 15 bytes, 2 bytes, 4 and 12 bytes in) and the codecs restated.
"""
import os

import pytest

import sanitized_build
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
    return sanitized_build.build_translation_unit(translation_unit(), tmp_path_factory.mktemp('format_emulation'))


def test_kernels_convert_exactly_and_touch_nothing_else(emulator):
    run = sanitized_build.run(emulator)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    # 3 formats x 2 directions x 3 x 2 base offsets x (3 frame matrices + 3 packet matrices)
    assert 'format kernels ok: 216 cases' in run.stdout, run.stdout[-2000:]
