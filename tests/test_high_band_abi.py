"""
The high-band entry points of the C ABI (include/pv_koala_batch.h: pv_koala_batch_set_high_band / get_high_band) and the refusals that hold
while the carry is on, under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU: tests/abi_high_band/driver.cpp, a stand-alone
program linked with the shim and a recording copy of the unchanged host-only engine double of tests/abi_sanitizer
(tests/test_channel_link_abi.recording_double), which keeps the kns::Call that reaches the engine.  No Python in the program, nothing preloaded.
"""
import glob
import os

import pytest

import sanitized_build
from conftest import ROOT, model_file
from test_channel_link_abi import recording_double


def test_high_band_entry_points_under_asan_and_ubsan(tmp_path):
    gxx = sanitized_build.sanitizer_gxx()
    if not os.path.isdir(os.path.join(sanitized_build.HIP_INCLUDE, 'hip')):
        pytest.skip('needs the HIP headers')
    csrc = sanitized_build.CSRC
    sources = sorted(glob.glob(os.path.join(csrc, 'pv_api*.cpp'))) + [recording_double(tmp_path), os.path.join(ROOT, 'tests', 'abi_high_band', 'driver.cpp')]
    flags = ['-D__HIP_PLATFORM_AMD__', '-I' + sanitized_build.HIP_INCLUDE, '-I' + os.path.join(ROOT, 'include'), '-I' + csrc,
             '-Wno-deprecated-declarations', '-Wno-unused-result']
    exe = sanitized_build._build(gxx, flags, sources, os.path.join(str(tmp_path), 'abi_high_band_driver'))
    run = sanitized_build.run(exe, model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
