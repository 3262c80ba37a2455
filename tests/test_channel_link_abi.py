"""
The channel-link entry points of the C ABI (include/pv_koala_batch.h: pv_koala_batch_set_channel_link / get_channel_link) under
AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU: tests/abi_channel_link/driver.cpp, a stand-alone program linked with the shim
and the unchanged host-only engine double of tests/abi_sanitizer; and tests/abi_channel_link/forwarding.cpp, which reads the kns::Call and
kns::PacketCall that reach the engine from a recording copy of that double.
"""
import glob
import os

import sanitized_build
from conftest import ROOT, model_file


def test_channel_link_entry_points_under_asan_and_ubsan(tmp_path):
    run = sanitized_build.run(sanitized_build.build_abi_driver('abi_channel_link', tmp_path), model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])


def recording_double(directory):
    """tests/abi_sanitizer/engine_stub.cpp as it is, but process() and run_packets() keep the call they were given"""
    text = open(os.path.join(ROOT, 'tests', 'abi_sanitizer', 'engine_stub.cpp')).read()
    keep = (('Status Engine::process(const Call &c, std::string *err) {\n',
             'Call g_seen_call{};\nint g_seen_calls = 0;\n', '    g_seen_call = c, ++g_seen_calls;\n'),
            ('Status Engine::run_packets(const PacketCall &c, std::string *) {\n',
             'PacketCall g_seen_packets{};\nint g_seen_packet_calls = 0;\n', '    g_seen_packets = c, ++g_seen_packet_calls;\n'))
    for head, variables, line in keep:
        assert text.count(head) == 1, head
        text = text.replace(head, variables + head + line)
    path = os.path.join(str(directory), 'recording_engine.cpp')
    with open(path, 'w') as f:
        f.write(text)
    return path


def test_the_call_structs_reach_the_engine_with_the_setting(tmp_path):
    gxx = sanitized_build.sanitizer_gxx()
    if not os.path.isdir(os.path.join(sanitized_build.HIP_INCLUDE, 'hip')):
        import pytest
        pytest.skip('needs the HIP headers')
    csrc = sanitized_build.CSRC
    sources = sorted(glob.glob(os.path.join(csrc, 'pv_api*.cpp'))) + [recording_double(tmp_path),
                                                                        os.path.join(ROOT, 'tests', 'abi_channel_link', 'forwarding.cpp')]
    flags = ['-D__HIP_PLATFORM_AMD__', '-I' + sanitized_build.HIP_INCLUDE, '-I' + os.path.join(ROOT, 'include'), '-I' + csrc,
             '-Wno-deprecated-declarations', '-Wno-unused-result']
    exe = sanitized_build._build(gxx, flags, sources, os.path.join(str(tmp_path), 'forwarding'))
    run = sanitized_build.run(exe, model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
