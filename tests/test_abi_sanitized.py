"""
The C-ABI shim (koala_amd/csrc/pv_api.cpp, pv_api_extensions.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer:
every entry point of include/pv_koala.h, include/picovoice.h and include/pv_koala_batch.h driven through its argument checks, its
thread-local error stack (reference contract: include/picovoice.h:73-86, binding/python/_koala.py:299-312) and its ownership rules by a
C++ host (tests/abi_sanitizer/driver.cpp), with the engine replaced by a host-only double (engine_stub.cpp): no GPU, no HIP runtime.
"""
import sanitized_build
from conftest import model_file


def test_c_abi_shim_under_asan_and_ubsan(tmp_path):
    exe = sanitized_build.build_abi_driver('abi_sanitizer', tmp_path)
    garbage = tmp_path / 'garbage.bin'
    garbage.write_bytes(b'this is not a model file at all')
    run = sanitized_build.run(exe, model_file('random', 1234), garbage, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
