"""
The one recipe of the host-only sanitizer tests: stand-alone programs under AddressSanitizer + UndefinedBehaviorSanitizer, built with g++
and run as they are.  Two kinds: a driver of the C ABI (tests/abi_*/driver.cpp) linked with every koala_amd/csrc/pv_api*.cpp and the
host-only engine double (tests/abi_sanitizer/engine_stub.cpp), and a kernel emulator, one generated translation unit (tests/*_emulation).

The sanitizer runtimes are linked STATICALLY: a runtime inside the program does not care what else the loader brings into the process, or
in which order, so the programs run in the environment as it is.  The runtimes are looked for BEFORE any build: a machine without them
skips, and every failure of a build is a failure of the test.
"""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'koala_amd', 'csrc')
HIP_INCLUDE = '/opt/rocm/include'
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan']
COMMON = ['-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer'] + SANITIZE
# what the programs' own sanitizers are told
SANITIZER_OPTIONS = dict(ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')


def sanitizer_gxx():
    """g++, once it is known to have the static sanitizer runtimes (skips otherwise)"""
    gxx = shutil.which('g++')
    if not gxx:
        pytest.skip('needs g++')
    for runtime in ('libasan.a', 'libubsan.a'):
        found = subprocess.run([gxx, '-print-file-name=' + runtime], capture_output=True, text=True, timeout=60).stdout.strip()
        if not os.path.isabs(found):  # (g++ echoes the bare name back when it has no such file)
            pytest.skip('g++ has no %s' % runtime)
    return gxx


def _build(gxx, flags, sources, exe):
    build = subprocess.run([gxx] + COMMON + flags + sources + ['-o', exe, '-lpthread'], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def build_abi_driver(folder, directory):
    """tests/<folder>/driver.cpp against the whole C ABI and the engine double -> the program's path (in `directory`)"""
    gxx = sanitizer_gxx()
    if not os.path.isdir(os.path.join(HIP_INCLUDE, 'hip')):  # (kns_engine.h names HIP types; nothing of HIP is linked)
        pytest.skip('needs the HIP headers')
    sources = sorted(glob.glob(os.path.join(CSRC, 'pv_api*.cpp')))
    assert len(sources) >= 2, sources
    sources += [os.path.join(ROOT, 'tests', 'abi_sanitizer', 'engine_stub.cpp'), os.path.join(ROOT, 'tests', folder, 'driver.cpp')]
    flags = ['-D__HIP_PLATFORM_AMD__', '-I' + HIP_INCLUDE, '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC,
             '-Wno-deprecated-declarations', '-Wno-unused-result']
    return _build(gxx, flags, sources, os.path.join(str(directory), folder + '_driver'))


def build_translation_unit(text, directory, flags=()):
    """one generated translation unit (a kernel emulator: shim + the kernels' own source + driver) -> the program's path"""
    gxx = sanitizer_gxx()
    source = os.path.join(str(directory), 'emu.cpp')
    with open(source, 'w') as f:
        f.write(text)
    return _build(gxx, list(flags), [source], os.path.join(str(directory), 'emu'))


def run(exe, *args, timeout=600):
    """the program in the environment as it is, but for the sanitizers' options and the engine double's switches (STUB_*), which belong to
    the drivers: they set and clear them themselves"""
    env = {k: v for k, v in os.environ.items() if not k.startswith('STUB_')}
    env.update(SANITIZER_OPTIONS)
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=env)
