"""
Per-stream attenuation limit (include/pv_koala_batch.h: pv_koala_batch_set_min_gain / get_min_gain, pv_koala_set_min_gain / get_min_gain)
without a GPU: the symbols and their NULL checks, the C-ABI shim's new entry points under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/abi_min_gain/driver.cpp with the engine double of tests/abi_sanitizer), the gfx950 build of every synthesis kernel form, and the
Python dB -> gain conversion.  tests/test_gpu_min_gain.py checks the samples on the GPU.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import koala_amd
import sanitized_build
from conftest import ROOT, model_file

sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
SYMBOLS = ('pv_koala_batch_set_min_gain', 'pv_koala_batch_get_min_gain', 'pv_koala_set_min_gain', 'pv_koala_get_min_gain')
PV_STATUS_INVALID_ARGUMENT = 3


def test_symbols_are_exported_and_declared(native_library):
    header = open(os.path.join(ROOT, 'include', 'pv_koala_batch.h')).read()
    for path in (native_library, koala_amd.developer_library_path()):
        lib = ctypes.CDLL(path)
        for sym in SYMBOLS:
            assert hasattr(lib, sym), (path, sym)
    for sym in SYMBOLS:
        assert re.search(r'PV_API pv_status_t %s\(' % sym, header), sym
    # the single-stream header stays the reference's
    assert 'min_gain' not in open(os.path.join(ROOT, 'include', 'pv_koala.h')).read()


def _stack(lib):
    msgs, depth = ctypes.POINTER(ctypes.c_char_p)(), ctypes.c_int32()
    status = lib.pv_get_error_stack(ctypes.byref(msgs), ctypes.byref(depth))
    if depth.value == 0:  # (nothing pending: PV_STATUS_INVALID_STATE and nothing to free)
        return []
    assert status == 0
    out = [msgs[i].decode() for i in range(depth.value)]
    lib.pv_free_error_stack(msgs)
    return out


def test_null_arguments_are_refused_without_a_gpu(native_library):
    """(everything that needs a handle -- ranges, NaN, duplicate slots, "a refused call changes nothing" -- runs against the engine double
    in test_min_gain_entry_points_under_asan_and_ubsan)"""
    lib = ctypes.CDLL(native_library)
    lib.pv_get_error_stack.argtypes = [ctypes.POINTER(ctypes.POINTER(ctypes.c_char_p)), ctypes.POINTER(ctypes.c_int32)]
    lib.pv_free_error_stack.argtypes = [ctypes.POINTER(ctypes.c_char_p)]
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    lib.pv_koala_batch_set_min_gain.argtypes = [vp, i32, vp, vp]
    lib.pv_koala_batch_get_min_gain.argtypes = [vp, vp]
    lib.pv_koala_set_min_gain.argtypes = [vp, f32]
    lib.pv_koala_get_min_gain.argtypes = [vp, vp]
    gains = (ctypes.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    one = ctypes.c_float(-7.0)
    calls = [lambda: lib.pv_koala_batch_set_min_gain(None, 4, None, gains),
             lambda: lib.pv_koala_batch_set_min_gain(None, 4, None, None),
             lambda: lib.pv_koala_batch_get_min_gain(None, gains),
             lambda: lib.pv_koala_batch_get_min_gain(None, None),
             lambda: lib.pv_koala_set_min_gain(None, 0.5),
             lambda: lib.pv_koala_get_min_gain(None, ctypes.byref(one)),
             lambda: lib.pv_koala_get_min_gain(None, None)]
    for call in calls:
        assert call() == PV_STATUS_INVALID_ARGUMENT
        msgs = _stack(lib)
        assert len(msgs) == 1 and 'NULL' in msgs[0], msgs
        assert _stack(lib) == []  # drained
    assert one.value == -7.0 and list(gains) == [0.5] * 4


def test_min_gain_entry_points_under_asan_and_ubsan(tmp_path):
    run = sanitized_build.run(sanitized_build.build_abi_driver('abi_min_gain', tmp_path), model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_every_synthesis_kernel_form_builds_for_gfx950_without_spills(tmp_path):
    """synthesis_kernel<kRecompute, kMaskH, kMaskIn, kResets, kMinGain>: the nine forms the engine launches, each with and without the
    minimum gain; none spills, and a kMinGain form keeps the occupancy (waves per SIMD) of its plain counterpart."""
    import isa_scan
    src = 'kns_stft.hip'
    out = tmp_path / (src + '.s')
    mk = open(os.path.join(ROOT, 'koala_amd', 'Makefile')).read()
    cxx = re.search(r'^CXXFLAGS\s*=\s*(.*)$', mk, re.M).group(1).split()
    m = re.search(r'^FLAGS_%s\s*=\s*(.*)$' % src.split('.')[0], mk, re.M)
    flags = [f for f in cxx if f not in ('-fPIC',)] + (m.group(1).split() if m else [])
    subprocess.check_call([HIPCC, '--offload-arch=gfx950'] + flags +
                          ['-S', '--cuda-device-only', '-x', 'hip', os.path.join(ROOT, 'koala_amd', 'csrc', src), '-o', str(out)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    assert isa_scan.scan(text) == []
    info = {}
    for name, body in re.findall(r'\.set (\S+)\.has_indirect_call, \d+\n[^\n]*\n; Kernel info:\n((?:;[^\n]*\n)*)', text):
        form = re.search(r'synthesis_kernelI((?:Lb[01]E)+)E', name)
        if form:
            bits = tuple(int(b) for b in re.findall(r'Lb([01])E', form.group(1)))
            info[bits] = {k: int(re.search(r'; %s: (\d+)' % k, body).group(1)) for k in ('ScratchSize', 'Occupancy', 'NumVgprs')}
    forms = [(1, 1, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (1, 1, 0, 1), (1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 0, 1), (0, 1, 1, 0)]
    assert sorted(info) == sorted(f + (g,) for f in forms for g in (0, 1)), sorted(info)
    for f in forms:
        plain, limited = info[f + (0,)], info[f + (1,)]
        print(f, 'plain', plain, 'kMinGain', limited)
        assert plain['ScratchSize'] == 0 and limited['ScratchSize'] == 0, (f, plain, limited)
        assert limited['Occupancy'] == plain['Occupancy'], (f, plain, limited)
        if not f[2]:  # (the one-frame form with the mask head inside is one workgroup of eight waves per CU by its launch bounds)
            assert plain['Occupancy'] >= 3 and limited['NumVgprs'] <= 168, (f, plain, limited)


def test_attenuation_limit_in_db_becomes_a_gain():
    f = koala_amd.attenuation_limit_to_gain
    assert f(None) == 0.0 and f(float('inf')) == 0.0 and f(0) == 1.0 and f(0.0).dtype == np.float32
    for db in (3, 6.0, 12, 20, 40.5, 1e-3, 200.0):
        assert f(db) == np.float32(10.0 ** (-float(db) / 20.0)), db
    assert f(20) == np.float32(0.1) and f(12) == np.float32(0.251188643150958)
    a = f([6, np.inf, 0, 20.0])
    assert a.dtype == np.float32 and a.shape == (4,)
    assert np.array_equal(a, np.array([10.0 ** -0.3, 0.0, 1.0, 0.1], np.float64).astype(np.float32))
    assert f(np.zeros((2, 3))).shape == (2, 3)
    assert ((f(np.linspace(0, 150, 301)) >= 0) & (f(np.linspace(0, 150, 301)) <= 1)).all()
    for bad in (-1, -1e-9, float('nan'), float('-inf'), [6, -3], [np.nan, 6]):
        with pytest.raises(ValueError):
            f(bad)
