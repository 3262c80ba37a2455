"""
Band profile (include/pv_koala_batch.h: pv_koala_batch_set_band_profile / get_band_profile, pv_koala_set_band_profile / get_band_profile)
without a GPU: the rule's exact properties on the recipe, the curve builders of koala_amd.bands, the Python-side argument checks (made before
any library is loaded), the symbols and their NULL checks, the C refusals and their messages through the host-only engine double
(tests/abi_band_profile/driver.cpp, a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer), and the gfx950 build of
the profile kernels.  tests/test_gpu_band_profile.py checks the samples on the GPU.
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
from band_profile_recipe import K, profiles, shaped
from conftest import ROOT, model_file
from koala_amd import bands

sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
SYMBOLS = ('pv_koala_batch_set_band_profile', 'pv_koala_batch_get_band_profile', 'pv_koala_set_band_profile', 'pv_koala_get_band_profile')
PV_STATUS_INVALID_ARGUMENT = 3
F32 = np.float32


def _masks(n=64, seed=1):
    """sigmoid outputs, the ends of the range among them"""
    m = np.random.default_rng(seed).random((n, K), dtype=F32)
    m[0, :4] = [0.0, 1.0, np.float32(2.0 ** -24), np.float32(1.0 - 2.0 ** -24)]
    return m


# ------------------------------------------------------------------------------------------------ the rule

def test_the_rule_and_its_exact_properties():
    m = _masks()
    zeros, ones = np.zeros(K, F32), np.ones(K, F32)
    for g in (F32(0), F32(0.25), F32(0.1), F32(1)):
        u = F32(1) - g
        m1 = (g + (u * m).astype(F32)).astype(F32)
        for row in m:
            assert np.array_equal(shaped(row, g, zeros, ones).view(np.uint32), (g + (u * row).astype(F32)).astype(F32).view(np.uint32))  # neutral
            assert np.array_equal(shaped(row, g, ones, ones), ones)  # floor = ceil = 1: a unity mask, the pure delay
            assert not shaped(row, g, zeros, zeros).any()  # ceil = 0: nothing comes out
        lo, hi = profiles(m.shape[0], seed=3)
        out = np.stack([shaped(m[i], g, lo[i], hi[i]) for i in range(m.shape[0])])
        assert out.dtype == F32 and (out >= lo).all() and (out <= hi).all()
        inside = (m1 >= lo) & (m1 <= hi)
        assert inside.any() and np.array_equal(out[inside], m1[inside])  # a clamp adds no rounding
        assert np.array_equal(out[m1 < lo], lo[m1 < lo]) and np.array_equal(out[m1 > hi], hi[m1 > hi])
        # the package's statement of the rule is the recipe's, bit for bit, for a batch and per-stream gains
        assert np.array_equal(bands.apply(m, g, lo, hi).view(np.uint32), out.view(np.uint32))
    gs = np.resize(np.array([0, 0.25, 1], F32), m.shape[0])
    want = np.stack([shaped(m[i], gs[i], lo[i], hi[i]) for i in range(m.shape[0])])
    assert np.array_equal(bands.apply(m, gs, lo, hi).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(bands.apply(m), m)
    # g = 0 gives m itself: 0 + 1 m
    assert np.array_equal(shaped(m[0], 0.0, zeros, ones).view(np.uint32), m[0].view(np.uint32))


# ------------------------------------------------------------------------------------------------ the curve builders

def test_curve_builders():
    f = np.arange(K) * bands.BIN_HZ
    assert bands.NUM_BINS == K and bands.BIN_HZ == 31.25
    lo0, hi0 = bands.neutral()
    assert not lo0.any() and (hi0 == 1).all() and lo0.dtype == hi0.dtype == F32
    for hz in (0.0, 50.0, 90.0, 300.0, 7990.0, 8000.0):
        for width in (0.0, 31.25, 62.5, 500.0):
            c = bands.highpass(hz, width)
            assert c.dtype == F32 and c.shape == (K,) and (c >= 0).all() and (c <= 1).all()
            assert (np.diff(c) >= 0).all()  # monotone
            assert (c[f < hz - width / 2] == 0).all() and (c[f >= hz + width / 2] == 1).all()
    hp = bands.highpass(90.0)
    assert hp[0] == 0 and hp[1] == 0 and hp[4] == 1  # nothing at DC and 31.25 Hz (50 / 60 Hz hum lies in the edge), everything from 125 Hz
    bp = bands.bandpass(300.0, 3400.0)
    assert bp.dtype == F32 and (bp >= 0).all() and (bp <= 1).all()
    peak = int(np.argmax(bp))
    assert (np.diff(bp[:peak + 1]) >= 0).all() and (np.diff(bp[peak:]) <= 0).all()  # up, then down
    assert (bp[f <= 300 - 31.25] == 0).all() and (bp[f >= 3400 + 31.25] == 0).all() and (bp[(f >= 350) & (f <= 3350)] == 1).all()
    fl = bands.depth_limit_db([(0, 6), (300, 18)])
    assert fl.dtype == F32 and (fl >= 0).all() and (fl <= 1).all() and (np.diff(fl) <= 0).all()  # deeper above: the floor falls
    assert fl[0] == F32(10.0 ** -0.3) and fl[-1] == F32(10.0 ** -0.9)
    assert np.allclose(bands.depth_limit_db([(0, 20)]), 0.1) and not bands.depth_limit_db([(0, np.inf)]).any()
    up = bands.depth_limit_db([(0, np.inf), (4000, 0), (8000 - 62.5, 0)])  # "leave 4-8 kHz alone"
    assert (np.diff(up) >= 0).all() and up[0] == 0 and up[-1] == 1
    # a floor and a ceiling built this way go together only where floor <= ceiling: the check says so
    with pytest.raises(ValueError):
        bands.check(fl, hp)
    lo, hi = bands.check(np.minimum(fl, hp), hp)
    assert (lo <= hi).all()
    for bad in (lambda: bands.highpass(-1), lambda: bands.highpass(9000), lambda: bands.highpass(100, -1), lambda: bands.bandpass(3400, 300),
                lambda: bands.bandpass(0, 9000), lambda: bands.depth_limit_db([]), lambda: bands.depth_limit_db([(300, 6), (0, 18)]),
                lambda: bands.depth_limit_db([(0, -3)]), lambda: bands.depth_limit_db([(0, float('nan'))])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ Python-side argument checks

def test_python_refuses_bad_profiles_before_any_library_is_loaded(tmp_path):
    missing = str(tmp_path / 'no_such_library.so')  # (loading it would raise another error: the argument checks come first)
    ok = np.ones(K, F32)
    for bad in ((ok, ok, ok), 'carry', (ok,), (np.ones(K - 1, F32), ok), (np.full(K, 1.5, F32), ok), (np.full(K, np.nan, F32), ok),
                (np.full(K, 0.5, F32), np.full(K, 0.25, F32)), (None, np.full(K, -0.1, F32)), (np.ones((3, K), F32), None)):
        with pytest.raises(koala_amd.KoalaInvalidArgumentError):
            koala_amd.create_batch('key', 2, 1, model_path=model_file('random', 1234), library_path=missing, band_profile=bad)
    lo, hi = bands.check(None, None, rows=3)
    assert lo.shape == hi.shape == (3, K) and not lo.any() and (hi == 1).all()
    lo, hi = bands.check(np.full(K, -0.0, F32), None)
    assert not np.signbit(lo).any()
    lo, hi = bands.check(np.full(K, 0.5, F32), None, rows=4)  # one curve for every listed stream
    assert lo.shape == (4, K) and lo.flags['C_CONTIGUOUS']


# ------------------------------------------------------------------------------------------------ the C ABI

def test_symbols_are_exported_and_declared(native_library):
    header = open(os.path.join(ROOT, 'include', 'pv_koala_batch.h')).read()
    for path in (native_library, koala_amd.developer_library_path()):
        lib = ctypes.CDLL(path)
        for sym in SYMBOLS:
            assert hasattr(lib, sym), (path, sym)
    for sym in SYMBOLS:
        assert re.search(r'PV_API pv_status_t %s\(' % sym, header), sym
    assert 'band_profile' not in open(os.path.join(ROOT, 'include', 'pv_koala.h')).read()  # the single-stream header stays the reference's


def test_null_objects_are_refused_without_a_gpu(native_library):
    lib = ctypes.CDLL(native_library)
    lib.pv_get_error_stack.argtypes = [ctypes.POINTER(ctypes.POINTER(ctypes.c_char_p)), ctypes.POINTER(ctypes.c_int32)]
    lib.pv_free_error_stack.argtypes = [ctypes.POINTER(ctypes.c_char_p)]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.pv_koala_batch_set_band_profile.argtypes = [vp, i32, vp, vp, vp]
    lib.pv_koala_batch_get_band_profile.argtypes = [vp, i32, vp, vp]
    lib.pv_koala_set_band_profile.argtypes = [vp, vp, vp]
    lib.pv_koala_get_band_profile.argtypes = [vp, vp, vp]
    curve = (ctypes.c_float * K)(*([0.5] * K))
    for call in (lambda: lib.pv_koala_batch_set_band_profile(None, 1, None, curve, curve), lambda: lib.pv_koala_batch_get_band_profile(None, 0, curve, curve),
                 lambda: lib.pv_koala_set_band_profile(None, curve, None), lambda: lib.pv_koala_get_band_profile(None, curve, curve)):
        assert call() == PV_STATUS_INVALID_ARGUMENT
        msgs, depth = ctypes.POINTER(ctypes.c_char_p)(), ctypes.c_int32()
        assert lib.pv_get_error_stack(ctypes.byref(msgs), ctypes.byref(depth)) == 0 and depth.value == 1 and b'NULL' in msgs[0]
        lib.pv_free_error_stack(msgs)
    assert list(curve) == [0.5] * K


def test_band_profile_entry_points_under_asan_and_ubsan(tmp_path):
    """table validation, revision handling, "a refused call changes nothing" and the two not-yet refusals, against the engine double"""
    run = sanitized_build.run(sanitized_build.build_abi_driver('abi_band_profile', tmp_path), model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])


# ------------------------------------------------------------------------------------------------ the kernels

@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_every_profile_kernel_form_builds_for_gfx950_without_spills(tmp_path):
    """synthesis_profile_kernel<kReport, kRecompute, kMaskH, kMaskIn, kResets>: the nine forms, each with and without the report; none
    spills, and each keeps the occupancy (waves per SIMD) of the kMinGain form of the same kernel."""
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
        form = re.search(r'(synthesis_kernel|synthesis_report_kernel|synthesis_profile_kernel)I((?:Lb[01]E)+)E', name)
        if form:
            bits = tuple(int(b) for b in re.findall(r'Lb([01])E', form.group(2)))
            info[(form.group(1), bits)] = {k: int(re.search(r'; %s: (\d+)' % k, body).group(1)) for k in ('ScratchSize', 'Occupancy', 'NumVgprs')}
    forms = [(1, 1, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (1, 1, 0, 1), (1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 0, 1), (0, 1, 1, 0)]
    assert sorted(k[1] for k in info if k[0] == 'synthesis_profile_kernel') == sorted((r,) + f for f in forms for r in (0, 1))
    for f in forms:
        for report in (0, 1):
            limited = info[('synthesis_report_kernel' if report else 'synthesis_kernel', f + (1,))]
            profiled = info[('synthesis_profile_kernel', (report,) + f)]
            print(f, 'report' if report else 'plain ', 'kMinGain', limited, 'kProfile', profiled)
            assert profiled['ScratchSize'] == 0 and profiled['Occupancy'] == limited['Occupancy'], (f, report, limited, profiled)
            if not f[2]:
                assert profiled['Occupancy'] >= 3 and profiled['NumVgprs'] <= 168, (f, report, profiled)
