"""
Comfort noise on the CPU (include/pv_koala_batch.h: COMFORT NOISE; DESIGN.md section 2, twelfth extension): koala_amd.comfort against the
recipe of the GPU suite (tests/comfort_recipe.py) and against literals, the variates' statistics, the calibration of `curve` through the
oracle's synthesis, and the C ABI through the host-only engine double.  Nothing here needs a GPU.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sanitized_build
from comfort_recipe import K, ONES, filled, hashed, noise
from conftest import ROOT, model_file
from koala_amd import comfort
from oracle import oracle

F32 = np.float32

# (seed, n, k, the hashed word): computed once by a C program from the header's five lines
LITERALS = [(0x0, 0x0, 0, 0x00000000), (0x1, 0x2, 3, 0xA536451F), (0xDEADBEEF, 0xFFFFFFFF, 256, 0x57D39303), (0x3039, 0x3E8, 17, 0xDD8C8318),
            (0x7, 0x1, 255, 0xB629449D)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_the_hash_is_pinned_by_literals():
    for seed, n, k, v in LITERALS:
        assert int(hashed(seed, n)[k]) == v
        z_re, z_im = comfort.variates(seed, n)
        assert z_re[k] == F32((F32(v & 0xFFFF) - F32(32767.5)) / F32(32768.0))
        assert z_im[k] == (0 if k in (0, 256) else F32((F32(v >> 16) - F32(32767.5)) / F32(32768.0)))


def test_the_package_states_the_recipe_bit_for_bit():
    rng = np.random.default_rng(1)
    for _ in range(20):
        seed, n = (int(v) for v in rng.integers(0, 2 ** 32, 2))
        spec = rng.standard_normal((K, 2)).astype(F32)
        spec[0, 1] = spec[256, 1] = 0
        mp, amp = rng.random(K, dtype=F32), (rng.random(K, dtype=F32) * F32(0.1)).astype(F32)
        z = comfort.variates(seed, n)
        for a, b in zip(z, noise(seed, n)):
            assert np.array_equal(bits(a), bits(b))
        assert np.array_equal(bits(comfort.apply(spec, mp, amp, seed, n)), bits(filled(spec, mp, amp, seed, n)))
    # arrays of seeds and counters: one row per stream
    seeds, ns = rng.integers(0, 2 ** 32, 4), rng.integers(0, 2 ** 32, 4)
    z_re, z_im = comfort.variates(seeds, ns)
    for b in range(4):
        assert np.array_equal(bits(z_re[b]), bits(noise(seeds[b], ns[b])[0])) and np.array_equal(bits(z_im[b]), bits(noise(seeds[b], ns[b])[1]))
    # m' = 1: Y is X; A = 0: Y is m' X
    x = rng.standard_normal((K, 2)).astype(F32)
    assert np.array_equal(comfort.apply(x, np.ones(K, F32), np.ones(K, F32), 5, 6), x)
    assert np.array_equal(comfort.apply(x, mp, np.zeros(K, F32), 5, 6), (mp[:, None] * x).astype(F32))


def test_the_variates_are_centred_and_uncorrelated():
    """N = 200 x 257 variates: the mean and the correlations of re with im, of bin k with k + 1 and of frame n with n + 1 each stay inside
    5 / sqrt(N) -- five standard errors of a correlation of N independent pairs, a bound from the count, not from a run"""
    frames = 200
    for seed in (0, 12345):
        z_re, z_im = comfort.variates(np.full(frames, seed), np.arange(frames))
        z_re, z_im = z_re.astype(np.float64), z_im[:, 1:256].astype(np.float64)
        N = frames * K
        bar = 5.0 / np.sqrt(N)
        sd = np.sqrt(1.0 / 3.0)
        corr = lambda a, b: float(np.mean(a * b)) / (sd * sd)
        figures = dict(mean_re=float(z_re.mean()) / sd, mean_im=float(z_im.mean()) / sd, re_im=corr(z_re[:, 1:256], z_im),
                       bins=corr(z_re[:, :-1], z_re[:, 1:]), frames=corr(z_re[:-1], z_re[1:]), bins_im=corr(z_im[:, :-1], z_im[:, 1:]),
                       frames_im=corr(z_im[:-1], z_im[1:]))
        print(seed, bar, figures)
        assert abs(z_re.var() / (sd * sd) - 1.0) < 0.02
        for name, v in figures.items():
            assert abs(v) < bar, (name, v, bar)


@pytest.mark.parametrize('shape', comfort.SHAPES)
def test_curve_is_calibrated_through_the_synthesis(shape):
    """curve(-60) with X = 0 and m' = 0 through oracle.synthesis for 200 frames: the RMS within 0.5 dB of -60 dBFS (the estimator's own
    standard error at that length is some hundredths of a dB; the rest is room for the int16 rounding at 33 LSB RMS)"""
    amp = comfort.curve(-60.0, shape)
    tail = np.zeros(256, F32)
    zero, none = np.zeros((K, 2), F32), np.zeros(K, F32)
    out = [oracle.synthesis(comfort.apply(zero, none, amp, 99, n), ONES, tail) for n in range(201)][1:]  # (the first frame has no overlap)
    x = np.concatenate(out).astype(np.float64) / 32768.0
    db = 10.0 * np.log10(np.mean(x * x))
    print(shape, 'RMS %.3f dBFS' % db)
    assert abs(db + 60.0) < 0.5
    assert amp.dtype == F32 and amp.shape == (K,) and (amp > 0).all()


def test_curve_and_check_refuse_what_the_library_refuses():
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            comfort.curve(bad)
    with pytest.raises(ValueError):
        comfort.curve(-60, 'brown')
    a = comfort.curve(-50.0, 'pink')
    assert np.array_equal(comfort.check(a, 3), np.broadcast_to(a, (3, K)))
    for v in (np.nan, -1e-30, np.inf):
        b = a.copy()
        b[17] = v
        with pytest.raises(ValueError):
            comfort.check(b)
    with pytest.raises(ValueError):
        comfort.check(np.zeros(256, F32))
    assert 20 * np.log10(comfort.curve(-40.0)[5] / comfort.curve(-60.0)[5]) == pytest.approx(20.0, abs=1e-4)


def test_abi_through_the_engine_double(tmp_path):
    """tests/abi_comfort/driver.cpp (with koala_amd/csrc/pv_comfort.cpp) against koala_amd/csrc/pv_api*.cpp and the engine double the other
    ABI tests use: a stand-alone program, built without a sanitizer; nothing is loaded into python"""
    gxx = shutil.which('g++')
    assert gxx, 'the ABI driver needs g++ (a missing toolchain is a failure here, not a skip: nothing else covers these entry points)'
    assert os.path.isdir(os.path.join(sanitized_build.HIP_INCLUDE, 'hip')), 'the ABI driver needs the HIP headers (kns_engine.h names HIP types)'
    csrc = sanitized_build.CSRC
    sources = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.startswith('pv_api') and f.endswith('.cpp'))
    sources += [os.path.join(ROOT, 'tests', 'abi_sanitizer', 'engine_stub.cpp'), os.path.join(ROOT, 'tests', 'abi_comfort', 'driver.cpp')]
    exe = os.path.join(str(tmp_path), 'abi_comfort_driver')
    flags = ['-std=c++17', '-O1', '-g', '-D__HIP_PLATFORM_AMD__', '-I' + sanitized_build.HIP_INCLUDE, '-I' + os.path.join(ROOT, 'include'), '-I' + csrc,
             '-Wno-deprecated-declarations', '-Wno-unused-result']
    build = subprocess.run([gxx] + flags + sources + ['-o', exe, '-lpthread'], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith('STUB_')}
    run = subprocess.run([exe, model_file('random', 1234)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
