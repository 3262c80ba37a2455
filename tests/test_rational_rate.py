"""
The general stage "up U, down D" of the sample-rate handles (third extension, generalised) without a GPU: the stage of
tests/sample_rate_recipe.py against the interpolator and the decimator it generalises, restated here on their own, and against a float64
restatement with no fixed order; the gfx950 build of the rational kernels of koala_amd/csrc/kns_resample.hip; and the constants of 12 and
24 kHz through the C ABI under AddressSanitizer + UndefinedBehaviorSanitizer (tests/abi_rational_rate/driver.cpp).
tests/test_sample_rate.py holds the recipe's own tests, tests/test_gpu_rational_rate.py checks the samples on the GPU.
"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sample_rate_recipe as srr
import sanitized_build
from conftest import ROOT, model_file

sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
PAIRS = [(2, 3), (3, 2), (4, 3), (3, 4)]


def full_range(rows, n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, size=(rows, n)).astype(np.int16)


def interpolate(hist, a, R, hi):
    """the interpolator as DESIGN.md states it on its own: hist int16 [n, 48] (the samples in front of a), a int16 [n, N] -> int16 [n, R N]"""
    n, N = a.shape
    x = np.concatenate([hist, a], axis=1).astype(np.float32)
    out = np.empty((n, N * R), np.int16)
    for p in range(R):
        acc = np.zeros((n, N), np.float32)
        j = 0
        while p + R * j <= 48 * R:
            acc = srr.fma32(np.full((n, N), hi[p + R * j], np.float32), x[:, 48 - j:48 - j + N], acc)
            j += 1
        out[:, p::R] = srr.to_pcm(acc)
    return out


def decimate(hist, a, R, hd):
    """the decimator as DESIGN.md states it on its own: hist int16 [n, 48 R], a int16 [n, R N] -> int16 [n, N]"""
    n, M = a.shape
    N, H = M // R, 48 * R
    x = np.concatenate([hist, a], axis=1).astype(np.float32)
    acc = np.zeros((n, N), np.float32)
    for i in range(H + 1):
        acc = srr.fma32(np.full((n, N), hd[i], np.float32), x[:, H - i:H - i + M:R], acc)
    return srr.to_pcm(acc)


@pytest.mark.parametrize('R', [2, 3])
def test_general_stage_is_the_interpolator_and_the_decimator(R):
    g = srr.prototype(R)
    hd, hi = g.astype(np.float32), (R * g).astype(np.float32)
    assert np.array_equal(srr.table(R, R), hi) and np.array_equal(srr.table(R, 1), hd)
    a = full_range(3, 6 * 37 * R, seed=R)  # (a length both stages take: a multiple of R)
    h_up, h_down = full_range(3, 48, seed=10 + R), full_range(3, 48 * R, seed=20 + R)
    assert srr.hist_length(R, R) == 48 and srr.hist_length(R, 1) == 48 * R
    assert np.array_equal(srr.stage(h_up, a, R, 1, hi), interpolate(h_up, a, R, hi))
    assert np.array_equal(srr.stage(h_down, a, 1, R, hd), decimate(h_down, a, R, hd))


@pytest.mark.parametrize('U,D', PAIRS + [(2, 1), (1, 2), (3, 1), (1, 3)])
def test_stage_is_within_one_lsb_of_a_float64_convolution(U, D):
    """zero-stuff, np.convolve with U g, every D-th sample, in double and in no fixed order.  At most 97 float32 fmas on values up to 2^15
    accumulate well under 0.5 LSB before the single rounding to int16, so the recipe is within 1 LSB of the unrounded double value."""
    K = max(U, D)
    g = srr.prototype(K)
    Q = 200
    a = full_range(2, D * Q, seed=7 * U + D)
    got = srr.stage(np.zeros((2, srr.hist_length(K, U)), np.int16), a, U, D, srr.table(K, U))
    assert got.shape == (2, U * Q)
    worst = 0.0
    for r in range(2):
        up = np.zeros(U * D * Q, np.float64)
        up[::U] = a[r]
        ref = np.clip(np.convolve(up, U * g)[:U * D * Q:D], -32768, 32767)
        worst = max(worst, float(np.abs(got[r].astype(np.float64) - ref).max()))
    print('(%d, %d): largest distance from the float64 convolution %.4f LSB' % (U, D, worst))
    assert worst <= 1.0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_rational_kernels_build_for_gfx950_without_scratch_or_spills(tmp_path):
    import isa_scan
    src = 'kns_resample.hip'
    out = tmp_path / (src + '.s')
    mk = open(os.path.join(ROOT, 'koala_amd', 'Makefile')).read()
    cxx = re.search(r'^CXXFLAGS\s*=\s*(.*)$', mk, re.M).group(1).split()
    subprocess.check_call([HIPCC, '--offload-arch=gfx950'] + [f for f in cxx if f != '-fPIC'] +
                          ['-S', '--cuda-device-only', '-x', 'hip', os.path.join(ROOT, 'koala_amd', 'csrc', src), '-o', str(out)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    assert isa_scan.scan(text) == []
    info = {}
    for name, body in re.findall(r'\.set (\S+)\.has_indirect_call, \d+\n[^\n]*\n; Kernel info:\n((?:;[^\n]*\n)*)', text):
        info[name] = {k: int(re.search(r'; %s: (\d+)' % k, body).group(1)) for k in ('ScratchSize', 'NumVgprs', 'Occupancy')}
    meta = re.findall(r'\.name:\s+(\S+)\n(?:(?!\.name:).*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:(?!\.name:).*\n)*?\s+\.vgpr_spill_count:\s+(\d+)', text)
    spills = {name: (int(s), int(v)) for name, s, v in meta}
    # four (U, D) pairs, each with and without the reset arm
    want = ['resample_kernelILi%dELi%dELb%dEEEvNS_12ResampleArgsE' % (U, D, r) for U, D in PAIRS for r in (0, 1)]
    kernels = sorted(k for k in info if 'resample_kernel' in k and any(w in k for w in want))
    assert len(kernels) == 8 and all(any(w in k for k in kernels) for w in want), kernels
    for k in kernels:
        print(k, info[k], 'spills (sgpr, vgpr):', spills.get(k))
        assert info[k]['ScratchSize'] == 0, (k, info[k])
        assert spills[k] == (0, 0), (k, spills[k])
    # the tap loops are straight-line code whose taps are scalar loads of the argument segment: one fma per tap, no vector-memory load
    # beyond the staging of one chunk
    for U, D in PAIRS:
        body = text.split('resample_kernelILi%dELi%dELb0EEEvNS_12ResampleArgsE:' % (U, D))[1].split('s_endpgm')[0]
        L = 48 * max(U, D) + 1
        assert len(re.findall(r'\bv_fmac?_f32', body)) >= L and len(re.findall(r'\bs_load_dword', body)) >= 10, (U, D)
        assert len(re.findall(r'\b(global|flat|buffer)_load', body)) <= 16, (U, D)


def test_constants_through_the_c_abi_under_asan_and_ubsan(tmp_path):
    run = sanitized_build.run(sanitized_build.build_abi_driver('abi_rational_rate', tmp_path), model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
