"""
Batch handles at 12 and 24 kHz (include/pv_koala_batch.h: pv_koala_batch_init_rate; DESIGN.md section 2, third extension, generalised)
without a GPU: the general stage "up U, down D" of tests/rational_rate_recipe.py against the whole-number stages it generalises and against
a float64 restatement with no fixed order, the recipe against itself in other cuts and across a record, the refusals, the gfx950 build of
the new kernels of koala_amd/csrc/kns_resample.hip, and the constants through the C ABI under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/abi_rational_rate/driver.cpp).  tests/test_gpu_rational_rate.py checks the samples on the GPU.
"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import koala_amd
import rational_rate_recipe as rrr
import sample_rate_recipe as srr
from conftest import ROOT, model_file, synth_streams

sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
PAIRS = [(2, 3), (3, 2), (4, 3), (3, 4)]


def full_range(rows, n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, size=(rows, n)).astype(np.int16)


@pytest.mark.parametrize('R', [2, 3])
def test_general_stage_is_the_interpolator_and_the_decimator(R):
    g, hd, hi = srr.prototype(R)
    assert np.array_equal(rrr.table(R, R), hi) and np.array_equal(rrr.table(R, 1), hd)
    a = full_range(3, 6 * 37 * R, seed=R)  # (a length both stages take: a multiple of R)
    h_up, h_down = full_range(3, 48, seed=10 + R), full_range(3, 48 * R, seed=20 + R)
    assert rrr.hist_length(R, R) == 48 and rrr.hist_length(R, 1) == 48 * R
    assert np.array_equal(rrr.stage(h_up, a, R, 1, hi), srr.interpolate(h_up, a, R, hi))
    assert np.array_equal(rrr.stage(h_down, a, 1, R, hd), srr.decimate(h_down, a, R, hd))


@pytest.mark.parametrize('U,D', PAIRS)
def test_stage_is_within_one_lsb_of_a_float64_convolution(U, D):
    """zero-stuff, np.convolve with U g, every D-th sample, in double and in no fixed order.  At most 97 float32 fmas on values up to 2^15
    accumulate well under 0.5 LSB before the single rounding to int16, so the recipe is within 1 LSB of the unrounded double value."""
    K = max(U, D)
    g = srr.prototype(K)[0]
    Q = 200
    a = full_range(2, D * Q, seed=7 * U + D)
    got = rrr.stage(np.zeros((2, rrr.hist_length(K, U)), np.int16), a, U, D, rrr.table(K, U))
    assert got.shape == (2, U * Q)
    worst = 0.0
    for r in range(2):
        up = np.zeros(U * D * Q, np.float64)
        up[::U] = a[r]
        ref = np.clip(np.convolve(up, U * g)[:U * D * Q:D], -32768, 32767)
        worst = max(worst, float(np.abs(got[r].astype(np.float64) - ref).max()))
    print('(%d, %d): largest distance from the float64 convolution %.4f LSB' % (U, D, worst))
    assert worst <= 1.0


def test_constants_of_the_recipe_are_the_specs():
    assert [rrr.common_k(r) for r in rrr.RATES] == [4, 3]
    assert [rrr.frame_length(r) for r in rrr.RATES] == [192, 384] and [rrr.delay_sample(r) for r in rrr.RATES] == [240, 456]
    for rate, hists, tail in ((12000, (48, 64), 224), (24000, (72, 48), 240)):
        rec = rrr.Recipe(None, 1, 'fp32', rate)
        assert (rec.s_in.hist.shape[1], rec.s_out.hist.shape[1]) == hists and rec.rs_state().shape == (1, tail)
    # at K = 3 the prototype is the 48 kHz handle's, value for value
    assert np.array_equal(rrr.table(3, 1), srr.prototype(3)[1]) and np.array_equal(rrr.table(3, 3), srr.prototype(3)[2])


@pytest.mark.parametrize('rate', rrr.RATES)
def test_a_1_khz_tone_keeps_its_level_and_shows_the_stated_delay(rate):
    fl, N = rrr.frame_length(rate), 16 * rrr.frame_length(rate)
    x = np.round(8000.0 * np.sin(2 * np.pi * 1000.0 * np.arange(N) / rate)).astype(np.int16).reshape(1, N)
    z = rrr.Recipe(None, 1, 'fp32', rate).process(x)[0].astype(np.float64)
    d = rrr.delay_sample(rate)
    xs = x[0].astype(np.float64)
    dist = [float(np.sum((z - np.concatenate([np.zeros(k), xs[:N - k]])) ** 2)) for k in range(d - 40, d + 41)]
    assert int(np.argmin(dist)) == 40, (rate, int(np.argmin(dist)) + d - 40)
    steady = slice(d + 2 * fl, N)
    level = 20 * np.log10(np.sqrt(np.mean(z[steady] ** 2)) / np.sqrt(np.mean(xs[2 * fl:N - d] ** 2)))
    print('%d Hz: delay %d samples, level %+.4f dB' % (rate, d, level))
    assert abs(level) <= 0.1 and not z[:fl].any()


def test_python_refuses_other_rates_and_takes_the_two_new_ones(random_model, monkeypatch):
    for bad in (44100, 96000, 16001, 0):
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='sample_rate'):
            koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, sample_rate=bad)
    # create_batch's own check takes 12 000 and 24 000: the refusal, if any, comes from further on (the library: a GPU is needed there)
    import koala_amd._batch as kb

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(kb, 'load_library', stop)
    for rate in rrr.RATES:
        with pytest.raises(Reached):
            koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, sample_rate=rate)
    with pytest.raises(koala_amd.KoalaInvalidArgumentError):
        koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, sample_rate=44100)


@pytest.mark.parametrize('rate', rrr.RATES)
def test_recipe_in_calls_of_1_2_and_5_frames_is_the_recipe_in_one_call(random_model, rate):
    n, T, fl = 2, 8, rrr.frame_length(rate)
    x = np.ascontiguousarray(synth_streams(n, T * fl // 256 + 1, seed=5)[:, :T * fl])  # (any int16 signal serves: samples at `rate`)
    one = rrr.Recipe(random_model, n, 'fp32', rate).process(x)
    for cuts in ([1, 2, 5], [5, 2, 1], [1] * T):
        r, out, t0 = rrr.Recipe(random_model, n, 'fp32', rate), [], 0
        for c in cuts:
            out.append(r.process(np.ascontiguousarray(x[:, t0 * fl:(t0 + c) * fl])))
            t0 += c
        assert t0 == T and np.array_equal(np.concatenate(out, axis=1), one), (rate, cuts)
    # per-frame resets: the call cut at its frames == fresh streams from there
    reset = np.zeros((n, T), np.uint8)
    reset[1, 3] = 1
    got = rrr.Recipe(random_model, n, 'fp32', rate).process_resets(x, reset)
    fresh = rrr.Recipe(random_model, n, 'fp32', rate).process(np.ascontiguousarray(x[:, 3 * fl:]))
    assert np.array_equal(got[0], one[0]) and np.array_equal(got[1, :3 * fl], one[1, :3 * fl]) and np.array_equal(got[1, 3 * fl:], fresh[1])


@pytest.mark.parametrize('rate', rrr.RATES)
def test_a_record_taken_mid_stream_continues_in_a_fresh_recipe(rate):
    n, T, fl = 3, 6, rrr.frame_length(rate)
    x = full_range(n, T * fl, seed=rate)
    a = rrr.Recipe(None, n, 'fp32', rate)
    one = rrr.Recipe(None, n, 'fp32', rate).process(x)
    head = a.process(np.ascontiguousarray(x[:, :2 * fl]))
    blob, inner = a.rs_state(), a.o.prev.copy()  # (the stages' part of the record, and the inner engine's: here one frame of samples)
    assert blob.shape[1] == {12000: 224, 24000: 240}[rate] and blob.any()
    b = rrr.Recipe(None, n, 'fp32', rate)
    b.set_rs_state(blob)
    b.o.prev = inner
    assert np.array_equal(b.rs_state(), blob)
    tail = b.process(np.ascontiguousarray(x[:, 2 * fl:]))
    assert np.array_equal(np.concatenate([head, tail], axis=1), one)
    # and without the stages' part it does not
    c = rrr.Recipe(None, n, 'fp32', rate)
    c.o.prev = inner
    assert not np.array_equal(c.process(np.ascontiguousarray(x[:, 2 * fl:])), tail)


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
    gxx = shutil.which('g++')
    if not gxx or not os.path.isdir('/opt/rocm/include/hip'):
        pytest.skip('needs g++ and the HIP headers')
    exe = str(tmp_path / 'rational_rate_driver')
    csrc = os.path.join(ROOT, 'koala_amd', 'csrc')
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include', '-I' + os.path.join(ROOT, 'include'), '-I' + csrc,
           '-Wno-deprecated-declarations', '-Wno-unused-result',
           os.path.join(csrc, 'pv_api.cpp'), os.path.join(csrc, 'pv_api_packets.cpp'),
           os.path.join(ROOT, 'tests', 'abi_sanitizer', 'engine_stub.cpp'), os.path.join(ROOT, 'tests', 'abi_rational_rate', 'packets_stub.cpp'),
           os.path.join(ROOT, 'tests', 'abi_rational_rate', 'driver.cpp'), '-o', exe, '-lpthread']
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and 'sanitizer' in build.stderr.lower() and 'cannot find' in build.stderr.lower():
        pytest.skip('sanitizer runtimes not installed: ' + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    for k in ('STUB_GPUS', 'STUB_OOM', 'STUB_FAIL_PROCESS', 'STUB_THROW', 'STUB_FRONT_TAPS', 'LD_PRELOAD'):
        env.pop(k, None)
    run = subprocess.run([exe, model_file('random', 1234)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
