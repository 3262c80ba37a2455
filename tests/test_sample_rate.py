"""
Batch handles at 8, 12, 24, 32 and 48 kHz (include/pv_koala_batch.h: pv_koala_batch_init_rate; DESIGN.md section 2, third extension) without a
GPU: the prototype low-pass, the numpy recipe (tests/sample_rate_recipe.py) against its pinned constants and against itself -- chunkings,
level, delay, a record -- the gfx950 build of koala_amd/csrc/kns_resample.hip, the new symbols, and the C-ABI shim's new entry points under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/abi_sample_rate/driver.cpp with the engine double of tests/abi_sanitizer), and the
stage kernel's own source on the CPU under the same two sanitizers (tests/highband_emulation, tests/high_band_emulator.py).
tests/test_rational_rate.py holds the general stage against the interpolator, the decimator and a float64 convolution;
tests/test_gpu_sample_rate.py and tests/test_gpu_rational_rate.py check the samples on the GPU.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import high_band_emulator
import koala_amd
import sample_rate_recipe as srr
import sanitized_build
from conftest import ROOT, model_file, synth_streams

sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
SYMBOLS = ('pv_koala_batch_init_rate', 'pv_koala_batch_sample_rate', 'pv_koala_batch_frame_length')
# koala_amd/csrc/kns_kernels.h's static_asserts, as literals: frame length, delay_sample, record tail, (in-stage, out-stage) history
FRAME = {8000: 128, 12000: 192, 24000: 384, 32000: 512, 48000: 768}
DELAY = {8000: 176, 12000: 240, 24000: 456, 32000: 608, 48000: 912}
TAIL = {8000: 288, 12000: 224, 24000: 240, 32000: 288, 48000: 384}
HISTS = {8000: (48, 96), 12000: (48, 64), 24000: (72, 48), 32000: (96, 48), 48000: (144, 48)}


def test_fma32_is_the_single_rounding_for_operands_of_any_sign():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(600).astype(np.float32)
    b = (rng.standard_normal(600) * 3e4).astype(np.float32)
    c = (rng.standard_normal(600) * 1e4).astype(np.float32)
    c[:150] = (-a[:150].astype(np.float64) * b[:150]).astype(np.float32)  # (cancellation)
    got = srr.fma32(a, b, c)
    for i in range(a.size):
        v = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(v))
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        best = min(cands, key=lambda q: (abs(Fraction(float(q)) - v), int(np.float32(q).view(np.int32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i])


@pytest.mark.parametrize('R', [2, 3])
def test_prototype_passes_the_low_band_and_stops_its_images(R):
    g, hd, hi = srr.prototype(R), srr.table(R, 1), srr.table(R, R)
    assert len(g) == 48 * R + 1 and abs(g.sum() - 1.0) < 1e-12 and np.allclose(g, g[::-1], rtol=0, atol=1e-15)
    assert np.array_equal(hd, g.astype(np.float32)) and np.array_equal(hi, (R * g).astype(np.float32))
    nyq = 0.5 / R  # the low rate's Nyquist frequency, in cycles per high-rate sample
    i = np.arange(len(g))
    for name, taps in (('double', g), ('hd', hd.astype(np.float64)), ('hi / R', hi.astype(np.float64) / R)):
        resp = lambda f: 20 * np.log10(np.abs(np.exp(-2j * np.pi * np.outer(f, i)) @ taps) + 1e-300)
        pb = resp(np.linspace(0, 0.8 * nyq, 801))
        sb = resp(np.linspace(1.1 * nyq, 0.5, 1601))
        print('R = %d %s: pass band %+.4f .. %+.4f dB, stop band max %.1f dB' % (R, name, pb.min(), pb.max(), sb.max()))
        assert np.abs(pb).max() <= 0.1 and sb.max() <= -80.0


def test_constants_of_the_recipe_are_the_specs():
    assert srr.RATES == tuple(FRAME) and [srr.frame_length(r) for r in srr.RATES] == list(FRAME.values())
    assert [srr.delay_sample(r) for r in srr.RATES] == list(DELAY.values()) and [srr.record_tail(r) for r in srr.RATES] == list(TAIL.values())
    assert [max(srr.STAGES[r][0]) for r in (12000, 24000)] == [4, 3]
    for rate, hists in HISTS.items():
        rec = srr.Recipe(None, 1, 'fp32', rate)
        assert (rec.s_in.hist.shape[1], rec.s_out.hist.shape[1]) == hists and rec.rs_state().shape == (1, TAIL[rate])
        assert srr.STAGES[rate][1] == srr.STAGES[rate][0][::-1]
    # the tables are the prototype of K times U, rounded once
    assert np.array_equal(srr.table(3, 1), srr.prototype(3).astype(np.float32))
    assert np.array_equal(srr.table(3, 3), (3 * srr.prototype(3)).astype(np.float32))


@pytest.mark.parametrize('rate', srr.RATES)
def test_recipe_in_any_chunking_is_the_recipe_in_one_shot(random_model, rate):
    """12 frames in the cuts 8, 32 and 48 kHz have had, 8 frames in those of 12 and 24 kHz (calls of 1, 2 and 5 frames)"""
    for T, at, cutss in ((12, 7, ([1] * 12, [5, 1, 3, 2, 1], [11, 1])), (8, 3, ([1, 2, 5], [5, 2, 1], [1] * 8))):
        n, fl = 2, srr.frame_length(rate)
        x = np.ascontiguousarray(synth_streams(n, T * fl // 256 + 1, seed=5)[:, :T * fl])  # (any int16 signal serves: samples at `rate`)
        one = srr.Recipe(random_model, n, 'fp32', rate).process(x)
        for cuts in cutss:
            r, out, t0 = srr.Recipe(random_model, n, 'fp32', rate), [], 0
            for c in cuts:
                out.append(r.process(np.ascontiguousarray(x[:, t0 * fl:(t0 + c) * fl])))
                t0 += c
            assert t0 == T and np.array_equal(np.concatenate(out, axis=1), one), (rate, cuts)
        # per-frame resets: the call cut at its frames == fresh streams from there
        reset = np.zeros((n, T), np.uint8)
        reset[1, at] = 1
        got = srr.Recipe(random_model, n, 'fp32', rate).process_resets(x, reset)
        fresh = srr.Recipe(random_model, n, 'fp32', rate).process(np.ascontiguousarray(x[:, at * fl:]))
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1, :at * fl], one[1, :at * fl])
        assert np.array_equal(got[1, at * fl:], fresh[1])


@pytest.mark.parametrize('rate', srr.RATES)
def test_a_1_khz_tone_keeps_its_level_and_shows_the_stated_delay(rate):
    fl, N = srr.frame_length(rate), 16 * srr.frame_length(rate)
    x = np.round(8000.0 * np.sin(2 * np.pi * 1000.0 * np.arange(N) / rate)).astype(np.int16).reshape(1, N)
    r = srr.Recipe(None, 1, 'fp32', rate)
    y = r.s_out.run(r.s_in.run(x))[0].astype(np.float64)  # both stages, without the engine's frame
    d = srr.delay_sample(rate)
    want = d - fl
    assert d == DELAY[rate] and want == HISTS[rate][0]
    xs = x[0].astype(np.float64)
    # the distance between y and x delayed by k (zeros in front: the tone starts at sample 0, so one lag fits its onset as well)
    dist = [float(np.sum((y - np.concatenate([np.zeros(k), xs[:N - k]])) ** 2)) for k in range(2 * want + 1)]
    assert int(np.argmin(dist)) == want, (rate, int(np.argmin(dist)))
    steady = slice(want + 2 * fl, N)
    level = 20 * np.log10(np.sqrt(np.mean(y[steady] ** 2)) / np.sqrt(np.mean(xs[2 * fl:N - want] ** 2)))
    err = np.abs(y[steady] - xs[2 * fl:N - want]).max()
    print('%d Hz: delay %d samples, level %+.4f dB, max |y[n] - x[n - delay]| = %.1f of 8000' % (rate, want, level, err))
    assert abs(level) <= 0.1
    # and through the whole recipe with the engine as a pure delay: delay_sample, among the lags 40 either side of it
    z = srr.Recipe(None, 1, 'fp32', rate).process(x)[0].astype(np.float64)
    assert np.array_equal(z[d:], y[want:N - fl]) and not z[:fl].any()
    dist = [float(np.sum((z - np.concatenate([np.zeros(k), xs[:N - k]])) ** 2)) for k in range(d - 40, d + 41)]
    assert int(np.argmin(dist)) == 40, (rate, int(np.argmin(dist)) + d - 40)
    steady = slice(d + 2 * fl, N)
    level = 20 * np.log10(np.sqrt(np.mean(z[steady] ** 2)) / np.sqrt(np.mean(xs[2 * fl:N - d] ** 2)))
    print('%d Hz: delay %d samples, level %+.4f dB' % (rate, d, level))
    assert abs(level) <= 0.1


@pytest.mark.parametrize('rate', srr.RATES)
def test_a_record_taken_mid_stream_continues_in_a_fresh_recipe(rate):
    n, T, fl = 3, 6, srr.frame_length(rate)
    x = np.random.default_rng(rate).integers(-32768, 32768, size=(n, T * fl)).astype(np.int16)
    a = srr.Recipe(None, n, 'fp32', rate)
    one = srr.Recipe(None, n, 'fp32', rate).process(x)
    head = a.process(np.ascontiguousarray(x[:, :2 * fl]))
    blob, inner = a.rs_state(), a.o.prev.copy()  # (the stages' part of the record, and the inner engine's: here one frame of samples)
    assert blob.shape[1] == TAIL[rate] and blob.any()
    b = srr.Recipe(None, n, 'fp32', rate)
    b.set_rs_state(blob)
    b.o.prev = inner
    assert np.array_equal(b.rs_state(), blob)
    tail = b.process(np.ascontiguousarray(x[:, 2 * fl:]))
    assert np.array_equal(np.concatenate([head, tail], axis=1), one)
    # and without the stages' part it does not
    c = srr.Recipe(None, n, 'fp32', rate)
    c.o.prev = inner
    assert not np.array_equal(c.process(np.ascontiguousarray(x[:, 2 * fl:])), tail)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_resample_kernels_build_for_gfx950_without_scratch_or_spills(tmp_path):
    import isa_scan
    src = 'kns_resample.hip'
    out = tmp_path / (src + '.s')
    mk = open(os.path.join(ROOT, 'koala_amd', 'Makefile')).read()
    assert 'csrc/' + src in mk and 'obj/kns_resample.o' in mk
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
    kernels = [k for k in info if 'resample_' in k]
    # interpolator (R, 1) and decimator (1, R), R = 2 and 3, with and without the reset arm; the reset and the record kernels
    whole = ['resample_kernelILi%dELi%dELb%dEEEvNS_12ResampleArgsE' % (U, D, r) for U, D in ((2, 1), (3, 1), (1, 2), (1, 3)) for r in (0, 1)]
    assert all(len([k for k in kernels if w in k]) == 1 for w in whole), kernels
    assert any('resample_reset_kernel' in k for k in kernels) and any('resample_state_kernel' in k for k in kernels)
    for k in kernels:
        print(k, info[k], 'spills (sgpr, vgpr):', spills.get(k))
        assert info[k]['ScratchSize'] == 0, (k, info[k])
        assert spills[k] == (0, 0), (k, spills[k])
    # the tap loops are straight-line code whose taps are scalar loads of the argument segment: no vector-memory load of a tap
    body = text.split('resample_kernelILi1ELi3ELb0EEEvNS_12ResampleArgsE:')[1].split('s_endpgm')[0]
    assert len(re.findall(r'\bv_fmac?_f32', body)) >= 145 and len(re.findall(r'\bs_load_dword', body)) >= 10
    assert len(re.findall(r'\b(global|flat|buffer)_load', body)) <= 16, 'vector-memory loads beyond the staging of one chunk'


def test_symbols_are_exported_and_declared(native_library):
    header = open(os.path.join(ROOT, 'include', 'pv_koala_batch.h')).read()
    for path in (native_library, koala_amd.developer_library_path()):
        lib = ctypes.CDLL(path)
        for sym in SYMBOLS:
            assert hasattr(lib, sym), (path, sym)
    for sym in SYMBOLS:
        assert re.search(r'PV_API pv_status_t %s\(' % sym, header), sym
    # the single-stream header stays the reference's
    assert 'sample_rate' not in open(os.path.join(ROOT, 'include', 'pv_koala.h')).read()


def test_python_refuses_other_rates_and_takes_the_five(random_model, monkeypatch):
    for bad in (44100, 96000, 16001, 0):
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='sample_rate'):
            koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, sample_rate=bad)
    # create_batch's own check takes the five rates: the refusal, if any, comes from further on (the library: a GPU is needed there)
    import koala_amd._batch as kb

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(kb, 'load_library', stop)
    for rate in srr.RATES:
        with pytest.raises(Reached):
            koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, sample_rate=rate)
    with pytest.raises(koala_amd.KoalaInvalidArgumentError):
        koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, sample_rate=44100)


def test_sample_rate_entry_points_under_asan_and_ubsan(tmp_path):
    run = sanitized_build.run(sanitized_build.build_abi_driver('abi_sample_rate', tmp_path), model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])


@pytest.mark.parametrize('rate,k', high_band_emulator.STAGE_CASES)
def test_the_stage_kernels_own_source_on_the_cpu_equals_the_recipe_under_asan_and_ubsan(rate, k, tmp_path_factory, tmp_path):
    """resample_kernel<U, D, kResets> of both stages of all five rates, 256 OS threads a workgroup, B = 3, calls of 1, 1, 3, 2, 16 frames,
    rows, flags and both copies of the state heap allocations of exactly their size: samples and state == sample_rate_recipe.Stage's after
    every call.  Per-frame flags in the 3-frame call (frame 0 and the last) and in the 16-frame call (frame 0; adjacent frames; the last);
    the reset kernel with null and with a mask; stream 0 full-range, stream 2 on the rails."""
    seen = high_band_emulator.check_stage(high_band_emulator.program(tmp_path_factory), tmp_path, rate, k)
    assert [T for T, _, _ in seen] == [1, 1, 3, 2, 16] and [m for _, m, _ in seen] == [False, False, False, True, False]
    assert seen[2][2].tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 1]] and not seen[3][2].size
    f = seen[4][2]
    assert f[0, 0] and f[1, 15] and f[1, 5] and f[1, 6] and f.sum() == 4
