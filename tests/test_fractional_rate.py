"""
Packet handles at 44 100 and 22 050 Hz (include/pv_koala_batch.h: pv_koala_batch_init_config; DESIGN.md section 2, sixth extension) without
a GPU: the recipe of tests/fractional_rate_recipe.py against itself in other cuts and around a pure delay, koala_amd.packets' restatement
of the inner counts against a brute-force count, what Python accepts and refuses, the gfx950 build of koala_amd/csrc/kns_fractional.hip,
the kernels' own source on the CPU (tests/fractional_emulation) and the C ABI (tests/abi_fractional_rate/driver.cpp), both as stand-alone
programs under AddressSanitizer + UndefinedBehaviorSanitizer.  tests/test_gpu_fractional_rate.py checks the samples on the GPU.
"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fractional_rate_recipe as frr
import koala_amd
import sanitized_build
from conftest import ROOT, model_file
from koala_amd import packets

sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
DELAY = {44100: 1541, 22050: 771}


def full_range(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, size=n).astype(np.int16)


def two_tone(rate, n, fade):
    """1 kHz and 3.1 kHz, faded in over `fade` samples (0: an abrupt start)"""
    t = np.arange(n)
    x = 6000.0 * np.sin(2 * np.pi * 1000.0 * t / rate) + 3000.0 * np.sin(2 * np.pi * 3100.0 * t / rate)
    if fade:
        x *= np.where(t < fade, 0.5 - 0.5 * np.cos(np.pi * t / fade), 1.0)
    return np.round(x).astype(np.int16)


def test_constants_of_the_recipe_are_the_specs():
    assert [frr.shift(r) for r in frr.RATES] == [41, 201] and [frr.delay_sample(r) for r in frr.RATES] == [1541, 771]
    assert [frr.in_taps(r) for r in frr.RATES] == [133, 67] and frr.L == 21169
    for rate in frr.RATES:
        U = frr.UP[rate]
        assert 16000 * 441 == rate * U
        n = np.arange(0, 3000)
        assert np.array_equal(frr.inner_samples(n, rate), -(-U * n // 441)) and frr.inner_samples(0, rate) == 0
        # an in-stage output has at most 133 / 67 taps, an out-stage output 48 or 49
        assert max(len(range(r, frr.L, U)) for r in range(U)) == frr.in_taps(rate)
        assert sorted({len(range(r, frr.L, 441)) for r in range(441)}) == [48, 49]


@pytest.mark.parametrize('rate', frr.RATES)
def test_recipe_in_any_cuts_is_the_recipe_in_one_piece(rate):
    N = 9000
    x = full_range(N, seed=rate)
    one = frr.Stream(rate, frr.DelayInner()).push(x)
    assert one.size == N
    rng = np.random.default_rng(3)
    menus = ([1] * 60 + [0, 441, 882, 0, 1, 440, 442, 2, 3], [441] * 5 + [0] + [882] * 3, None)
    for menu in menus:
        s, out, pos, zero_inner = frr.Stream(rate, frr.DelayInner()), [], 0, 0
        k = 0
        while pos < N:
            c = menu[k % len(menu)] if menu else int(rng.choice([0, 1, 2, 441, 882, int(rng.integers(0, 1000))]))
            c, k = min(c, N - pos), k + 1
            zero_inner += c > 0 and s.due(c) == 0
            before = (s.phase, s.hist_in.copy(), s.hist_out.copy())
            out.append(s.push(x[pos:pos + c]))
            assert out[-1].size == c
            if c == 0:
                assert before[0] == s.phase and np.array_equal(before[1], s.hist_in) and np.array_equal(before[2], s.hist_out)
            pos += c
        assert np.array_equal(np.concatenate(out), one), (rate, menu)
        # sum of the counts = N: the inner stream got exactly M(N) samples
        assert sum(y.size for y in s.fed) == int(frr.inner_samples(N, rate))
        if menu and menu[0] == 1:
            assert zero_inner > 0  # (1-sample calls: some feed the inner path nothing, and still deliver their sample)


@pytest.mark.parametrize('rate', frr.RATES)
def test_around_a_pure_delay_the_output_is_the_input_delay_sample_later(rate):
    """The chain's delay is 246 519 + c ticks = 1541 / 771 samples exactly.  The signal fades in over 4000 samples: an abrupt start has
    energy above the converters' pass band, which a linear-phase filter spreads to both sides of its delay; a stream that starts smoothly
    shows nothing in front of it.  Whatever the signal, every output whose time base U n - c lies in front of inner sample 511 is 0."""
    N, d, U = 16000, DELAY[rate], frr.UP[rate]
    x = two_tone(rate, N, 4000)
    z = frr.Stream(rate, frr.DelayInner()).push(x).astype(np.float64)
    xs = x.astype(np.float64)
    dist = [float(np.sum((z - np.concatenate([np.zeros(k), xs[:N - k]])) ** 2)) for k in range(d - 40, d + 41)]
    assert int(np.argmin(dist)) == 40, (rate, int(np.argmin(dist)) + d - 40)
    assert not z[:d].any()
    err = np.abs(z[d:] - xs[:N - d])
    steady = slice(d + 6000, N)
    level = 20 * np.log10(np.sqrt(np.mean(z[steady] ** 2)) / np.sqrt(np.mean(xs[6000:N - d] ** 2)))
    print('%d Hz: delay %d samples, level %+.4f dB, largest distance %.0f LSB' % (rate, d, level, err.max()))
    assert abs(level) <= 0.1 and err.max() <= 1
    # full-range noise from sample 0: the structural zeros
    zero = int(np.sum((U * np.arange(N) - frr.shift(rate)) // 441 < frr.INNER_DELAY))
    assert zero > 0.9 * d and not frr.Stream(rate, frr.DelayInner()).push(full_range(N, seed=5))[:zero].any()


@pytest.mark.parametrize('rate', frr.RATES)
def test_inner_counts_of_packets_py_are_a_brute_force_count(rate):
    U = frr.UP[rate]
    rng = np.random.default_rng(rate)
    N, count = rng.integers(0, 200000, 3000), rng.integers(0, 3000, 3000)
    count[:50] = 0
    got, phase = packets.inner_due(N % 441, count, rate)
    for n, c, g, p in zip(N.tolist(), count.tolist(), got.tolist(), phase.tolist()):
        # inner sample m exists once 441 m <= U n' - 1 for the n' samples received, i.e. its newest input sample has arrived
        brute = sum(1 for m in range(U * n // 441, U * (n + c) // 441 + 2) if U * n - 1 < 441 * m <= U * (n + c) - 1)
        assert g == brute and p == (n + c) % 441, (n, c, g, brute)
    # sum of counts = N  ->  sum of inner = M(N), from the mirror of N mod 441 alone
    phase, total, fed = np.zeros(1, np.int32), 0, 0
    for c in rng.integers(0, 1200, 400).tolist():
        inner, phase = packets.inner_due(phase, [c], rate)
        total, fed = total + c, fed + int(inner[0])
        assert fed == packets.inner_samples(total, rate) == int(frr.inner_samples(total, rate))
    assert packets.inner_samples(0, rate) == 0 and isinstance(packets.inner_samples(5, rate), int)


def test_python_takes_the_two_rates_as_packet_handles_only(random_model, monkeypatch):
    for rate in frr.RATES:  # without packet_samples: refused before anything is loaded, as it has always been
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='sample_rate'):
            koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, sample_rate=rate)
    for bad in (11025, 96000, 0):
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='sample_rate'):
            koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, sample_rate=bad, packet_samples=480)
    import koala_amd._batch as kb

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(kb, 'load_library', stop)
    for rate in frr.RATES:
        for fmt in ('s16', 'ulaw'):
            with pytest.raises(Reached):
                koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, sample_rate=rate, packet_samples=1000, sample_format=fmt)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_fractional_kernels_build_for_gfx950_without_scratch_or_spills(tmp_path):
    import isa_scan
    src = 'kns_fractional.hip'
    out = tmp_path / (src + '.s')
    mk = open(os.path.join(ROOT, 'koala_amd', 'Makefile')).read()
    assert 'csrc/' + src in mk and 'obj/kns_fractional.o' in mk
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
    want = ['fractional_%s_kernelILi%dEEEvNS_14FractionalArgsE' % (d, U) for d in ('in', 'out') for U in (160, 320)] + ['fractional_reset_kernel']
    kernels = [k for k in info if 'fractional_' in k]
    assert len(kernels) == 5 and all(len([k for k in kernels if w in k]) == 1 for w in want), kernels
    for k in kernels:
        print(k, info[k], 'spills (sgpr, vgpr):', spills.get(k))
        assert info[k]['ScratchSize'] == 0, (k, info[k])
        assert spills[k] == (0, 0), (k, spills[k])
    # the tap loop: per tap one table load, one LDS read (two taps may share a ds_read2) and one fma; nothing else touches memory there
    for w in want[:4]:
        name = [k for k in kernels if w in k][0]
        body = text.split(name + ':')[1].split('s_endpgm')[0]
        lines = body.splitlines()
        fma = [i for i, line in enumerate(lines) if re.search(r'\bv_fmac?_f32', line)]
        loads = [i for i, line in enumerate(lines) if re.search(r'\bglobal_load_dword\b', line)]
        assert len(fma) == 7 and len(loads) == 7, (name, len(fma), len(loads))  # (the loop is unrolled by 7)
        assert not [x for x in lines[loads[0]:fma[-1] + 1] if re.search(r'\b(global|flat|buffer|scratch)_(store|atomic)|\bds_write|\bs_barrier', x)], name


def translation_unit():
    src = os.path.join(ROOT, 'tests', 'fractional_emulation')
    header = open(os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_kernels.h')).read()
    kernels = open(os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_fractional.hip')).read().replace('#include "kns_kernels.h"', '')
    kernels = kernels[:kernels.index('void launch_fractional_in(')] + '}\n'
    section = (header[header.index('constexpr int kFrDown'):header.index('void launch_fractional_in')] +
               header[header.index('struct FractionalStateArgs {'):header.index('void launch_fractional_reset')])
    return (open(os.path.join(src, 'shim.inc')).read() + 'namespace kns {\n' + section + '}\n' + kernels +
            open(os.path.join(src, 'driver.inc')).read())


@pytest.fixture(scope='module')
def emulator(tmp_path_factory):
    return sanitized_build.build_translation_unit(translation_unit(), tmp_path_factory.mktemp('fractional_emulation'), ['-ffp-contract=off'])


@pytest.mark.parametrize('U', [160, 320])
def test_kernels_are_the_definition_and_touch_nothing_else(emulator, U):
    """the kernels' own source, 256 threads a workgroup, against a plain C++ loop of the definition: B = 3 streams out of phase, counts from
    {0, 1, 2, 3, 440, 441, 442, 882, 1000}, max_samples 1000, a masked reset mid-run"""
    run = sanitized_build.run(emulator, U)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count('samples ok') == 3


def test_constructor_queries_and_refusals_through_the_c_abi_under_asan_and_ubsan(tmp_path):
    run = sanitized_build.run(sanitized_build.build_abi_driver('abi_fractional_rate', tmp_path), model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
