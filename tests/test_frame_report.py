"""
Frame report (include/pv_koala_batch.h: pv_koala_batch_process_call, pv_koala_process_report) without a GPU: the
numpy restatement of the spec (tests/frame_report_recipe.py) against a float64 sum and its exact identities, the gfx950 build of every
report form of the synthesis kernel, the symbols, and the Python side's argument handling.  tests/test_gpu_frame_report.py checks the
values on the GPU.
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

import koala_amd
from conftest import ROOT, synth_streams
from frame_report_recipe import F32, ReportRecipe, applied_mask, energy_terms, fma32, report_rows, row_sum, sum64
from koala_amd import report as rp

sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
SYMBOLS = ('pv_koala_batch_process_call', 'pv_koala_process_report')
PV_STATUS_INVALID_ARGUMENT = 3
# Every term of the three sums is non-negative, so any order of n - 1 float32 adds stays within (n - 1) 2^-24 relative of the exact sum of the
# terms (each add errs by at most 2^-24 of a partial sum, and no partial sum exceeds the total): n = 257 bins, and the float64 sum of the same
# terms is exact at this scale.
SUM_BAR = 257 * 2.0 ** -24


def test_fma32_is_the_single_rounding_of_the_exact_value():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(F32)
    c = (np.abs(rng.standard_normal(4000)) * 10.0 ** rng.integers(-12, 12, 4000)).astype(F32)
    # ties and near-ties of the float32 rounding: a * a = 1 + 2^-11 + 2^-24 next to addends far below an ulp
    a[:8] = F32(1.0 + 2.0 ** -12)
    c[:8] = np.array([2.0 ** -24 - 2.0 ** -23, 2.0 ** -60, 0.0, 2.0 ** -30, 2.0 ** -47, 2.0 ** -49, 2.0 ** -24, 2.0 ** -25], F32).clip(0)
    got = fma32(a, a, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) ** 2 + Fraction(float(c[i]))
        lo = F32(float(exact))  # (Fraction -> float64 is correctly rounded; the float32 candidates are its two neighbours)
        cands = {float(lo), float(np.nextafter(lo, F32(np.inf))), float(np.nextafter(lo, F32(-np.inf)))}
        best = min(cands, key=lambda v: (abs(Fraction(v) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert float(got[i]) == best, (i, a[i], c[i])


@pytest.mark.parametrize('kind', ['random', 'default'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_recipe_against_a_float64_sum(random_model, gate_model, kind, precision):
    n, T = 6, 12
    x = synth_streams(n, T, seed=31)
    gains = np.array([0.0, 1.0, 0.25, 0.5, 0.1, 0.9], F32)
    rec = ReportRecipe(random_model if kind == 'random' else gate_model, n, precision)
    spec, m = rec.stages(x)
    worst = 0.0
    for b in range(n):
        mp = applied_mask(m[b], gains[b])
        y = np.stack([(mp * spec[b, ..., 0]).astype(F32), (mp * spec[b, ..., 1]).astype(F32)], axis=-1)
        y[..., 0, 1] = y[..., 256, 1] = 0
        rows = report_rows(spec[b], m[b], gains[b])
        for idx, terms in ((0, energy_terms(spec[b])), (1, energy_terms(y)), (2, m[b])):
            ref = sum64(terms)
            assert (ref > 0).all()
            rel = np.abs(rows[:, idx].astype(np.float64) - ref) / ref
            worst = max(worst, float(rel.max()))
        assert (rows[:, 3] == 0).all()
    print('%s %s: largest |recipe - float64 sum| / sum = %.3g (bar %.3g)' % (kind, precision, worst, SUM_BAR))
    assert worst <= SUM_BAR


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_exact_identities_of_the_recipe(random_model, unity_model, precision):
    n, T = 4, 6
    x = synth_streams(n, T, seed=32)
    x[2] = 0  # digital silence
    spec, m = ReportRecipe(random_model, n, precision).stages(x)
    for b in range(n):
        one = report_rows(spec[b], m[b], 1.0)  # g = 1: m' = 1, Y = X
        assert np.array_equal(one[:, 0], one[:, 1])
        assert np.array_equal(one[:, 2], report_rows(spec[b], m[b], 0.0)[:, 2])  # the raw mask, whatever the limit
    silent = report_rows(spec[2], m[2], 0.25)
    assert not silent[:, :2].any() and not silent[:, 3].any()
    spec, m = ReportRecipe(unity_model, n, precision).stages(x)
    assert (m == 1.0).all()
    for g in (0.0, 0.3):
        rows = report_rows(spec, m, g)
        assert (rows[..., 2] == F32(257.0)).all() and np.array_equal(rows[..., 0], rows[..., 1])
    # the tree is the butterfly over lane ^ 1, ^ 2, ^ 4, ^ 8 of fft_column's layout: a sum of powers of two far apart tells the order
    t = np.zeros(257, F32)
    t[[0, 8, 1, 15]] = [1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24]
    assert row_sum(t) == F32(1.0 + 2.0 ** -23)  # Q0 = P0 + P8 rounds to 1 (tie to even), Q1 = P1 + P15 = 2^-23 (one chain would stay at 1)
    t[15] = 0
    assert row_sum(t) == F32(1.0)  # Q0 = 1, then R0 = 1 + 2^-24 is a tie again (P8 + P1 first would reach 1 + 2^-23)


def test_report_helpers():
    rows = np.array([[65536.0, 6553.6, 257.0, 0], [0, 0, 128.5, 0], [32768.0, 0, 0, 0]], F32)
    assert np.allclose(rp.mean_gain(rows), [1.0, 0.5, 0.0]) and rp.mean_gain(rows).dtype == np.float32
    s = rp.suppression_db(rows)
    assert abs(s[0] + 10.0) < 1e-5 and np.isnan(s[1]) and s[2] == -np.inf
    d = rp.input_dbfs(rows)
    assert d[0] == 0.0 and d[1] == -np.inf and abs(d[2] + 3.0103) < 1e-3
    # the constant: a stationary input of mean square P reports e_in = 65536 P (Parseval under the sqrt-Hann window) -- a full-scale square wave
    n = np.arange(512)
    yw = np.sin(np.pi * n / 512.0) * np.where((n // 7) % 2, 1.0, -1.0)
    Y = np.fft.rfft(yw)
    assert abs(10 * np.log10((np.abs(Y) ** 2).sum() / rp.ENERGY_AT_FULL_SCALE)) < 0.1
    assert rp.mean_gain(np.zeros((3, 5, 4))).shape == (3, 5)


def test_symbols_are_exported_and_declared(native_library):
    header = open(os.path.join(ROOT, 'include', 'pv_koala_batch.h')).read()
    for path in (native_library, koala_amd.developer_library_path()):
        lib = ctypes.CDLL(path)
        for sym in SYMBOLS:
            assert hasattr(lib, sym), (path, sym)
    for sym in SYMBOLS:
        assert re.search(r'PV_API pv_status_t %s\(' % sym, header), sym
    assert 'pv_koala_batch_call_t' in header and 'report' not in open(os.path.join(ROOT, 'include', 'pv_koala.h')).read()
    from koala_amd._batch import BatchCall
    assert ctypes.sizeof(BatchCall) == 56  # two int32, five pointers, one int32 + padding: the struct_size the library checks


def test_null_arguments_are_refused_without_a_gpu(native_library):
    lib = ctypes.CDLL(native_library)
    lib.pv_get_error_stack.argtypes = [ctypes.POINTER(ctypes.POINTER(ctypes.c_char_p)), ctypes.POINTER(ctypes.c_int32)]
    lib.pv_free_error_stack.argtypes = [ctypes.POINTER(ctypes.c_char_p)]
    vp = ctypes.c_void_p
    lib.pv_koala_batch_process_call.argtypes = [vp, vp]
    lib.pv_koala_process_report.argtypes = [vp, vp, vp, vp]
    frame = (ctypes.c_int16 * 256)()
    row = (ctypes.c_float * 4)(7, 7, 7, 7)
    for call in (lambda: lib.pv_koala_batch_process_call(None, None), lambda: lib.pv_koala_process_report(None, frame, frame, row)):
        assert call() == PV_STATUS_INVALID_ARGUMENT
        msgs, depth = ctypes.POINTER(ctypes.c_char_p)(), ctypes.c_int32()
        assert lib.pv_get_error_stack(ctypes.byref(msgs), ctypes.byref(depth)) == 0 and depth.value == 1
        assert b'NULL' in msgs[0]
        lib.pv_free_error_stack(msgs)
    assert list(row) == [7.0] * 4


class _FakeLib:
    """stands in for the native library: records the pv_koala_batch_process_call it is given"""

    def __init__(self):
        self.calls = []

    def pv_koala_batch_process_call(self, handle, call):
        c = call._obj
        self.calls.append({f: getattr(c, f) for f, _ in c._fields_})
        return koala_amd.KoalaBatch.__init__.__globals__['PicovoiceStatuses'].SUCCESS


def _fake_batch(B, Tmax):
    kb = koala_amd.KoalaBatch.__new__(koala_amd.KoalaBatch)
    kb._lib, kb._handle, kb._pinned = _FakeLib(), ctypes.c_void_p(1), []
    kb.num_streams, kb.max_frames_per_call, kb.frame_length = B, Tmax, 256
    return kb


def test_python_argument_handling_without_a_device():
    from koala_amd._batch import BatchCall
    kb = _fake_batch(3, 4)
    x = np.zeros((3, 512), np.int16)
    out = kb.process_call(x)
    assert isinstance(out, np.ndarray) and out.shape == x.shape
    c = kb._lib.calls[-1]
    assert c['struct_size'] == ctypes.sizeof(BatchCall) and c['num_frames'] == 2 and not c['report'] and not c['reset'] and not c['hold']
    assert c['asynchronous'] == 0 and c['pcm'] == x.ctypes.data
    out, rep = kb.process_call(x, reset=np.zeros((3, 2), np.uint8), report=True)
    assert rep.shape == (3, 2, 4) and rep.dtype == np.float32
    c = kb._lib.calls[-1]
    assert c['report'] == rep.ctypes.data and c['reset'] and not c['hold']
    kb.process_call(x, hold=np.array([0, 1, 0]))
    assert kb._lib.calls[-1]['hold'] and not kb._lib.calls[-1]['reset']
    kb.process_device_call(2, 0x1000, 0x2000, 0x3000)
    c = kb._lib.calls[-1]
    assert (c['pcm'], c['enhanced'], c['report'], c['asynchronous']) == (0x1000, 0x2000, 0x3000, 0)
    kb.process_device_call(2, 0x1000, 0x2000)
    assert not kb._lib.calls[-1]['report']
    y, r = np.zeros_like(x), np.zeros((3, 2, 4), np.float32)
    kb.process_async_call(x, y, report=r)
    c = kb._lib.calls[-1]
    assert c['asynchronous'] == 1 and c['report'] == r.ctypes.data and c['enhanced'] == y.ctypes.data
    n = len(kb._lib.calls)
    Bad = koala_amd.KoalaInvalidArgumentError
    for bad in (lambda: kb.process_call(np.zeros((2, 512), np.int16)), lambda: kb.process_call(np.zeros((3, 500), np.int16)),
                lambda: kb.process_call(x, reset=np.zeros((3, 3), np.uint8)), lambda: kb.process_call(x, hold=np.zeros(2, np.uint8)),
                lambda: kb.process_async_call(x, y, report=np.zeros((3, 2, 4), np.float64)),
                lambda: kb.process_async_call(x, y, report=np.zeros((3, 1, 4), np.float32)),
                lambda: kb.process_async_call(x, np.zeros((3, 256), np.int16))):
        with pytest.raises(Bad):
            bad()
    assert len(kb._lib.calls) == n  # nothing reached the library


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_every_report_form_builds_for_gfx950_without_spills(tmp_path):
    """synthesis_report_kernel<kRecompute, kMaskH, kMaskIn, kResets, kMinGain>: the nine forms the engine launches, each with and without the
    minimum gain; none spills, the multi-frame forms stay within the budget of three waves per SIMD (168 VGPRs), and each keeps the occupancy
    of the plain kernel it is the twin of."""
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
    info = {'synthesis_kernel': {}, 'synthesis_report_kernel': {}}
    for name, body in re.findall(r'\.set (\S+)\.has_indirect_call, \d+\n[^\n]*\n; Kernel info:\n((?:;[^\n]*\n)*)', text):
        form = re.search(r'\d+(synthesis_kernel|synthesis_report_kernel)I((?:Lb[01]E)+)E', name)
        if form:
            bits = tuple(int(b) for b in re.findall(r'Lb([01])E', form.group(2)))
            info[form.group(1)][bits] = {k: int(re.search(r'; %s: (\d+)' % k, body).group(1)) for k in ('ScratchSize', 'Occupancy', 'NumVgprs')}
    forms = [(1, 1, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (1, 1, 0, 1), (1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 0, 1), (0, 1, 1, 0)]
    want = sorted(f + (g,) for f in forms for g in (0, 1))
    assert sorted(info['synthesis_report_kernel']) == want and sorted(info['synthesis_kernel']) == want
    for f in want:
        plain, rep = info['synthesis_kernel'][f], info['synthesis_report_kernel'][f]
        print(f, 'plain', plain, 'kReport', rep)
        assert rep['ScratchSize'] == 0, (f, rep)
        assert rep['Occupancy'] == plain['Occupancy'], (f, plain, rep)
        if not f[2]:  # (the one-frame form with the mask head inside is one workgroup of eight waves per CU by its launch bounds)
            assert rep['Occupancy'] >= 3 and rep['NumVgprs'] <= 168, (f, rep)
    # The report rows leave through buffer stores that nothing guards: no conditional vector-memory operation in the frame loop.  A descriptor
    # that hipcc cannot prove wave-uniform is stored through a "waterfall" -- v_readfirstlane of its words, s_and_saveexec, the store, s_xor
    # exec, s_cbranch_execnz back -- so in EVERY report form: no s_cbranch_execnz at all (the plain kernels have none), not one exec-masked
    # region more than the plain twin has, no buffer store within reach of a saveexec, and the four dword stores and DPP adds are there.
    bodies = {}
    for m in re.finditer(r'^_ZN3kns\d+(synthesis_kernel|synthesis_report_kernel)I((?:Lb[01]E)+)EEvNS_13SynthesisArgsE:(.*?)^\.Lfunc_end', text, re.M | re.S):
        bodies[(m.group(1), tuple(int(b) for b in re.findall(r'Lb([01])E', m.group(2))))] = re.sub(r';.*', '', m.group(3))
    assert len(bodies) == 36
    for f in want:
        plain, rep = bodies[('synthesis_kernel', f)], bodies[('synthesis_report_kernel', f)]
        assert 's_cbranch_execnz' not in rep and 's_cbranch_execnz' not in plain, f
        assert rep.count('saveexec') <= plain.count('saveexec'), (f, rep.count('saveexec'), plain.count('saveexec'))
        lines = [l.strip() for l in rep.splitlines() if l.strip()]
        for i, l in enumerate(lines):
            if l.startswith('buffer_store'):
                assert not any('saveexec' in p or 'v_readfirstlane' in p for p in lines[max(0, i - 6):i]), (f, lines[max(0, i - 6):i + 1])
        assert rep.count('buffer_store_dword ') == plain.count('buffer_store_dword ') + 4, f
        assert rep.count('_dpp') >= plain.count('_dpp') + 12, f  # three sums x four butterfly steps
