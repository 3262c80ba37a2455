"""
Batch handles at 8, 32 and 48 kHz (include/pv_koala_batch.h: pv_koala_batch_init_rate; DESIGN.md section 2, third extension) on a real MI355X:
koala_amd/csrc/kns_resample.hip's stages around the unchanged 16 kHz call, through the product library.  The tests that hold at every rate are written
for all five -- 8, 12, 24, 32 and 48 kHz -- and parametrised here over the three whole-number rates; tests/test_gpu_rational_rate.py runs the
same functions at 12 and 24 kHz with its own batch sizes and modes.  Where the frames per call differ between the rates, the per-rate
literal stands in the test: they are part of a case.

Expected samples come from tests/sample_rate_recipe.py: in-stage -> oracle.Oracle.process -> out-stage in numpy float32, held to the bar of
tests/sample_rate_cases.py (fp32: ==; bf16: a bound on the distance and on the share further than 1 LSB).  Wherever the inner engine is a
pure delay (a unity-mask model, min_gain = 1) the samples are == in both precisions.
"""
import ctypes

import numpy as np
import pytest

import koala_amd
import sample_rate_recipe as srr
from conftest import model_file, synth_streams
from gpu_kit import call
from sample_rate_cases import CALLS, NCLS, TMAX, batch, check, classes, cut, expected, signal

pytestmark = pytest.mark.gpu

RATES = (8000, 32000, 48000)
RATE_PREC = [(r, p) for r in RATES for p in ('fp32', 'bf16')]
# koala_amd/csrc/kns_kernels.h's static_asserts, as literals: the recipe's own constants are held to them, not the other way round
FRAME = {8000: 128, 12000: 192, 24000: 384, 32000: 512, 48000: 768}
DELAY = {8000: 176, 12000: 240, 24000: 456, 32000: 608, 48000: 912}
TAIL = {8000: 288, 12000: 224, 24000: 240, 32000: 288, 48000: 384}


# ------------------------------------------------------------------------------------------------ the recipe, call after call

@pytest.mark.parametrize('B,mode', [(NCLS, 'host'), (NCLS, 'device'), (832, 'device'), (832, 'host'), (40, 'inplace')])
@pytest.mark.parametrize('kind', ['random', 'unity'])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_calls_of_mixed_lengths_are_the_recipe(rate, precision, kind, B, mode):
    x, want = expected(kind, precision, rate)
    jit = expected(kind, precision, rate, 1)[1] if precision == 'bf16' and kind == 'random' else None
    cls = classes(B)
    kb = batch(model_file(kind if kind == 'unity' else 'random', 1234), B, TMAX[rate], precision, rate)
    try:
        assert (kb.sample_rate, kb.frame_length, kb.delay_sample) == (rate, FRAME[rate], DELAY[rate])
        assert kb.state_size == 10240 + TAIL[rate]
        got, t0 = [], 0
        for T in CALLS[rate]:
            got.append(call(kb, np.ascontiguousarray(cut(x, rate, t0, t0 + T)[cls]), mode))
            t0 += T
    finally:
        kb.delete()
    got, wantc = np.concatenate(got, axis=1), np.concatenate(want, axis=1)[cls]
    check(got, wantc, precision, rate, '%s %dx%s' % (kind, B, mode), None if jit is None else np.concatenate(jit, axis=1)[cls])


@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_min_gain_one_is_both_stages_around_a_pure_delay(random_model, rate, precision):
    x, want = expected('unity', precision, rate)
    kb = batch(random_model, NCLS, TMAX[rate], precision, rate)
    try:
        kb.set_min_gain(1.0)
        got, t0 = [], 0
        for T in CALLS[rate]:
            got.append(call(kb, cut(x, rate, t0, t0 + T), 'device'))
            t0 += T
    finally:
        kb.delete()
    assert np.array_equal(np.concatenate(got, axis=1), np.concatenate(want, axis=1))


@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_whole_number_rates_at_workgroup_edges(random_model, rate, precision):
    """Where the stage kernel's workgroup of 256 groups does not line up with the call: a half-filled last workgroup (8 kHz, T = 1: 128
    groups), a frame boundary and a reset floor inside a workgroup (8 kHz, T = 3: 384 groups), a chunk boundary inside a frame (32 and
    48 kHz out-stage: 2 and 3 output samples per group), full-range samples through the LDS output assembly.  min_gain = 1 makes the
    inner engine the bit-exact 256-sample delay in either precision, so every sample is the recipe's."""
    B, fl = 3, srr.frame_length(rate)
    x = np.random.default_rng(rate).integers(-32768, 32768, size=(B, 6 * fl)).astype(np.int16)
    reset = np.zeros((B, 3), np.uint8)
    reset[1, 1] = reset[2, 2] = 1
    rec = srr.Recipe(None, B, precision, rate)
    kb = batch(random_model, B, 3, precision, rate)
    try:
        kb.set_min_gain(1.0)
        x0, x1, x2 = cut(x, rate, 0, 1), cut(x, rate, 1, 4), cut(x, rate, 4, 6)
        assert np.array_equal(call(kb, x0, 'device'), rec.process(x0))
        assert np.array_equal(call(kb, x1, 'device', reset=reset), rec.process_resets(x1, reset))
        assert np.array_equal(call(kb, x2, 'device'), rec.process(x2))
        assert np.array_equal(kb.export_state()[:, 10240:], rec.rs_state())
    finally:
        kb.delete()


@pytest.mark.parametrize('T', [8, 4])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_rate_16000_through_init_rate_is_the_plain_handle(random_model, precision, T):
    x = np.ascontiguousarray(synth_streams(NCLS, T + 1, seed=3))
    plain = koala_amd.create_batch('key', NCLS, T, precision, model_path=random_model)
    other = koala_amd.create_batch('key', NCLS, T, precision, model_path=random_model)
    try:
        lib = other._lib
        lib.pv_koala_batch_init_rate.argtypes = [ctypes.c_char_p] * 3 + [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_void_p)]
        lib.pv_koala_batch_init_rate.restype = ctypes.c_int
        h = ctypes.c_void_p()
        assert lib.pv_koala_batch_init_rate(b'key', random_model.encode(), b'best', NCLS, T, 1 if precision == 'bf16' else 0, 16000,
                                            ctypes.byref(h)) == 0
        lib.pv_koala_batch_delete(other._handle)
        other._handle = h  # (the Python class on the handle pv_koala_batch_init_rate made)
        assert other.state_size == plain.state_size == 10240 and (other.frame_length, other.delay_sample) == (256, 256)
        for a, b in ((0, T), (T, T + 1)):
            xa = np.ascontiguousarray(x[:, a * 256:b * 256])
            assert np.array_equal(plain.process(xa), other.process(xa))
        ra, rb = plain.export_state(), other.export_state()
        assert np.array_equal(ra, rb) and ra[0, 4:8].view(np.uint32)[0] == 1
        other.import_state(ra)
    finally:
        plain.delete()
        other.delete()


# ------------------------------------------------------------------------------------------------ resets

@pytest.mark.parametrize('B,mode', [(NCLS, 'host'), (832, 'device')])
@pytest.mark.parametrize('rate', RATES)
def test_every_kind_of_reset_is_a_fresh_stream(random_model, rate, B, mode):
    T = {8000: 6, 12000: 5, 24000: 5, 32000: 6, 48000: 6}[rate]
    x = signal(rate, 3 * T, seed=21)
    cls = classes(B)
    rec = srr.Recipe(random_model, NCLS, 'fp32', rate)
    kb = batch(random_model, B, T, 'fp32', rate)
    try:
        x0, x1, x2 = (cut(x, rate, i * T, (i + 1) * T) for i in range(3))
        assert np.array_equal(call(kb, x0[cls], mode), rec.process(x0)[cls])
        # per-frame resets: frame 0, adjacent frames, a frame t > 0, the last frame
        reset = np.zeros((NCLS, T), np.uint8)
        for b, t in ((0, 0), (1, 2), (1, 3), (2, 5), (3, 1)) if T == 6 else ((0, 0), (1, 2), (2, 4), (3, 1), (3, 2)):
            reset[b, t] = 1
        got = call(kb, x1[cls], mode, reset=np.ascontiguousarray(reset[cls]))
        assert np.array_equal(got, rec.process_resets(x1, reset)[cls])
        # a masked reset, then a full one
        rows = np.zeros(NCLS, bool)
        rows[[1, 4]] = True
        kb.reset(rows[cls].astype(np.uint8))
        rec.reset(rows)
        assert np.array_equal(call(kb, x2[cls], mode), rec.process(x2)[cls])
        kb.reset()
        fresh = srr.Recipe(random_model, NCLS, 'fp32', rate).process(x0)[cls]
        assert np.array_equal(call(kb, x0[cls], mode), fresh)
        # frame 0 of every stream (the reset kernel in front of the call) == the same fresh streams again
        r0 = np.zeros((B, T), np.uint8)
        r0[:, 0] = 1
        assert np.array_equal(call(kb, x0[cls], mode, reset=r0), fresh)
    finally:
        kb.delete()


@pytest.mark.parametrize('rate', RATES)
def test_per_frame_resets_after_frame_0_stay_refused_for_a_five_frame_front_end(random5_model, rate):
    T = 4
    x = signal(rate, 2 * T, seed=23)
    a, b = batch(random5_model, NCLS, T, 'fp32', rate), batch(random5_model, NCLS, T, 'fp32', rate)
    try:
        x0, x1 = cut(x, rate, 0, T), cut(x, rate, T, 2 * T)
        assert np.array_equal(a.process(x0), b.process(x0))
        late = np.zeros((NCLS, T), np.uint8)
        late[2, 1] = 1
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='frame 0 only'):
            a.process_resets(x1, late)
        first = np.zeros((NCLS, T), np.uint8)
        first[2, 0] = 1
        # (the refused call has advanced nothing, the converters included)
        assert np.array_equal(a.process_resets(x1, first), b.process_resets(x1, first))
    finally:
        a.delete()
        b.delete()


# ------------------------------------------------------------------------------------------------ held streams, stream records

@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_a_held_stream_is_not_advanced(random_model, rate, precision):
    T = {8000: 5, 12000: 3, 24000: 3, 32000: 5, 48000: 5}[rate]
    x = signal(rate, 3 * T, seed=31)
    x0, x1, x2 = (cut(x, rate, i * T, (i + 1) * T) for i in range(3))
    a, b, c = (batch(random_model, NCLS, T, precision, rate) for _ in range(3))
    try:
        hold = np.zeros(NCLS, np.uint8)
        hold[[1, 3]] = 1
        a.process(x0)
        b.process(x0)
        before = a.export_state()
        got = call(a, x1, 'device', hold=hold)
        after = a.export_state()
        # bit for bit what it was, converters included (the record's tail); the others moved
        assert np.array_equal(before[hold != 0], after[hold != 0]) and before[hold != 0][:, 10240:].any()
        assert not np.array_equal(before[hold == 0], after[hold == 0])
        assert not np.array_equal(before[hold == 0][:, 10240:], after[hold == 0][:, 10240:])
        full = b.process(x1)
        assert np.array_equal(got[hold == 0], full[hold == 0])
        # the held streams continue as if the call had not happened: they see x2 right after x0
        c.process(x0)
        want_held = c.process(x2)
        got2, full2 = a.process(x2), b.process(x2)
        assert np.array_equal(got2[hold != 0], want_held[hold != 0]) and np.array_equal(got2[hold == 0], full2[hold == 0])
    finally:
        for h in (a, b, c):
            h.delete()


@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_records_carry_the_converters_between_handles(random_model, rate, precision):
    T = {8000: 4, 12000: 3, 24000: 3, 32000: 4, 48000: 4}[rate]
    x = signal(rate, 2 * T, seed=37)
    x0, x1 = cut(x, rate, 0, T), cut(x, rate, T, 2 * T)
    rec = srr.Recipe(random_model, NCLS, precision, rate)
    a, big = batch(random_model, NCLS, T, precision, rate), batch(random_model, 40, T, precision, rate)
    try:
        want0 = rec.process(x0)
        got0 = a.process(x0)
        if precision == 'fp32':
            assert np.array_equal(got0, want0)
        blobs = a.export_state()
        assert a.state_size == 10240 + TAIL[rate] and blobs.shape == (NCLS, a.state_size)
        hdr = blobs[:, :32].copy().view(np.uint32)
        assert (hdr[:, 1] == 2).all() and (hdr[:, 6] == rate).all() and not hdr[:, 7].any()
        rs = blobs[:, 10240:]
        # rs_in is the input's tail in both precisions; rs_out the enhanced 16 kHz samples' (fp32: the recipe's)
        n_in = rec.s_in.hist.shape[1] * 2
        assert np.array_equal(rs[:, :n_in], rec.rs_state()[:, :n_in])
        if precision == 'fp32':
            assert np.array_equal(rs, rec.rs_state())
        # into other slots of a handle of another size, in another order: sample for sample what the first handle goes on to produce
        slots = np.array([33, 2, 17, 39, 0, 8], np.int32)
        big.import_state(blobs, streams=slots)
        xb = np.zeros((40, x1.shape[1]), np.int16)
        xb[slots] = x1
        cont, moved = a.process(x1), big.process(xb)[slots]
        assert np.array_equal(moved, cont)
        if precision == 'fp32':
            assert np.array_equal(cont, rec.process(x1))
        assert np.array_equal(big.export_state(streams=slots), a.export_state())
    finally:
        a.delete()
        big.delete()


def test_records_do_not_cross_rates_or_versions(random_model):
    h8, h32, h16 = (batch(random_model, 2, 2, 'fp32', r) for r in (8000, 32000, 16000))
    try:
        x = signal(8000, 2, seed=41)[:2]
        h8.process(x)
        r8, r16 = h8.export_state(), h16.export_state()
        assert r8.shape[1] == h32.state_size  # (R = 2 both: only the header tells them apart)
        before = h32.export_state()
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='sample_rate 8000'):
            h32.import_state(r8)
        v1 = np.zeros_like(r8)
        v1[:, :r16.shape[1]] = r16
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='version 1 is not 2'):
            h8.import_state(v1)
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='version 2 is not 1'):
            h16.import_state(np.ascontiguousarray(r8[:, :r16.shape[1]]))
        assert np.array_equal(h32.export_state(), before) and np.array_equal(h8.export_state(), r8)
        h8.import_state(r8)
    finally:
        for h in (h8, h32, h16):
            h.delete()


# ------------------------------------------------------------------------------------------------ the frame report, the asynchronous refusal

@pytest.mark.parametrize('mode', ['host', 'device'])
@pytest.mark.parametrize('rate,precision', [pytest.param(r, 'fp32', id=str(r)) for r in RATES])
def test_the_frame_report_is_the_inner_16_khz_streams(random_model, rate, precision, mode):
    T = {8000: 6, 12000: 3, 24000: 3, 32000: 6, 48000: 6}[rate]
    x = signal(rate, 2 * T, seed=43)
    rec = srr.Recipe(None, NCLS, 'fp32', rate)
    kb, inner = batch(random_model, NCLS, T, precision, rate), batch(random_model, NCLS, T, precision, 16000)
    try:
        gains = np.linspace(0.0, 0.5, NCLS).astype(np.float32)
        kb.set_min_gain(gains)
        inner.set_min_gain(gains)
        for i in range(2):
            xi = cut(x, rate, i * T, (i + 1) * T)
            got, rep = call(kb, xi, mode, report=True)
            want_y, want_rep = call(inner, rec.inner(xi), mode, report=True)
            assert rep.shape == (NCLS, T, 4) and np.array_equal(rep, want_rep)
            assert np.array_equal(got, rec.s_out.run(want_y))
    finally:
        kb.delete()
        inner.delete()


def test_asynchronous_calls_are_refused_and_change_nothing(random_model, rate=8000):
    T = 2
    x = signal(rate, 2 * T, seed=47)
    a, b = batch(random_model, NCLS, T, 'fp32', rate), batch(random_model, NCLS, T, 'fp32', rate)
    try:
        x0, x1 = cut(x, rate, 0, T), cut(x, rate, T, 2 * T)
        assert np.array_equal(a.process(x0), b.process(x0))
        pin, pout = a.alloc_host(T), a.alloc_host(T)
        pin[:] = x1
        pout[:] = -7
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='16000'):
            a.process_async(pin, pout)
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='16000'):
            a.process_async_call(pin, pout)
        a.synchronize()
        assert (pout == -7).all()
        assert np.array_equal(a.export_state(), b.export_state())
        assert np.array_equal(a.process(x1), b.process(x1))
    finally:
        a.delete()
        b.delete()
