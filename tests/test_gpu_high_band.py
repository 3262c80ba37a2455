"""
The high-band carry (include/pv_koala_batch.h: HIGH-BAND CARRY; DESIGN.md section 2, ninth extension) on a real MI355X: high_band_kernel<R>
(koala_amd/csrc/kns_highband.hip) through the product library.  4 streams, max_frames_per_call = 3, the call sequence T = 1, 1, 1, 3, 2, 1
(D is longer than a frame, so the input history spans two earlier one-frame calls and the pair of gains spans calls), 32 and 48 kHz, both
precisions, the `random` model, seeded noise with energy up to Nyquist and one stream of digital silence.

The carry is a function of what the plain handle delivers: handle A is plain and asked for its report, handle B carries; B's samples must
equal tests/high_band_recipe.HighBand(x, A's samples, A's mask_sum, the limit) with array_equal -- in both precisions, since the kernel
sees int16 samples and the float report only.

Every size beyond B = 4 -- the routes of Engine::run_device other than the low-latency layer kernel and the wavefront, ragged m-tiles,
calls longer than 3 frames -- and inputs at the rails: tests/test_gpu_high_band_routes.py.
"""
import ctypes

import numpy as np
import pytest

import koala_amd
from conftest import model_file
from gpu_kit import batch, call, cut, same
from high_band_recipe import HighBand
from koala_amd import KoalaInvalidArgumentError, formats
from koala_amd.channels import deinterleave, interleave

pytestmark = pytest.mark.gpu

B, TMAX = 4, 3
SEQ = (1, 1, 1, 3, 2, 1)


def make(rate, precision, carry, **kw):
    return batch(model_file('random'), B, TMAX, precision, sample_rate=rate, high_band='carry' if carry else None, **kw)


def noise(rate, frames, seed, peak=20000):
    """white noise (flat to Nyquist), every stream its own; the last stream is digital silence"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-peak, peak + 1, size=(B, frames * rate * 256 // 16000)).astype(np.int16)
    x[B - 1] = 0
    return x


@pytest.mark.parametrize('mode', ['device', 'host'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('rate', [32000, 48000])
def test_carry_equals_the_recipe_over_the_plain_handle(rate, precision, mode):
    """case 1: no limit, then (after a reset of everything) limits 0, 0.25 and 1 on different streams, changed between two calls"""
    ka, kb = make(rate, precision, False), make(rate, precision, True)
    assert kb.high_band == 'carry' and ka.high_band is None and kb.delay_sample == 304 * (rate // 16000)
    ref = HighBand(B, rate)
    for phase, gains in enumerate([None, (np.array([0.0, 0.25, 1.0, 0.25], np.float32), np.array([1.0, 0.0, 0.25, 1.0], np.float32))]):
        g = np.zeros(B, np.float32)
        for i, x in enumerate(cut(noise(rate, sum(SEQ), 5 + phase), rate, SEQ)):
            if gains is not None and i in (0, 3):
                g = gains[i // 3]
                ka.set_min_gain(g), kb.set_min_gain(g)
            e, rep = call(ka, x, mode, report=True)
            if i % 2:  # (B's report, when asked for, is A's; a call that asks for none reads the engine's own buffer)
                y, rep_b = call(kb, x, mode, report=True)
                assert same(rep_b, rep), (phase, i)
            else:
                y = call(kb, x, mode)
            want = ref.process(x, e, rep[:, :, 2], g)
            assert np.array_equal(y, want), (phase, i, int(np.abs(y.astype(int) - want).max()))
            if phase == 0 and i == len(SEQ) - 1:
                assert np.abs(y[:B - 1].astype(int) - e[:B - 1]).max() > 100 and not y[B - 1].any()  # (a band was added; silence stays silence)
        ka.reset(), kb.reset(), ref.reset()
    ka.delete(), kb.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('rate', [32000, 48000])
def test_with_the_bypass_gain_the_handle_is_a_pure_delay_to_one_lsb(rate, precision):
    """case 2: g = 1 on every stream, noise at a quarter of full scale (Lf cannot clip: tests/test_high_band.py); the plain handle is a
    low-pass and misses the same bound by thousands of LSB"""
    ka, kb = make(rate, precision, False), make(rate, precision, True)
    ka.set_min_gain(1.0), kb.set_min_gain(1.0)
    x = noise(rate, sum(SEQ), 9, peak=8192)
    ya = np.concatenate([call(ka, p, 'device') for p in cut(x, rate, SEQ)], axis=1)
    yb = np.concatenate([call(kb, p, 'device') for p in cut(x, rate, SEQ)], axis=1)
    F, D = rate * 256 // 16000, kb.delay_sample
    xd = np.concatenate([np.zeros((B, D), np.int16), x], axis=1)[:, :x.shape[1]].astype(int)
    err_b, err_a = np.abs(yb.astype(int) - xd)[:, 2 * F:], np.abs(ya.astype(int) - xd)[:, 2 * F:]
    print('carry: max |out - x delayed| =', err_b.max(), ' plain:', err_a[:B - 1].max())
    assert err_b.max() <= 1
    assert err_a[:B - 1].max() > 1000
    ka.delete(), kb.delete()


@pytest.mark.parametrize('rate', [32000, 48000])
def test_resets_restart_the_high_band_with_the_stream(rate):
    """case 3: a masked reset of streams 1 and 2, then a call with frame-0 resets of streams 0 and 3"""
    ka, kb, ref = make(rate, 'bf16', False), make(rate, 'bf16', True), HighBand(B, rate)
    parts = cut(noise(rate, 9, 21), rate, (1, 2, 1, 3, 2))
    masked, flags = np.array([0, 1, 1, 0], np.uint8), np.zeros((B, 3), np.uint8)
    flags[0, 0] = flags[3, 0] = 1
    for i, x in enumerate(parts):
        kw = {}
        if i == 2:
            ka.reset(masked), kb.reset(masked), ref.reset(masked)
        if i == 3:
            kw = {'reset': flags}
            ref.reset(flags[:, 0])
        e, rep = call(ka, x, 'device', report=True, **kw)
        y = call(kb, x, 'device', **kw)
        assert np.array_equal(y, ref.process(x, e, rep[:, :, 2])), i
    ka.delete(), kb.delete()


@pytest.mark.parametrize('rate', [32000, 48000])
def test_off_is_the_plain_handle_and_on_again_starts_the_high_band_afresh(rate):
    """case 4"""
    ka, kb, ref = make(rate, 'bf16', False), make(rate, 'bf16', True), HighBand(B, rate)
    for i, x in enumerate(cut(noise(rate, sum(SEQ), 31), rate, SEQ)):
        if i == 2:
            kb.set_high_band(None)
            assert kb.high_band is None
        if i == 4:
            kb.set_high_band('carry')
            fresh = HighBand(B, rate)  # (the high band of streams that begin here; the handle's own in-stage goes on)
            fresh.s_in.hist = ref.s_in.hist.copy()
            ref = fresh
        e, rep = call(ka, x, 'device', report=True)
        y = call(kb, x, 'device')
        want = ref.process(x, e, rep[:, :, 2])
        assert np.array_equal(y, e if i in (2, 3) else want), i
    ka.delete(), kb.delete()


@pytest.mark.parametrize('mode', ['device', 'inplace', 'host'])
def test_formats_channels_and_the_link_stay_outside(mode):
    """case 5: float32 samples, two interleaved channels, linked masks, 48 kHz: encode(interleave(recipe)), s the group's max"""
    rate, C = 48000, 2
    kw = dict(sample_format='f32', channels=C, channel_link='max')
    ka, kb, ref = make(rate, 'bf16', False, **kw), make(rate, 'bf16', True, **kw), HighBand(B, rate, channels=C)
    g = np.array([0.0, 0.25, 0.25, 0.0], np.float32)
    ka.set_min_gain(g), kb.set_min_gain(g)
    x = noise(rate, sum(SEQ), 41)
    x[B - 1] = x[0] // 2  # (every channel a signal: the group max is taken over unequal masks)
    for i, p in enumerate(cut(x, rate, SEQ)):
        xf = formats.encode('f32', interleave(p, C))
        e, rep = call(ka, xf, mode, report=True)
        y = call(kb, xf, mode)
        want = ref.process(p, deinterleave(formats.decode('f32', e), C), rep[:, :, 2], g)
        assert same(y, formats.encode('f32', interleave(want, C))), i
    assert np.abs(rep[0, :, 2] - rep[1, :, 2]).max() > 0  # (the channels' own masks differ: the max matters)
    ka.delete(), kb.delete()


def test_refusals_on_the_device_build_touch_nothing():
    """case 6"""
    import torch
    for kw, word in ((dict(sample_rate=16000), 'sample_rate'), (dict(sample_rate=24000), 'sample_rate'), (dict(sample_rate=8000), 'sample_rate'),
                     (dict(sample_rate=48000, packet_samples=960), 'packet')):
        k = koala_amd.create_batch('key', B, TMAX, 'bf16', model_path=model_file('random'), **kw)
        k.set_high_band(None)
        with pytest.raises(KoalaInvalidArgumentError, match=word):
            k.set_high_band('carry')
        assert k.high_band is None
        k.delete()
    rate = 48000
    ka, kb, ref = make(rate, 'bf16', False), make(rate, 'bf16', True), HighBand(B, rate)
    parts = cut(noise(rate, 5, 51), rate, (3, 2))
    e, rep = call(ka, parts[0], 'device', report=True)
    assert np.array_equal(call(kb, parts[0], 'device'), ref.process(parts[0], e, rep[:, :, 2]))
    n = B * 2 * 768
    src, dst = torch.from_numpy(parts[1].reshape(-1)).cuda(), torch.full((n,), 0x5A5A, dtype=torch.int16, device='cuda')
    hold, late = np.array([0, 1, 0, 0], np.uint8), np.zeros((B, 2), np.uint8)
    late[2, 1] = 1
    with pytest.raises(KoalaInvalidArgumentError, match='hold'):
        kb.process_device_hold(2, src.data_ptr(), dst.data_ptr(), hold)
    with pytest.raises(KoalaInvalidArgumentError, match=r'reset\[2\]\[1\]'):
        kb.process_device_resets(2, src.data_ptr(), dst.data_ptr(), late)
    with pytest.raises(KoalaInvalidArgumentError, match='high-band'):
        kb.export_state()
    with pytest.raises(KoalaInvalidArgumentError, match='high-band'):
        kb.import_state(np.zeros((B, kb.state_size), np.uint8))
    size = ctypes.c_int32(-7)
    assert kb._lib.pv_koala_batch_state_size(kb._handle, ctypes.byref(size)).name == 'INVALID_ARGUMENT' and size.value == -7
    kb.synchronize()
    assert (dst.cpu().numpy() == 0x5A5A).all()
    e, rep = call(ka, parts[1], 'device', report=True)  # the streams and the carry's state are where they were
    assert np.array_equal(call(kb, parts[1], 'device'), ref.process(parts[1], e, rep[:, :, 2]))
    kb.set_high_band(None)
    assert kb.export_state().shape == (B, kb.state_size)  # (off: the handle it was)
    ka.delete(), kb.delete()
