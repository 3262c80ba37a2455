"""
Batch handles at 12 and 24 kHz (include/pv_koala_batch.h: pv_koala_batch_init_rate; DESIGN.md section 2, third extension, generalised) on a
real MI355X: koala_amd/csrc/kns_resample.hip's rational stages around the unchanged 16 kHz call, through the product library.
The tests that hold at every rate are tests/test_gpu_sample_rate.py's, written for all five rates; here they run at 12 and 24 kHz with this
module's batch sizes and modes, under the names these cases have had.  What exists at 24 kHz only is written here.
"""
import numpy as np
import pytest

import koala_amd
import sample_format_recipe as sf
import test_gpu_sample_rate as every_rate
from gpu_kit import BF16_TOL, BF16_WITHIN_1, call
from sample_rate_cases import CALLS, NCLS, batch, signal

pytestmark = pytest.mark.gpu

RATES = (12000, 24000)
RATE_PREC = [(r, p) for r in RATES for p in ('fp32', 'bf16')]
TMAX = max(CALLS[24000])


# ------------------------------------------------------------------------------------------------ the recipe, call after call

@pytest.mark.parametrize('B,mode', [(3, 'host'), (3, 'device'), (70, 'inplace')])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_calls_of_mixed_lengths_are_the_recipe(rate, precision, B, mode):
    every_rate.test_calls_of_mixed_lengths_are_the_recipe(rate, precision, 'random', B, mode)


@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_min_gain_one_is_both_stages_around_a_pure_delay(random_model, rate, precision):
    every_rate.test_min_gain_one_is_both_stages_around_a_pure_delay(random_model, rate, precision)


# ------------------------------------------------------------------------------------------------ resets

@pytest.mark.parametrize('B,mode', [(NCLS, 'host'), (70, 'device')])
@pytest.mark.parametrize('rate', RATES)
def test_every_kind_of_reset_is_a_fresh_stream(random_model, rate, B, mode):
    every_rate.test_every_kind_of_reset_is_a_fresh_stream(random_model, rate, B, mode)


# ------------------------------------------------------------------------------------------------ held streams, stream records

@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_a_held_stream_is_not_advanced(random_model, rate, precision):
    every_rate.test_a_held_stream_is_not_advanced(random_model, rate, precision)


@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_records_carry_the_converters_between_handles(random_model, rate, precision):
    every_rate.test_records_carry_the_converters_between_handles(random_model, rate, precision)


def test_a_24_khz_record_is_refused_at_other_rates_with_the_field_named(random_model):
    h24, h12, h48, h16 = (batch(random_model, 2, 2, 'fp32', r) for r in (24000, 12000, 48000, 16000))
    try:
        h24.process(signal(24000, 2, seed=41)[:2])
        r24 = h24.export_state()
        assert r24.shape[1] == 10480

        def sized(n):  # (the record in a buffer of the other handle's record size: the header is what tells them apart)
            out = np.zeros((2, n), np.uint8)
            out[:, :min(n, r24.shape[1])] = r24[:, :n]
            return out
        for h, field in ((h12, 'sample_rate 24000'), (h48, 'sample_rate 24000'), (h16, 'version 2 is not 1')):
            before = h.export_state()
            with pytest.raises(koala_amd.KoalaInvalidArgumentError, match=field):
                h.import_state(sized(h.state_size))
            assert np.array_equal(h.export_state(), before)
        h24.import_state(r24)
        assert np.array_equal(h24.export_state(), r24)
    finally:
        for h in (h24, h12, h48, h16):
            h.delete()


# ------------------------------------------------------------------------------------------------ packet and format handles at 24 kHz

@pytest.mark.parametrize('P', [240, 480])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_packets_at_24_khz_are_the_frame_handle_behind_383_zeros(random_model, precision, P):
    rate, F, B, n = 24000, 384, 4, 2880  # 12 packets of 10 ms or 6 of 20 ms: 7.5 frames
    calls, stall, restart_at = n // P, 2, 3
    x = signal(rate, 8, seed=51)[:B]
    kp = batch(random_model, B, 1, precision, rate, packet_samples=P)
    kf = batch(random_model, B, 8, precision, rate)
    try:
        assert kp.delay_sample == 839 == kf.delay_sample + F - 1 and kp.frame_length == F
        assert kp.state_size == kf.state_size + (4 + 2 * (F - 1) + 15) // 16 * 16
        pos, got = np.zeros(B, int), [[] for _ in range(B)]
        for i in range(calls):
            counts = np.full(B, P, np.int32)
            counts[2] = 0 if i == stall else P  # stream 2 stalls once; stream 3 is fresh before packet `restart_at`
            restart = np.array([0, 0, 0, 1], np.uint8) if i == restart_at else None
            pcm = np.zeros((B, P), np.int16)
            for b in range(B):
                pcm[b, :counts[b]] = x[b, pos[b]:pos[b] + counts[b]]
            out = kp.process_packets(pcm, counts, restart=restart)
            for b in range(B):
                got[b].append(out[b, :counts[b]].copy())
            pos += counts
        got = [np.concatenate(g) for g in got]
        assert [len(g) for g in got] == [n, n, n - P, n]
        # the frame handle: the streams' whole frames, then (fresh) stream 3's from its restart on
        e = kf.process(np.ascontiguousarray(x[:, :7 * F]))
        kf.reset()
        cutp = restart_at * P
        k = (n - cutp) // F
        x3 = np.zeros((B, k * F), np.int16)
        x3[3] = x[3, cutp:cutp + k * F]
        e3 = kf.process(x3)[3]
        zeros = np.zeros(F - 1, np.int16)
        want = [np.concatenate([zeros, e[b]])[:len(got[b])] for b in range(3)]
        want.append(np.concatenate([np.concatenate([zeros, e[3]])[:cutp], np.concatenate([zeros, e3])[:n - cutp]]))
        for b in range(B):
            d = np.abs(got[b].astype(np.int32) - want[b].astype(np.int32))
            print('%s P=%d stream %d: max distance %d LSB, within 1 LSB %.4f' % (precision, P, b, int(d.max()), float((d <= 1).mean())))
            if precision == 'fp32':
                assert np.array_equal(got[b], want[b]), b
            else:  # (the frame handle ran in other cuts: the bars of tests/test_gpu_packets.py)
                assert d.max() <= BF16_TOL and (d <= 1).mean() >= BF16_WITHIN_1, b
    finally:
        kp.delete()
        kf.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_an_f32_handle_at_24_khz_is_encode_of_the_s16_handle_of_decode(random_model, precision):
    rate, B, F = 24000, 5, 384
    rng = np.random.default_rng(61)
    x = rng.integers(-32768, 32768, (B, 8 * F)).astype(np.int16).astype(np.float32) * np.float32(1.0 / 32768)
    x[B - 1] = np.resize(sf.F32_EDGES, x.shape[1])
    kf, ks = batch(random_model, B, TMAX, precision, rate, sample_format='f32'), batch(random_model, B, TMAX, precision, rate)
    try:
        assert (kf.delay_sample, kf.frame_length, kf.state_size) == (ks.delay_sample, ks.frame_length, ks.state_size)
        for mode in ('host', 'device'):
            kf.reset(), ks.reset()
            t = 0
            for T in (1, 2, 5):
                part = np.ascontiguousarray(x[:, t * F:(t + T) * F])
                got, want = call(kf, part, mode), sf.encode(sf.F32, call(ks, sf.decode(sf.F32, part), mode))
                assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (mode, t, T)
                t += T
    finally:
        kf.delete()
        ks.delete()


# ------------------------------------------------------------------------------------------------ the asynchronous refusal, the frame report

@pytest.mark.parametrize('rate', RATES)
def test_asynchronous_calls_are_refused_and_change_nothing(random_model, rate):
    every_rate.test_asynchronous_calls_are_refused_and_change_nothing(random_model, rate)


@pytest.mark.parametrize('mode', ['host', 'device'])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_the_frame_report_is_the_inner_16_khz_streams(random_model, rate, precision, mode):
    every_rate.test_the_frame_report_is_the_inner_16_khz_streams(random_model, rate, precision, mode)
