"""
Batch handles at 12 and 24 kHz (include/pv_koala_batch.h: pv_koala_batch_init_rate; DESIGN.md section 2, third extension, generalised) on a
real MI355X: koala_amd/csrc/kns_resample.hip's rational stages around the unchanged 16 kHz call, through the product library.

Expected samples come from tests/rational_rate_recipe.py: in-stage -> oracle.Oracle.process -> out-stage in numpy float32.  fp32: ==.  bf16:
the bar of tests/test_gpu_sample_rate.py -- the largest distance is at most ceil(BF16_TOL * S) + 1 LSB, S = the out-stage's largest sum of
|tap| over an output phase, and the share of samples further than 1 LSB from the recipe is at most 4 x the share by which the jittered
bf16 oracle misses the plain one through the same recipe on the same inputs.  Wherever the inner engine is a pure delay (min_gain = 1) the
samples are == in both precisions.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import koala_amd
import rational_rate_recipe as rrr
import sample_format_recipe as sf
import sample_rate_recipe as srr
from conftest import model_file, synth_streams
from oracle import oracle

pytestmark = pytest.mark.gpu

BF16_TOL = 5            # tests/test_gpu_parity.py
BF16_WITHIN_1 = 0.99    # tests/test_gpu_parity.py (a packet handle against a frame handle in other cuts: tests/test_gpu_packets.py)
NCLS = 6                # distinct streams; a batch repeats them (cls[b]) so that the CPU side stays small
CALLS = (1, 2, 5, 5, 2, 1)
TMAX = 5
RATE_PREC = [(r, p) for r in rrr.RATES for p in ('fp32', 'bf16')]
DELAY = {12000: 240, 24000: 456}
FRAME = {12000: 192, 24000: 384}
TAIL = {12000: 224, 24000: 240}


def batch(model, B, T, precision, rate, **kw):
    return koala_amd.create_batch('key', B, T, precision, model_path=model, sample_rate=rate, **kw)


def classes(B):
    return np.arange(B) % NCLS


def signal(rate, T, seed):
    """int16 [NCLS, T * frame_length]: the suite's synthetic streams, taken as samples at `rate`"""
    fl = rrr.frame_length(rate)
    return np.ascontiguousarray(synth_streams(NCLS, T * fl // 256 + 1, seed=seed)[:, :T * fl])


def cut(x, rate, t0, t1):
    fl = rrr.frame_length(rate)
    return np.ascontiguousarray(x[:, t0 * fl:t1 * fl])


def call(kb, x, mode, **kw):
    """one call -> enhanced (or (enhanced, report)): 'host' (pageable), 'device', 'inplace' (device, enhanced == pcm)"""
    T = x.shape[1] // kb.frame_length
    if mode == 'host':
        return kb.process_call(x, **kw)
    import torch
    report = kw.pop('report', False)
    xd = torch.from_numpy(x).cuda()
    yd = xd if mode == 'inplace' else torch.zeros_like(xd)
    rd = torch.full((x.shape[0], T, 4), -1.0, dtype=torch.float32, device='cuda') if report else None
    torch.cuda.synchronize()
    kb.process_device_call(T, xd.data_ptr(), yd.data_ptr(), rd.data_ptr() if report else 0, **kw)
    kb.synchronize()
    return (yd.cpu().numpy(), rd.cpu().numpy()) if report else yd.cpu().numpy()


@functools.lru_cache(maxsize=None)
def expected(kind, precision, rate, jitter=0):
    """the recipe over CALLS on the NCLS class streams -> (input, [enhanced per call]); kind 'unity': the inner engine as a pure delay"""
    x = signal(rate, sum(CALLS), seed=11)
    oracle.set_jitter(jitter)
    try:
        rec = rrr.Recipe(None if kind == 'unity' else model_file('random', 1234), NCLS, precision, rate)
        out, t0 = [], 0
        for T in CALLS:
            out.append(rec.process(cut(x, rate, t0, t0 + T)))
            t0 += T
    finally:
        oracle.set_jitter(0)
    return x, out


def check(got, want, precision, rate, what, jitter_want=None):
    """prints the figures before it asserts"""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((d > 1).mean())
    print('%s %s %d Hz: max distance %d LSB, share > 1 LSB %.3e' % (what, precision, rate, int(d.max()), share), end='')
    if precision == 'fp32' or jitter_want is None:
        print()
        assert np.array_equal(got, want), what
        return
    (uo, do), K = rrr.STAGES[rate][1], rrr.common_k(rate)
    bound = math.ceil(BF16_TOL * rrr.Stage(1, K, uo, do).abs_tap_sum()) + 1
    jshare = float((np.abs(jitter_want.astype(np.int32) - want.astype(np.int32)) > 1).mean())
    print(', bound %d LSB; jittered oracle misses %.3e -> allowed %.3e' % (bound, jshare, 4 * jshare))
    assert d.max() <= bound, (what, int(d.max()), bound)
    assert share <= 4 * jshare, (what, share, jshare)


# ------------------------------------------------------------------------------------------------ the recipe, call after call

@pytest.mark.parametrize('B,mode', [(3, 'host'), (3, 'device'), (70, 'inplace')])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_calls_of_mixed_lengths_are_the_recipe(random_model, rate, precision, B, mode):
    x, want = expected('random', precision, rate)
    jit = expected('random', precision, rate, 1)[1] if precision == 'bf16' else None
    cls = classes(B)
    kb = batch(random_model, B, TMAX, precision, rate)
    try:
        assert (kb.sample_rate, kb.frame_length, kb.delay_sample) == (rate, FRAME[rate], DELAY[rate])
        assert kb.state_size == 10240 + TAIL[rate]
        got, t0 = [], 0
        for T in CALLS:
            got.append(call(kb, np.ascontiguousarray(cut(x, rate, t0, t0 + T)[cls]), mode))
            t0 += T
    finally:
        kb.delete()
    got, wantc = np.concatenate(got, axis=1), np.concatenate(want, axis=1)[cls]
    check(got, wantc, precision, rate, '%dx%s' % (B, mode), None if jit is None else np.concatenate(jit, axis=1)[cls])


@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_min_gain_one_is_both_stages_around_a_pure_delay(random_model, rate, precision):
    x, want = expected('unity', precision, rate)
    kb = batch(random_model, NCLS, TMAX, precision, rate)
    try:
        kb.set_min_gain(1.0)
        got, t0 = [], 0
        for T in CALLS:
            got.append(call(kb, cut(x, rate, t0, t0 + T), 'device'))
            t0 += T
    finally:
        kb.delete()
    assert np.array_equal(np.concatenate(got, axis=1), np.concatenate(want, axis=1))


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_rate_16000_through_init_rate_is_untouched(random_model, precision):
    x = np.ascontiguousarray(synth_streams(NCLS, 5, seed=3))
    plain = koala_amd.create_batch('key', NCLS, 4, precision, model_path=random_model)
    other = koala_amd.create_batch('key', NCLS, 4, precision, model_path=random_model)
    try:
        lib = other._lib
        lib.pv_koala_batch_init_rate.argtypes = [ctypes.c_char_p] * 3 + [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_void_p)]
        lib.pv_koala_batch_init_rate.restype = ctypes.c_int
        h = ctypes.c_void_p()
        assert lib.pv_koala_batch_init_rate(b'key', random_model.encode(), b'best', NCLS, 4, 1 if precision == 'bf16' else 0, 16000,
                                            ctypes.byref(h)) == 0
        lib.pv_koala_batch_delete(other._handle)
        other._handle = h  # (the Python class on the handle pv_koala_batch_init_rate made)
        assert other.state_size == plain.state_size == 10240 and (other.frame_length, other.delay_sample) == (256, 256)
        for a, b in ((0, 4), (4, 5)):
            xa = np.ascontiguousarray(x[:, a * 256:b * 256])
            assert np.array_equal(plain.process(xa), other.process(xa))
        ra, rb = plain.export_state(), other.export_state()
        assert np.array_equal(ra, rb) and ra[0, 4:8].view(np.uint32)[0] == 1
    finally:
        plain.delete()
        other.delete()


# ------------------------------------------------------------------------------------------------ resets

@pytest.mark.parametrize('B,mode', [(NCLS, 'host'), (70, 'device')])
@pytest.mark.parametrize('rate', rrr.RATES)
def test_every_kind_of_reset_is_a_fresh_stream(random_model, rate, B, mode):
    T = 5
    x = signal(rate, 3 * T, seed=21)
    cls = classes(B)
    rec = rrr.Recipe(random_model, NCLS, 'fp32', rate)
    kb = batch(random_model, B, T, 'fp32', rate)
    try:
        x0, x1, x2 = (cut(x, rate, i * T, (i + 1) * T) for i in range(3))
        assert np.array_equal(call(kb, x0[cls], mode), rec.process(x0)[cls])
        # per-frame resets: frame 0, a middle frame, adjacent frames, the last frame of the 5-frame call
        reset = np.zeros((NCLS, T), np.uint8)
        reset[0, 0] = reset[1, 2] = reset[2, T - 1] = reset[3, 1] = reset[3, 2] = 1
        got = call(kb, x1[cls], mode, reset=np.ascontiguousarray(reset[cls]))
        assert np.array_equal(got, rec.process_resets(x1, reset)[cls])
        # a masked reset, then a full one
        rows = np.zeros(NCLS, bool)
        rows[[1, 4]] = True
        kb.reset(rows[cls].astype(np.uint8))
        rec.reset(rows)
        assert np.array_equal(call(kb, x2[cls], mode), rec.process(x2)[cls])
        kb.reset()
        fresh = rrr.Recipe(random_model, NCLS, 'fp32', rate).process(x0)[cls]
        assert np.array_equal(call(kb, x0[cls], mode), fresh)
        # frame 0 of every stream == the same fresh streams again
        r0 = np.zeros((B, T), np.uint8)
        r0[:, 0] = 1
        assert np.array_equal(call(kb, x0[cls], mode, reset=r0), fresh)
    finally:
        kb.delete()


# ------------------------------------------------------------------------------------------------ held streams, stream records

@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_a_held_stream_is_not_advanced(random_model, rate, precision):
    T = 3
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
    T = 3
    x = signal(rate, 2 * T, seed=37)
    x0, x1 = cut(x, rate, 0, T), cut(x, rate, T, 2 * T)
    rec = rrr.Recipe(random_model, NCLS, precision, rate)
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

@pytest.mark.parametrize('rate', rrr.RATES)
def test_asynchronous_calls_are_refused_and_change_nothing(random_model, rate):
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


@pytest.mark.parametrize('mode', ['host', 'device'])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_the_frame_report_is_the_inner_16_khz_streams(random_model, rate, precision, mode):
    T = 3
    x = signal(rate, 2 * T, seed=43)
    rec = rrr.Recipe(None, NCLS, 'fp32', rate)
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
