"""
Multi-channel batch handles (include/pv_koala_batch.h: CHANNELS; DESIGN.md section 2, seventh extension) on a real MI355X:
koala_amd/csrc/kns_channels.hip's two kernels around the unchanged call, through the product library.

Every comparison is == against  interleave(planar handle(deinterleave(x))):  the planar handle is created alongside with the same model,
precision, rate, kind and num_streams and is fed the same call sequence with the same per-stream arguments.  The frame calls of the planar
reference run with DEVICE pointers on one buffer IN PLACE: the channel handle's inner call is exactly that -- a device-pointer call, in
place on the handle's rows, in the same slots -- so the two run the same kernels on the same samples in both precisions and there is no
tolerance to grant.  (Packet calls move their samples through the packetiser's own buffers whatever the caller's pointers are; their
reference runs with host pointers.)  Every channel has its own signal (conftest.synth_streams: one seed per row), so a swapped or shifted
channel cannot pass.
"""
import ctypes

import numpy as np
import pytest

import koala_amd
import sample_format_recipe as sf
from conftest import model_file
from gpu_kit import MARK, call, flen, packet_call, same, streams
from koala_amd import KoalaInvalidArgumentError
from koala_amd._batch import BatchConfig
from koala_amd._koala import PicovoiceStatuses
from koala_amd.channels import deinterleave, interleave

pytestmark = pytest.mark.gpu


def pair(B, C, precision='fp32', rate=16000, T=3, packet_samples=0, sample_format='s16', model='random'):
    """(the channel handle, its planar twin)"""
    kw = dict(model_path=model_file(model), sample_rate=rate, packet_samples=packet_samples, sample_format=sample_format)
    return koala_amd.create_batch('key', B, T, precision, channels=C, **kw), koala_amd.create_batch('key', B, T, precision, **kw)


def planar_call(kp, x, C, report=False, **kw):
    """the reference: deinterleave, the planar handle with device pointers in place, interleave"""
    got = call(kp, deinterleave(x, C), 'inplace', report=report, **kw)
    return (interleave(got[0], C), got[1]) if report else interleave(got, C)


# ------------------------------------------------------------------------------------------------ 1. pure delay

@pytest.mark.parametrize('mode', ['host', 'device', 'inplace', 'offset'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_bypass_gain_returns_every_channel_delayed_by_256_samples(precision, mode):
    C, B, T, calls = 2, 6, 3, 4
    G, n = B // C, T * 256
    kc = koala_amd.create_batch('key', B, T, precision, model_path=model_file('random'), channels=C)
    assert (kc.channels, kc.num_streams, kc.delay_sample, kc.frame_length) == (C, B, 256, 256)
    kc.set_min_gain(1.0)
    x = interleave(streams(B, calls * n), C)  # [G, calls n C]
    parts = [np.ascontiguousarray(x[:, k * n * C:(k + 1) * n * C]) for k in range(calls)]
    y = np.concatenate([call(kc, p, mode) for p in parts], axis=1)
    assert y.shape == (G, calls * n * C)
    assert np.array_equal(y[:, 256 * C:], x[:, :-256 * C]) and not y[:, :256 * C].any()
    px, py = deinterleave(x, C), deinterleave(y, C)
    for s in range(B):  # ... said per stream: enhanced[g][(i + 256) C + c] == pcm[g][i C + c]
        assert np.array_equal(py[s, 256:], px[s, :-256]), s
    kc.delete()


def test_the_three_dimensional_shape_is_the_same_memory():
    C, B, T = 2, 6, 3
    kc, kp = pair(B, C)
    x = interleave(streams(B, T * 256, seed=3), C)
    want = kc.process(x)
    kc.reset()
    got = kc.process(x.reshape(B // C, T * 256, C))
    assert got.shape == (B // C, T * 256, C) and np.array_equal(got.reshape(want.shape), want)
    assert np.array_equal(want, planar_call(kp, x, C))
    kc.delete(), kp.delete()


# ------------------------------------------------------------------------------------------------ 2. equals the planar handle

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('rate,T', [(16000, 3), (8000, 2), (48000, 1)])
@pytest.mark.parametrize('C,B', [(2, 6), (3, 6), (8, 8)])
def test_a_channel_handle_is_interleave_of_the_planar_handle_of_deinterleave(C, B, rate, T, precision):
    F = flen(rate)
    kc, kp = pair(B, C, precision, rate, T)
    assert (kc.delay_sample, kc.frame_length, kc.state_size, kc.num_streams) == (kp.delay_sample, kp.frame_length, kp.state_size, kp.num_streams)
    x = interleave(streams(B, 3 * T * F, seed=C), C)
    for k, mode in enumerate(('device', 'host', 'inplace')):
        part = np.ascontiguousarray(x[:, k * T * F * C:(k + 1) * T * F * C])
        got, want = call(kc, part, mode), planar_call(kp, part, C)
        assert same(got, want), (mode, int((got != want).sum()))
    kc.delete(), kp.delete()


# ------------------------------------------------------------------------------------------------ 3. formats

FMT = {'f32': sf.F32, 'ulaw': sf.ULAW}


def format_signal(fmt, G, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == 'f32':
        return rng.integers(-32768, 32768, (G, n)).astype(np.int16).astype(np.float32) * np.float32(1.0 / 32768)
    return rng.integers(0, 256, (G, n)).astype(np.uint8)


@pytest.mark.parametrize('fmt', ['f32', 'ulaw'])
def test_a_format_channel_frame_handle_is_encode_of_the_s16_channel_handle_of_decode(fmt):
    C, B, T = 2, 6, 3
    kw = dict(model_path=model_file('random'), channels=C)
    kf, ks = koala_amd.create_batch('key', B, T, 'fp32', sample_format=fmt, **kw), koala_amd.create_batch('key', B, T, 'fp32', **kw)
    x = format_signal(fmt, B // C, 3 * T * 256 * C, 5)
    for k, mode in enumerate(('host', 'device', 'offset')):
        part = np.ascontiguousarray(x[:, k * T * 256 * C:(k + 1) * T * 256 * C])
        got = call(kf, part, mode)
        want = sf.encode(FMT[fmt], ks.process(sf.decode(FMT[fmt], part)))
        assert same(got, want), mode
    kf.delete(), ks.delete()


@pytest.mark.parametrize('fmt', ['f32', 'ulaw'])
def test_a_format_channel_packet_handle_is_encode_of_the_s16_channel_handle_of_decode(fmt):
    C, B, M = 2, 6, 333
    kw = dict(model_path=model_file('random'), channels=C, packet_samples=M)
    kf, ks = koala_amd.create_batch('key', B, 1, 'fp32', sample_format=fmt, **kw), koala_amd.create_batch('key', B, 1, 'fp32', **kw)
    rng = np.random.default_rng(9)
    for k in range(6):
        counts = np.repeat(rng.choice([0, 1, 160, M, int(rng.integers(1, M))], B // C), C)
        x = format_signal(fmt, B // C, M * C, 20 + k)
        got, want = kf.process_packets(x, counts), sf.encode(FMT[fmt], ks.process_packets(sf.decode(FMT[fmt], x), counts))
        for g in range(B // C):
            w = counts[g * C] * C
            assert same(got[g, :w], want[g, :w]), (k, g)
            assert not got[g, w:].any(), (k, g)  # nothing behind counts C was written: the wrapper's zeros
    kf.delete(), ks.delete()


# ------------------------------------------------------------------------------------------------ 4. packet handles, ragged

@pytest.mark.parametrize('rate', [16000, 44100])
def test_ragged_packet_calls_equal_the_planar_packet_handle(rate):
    C, B, M = 2, 6, 999
    G = B // C
    kc, kp = pair(B, C, 'fp32', rate, 1, packet_samples=M)
    assert (kc.delay_sample, kc.packet_samples) == (kp.delay_sample, kp.packet_samples)
    rng = np.random.default_rng(rate)
    menu = [0, 1, 441, 999]
    for k in range(12):
        per_group = np.array([menu[(k + g) % 4] if (k + g) % 3 else int(rng.integers(1, M + 1)) for g in range(G)], np.int32)
        if k == 5:
            per_group[1] = 0  # (a stalled group in the middle of the run, and again below)
        if k == 6:
            per_group[:] = [999, 0, 1]
        counts = np.repeat(per_group, C)
        restart = None
        if k == 7:
            restart = np.zeros(B, np.uint8)
            restart[3] = 1  # one channel of group 1 alone
        planar = streams(B, M, seed=100 + k)
        x = interleave(planar, C)
        want, want_frames, want_rep = kp.process_packets(planar, counts, restart, report=True)
        if k % 2:
            got, frames, rep = kc.process_packets(x, counts, restart, report=True)
            assert same(rep, want_rep), k
        else:
            got, frames = packet_call(kc, x, counts, restart)
        assert np.array_equal(frames, want_frames), k
        for g in range(G):
            w = int(per_group[g]) * C
            assert np.array_equal(got[g, :w], interleave(want[g * C:(g + 1) * C, :per_group[g]], C)[0]), (k, g)
            assert (got[g, w:] == (0 if k % 2 else MARK)).all(), (k, g)  # nothing behind counts C of a group row is written
    # unequal counts inside a group: refused by name, nothing processed -- the next good call equals the planar handle's
    bad = np.full(B, 100, np.int32)
    bad[3] = 99
    planar = streams(B, M, seed=200)
    with pytest.raises(KoalaInvalidArgumentError, match=r'counts\[3\].*streams 2 and 3.*group 1'):
        kc.process_packets(interleave(planar, C), bad)
    counts = np.full(B, 700, np.int32)
    got, want = kc.process_packets(interleave(planar, C), counts), kp.process_packets(planar, counts)
    assert np.array_equal(got[:, :700 * C], interleave(want[:, :700], C))
    kc.delete(), kp.delete()


# ------------------------------------------------------------------------------------------------ 5. per-stream arguments

@pytest.mark.parametrize('mode', ['host', 'device'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_resets_held_streams_min_gain_and_report_stay_per_stream(precision, mode):
    C, B, T = 2, 6, 3
    n = T * 256
    kc, kp = pair(B, C, precision)
    x = interleave(streams(B, 6 * n, seed=17), C)
    parts = [np.ascontiguousarray(x[:, k * n * C:(k + 1) * n * C]) for k in range(6)]

    def both(k, rows=None, **kw):
        got, want = call(kc, parts[k], mode, **kw), planar_call(kp, parts[k], C, **kw)
        if kw.get('report'):
            keep = slice(None) if rows is None else rows
            assert same(got[1][keep], want[1][keep]), k  # report[B][T][4], indexed by stream
            got, want = got[0], want[0]
        if rows is None:
            assert same(got, want), k
        else:
            assert same(deinterleave(got, C)[rows], deinterleave(want, C)[rows]), k

    both(0, report=True)
    reset = np.zeros((B, T), np.uint8)
    reset[1, 1] = 1  # channel 1 of group 0 alone, in the middle of the call
    both(1, reset=reset)
    hold = np.zeros(B, np.uint8)
    hold[2] = 1  # channel 0 of group 1
    others = np.flatnonzero(hold == 0)
    both(2, rows=others, hold=hold, report=True)
    both(3)  # the held stream continues bit for bit (the planar handle's held stream does, by its own tests)
    for k in (kc, kp):
        k.set_min_gain([0.5], streams=[5])  # channel 1 of group 2
    both(4, report=True)
    both(5)
    kc.delete(), kp.delete()


# ------------------------------------------------------------------------------------------------ 6. records

def test_records_move_between_channel_and_planar_handles():
    C, B, T = 2, 6, 3
    n = T * 256
    model = model_file('random')
    kc = koala_amd.create_batch('key', B, T, 'fp32', model_path=model, channels=C)
    kp = koala_amd.create_batch('key', 4, T, 'fp32', model_path=model)
    assert kc.state_size == kp.state_size
    planar = streams(B, 3 * n, seed=31)
    whole = deinterleave(np.concatenate([kc.process(interleave(planar[:, k * n:(k + 1) * n], C)) for k in range(3)], axis=1), C)
    kc.reset()
    kc.process(interleave(planar[:, :n], C))
    kp.import_state(kc.export_state(streams=[3, 0]), streams=[1, 2])  # stream 3 = channel 1 of group 1
    feed = np.zeros((4, n), np.int16)
    feed[1], feed[2] = planar[3, n:2 * n], planar[0, n:2 * n]
    got = kp.process(feed)
    assert np.array_equal(got[1], whole[3, n:2 * n]) and np.array_equal(got[2], whole[0, n:2 * n])
    # ... and back, into other slots: channel 0 of group 2 continues stream 3, channel 1 of group 0 continues stream 0
    kc.reset()
    kc.import_state(kp.export_state(streams=[1, 2]), streams=[4, 1])
    feed = np.zeros((B, n), np.int16)
    feed[4], feed[1] = planar[3, 2 * n:], planar[0, 2 * n:]
    got = deinterleave(kc.process(interleave(feed, C)), C)
    assert np.array_equal(got[4], whole[3, 2 * n:]) and np.array_equal(got[1], whole[0, 2 * n:])
    kc.delete(), kp.delete()


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_asynchronous_calls_are_refused_by_message():
    C, B, T = 2, 6, 3
    kc = koala_amd.create_batch('key', B, T, 'fp32', model_path=model_file('random'), channels=C)
    a, b = kc.alloc_host(T), kc.alloc_host(T)  # [B, T F]: the same bytes as [G, T F C]
    a[:] = 0
    with pytest.raises(KoalaInvalidArgumentError, match='channels'):
        kc.process_async(a, b)
    with pytest.raises(KoalaInvalidArgumentError, match='channels'):
        kc.process_async_resets(a, b, np.zeros((B, T), np.uint8))
    with pytest.raises(KoalaInvalidArgumentError, match='channels'):
        kc.process_async_call(a, b)  # pv_koala_batch_process_call with asynchronous = 1
    kc.synchronize()
    kc.delete()


def test_the_c_entry_refuses_bad_channels_and_one_channel_is_init_config():
    lib = ctypes.CDLL(koala_amd.default_library_path())
    lib.pv_koala_batch_init_channels.argtypes = [ctypes.c_char_p] * 3 + [ctypes.POINTER(BatchConfig), ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    lib.pv_koala_batch_init_config.argtypes = [ctypes.c_char_p] * 3 + [ctypes.POINTER(BatchConfig), ctypes.POINTER(ctypes.c_void_p)]
    lib.pv_koala_batch_channels.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
    lib.pv_koala_batch_process_chunk.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.pv_koala_batch_delete.argtypes = [ctypes.c_void_p]
    lib.pv_koala_batch_delete.restype = None
    lib.pv_get_error_stack.argtypes = [ctypes.POINTER(ctypes.POINTER(ctypes.c_char_p)), ctypes.POINTER(ctypes.c_int32)]
    lib.pv_free_error_stack.argtypes = [ctypes.POINTER(ctypes.c_char_p)]
    lib.pv_free_error_stack.restype = None
    model = model_file('random').encode()

    def message():
        stack, depth = ctypes.POINTER(ctypes.c_char_p)(), ctypes.c_int32()
        assert lib.pv_get_error_stack(ctypes.byref(stack), ctypes.byref(depth)) == 0
        text = ' '.join(stack[i].decode() for i in range(depth.value))
        lib.pv_free_error_stack(stack)
        return text

    def make(B, channels, via_config=False):
        config = BatchConfig(ctypes.sizeof(BatchConfig), B, 3, 0, 0, 16000, 0)
        h = ctypes.c_void_p()
        if via_config:
            st = lib.pv_koala_batch_init_config(b'key', model, b'best', ctypes.byref(config), ctypes.byref(h))
        else:
            st = lib.pv_koala_batch_init_channels(b'key', model, b'best', ctypes.byref(config), channels, ctypes.byref(h))
        return st, h

    for B, channels in ((6, 0), (6, 9), (6, -1), (5, 2)):
        st, h = make(B, channels)
        assert st == PicovoiceStatuses.INVALID_ARGUMENT.value and not h.value, (B, channels)
        assert 'channels' in message(), (B, channels)
    st, h = make(0, 2)  # what init_config refuses stays refused with its own text
    assert st == PicovoiceStatuses.INVALID_ARGUMENT.value and 'num_streams' in message()
    x = streams(6, 768, seed=2)
    outs = []
    for via_config in (False, True):
        st, h = make(6, 1, via_config)
        assert st == 0
        c = ctypes.c_int32(-1)
        assert lib.pv_koala_batch_channels(h, ctypes.byref(c)) == 0 and c.value == 1
        y = np.empty_like(x)
        assert lib.pv_koala_batch_process_chunk(h, 3, x.ctypes.data, y.ctypes.data) == 0
        outs.append(y)
        lib.pv_koala_batch_delete(h)
    assert np.array_equal(outs[0], outs[1]) and outs[0].any()
    st, h = make(6, 3)
    c = ctypes.c_int32(-1)
    assert st == 0 and lib.pv_koala_batch_channels(h, ctypes.byref(c)) == 0 and c.value == 3
    lib.pv_koala_batch_delete(h)


# ------------------------------------------------------------------------------------------------ 8. other handles untouched

def test_a_planar_handle_made_after_a_channel_handle_gives_the_same_samples():
    B, T = 6, 3
    model = model_file('random')
    x = streams(B, 2 * T * 256, seed=41)
    before = koala_amd.create_batch('key', B, T, 'fp32', model_path=model)
    want = np.concatenate([before.process(np.ascontiguousarray(x[:, k * T * 256:(k + 1) * T * 256])) for k in range(2)], axis=1)
    kc = koala_amd.create_batch('key', B, T, 'fp32', model_path=model, channels=2)
    kc.process(interleave(x[:, :T * 256], 2))
    after = koala_amd.create_batch('key', B, T, 'fp32', model_path=model)
    assert after.channels == 1
    got = np.concatenate([after.process(np.ascontiguousarray(x[:, k * T * 256:(k + 1) * T * 256])) for k in range(2)], axis=1)
    assert np.array_equal(got, want)
    for k in (before, kc, after):
        k.delete()


# ------------------------------------------------------------------------------------------------ the demo

def test_the_stream_demo_filters_a_stereo_wav_like_the_planar_packet_handle(tmp_path):
    import wave
    from koala_amd.demo import koala_demo_stream
    C, rate, n = 2, 44100, 882  # (the demo's packets: 20 ms)
    planar = streams(C, 5 * n + 300, seed=51)  # a last packet that is not full
    src, dst = str(tmp_path / 'in.wav'), str(tmp_path / 'out.wav')
    with wave.open(src, 'wb') as w:
        w.setnchannels(C), w.setsampwidth(2), w.setframerate(rate)
        w.writeframes(interleave(planar, C).astype('<i2').tobytes())
    assert koala_demo_stream.main(['--input_path', src, '--output_path', dst, '--sample_rate', str(rate), '--channels', str(C),
                                   '--model_path', model_file('random')]) == 0
    with wave.open(dst, 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (C, 2, rate, planar.shape[1])
        got = np.frombuffer(w.readframes(w.getnframes()), '<i2').reshape(1, -1)
    kp = koala_amd.create_batch('key', C, 1, 'fp32', model_path=model_file('random'), sample_rate=rate, packet_samples=n)
    want = []
    for t in range(0, planar.shape[1], n):
        part = np.zeros((C, n), np.int16)
        m = min(n, planar.shape[1] - t)
        part[:, :m] = planar[:, t:t + m]
        want.append(kp.process_packets(part, [m] * C)[:, :m])
    kp.delete()
    assert np.array_equal(got, interleave(np.concatenate(want, axis=1), C))
    with pytest.raises(ValueError, match='channels'):
        koala_demo_stream.main(['--input_path', src, '--output_path', dst, '--sample_rate', str(rate), '--channels', '2', '--meter', '4'])
