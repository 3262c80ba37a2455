"""
Sample formats of batch handles (include/pv_koala_batch.h: pv_koala_batch_init_config; DESIGN.md section 2, fifth extension) on a real
MI355X: koala_amd/csrc/kns_format.hip's two kernels around the unchanged int16 call, through the product library.

Every comparison is == against  encode(S16 handle(decode(x))):  the S16 handle is created alongside with the same model, precision, rate and
kind and is fed the same call sequence (the inner call is the same kernels on the same int16 input, so there is no tolerance to grant, in
either precision); encode and decode are tests/sample_format_recipe.py.
"""
import ctypes

import numpy as np
import pytest

import koala_amd
import sample_format_recipe as sf
from conftest import model_file
from gpu_kit import call, flen, packet_call, same
from koala_amd import KoalaInvalidArgumentError, KoalaRuntimeError
from koala_amd._batch import BatchConfig
from koala_amd._koala import PicovoiceStatuses

pytestmark = pytest.mark.gpu

CALLS = (1, 3, 16, 2)  # frames per call; max_frames_per_call = 16
TMAX = 16
FMT = {'s16': sf.S16, 'f32': sf.F32, 'ulaw': sf.ULAW, 'alaw': sf.ALAW}
MATRIX = [('f32', 16000), ('ulaw', 16000), ('alaw', 16000), ('ulaw', 8000), ('alaw', 8000), ('f32', 48000)]


def dec(fmt, a):
    return sf.decode(FMT[fmt], a)


def enc(fmt, s):
    return sf.encode(FMT[fmt], s)


def signal(fmt, B, n, seed=7):
    """[B, n] elements of the format: random bytes with all 256 values present; s / 32768 for random int16 plus a row of the edge values"""
    rng = np.random.default_rng(seed)
    if fmt == 'f32':
        x = (rng.integers(-32768, 32768, (B, n)).astype(np.int16).astype(np.float32) * np.float32(1.0 / 32768))
        x[B - 1] = np.resize(sf.F32_EDGES, n)
        return x
    x = rng.integers(0, 256, (B, n)).astype(np.uint8)
    x.ravel()[:256] = rng.permutation(256)
    return x


def pair(model, B, precision, rate, fmt, T=TMAX, packet_samples=0):
    """(the format handle, its S16 twin)"""
    kw = dict(model_path=model, sample_rate=rate, packet_samples=packet_samples)
    return (koala_amd.create_batch('key', B, T, precision, sample_format=fmt, **kw), koala_amd.create_batch('key', B, T, precision, **kw))


# ------------------------------------------------------------------------------------------------ the format matrix

@pytest.mark.parametrize('B', [6, 40])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('fmt,rate', MATRIX)
def test_a_format_handle_is_encode_of_the_s16_handle_of_decode(fmt, rate, precision, B):
    F = flen(rate)
    kf, ks = pair(model_file('random'), B, precision, rate, fmt)
    assert kf.sample_format == fmt and (kf.delay_sample, kf.frame_length, kf.state_size) == (ks.delay_sample, ks.frame_length, ks.state_size)
    x = signal(fmt, B, sum(CALLS) * F)
    for mode in ('host', 'device', 'inplace'):
        kf.reset(), ks.reset()
        t = 0
        for T in CALLS:
            part = np.ascontiguousarray(x[:, t * F:(t + T) * F])
            got, want = call(kf, part, mode), enc(fmt, call(ks, dec(fmt, part), mode))
            assert same(got, want), (mode, t, T)
            t += T
    kf.delete(), ks.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('fmt', ['f32', 'ulaw', 'alaw'])
def test_unity_model_returns_the_input_delayed(fmt, precision):
    B, F = 6, 256
    kf = koala_amd.create_batch('key', B, TMAX, precision, model_path=model_file('unity'), sample_format=fmt)
    D = kf.delay_sample
    assert D == 256
    x = signal(fmt, B, sum(CALLS) * F)
    if fmt == 'f32':
        x[B - 1] = x[0]  # (s / 32768 only: the edge values are not fixed points)
    y = np.concatenate([kf.process(np.ascontiguousarray(x[:, t * F:(t + T) * F])) for t, T in zip(np.cumsum((0,) + CALLS), CALLS)], axis=1)
    want = np.concatenate([enc(fmt, np.zeros((B, D), np.int16)), x[:, :-D]], axis=1)
    if fmt == 'ulaw':  # both zeros decode to 0, which encodes to 0xFF
        assert (x == 0x7F).any()
        want[want == 0x7F] = 0xFF
    assert same(y, want)
    kf.delete()


# ------------------------------------------------------------------------------------------------ what the wrapper must not drop

@pytest.mark.parametrize('mode', ['host', 'device'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('fmt,rate', [('f32', 16000), ('ulaw', 8000)])
def test_report_min_gain_resets_and_held_streams_pass_through(fmt, rate, precision, mode):
    B, F, T = 6, flen(rate), 3
    kf, ks = pair(model_file('random'), B, precision, rate, fmt)
    x = signal(fmt, B, 7 * T * F, seed=11)
    parts = [np.ascontiguousarray(x[:, i * T * F:(i + 1) * T * F]) for i in range(7)]
    rng = np.random.default_rng(5)

    def both(i, rows=slice(None), **kw):
        got, want = call(kf, parts[i], mode, **kw), call(ks, dec(fmt, parts[i]), mode, **kw)
        if kw.get('report'):
            assert same(got[1][rows], want[1][rows]), i  # the rows of the decoded stream
            got, want = got[0], want[0]
        assert same(got[rows], enc(fmt, want)[rows]), i

    both(0, report=True)
    for k in (kf, ks):
        k.set_min_gain(0.25, streams=np.arange(B // 2))
    both(1, report=True)
    resets = (rng.random((B, T)) < 0.4).astype(np.uint8)
    resets[1, 2] = 1
    both(2, reset=resets)
    hold = np.array([0, 1, 0, 0, 1, 0], np.uint8)
    both(3, rows=hold == 0, hold=hold)
    both(4)  # the held streams continue from where they were
    mask = np.array([1, 0, 0, 1, 0, 0], np.uint8)
    kf.reset(mask), ks.reset(mask)
    both(5)
    kf.reset(), ks.reset()
    both(6, report=True)
    kf.delete(), ks.delete()


# ------------------------------------------------------------------------------------------------ packet handles

@pytest.mark.parametrize('mode', ['host', 'device'])
@pytest.mark.parametrize('N', [1, 80, 701])
@pytest.mark.parametrize('fmt,rate', [('f32', 16000), ('ulaw', 8000)])
def test_packet_handles_write_counted_rows_only_and_start_with_encoded_zeros(fmt, rate, N, mode):
    B, F, precision = 6, flen(rate), 'bf16' if N == 80 else 'fp32'
    kf, ks = pair(model_file('random'), B, precision, rate, fmt, T=1, packet_samples=N)
    assert (kf.delay_sample, kf.state_size) == (ks.delay_sample, ks.state_size)
    calls = F + 40 if N == 1 else 12
    x = signal(fmt, B, calls * N, seed=13)
    sentinel_f, sentinel_s = (np.float32(-7.5) if fmt == 'f32' else np.uint8(0x3C)), np.int16(-7)
    rng = np.random.default_rng(17)
    pos, firsts = np.zeros(B, int), [[] for _ in range(B)]
    for i in range(calls):
        counts = (rng.integers(0, N + 1, B) * (rng.random(B) > 0.2)).astype(np.int32)
        if i == 1:
            counts[:] = [0, 1 if N > 1 else 0, N, N, N // 2 | 1, N]
        restart = np.array([0, 0, 1, 0, 0, 1], np.uint8) if i == calls // 2 else None
        pcm = np.zeros((B, N), x.dtype)
        for b in range(B):
            pcm[b, :counts[b]] = x[b, pos[b]:pos[b] + counts[b]]
        got = packet_call(kf, pcm, counts, restart, mode, sentinel_f)[0]
        want = packet_call(ks, dec(fmt, pcm), counts, restart, mode, sentinel_s)[0]
        for b in range(B):
            c = counts[b]
            assert same(got[b, :c], enc(fmt, want[b, :c])), (i, b)
            assert same(got[b, c:], np.full(N - c, sentinel_f)) and (want[b, c:] == sentinel_s).all(), (i, b)  # the rest keeps its bytes
            if i < calls // 2:
                firsts[b].append(got[b, :c])
        pos += counts
    zero = enc(fmt, np.zeros(1, np.int16))[0]
    for b in range(B):  # the leading F - 1 outputs of a stream are encode(0): 0.0f, 0xFF
        head = np.concatenate(firsts[b])[:F - 1]
        assert head.size and same(head, np.full(head.size, zero)), b
    kf.delete(), ks.delete()


# ------------------------------------------------------------------------------------------------ misaligned device pointers

@pytest.mark.parametrize('fmt,offsets', [('ulaw', (1, 15)), ('alaw', (1, 15)), ('f32', (1,))])
def test_device_pointers_aligned_to_the_element_only(fmt, offsets):
    import torch
    B, T, F = 6, 3, 256
    kf = koala_amd.create_batch('key', B, TMAX, 'bf16', model_path=model_file('random'), sample_format=fmt)
    x = signal(fmt, B, T * F, seed=19)
    want = kf.process(x)
    for off in offsets:  # (elements: bytes for the 8-bit formats, one float = 4 bytes)
        kf.reset()
        xin = torch.zeros(x.size + 16 + off, dtype=torch.from_numpy(x).dtype, device='cuda')
        out = torch.zeros_like(xin)
        xin[off:off + x.size] = torch.from_numpy(x).cuda().flatten()
        xs, ys = xin[off:], out[off:]
        assert xs.data_ptr() % 16 == off * x.itemsize % 16
        torch.cuda.synchronize()
        kf.process_device(T, xs.data_ptr(), ys.data_ptr())
        kf.synchronize()
        got = out.cpu().numpy()
        assert same(got[off:off + x.size].reshape(x.shape), want), off
        assert not got[:off].any() and not got[off + x.size:].any(), off
    kf.delete()


# ------------------------------------------------------------------------------------------------ configuration, not state

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_records_move_between_formats(precision):
    B, rate, fmt = 6, 8000, 'ulaw'
    F = flen(rate)
    model = model_file('random')
    kf, ks = pair(model, B, precision, rate, fmt)
    kf2, ks2 = pair(model, B, precision, rate, fmt)
    assert kf.state_size == ks.state_size
    x = signal(fmt, B, 8 * F, seed=23)
    a, b = np.ascontiguousarray(x[:, :5 * F]), np.ascontiguousarray(x[:, 5 * F:])
    assert same(kf.process(a), enc(fmt, ks.process(dec(fmt, a))))
    rec_f, rec_s = kf.export_state(), ks.export_state()
    assert np.array_equal(rec_f, rec_s)  # the record is unchanged, in version and bytes
    ks2.import_state(rec_f)  # mu-law 8 kHz -> S16 8 kHz
    kf2.import_state(rec_s)  # ... and the other way round
    want = ks.process(dec(fmt, b))
    assert same(ks2.process(dec(fmt, b)), want) and same(kf2.process(b), enc(fmt, want)) and same(kf.process(b), enc(fmt, want))
    for k in (kf, ks, kf2, ks2):
        k.delete()


# ------------------------------------------------------------------------------------------------ pv_koala_batch_init_config itself

def init_config(lib, model, B, T, N, precision, rate, fmt, struct_size=None):
    lib.pv_koala_batch_init_config.argtypes = [ctypes.c_char_p] * 3 + [ctypes.POINTER(BatchConfig), ctypes.POINTER(ctypes.c_void_p)]
    lib.pv_koala_batch_init_config.restype = PicovoiceStatuses
    cfg = BatchConfig(ctypes.sizeof(BatchConfig) if struct_size is None else struct_size, B, T, N, 1 if precision == 'bf16' else 0, rate, fmt)
    handle = ctypes.c_void_p()
    return lib.pv_koala_batch_init_config(b'key', model.encode(), b'best', ctypes.byref(cfg), ctypes.byref(handle)), handle


@pytest.mark.parametrize('rate,N', [(16000, 0), (8000, 0), (48000, 0), (8000, 80)])
def test_init_config_with_s16_is_the_existing_constructors_handle(rate, N):
    B, F, precision = 6, flen(rate), 'bf16'
    model = model_file('random')
    kw = dict(model_path=model, sample_rate=rate, packet_samples=N)
    ka, kb = koala_amd.create_batch('key', B, TMAX, precision, **kw), koala_amd.create_batch('key', B, TMAX, precision, **kw)
    # kb's handle is replaced by one that pv_koala_batch_init_config made
    kb._lib.pv_koala_batch_delete(kb._handle)
    status, kb._handle = init_config(kb._lib, model, B, TMAX, N, precision, rate, 0)
    assert status is PicovoiceStatuses.SUCCESS
    value = ctypes.c_int32(-1)
    for name in ('state_size', 'delay_sample', 'sample_format'):
        fn = getattr(kb._lib, 'pv_koala_batch_' + name)
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)], PicovoiceStatuses
        assert fn(kb._handle, ctypes.byref(value)) is PicovoiceStatuses.SUCCESS
        assert value.value == {'state_size': ka.state_size, 'delay_sample': ka.delay_sample, 'sample_format': 0}[name]
    x = dec('s16', signal('ulaw', B, sum(CALLS) * F, seed=29).astype(np.int16) * 200 - 25000)
    t = 0
    for T in CALLS:
        if N:
            part = np.ascontiguousarray(x[:, t * N:(t + 1) * N])
            counts = np.array([N, 0, N // 2, N, 1, N], np.int32)
            assert same(kb.process_packets(part, counts), ka.process_packets(part, counts))
        else:
            part = np.ascontiguousarray(x[:, t * F:(t + T) * F])
            assert same(kb.process(part), ka.process(part))
        t += T
    assert np.array_equal(kb.export_state(), ka.export_state())
    ka.delete(), kb.delete()


def test_refusals_leave_the_streams_as_they_were():
    B, F, fmt = 6, 256, 'alaw'
    model = model_file('random')
    kf, ks = pair(model, B, 'bf16', 16000, fmt)
    x = signal(fmt, B, 4 * F, seed=31)
    a, b = np.ascontiguousarray(x[:, :2 * F]), np.ascontiguousarray(x[:, 2 * F:])
    assert same(kf.process(a), enc(fmt, ks.process(dec(fmt, a))))
    pin, pout = kf.alloc_host(2), kf.alloc_host(2)
    assert pin.dtype == np.uint8
    pin[:] = b
    pout[:] = 0x3C
    for refused in (lambda: kf.process_async(pin, pout), lambda: kf.process_async_resets(pin, pout, np.zeros((B, 2), np.uint8)),
                    lambda: kf.process_async_call(pin, pout)):
        with pytest.raises(KoalaInvalidArgumentError) as e:
            refused()
        assert 'sample format' in str(e.value) or 'sample format' in ' '.join(getattr(e.value, 'message_stack', []) or [])
    kf.synchronize()
    assert (pout == 0x3C).all()  # nothing processed
    assert same(kf.process(b), enc(fmt, ks.process(dec(fmt, b))))  # ... and nothing advanced
    lib = kf._lib
    for kwargs in (dict(fmt=1, struct_size=24), dict(fmt=1, struct_size=0), dict(fmt=4), dict(fmt=-1)):
        status, handle = init_config(lib, model, B, TMAX, 0, 'bf16', 16000, **kwargs)
        assert status is PicovoiceStatuses.INVALID_ARGUMENT and not handle.value, kwargs
    kf.delete(), ks.delete()


# ------------------------------------------------------------------------------------------------ the host-pointer boundary

BOUNDARY_B, BOUNDARY_T = 6, 3
MIXED_KINDS = '`pcm` and `enhanced` must both be host or both be device memory.'


def fill_value(fmt):
    return np.float32(-7.5) if fmt == 'f32' else np.uint8(0x3C)


def packet_report_call(kb, pcm, counts, mode, sentinel, rows=BOUNDARY_T):
    """one packet call with a report, into a sentinel-filled `enhanced` (in place: `pcm` itself) and report -> enhanced, report, frames"""
    N = pcm.shape[1]
    if mode == 'host':
        out, rep = np.full_like(pcm, sentinel), np.full((pcm.shape[0], rows, 4), -1.0, np.float32)
        frames = kb._packets(N, counts, pcm.ctypes.data, out.ctypes.data, None, rep.ctypes.data, rows)
        return out, rep, frames
    import torch
    xd = torch.from_numpy(pcm).cuda()
    yd = xd if mode == 'inplace' else torch.from_numpy(np.full_like(pcm, sentinel)).cuda()
    rd = torch.full((pcm.shape[0], rows, 4), -1.0, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    frames = kb.process_device_packets(N, counts, xd.data_ptr(), yd.data_ptr(), None, rd.data_ptr(), rows)
    kb.synchronize()
    return yd.cpu().numpy(), rd.cpu().numpy(), frames


@pytest.mark.parametrize('packets', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('fmt,rate', [('f32', 16000), ('ulaw', 8000), ('alaw', 48000)])
def test_host_device_and_in_place_are_one_call(fmt, rate, precision, packets):
    B, F = BOUNDARY_B, flen(rate)
    N = 5 * F // 2 if packets else 0  # 2.5 frames: a stream completes 2 or 3 frames of a full packet
    x = signal(fmt, B, 3 * max(N, 2 * F), seed=37)
    sentinel = fill_value(fmt)
    runs = {}
    for mode in ('host', 'device', 'inplace'):
        kb = koala_amd.create_batch('key', B, BOUNDARY_T, precision, model_path=model_file('random'), sample_rate=rate, sample_format=fmt,
                                    packet_samples=N)
        kb.set_min_gain(np.linspace(0.1, 0.6, B))
        outs, reps = [], []
        if packets:
            rng = np.random.default_rng(41)
            pos, fill = np.zeros(B, int), np.zeros(B, int)
            for i in range(3):
                counts = rng.integers(0, N + 1, B).astype(np.int32)
                k = (fill + counts) // F
                fill = fill + counts - k * F
                pcm = np.full((B, N), sentinel)  # (beyond counts[b] the sentinel: what an in-place call must leave there too)
                for b in range(B):
                    pcm[b, :counts[b]] = x[b, pos[b]:pos[b] + counts[b]]
                pos += counts
                out, rep, frames = packet_report_call(kb, pcm, counts, mode, sentinel)
                assert np.array_equal(frames, k), (mode, i)
                for b in range(B):  # only the counted elements and the completed frames' rows are written
                    assert same(out[b, counts[b]:], np.full(N - counts[b], sentinel)), (mode, i, b)
                    assert same(rep[b, k[b]:], np.full((BOUNDARY_T - k[b], 4), -1.0, np.float32)), (mode, i, b)
                outs.append(out), reps.append(rep)
        else:
            t = 0
            for T in (1, 3, 2):
                out, rep = call(kb, np.ascontiguousarray(x[:, t * F:(t + T) * F]), mode, report=True)
                outs.append(out), reps.append(rep)
                t += T
        runs[mode] = (outs, reps, kb.export_state())
        kb.delete()
    for mode in ('device', 'inplace'):
        for i in range(3):
            assert same(runs[mode][0][i], runs['host'][0][i]), (mode, i)
            assert same(runs[mode][1][i], runs['host'][1][i]), (mode, i)
        assert np.array_equal(runs[mode][2], runs['host'][2]), mode


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_a_refused_host_call_leaves_caller_and_streams_alone(precision):
    import torch
    B, T, model = BOUNDARY_B, BOUNDARY_T, model_file('random')

    def refuse(kb, error, words, refused, *untouched):
        before = kb.export_state()
        with pytest.raises(error) as e:
            refused()
        assert all(w in str(e.value) for w in words), str(e.value)
        kb.synchronize()
        for a, value in untouched:
            assert same(a, np.full_like(a, value)), words
        assert np.array_equal(kb.export_state(), before), words

    # ---- a format frame handle: A-law at 8 kHz
    fmt, F = 'alaw', flen(8000)
    kf, ks = pair(model, B, precision, 8000, fmt, T=T)
    x = signal(fmt, B, 4 * 2 * F, seed=43)
    parts = iter([np.ascontiguousarray(x[:, i * 2 * F:(i + 1) * 2 * F]) for i in range(4)])

    def accepted():
        part = next(parts)
        assert same(kf.process(part), enc(fmt, ks.process(dec(fmt, part))))

    accepted()
    pcm, out = signal(fmt, B, 2 * F, seed=47), np.full((B, 2 * F), np.uint8(0x3C))
    pcm_d = torch.from_numpy(pcm).cuda()
    torch.cuda.synchronize()
    resets, hold = np.zeros((B, 2), np.uint8), np.array([0, 1, 0, 0, 0, 0], np.uint8)
    resets[2, 0] = 1
    refuse(kf, KoalaInvalidArgumentError, ('held streams', 'resets'),
           lambda: kf._call(2, pcm.ctypes.data, out.ctypes.data, resets, hold, None, False), (out, 0x3C))
    accepted()
    refuse(kf, KoalaRuntimeError, (MIXED_KINDS,),
           lambda: kf._call(2, ctypes.c_void_p(pcm_d.data_ptr()), out.ctypes.data, None, None, None, False), (out, 0x3C))
    accepted()
    kf.delete(), ks.delete()

    # ---- a format packet handle: float32 at 16 kHz
    fmt, F = 'f32', 256
    N = 5 * F // 2
    kf, ks = pair(model, B, precision, 16000, fmt, T=T, packet_samples=N)
    x = signal(fmt, B, 4 * N, seed=53)
    parts = iter([np.ascontiguousarray(x[:, i * N:(i + 1) * N]) for i in range(4)])
    counts = np.array([N, 0, N // 2, N, 1, N], np.int32)
    fill = np.zeros(B, int)

    def accepted_packets():
        part = next(parts)
        got, want = packet_call(kf, part, counts, None, 'host', np.float32(-7.5))[0], packet_call(ks, dec(fmt, part), counts, None, 'host', np.int16(-7))[0]
        for b in range(B):
            assert same(got[b, :counts[b]], enc(fmt, want[b, :counts[b]])), b
        fill[:] = (fill + counts) % F

    accepted_packets()
    pcm, out = signal(fmt, B, N, seed=59), np.full((B, N), np.float32(-7.5))
    pcm_d = torch.from_numpy(pcm).cuda()
    torch.cuda.synchronize()
    kmax = int(((fill + counts) // F).max())
    assert kmax >= 2
    rep = np.full((B, kmax - 1, 4), -1.0, np.float32)
    refuse(kf, KoalaInvalidArgumentError, ('report_frames',),
           lambda: kf._packets(N, counts, pcm.ctypes.data, out.ctypes.data, None, rep.ctypes.data, kmax - 1), (out, -7.5), (rep, -1.0))
    accepted_packets()
    bad = counts.copy()
    bad[4] = N + 1
    refuse(kf, KoalaInvalidArgumentError, ('counts[4]',), lambda: kf._packets(N, bad, pcm.ctypes.data, out.ctypes.data, None, None, 0), (out, -7.5))
    accepted_packets()
    refuse(kf, KoalaInvalidArgumentError, (MIXED_KINDS,),
           lambda: kf._packets(N, counts, ctypes.c_void_p(pcm_d.data_ptr()), out.ctypes.data, None, None, 0), (out, -7.5))
    accepted_packets()
    kf.delete(), ks.delete()
