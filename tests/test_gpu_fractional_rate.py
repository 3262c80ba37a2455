"""
Packet handles at 44 100 and 22 050 Hz on the GPU (include/pv_koala_batch.h: pv_koala_batch_init_config; DESIGN.md section 2, sixth
extension) against tests/fractional_rate_recipe.py: about 40 calls of up to 1000 samples, per-stream counts from {0, 1, 441, 882, random},
the streams out of phase.  fp32 is the recipe sample for sample; bf16 is held to the bar of tests/sample_rate_cases.py -- the largest
distance is at most ceil(BF16_TOL * S) + 1 LSB, S = the out-stage's largest sum of |tap| over an output phase, and the share of samples
further than 1 LSB from the recipe is at most 4 x the share by which the jittered oracle misses it -- and, between two cuttings of one
stream, to the bar of tests/test_gpu_packets.py.  The recipe is pushed once per stream and shared.
"""
import functools
import math
from ctypes import POINTER, byref, c_int32, c_void_p, sizeof

import numpy as np
import pytest

import fractional_rate_recipe as frr
import koala_amd
import packet_recipe as pr
import sample_rate_recipe as srr
from conftest import model_file, synth_streams
from gpu_kit import BF16_TOL, BF16_WITHIN_1
from koala_amd import formats
from oracle import oracle

pytestmark = pytest.mark.gpu

NS = 5                  # streams
N_MAX = 1000            # max_samples
CALLS = 40
DELAY = {44100: 1541, 22050: 771}
RATE_PREC = [(r, p) for r in frr.RATES for p in ('fp32', 'bf16')]


def handle(model, B, precision, rate, N=N_MAX, **kw):
    return koala_amd.create_batch('key', B, 1, precision, model_path=model, sample_rate=rate, packet_samples=N, **kw)


@functools.lru_cache(maxsize=None)
def schedule(seed):
    """CALLS counts arrays [NS]: the first call hands stream b its own b + 1 samples (out of phase from then on), then every stream draws
    from {0, 1, 441, 882, random <= N_MAX}; one call in which every stream's count yields no inner sample; one full row"""
    rng = np.random.default_rng(seed)
    out = [np.arange(1, NS + 1)]
    for i in range(1, CALLS):
        pick = rng.integers(0, 5, NS)
        c = np.choose(pick, [np.zeros(NS, int), np.ones(NS, int), np.full(NS, 441), np.full(NS, 882), rng.integers(0, N_MAX + 1, NS)])
        out.append(c)
    out[7] = np.array([1, 0, 1, 2, 1])
    out[9] = np.full(NS, N_MAX)
    return tuple(c.astype(np.int32) for c in out)


@functools.lru_cache(maxsize=None)
def signal(seed=31):
    n = sum(int(c.max()) for c in schedule(0)) + sum(int(c.max()) for c in schedule(1))
    return np.ascontiguousarray(synth_streams(NS, n // 256 + 2, seed=seed)[:, :n])


def totals(counts_list):
    return np.sum(counts_list, axis=0)


@functools.lru_cache(maxsize=None)
def expected(kind, precision, rate, seed=0, jitter=0):
    """per stream, the recipe pushed in ONE piece (tests/test_fractional_rate.py: any cuts are the one piece) -> [NS] arrays; kind 'unity':
    the inner path as a pure delay of 511 samples"""
    x, n = signal(), totals(schedule(seed))
    oracle.set_jitter(jitter)
    try:
        return tuple(frr.Stream(rate, frr.DelayInner() if kind == 'unity' else frr.oracle_inner(model_file('random', 1234), precision)).push(x[b, :n[b]])
                     for b in range(NS))
    finally:
        oracle.set_jitter(0)


def feed(kb, x, counts_list, mode='host', report=False, restart=None, fmt='s16'):
    """feeds x [B, n] by the schedule -> ([B] output arrays, frames per call, [B] report rows); `restart`: {call index: mask [B]}"""
    B, N = x.shape[0], N_MAX
    pos = np.zeros(B, int)
    got, rows, frames_seen = [[] for _ in range(B)], [[] for _ in range(B)], []
    R = int(frr.inner_samples(N, kb.sample_rate)) // 256 + 1
    for i, counts in enumerate(counts_list):
        counts = np.asarray(counts[:B], np.int32)
        pcm = np.zeros((B, N), x.dtype)
        for b in range(B):
            pcm[b, :counts[b]] = x[b, pos[b]:pos[b] + counts[b]]
        rs = None if restart is None else restart.get(i)
        if mode == 'host':
            if report:
                out, fr, rep = kb.process_packets(pcm, counts, restart=rs, report=True)
            else:
                out = kb.process_packets(pcm, counts, restart=rs)
        else:
            import torch
            xd = torch.from_numpy(pcm).cuda()
            yd = xd if mode == 'inplace' else torch.full_like(xd, 7)
            rd = torch.full((B, R, 4), -1.0, dtype=torch.float32, device='cuda') if report else None
            torch.cuda.synchronize()
            fr = kb.process_device_packets(N, counts, xd.data_ptr(), yd.data_ptr(), rs, rd.data_ptr() if report else 0, R if report else 0)
            kb.synchronize()
            out = yd.cpu().numpy()
            rep = rd.cpu().numpy() if report else None
            if mode == 'device':  # nothing past counts[b] is written
                assert all((out[b, counts[b]:] == 7).all() for b in range(B))
        for b in range(B):
            got[b].append(out[b, :counts[b]].copy())
            if report:
                rows[b].append(rep[b, :fr[b]].copy())
        if report:
            frames_seen.append(np.asarray(fr).copy())
        pos += counts
    return [np.concatenate(g) for g in got], frames_seen, [np.concatenate(r) for r in rows] if report else None


def check(got, want, precision, rate, what, jitter_want=None):
    """prints the figures before it asserts"""
    got, want = np.concatenate(got), np.concatenate(want)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((d > 1).mean())
    print('%s %s %d Hz: max distance %d LSB, share > 1 LSB %.3e' % (what, precision, rate, int(d.max()), share), end='')
    if precision == 'fp32' or jitter_want is None:
        print()
        assert np.array_equal(got, want), what
        return
    bound = math.ceil(BF16_TOL * frr.out_abs_tap_sum(rate)) + 1
    jshare = float((np.abs(np.concatenate(jitter_want).astype(np.int32) - want.astype(np.int32)) > 1).mean())
    print(', bound %d LSB; jittered oracle misses %.3e -> allowed %.3e' % (bound, jshare, 4 * jshare))
    assert d.max() <= bound, (what, int(d.max()), bound)
    assert share <= 4 * jshare, (what, share, jshare)


# ------------------------------------------------------------------------------------------------ the recipe, call after call

@pytest.mark.parametrize('B,mode', [(1, 'host'), (5, 'device'), (5, 'inplace')])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_ragged_calls_are_the_recipe(random_model, rate, precision, B, mode):
    want = expected('random', precision, rate)[:B]
    jit = expected('random', precision, rate, 0, 1)[:B] if precision == 'bf16' else None
    kb = handle(random_model, B, precision, rate)
    try:
        assert (kb.sample_rate, kb.delay_sample, kb.frame_length, kb.packet_samples) == (rate, DELAY[rate], None, N_MAX)
        got, _, _ = feed(kb, signal()[:B], schedule(0), mode)
    finally:
        kb.delete()
    check(got, want, precision, rate, '%dx%s' % (B, mode), jit)


@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_min_gain_one_is_both_stages_around_a_pure_delay(random_model, rate, precision):
    want = expected('unity', precision, rate)
    kb = handle(random_model, NS, precision, rate)
    try:
        kb.set_min_gain(1.0)
        got, _, _ = feed(kb, signal(), schedule(0), 'device')
    finally:
        kb.delete()
    assert np.array_equal(np.concatenate(got), np.concatenate(want))


@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_another_cutting_of_the_same_streams(random_model, rate, precision):
    """the streams of schedule 0 cut by schedule 1 (as far as both reach): fp32 the same samples, bf16 within the bar for other cuts"""
    n = np.minimum(totals(schedule(0)), totals(schedule(1)))
    outs = []
    for seed in (0, 1):
        kb = handle(random_model, NS, precision, rate)
        try:
            got, _, _ = feed(kb, signal(), schedule(seed), 'host')
        finally:
            kb.delete()
        outs.append(np.concatenate([g[:n[b]] for b, g in enumerate(got)]))
    d = np.abs(outs[0].astype(np.int32) - outs[1].astype(np.int32))
    print('%s %d Hz, two cuttings: max distance %d LSB, within 1 LSB %.4f' % (precision, rate, int(d.max()), float((d <= 1).mean())))
    if precision == 'fp32':
        assert np.array_equal(outs[0], outs[1])
    else:
        assert d.max() <= BF16_TOL and (d <= 1).mean() >= BF16_WITHIN_1


# ------------------------------------------------------------------------------------------------ state

@pytest.mark.parametrize('rate', frr.RATES)
def test_a_stalled_stream_continues_bit_for_bit(random_model, rate):
    """stream 1 gets nothing for six calls in a row while the others advance, in fp32 under the model and in bf16 around the pure delay"""
    counts = [c.copy() for c in schedule(0)]
    for i in range(12, 18):
        counts[i][1] = 0
    n = totals(counts)
    for precision, kind in (('fp32', 'random'), ('bf16', 'unity')):
        kb = handle(random_model, NS, precision, rate)
        try:
            if kind == 'unity':
                kb.set_min_gain(1.0)
            got, _, _ = feed(kb, signal(), counts, 'device')
        finally:
            kb.delete()
        want = expected(kind, precision, rate)
        for b in range(NS):
            assert np.array_equal(got[b], want[b][:n[b]]), (precision, b)


@pytest.mark.parametrize('how', ['restart', 'masked', 'full'])
@pytest.mark.parametrize('rate', frr.RATES)
def test_every_reset_gives_a_fresh_stream(random_model, rate, how):
    x, head, tail = signal(), schedule(1)[:11], schedule(0)
    mask = np.array([0, 1, 0, 1, 1], np.uint8) if how != 'full' else np.ones(NS, np.uint8)
    kb = handle(random_model, NS, 'fp32', rate)
    try:
        first, _, _ = feed(kb, x, head, 'host')
        used = totals(head)
        # the streams go on with the samples behind what they were fed; the reset ones must then be fresh streams fed those samples
        n_tail = np.minimum(totals(tail), x.shape[1] - used)
        assert (n_tail == totals(tail)).all()
        xt = np.stack([np.pad(x[b, used[b]:used[b] + n_tail[b]], (0, int(n_tail.max() - n_tail[b]))) for b in range(NS)])
        if how == 'restart':
            second, _, _ = feed(kb, xt, tail, 'host', restart={0: mask})
        else:
            kb.reset(None if how == 'full' else mask)
            second, _, _ = feed(kb, xt, tail, 'host')
    finally:
        kb.delete()
    inner = lambda: frr.oracle_inner(model_file('random', 1234), 'fp32')
    for b in range(NS):
        if mask[b]:
            want = frr.Stream(rate, inner()).push(xt[b, :n_tail[b]])
        else:
            want = frr.Stream(rate, inner()).push(np.concatenate([x[b, :used[b]], xt[b, :n_tail[b]]]))[used[b]:]
        assert np.array_equal(second[b], want), (how, b)


# ------------------------------------------------------------------------------------------------ formats and reports

@pytest.mark.parametrize('fmt', ['ulaw', 'f32'])
def test_a_format_handle_at_44100_is_encode_of_the_s16_handle_of_decode(random_model, fmt):
    rate, counts = 44100, schedule(0)[:16]
    x = signal()
    coded = formats.encode(fmt, x)
    ks, kf = handle(random_model, NS, 'fp32', rate), handle(random_model, NS, 'fp32', rate, sample_format=fmt)
    try:
        assert kf.delay_sample == DELAY[rate] and kf.sample_format == fmt
        want, _, _ = feed(ks, formats.decode(fmt, coded), counts, 'host')
        for mode in ('host', 'device'):
            kf.reset()
            got, _, _ = feed(kf, coded, counts, mode)
            for b in range(NS):
                assert np.array_equal(got[b], formats.encode(fmt, want[b])), (fmt, mode, b)
    finally:
        ks.delete()
        kf.delete()


@pytest.mark.parametrize('rate,mode', [(44100, 'host'), (22050, 'device')])
def test_report_rows_and_frames_are_the_inner_16_khz_streams(random_model, rate, mode):
    """a 16 kHz packet handle fed the recipe's in-stage output, call by call, reports the same rows and the same frame counts"""
    counts, x = schedule(0), signal()
    streams = [frr.Stream(rate, frr.DelayInner()) for _ in range(NS)]
    pos = np.zeros(NS, int)
    inner_counts = []
    for c in counts:
        before = [sum(y.size for y in s.fed) for s in streams]
        for b in range(NS):
            streams[b].push(x[b, pos[b]:pos[b] + c[b]])
        inner_counts.append(np.array([sum(y.size for y in s.fed) - before[b] for b, s in enumerate(streams)], np.int32))
        pos += c
    fed = [np.concatenate(s.fed) for s in streams]
    M = int(frr.inner_samples(N_MAX, rate))
    kb = handle(random_model, NS, 'fp32', rate)
    k16 = koala_amd.create_batch('key', NS, 1, 'fp32', model_path=random_model, packet_samples=M)
    try:
        _, frames, rows = feed(kb, x, counts, mode, report=True)
        ipos, want = np.zeros(NS, int), [[] for _ in range(NS)]
        for i, ic in enumerate(inner_counts):
            pcm = np.zeros((NS, M), np.int16)
            for b in range(NS):
                pcm[b, :ic[b]] = fed[b][ipos[b]:ipos[b] + ic[b]]
            _, fr, rep = k16.process_packets(pcm, ic, report=True)
            assert np.array_equal(fr, frames[i]), i
            for b in range(NS):
                want[b].append(rep[b, :fr[b]].copy())
            ipos += ic
        for b in range(NS):
            w = np.concatenate(want[b])
            assert w.shape[0] >= 15 and np.array_equal(rows[b], w), b
    finally:
        kb.delete()
        k16.delete()


# ------------------------------------------------------------------------------------------------ refusals

def test_refused_calls_leave_all_state_unchanged(random_model):
    rate, counts, x = 44100, schedule(0)[:14], signal()
    kb = handle(random_model, NS, 'fp32', rate)
    try:
        lib, h = kb._lib, kb._handle
        got_a, _, _ = feed(kb, x, counts[:7], 'host')
        buf = np.zeros((NS, 1024), np.int16)
        out = np.full((NS, 1024), 7, np.int16)
        p, q = buf.ctypes.data, out.ctypes.data
        ok = koala_amd._koala.PicovoiceStatuses.SUCCESS
        d = c_int32(-5)
        lib.pv_koala_batch_frame_length.argtypes = [c_void_p, POINTER(c_int32)]
        lib.pv_koala_batch_frame_length.restype = koala_amd._koala.PicovoiceStatuses
        mask = np.zeros(NS, np.uint8)
        recs = np.full((NS, 20000), 0xee, np.uint8)
        lib.pv_koala_batch_process.argtypes = [c_void_p, c_void_p, c_void_p]
        lib.pv_koala_batch_process.restype = koala_amd._koala.PicovoiceStatuses
        calls = [koala_amd._batch.BatchCall(sizeof(koala_amd._batch.BatchCall), 1, p, q, None, None, None, a) for a in (0, 1)]
        refused = [lib.pv_koala_batch_process(h, p, q), lib.pv_koala_batch_process_call(h, byref(calls[0])),
                   lib.pv_koala_batch_process_call(h, byref(calls[1])), lib.pv_koala_batch_process_chunk(h, 1, p, q), lib.pv_koala_batch_process_chunk_async(h, 1, p, q),
                   lib.pv_koala_batch_process_chunk_resets(h, 1, p, q, mask.ctypes.data),
                   lib.pv_koala_batch_process_chunk_resets_async(h, 1, p, q, mask.ctypes.data),
                   lib.pv_koala_batch_process_chunk_hold(h, 1, p, q, mask.ctypes.data),
                   lib.pv_koala_batch_state_size(h, byref(d)), lib.pv_koala_batch_frame_length(h, byref(d)),
                   lib.pv_koala_batch_export_state(h, NS, None, recs.ctypes.data), lib.pv_koala_batch_import_state(h, NS, None, recs.ctypes.data)]
        assert all(s is not ok for s in refused), refused
        assert d.value == -5 and (out == 7).all() and (recs == 0xee).all()
        for bad in (dict(counts=[N_MAX + 1] + [0] * (NS - 1)), dict(counts=[-1] + [0] * (NS - 1))):
            with pytest.raises(koala_amd.KoalaInvalidArgumentError):
                kb.process_packets(np.zeros((NS, N_MAX), np.int16), bad['counts'])
        with pytest.raises(koala_amd.KoalaInvalidArgumentError):
            kb.process_packets(np.zeros((NS, N_MAX + 1), np.int16), [1] * NS)
        with pytest.raises(koala_amd.KoalaInvalidArgumentError):
            kb.export_state()
        used = totals(counts[:7])
        xt = np.stack([np.pad(x[b, used[b]:], (0, int(used[b] - used.min()))) for b in range(NS)])
        got_b, _, _ = feed(kb, xt, counts[7:], 'host')
    finally:
        kb.delete()
    want = expected('random', 'fp32', rate)
    for b in range(NS):
        assert np.array_equal(np.concatenate([got_a[b], got_b[b]]), want[b][:totals(counts)[b]]), b


# ------------------------------------------------------------------------------------------------ the other handles

@pytest.mark.parametrize('rate', [16000, 48000])
def test_packet_handles_at_the_older_rates_are_untouched(random_model, rate):
    F, B, N = rate * 256 // 16000, 3, 1000
    n = 6 * F + 100
    x = np.ascontiguousarray(synth_streams(B, n // 256 + 1, seed=9)[:, :n])
    kb = koala_amd.create_batch('key', B, 1, 'fp32', model_path=random_model, sample_rate=rate, packet_samples=N)
    try:
        got, pos = [[] for _ in range(B)], 0
        for c in (1, 441, 882, 1000, 0, 700):
            c = min(c, n - pos)
            pcm = np.zeros((B, N), np.int16)
            pcm[:, :c] = x[:, pos:pos + c]
            out = kb.process_packets(pcm, [c] * B)
            for b in range(B):
                got[b].append(out[b, :c])
            pos += c
    finally:
        kb.delete()
    for b in range(B):
        if rate == 16000:
            fn = pr.oracle_stream(random_model, 'fp32')
        else:
            rec = srr.Recipe(random_model, 1, 'fp32', rate)
            fn = lambda frames, rec=rec: rec.process(np.ascontiguousarray(frames[None]))[0]
        assert np.array_equal(np.concatenate(got[b]), pr.expected(fn, F, x[b, :pos])), (rate, b)
