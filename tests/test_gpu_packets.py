"""
Packet handles (include/pv_koala_batch.h: pv_koala_batch_init_packets, pv_koala_batch_process_packets; DESIGN.md section 2, fourth extension)
on a real MI355X: koala_amd/csrc/kns_packet.hip's two kernels around the unchanged frame call, through the product library.

The reference is a FRAME handle of the same model, precision and rate:
  - fed the same sub-call schedule (koala_amd.packets.plan: the same process_chunk_hold cuts) the packet handle's output is == in both
    precisions -- the kernels and the call sequence are the same;
  - fed the same samples in plain calls it is == in fp32 (FP32_TOL = 0) and within the suite's own bars in bf16 (BF16_TOL, BF16_WITHIN_1,
    quoted from tests/test_gpu_parity.py: the bars of a bf16 handle against the bf16 oracle).
Report rows: fp32 ==; bf16 e_in exact, the others to the bars quoted from tests/test_gpu_frame_report.py.
"""
import ctypes
import functools

import numpy as np
import pytest

import koala_amd
import sample_rate_recipe as srr
from conftest import model_file, synth_streams
from frame_report_recipe import BF16_E_OUT_REL, BF16_MEAN_GAIN_ABS
from gpu_kit import BF16_TOL, BF16_WITHIN_1, FP32_TOL, flen
from koala_amd import KoalaInvalidArgumentError, packets
from koala_amd._batch import BatchPackets
from koala_amd._koala import PicovoiceStatuses

pytestmark = pytest.mark.gpu

DELAY = {8000: 176, 16000: 256, 48000: 912, 32000: 608}  # the frame handles' delay_sample (include/pv_koala_batch.h)
FRAMES = 10
RATE_PREC = [(r, p) for r in (8000, 16000, 48000) for p in ('fp32', 'bf16')]


def packet_handle(model, B, N, precision, rate=16000):
    return koala_amd.create_batch('key', B, 1, precision, model_path=model, sample_rate=rate, packet_samples=N)


def frame_handle(model, B, T, precision, rate=16000):
    return koala_amd.create_batch('key', B, T, precision, model_path=model, sample_rate=rate)


def signal(B, rate, frames=FRAMES, seed=21):
    F = flen(rate)
    return np.ascontiguousarray(synth_streams(B, frames * F // 256 + 1, seed=seed)[:, :frames * F])


def schedule(B, n, pattern, rate, seed=0):
    """a list of counts arrays [B] that hand every stream its n samples, the streams deliberately out of phase"""
    rng = np.random.default_rng(seed)
    P = {'10ms': rate // 100, '20ms': rate // 50, 'random': 3 * flen(rate) // 2, 'ones': 1}[pattern]
    left = np.full(B, n)
    # the first packet of stream b is b's own phase: from then on the streams' fills differ
    first = (np.arange(B) * 37) % (P + 1)  # ('ones': 0 or 1 sample; the stalls below then spread the phases)
    out = [np.minimum(first, left)]
    left = left - out[0]
    while left.any():
        if pattern == 'random':
            c = rng.integers(0, P + 1, B) * (rng.random(B) > 0.2)
        else:
            c = np.full(B, P) * (rng.random(B) > 0.1)  # now and then a stream stalls
        c = np.minimum(c, left)
        out.append(c)
        left = left - c
    return [c.astype(np.int32) for c in out], max(int(max(c.max() for c in out)), 1)


def run_packets(kb, x, counts_list, N, mode='host', report=False, restart_first=None):
    """feeds x [B, n] by the schedule -> (out [B, n], frames per call, report rows per stream)"""
    B = x.shape[0]
    pos = np.zeros(B, int)
    got = [[] for _ in range(B)]
    rows = [[] for _ in range(B)]
    frames_seen = []
    for i, counts in enumerate(counts_list):
        pcm = np.zeros((B, N), np.int16)
        for b in range(B):
            pcm[b, :counts[b]] = x[b, pos[b]:pos[b] + counts[b]]
        restart = restart_first if i == 0 else None
        if mode == 'host':
            if report:
                out, fr, rep = kb.process_packets(pcm, counts, restart=restart, report=True)
            else:
                out = kb.process_packets(pcm, counts, restart=restart)
        else:
            import torch
            xd = torch.from_numpy(pcm).cuda()
            yd = xd if mode == 'inplace' else torch.full_like(xd, -7)
            R = N // kb.frame_length + 1
            rd = torch.full((B, R, 4), -1.0, dtype=torch.float32, device='cuda') if report else None
            torch.cuda.synchronize()
            fr = kb.process_device_packets(N, counts, xd.data_ptr(), yd.data_ptr(), restart, rd.data_ptr() if report else 0, R if report else 0)
            kb.synchronize()
            out = yd.cpu().numpy()
            rep = rd.cpu().numpy() if report else None
            if mode == 'device':  # nothing past counts[b] is written
                assert all((out[b, counts[b]:] == -7).all() for b in range(B))
        for b in range(B):
            got[b].append(out[b, :counts[b]].copy())
            if report:
                rows[b].append(rep[b, :fr[b]].copy())
        if report:
            frames_seen.append(np.asarray(fr).copy())
        pos += counts
    assert (pos == x.shape[1]).all()
    return np.stack([np.concatenate(g) for g in got]), frames_seen, [np.concatenate(r) if r else None for r in rows]


def run_frames_by_plan(kf, x, counts_list, max_frames):
    """the frame handle fed the packet handle's own sub-call schedule -> e [B, K F] per stream"""
    B, F = x.shape[0], kf.frame_length
    fill, done = np.zeros(B, int), np.zeros(B, int)
    e = [[] for _ in range(B)]
    holds = 0
    for counts in counts_list:
        k, new_fill = packets.frames_due(fill, counts, F)
        for c0, T, hold in packets.plan(k, max_frames):
            pcm = np.zeros((B, T * F), np.int16)
            run_ = np.ones(B, bool) if hold is None else hold == 0
            for b in np.flatnonzero(run_):
                pcm[b] = x[b, done[b] * F:(done[b] + T) * F]
            out = kf.process(pcm) if hold is None else kf.process_hold(pcm, hold)
            holds += hold is not None
            for b in np.flatnonzero(run_):
                e[b].append(out[b])
                done[b] += T
        fill = new_fill
    return e, holds


def behind_zeros(e_b, F, n):
    return np.concatenate([np.zeros(F - 1, np.int16)] + list(e_b))[:n]


def bf16_bars(got, want, what):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print('%s: max distance %d LSB, within 1 LSB %.4f' % (what, int(d.max()), float((d <= 1).mean())))
    assert d.max() <= BF16_TOL and (d <= 1).mean() >= BF16_WITHIN_1, (what, int(d.max()), float((d <= 1).mean()))


# ------------------------------------------------------------------------------------------------ against a frame handle

@pytest.mark.parametrize('B,pattern,mode', [(24, '10ms', 'host'), (24, 'random', 'device'), (832, '10ms', 'device'), (832, '20ms', 'inplace'),
                                            (832, 'random', 'host')])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_packets_are_the_frame_handle_behind_f_minus_1_zeros(random_model, rate, precision, B, pattern, mode):
    F = flen(rate)
    x = signal(B, rate)
    counts_list, N = schedule(B, x.shape[1], pattern, rate, seed=B)
    kp = packet_handle(random_model, B, N, precision, rate)
    kf = frame_handle(random_model, B, kp.max_frames_per_call, precision, rate)
    try:
        assert kp.delay_sample == DELAY[rate] + F - 1 and kp.frame_length == F and kp.sample_rate == rate
        assert kp.state_size == kf.state_size + (4 + 2 * (F - 1) + 15) // 16 * 16
        got, _, _ = run_packets(kp, x, counts_list, N, mode)
        e, holds = run_frames_by_plan(kf, x, counts_list, kp.max_frames_per_call)
        assert holds >= len(counts_list) // 4, (holds, len(counts_list))  # the schedule does exercise sub-calls with holds
        want = np.stack([behind_zeros(e[b], F, x.shape[1]) for b in range(B)])
        assert np.array_equal(got, want), 'same sub-call schedule'
        kf.reset()
        T = kp.max_frames_per_call
        plain = np.concatenate([kf.process(np.ascontiguousarray(x[:, t * F:(t + T) * F])) for t in range(0, FRAMES - FRAMES % T, T)] +
                               ([kf.process(np.ascontiguousarray(x[:, (FRAMES - FRAMES % T) * F:]))] if FRAMES % T else []), axis=1)
        want = np.concatenate([np.zeros((B, F - 1), np.int16), plain], axis=1)[:, :x.shape[1]]
        if precision == 'fp32':
            assert np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= FP32_TOL, 'plain calls'
        else:
            bf16_bars(got, want, 'plain calls %d Hz B=%d %s' % (rate, B, pattern))
    finally:
        kp.delete()
        kf.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_one_sample_packets(random_model, precision):
    B, F = 5, 256
    x = signal(B, 16000, frames=3)
    counts_list, N = schedule(B, x.shape[1], 'ones', 16000)
    kp, kf = packet_handle(random_model, B, 1, precision), frame_handle(random_model, B, 1, precision)
    try:
        got, _, _ = run_packets(kp, x, counts_list, N, 'device')
        e, _ = run_frames_by_plan(kf, x, counts_list, 1)
        assert np.array_equal(got, np.stack([behind_zeros(e[b], F, x.shape[1]) for b in range(B)]))
    finally:
        kp.delete()
        kf.delete()


# ------------------------------------------------------------------------------------------------ pure delay

NCLS = 4  # distinct streams of the pure-delay test; a batch repeats them so that the numpy side stays small


@functools.lru_cache(maxsize=None)
def delayed_input(rate, frames):
    """(x [NCLS, frames F], x through a frame handle that is a pure delay), in numpy alone: at 16 kHz x one frame later, at another rate
    tests/sample_rate_recipe.py's two stages around that delay (precision plays no part in either)"""
    x = signal(NCLS, rate, frames=frames, seed=3)
    if rate == 16000:
        return x, np.concatenate([np.zeros((NCLS, 256), np.int16), x], axis=1)[:, :x.shape[1]]
    return x, srr.Recipe(None, NCLS, 'fp32', rate).process(x)


@pytest.mark.parametrize('pattern', ['10ms', '20ms', 'random', 'ones'])
@pytest.mark.parametrize('kind', ['unity', 'min_gain'])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_unity_mask_is_a_pure_delay(random_model, unity_model, rate, precision, kind, pattern):
    F = flen(rate)
    B, frames = (5, 3) if pattern == 'ones' else (40, FRAMES)  # (one-sample packets: a call per sample)
    x4, delayed4 = delayed_input(rate, frames)
    cls = np.arange(B) % NCLS
    x, n = np.ascontiguousarray(x4[cls]), x4.shape[1]
    counts_list, N = schedule(B, n, pattern, rate, seed=7)
    model = unity_model if kind == 'unity' else random_model
    kp, kf = packet_handle(model, B, N, precision, rate), frame_handle(model, B, frames, precision, rate)
    try:
        if kind == 'min_gain':
            kp.set_min_gain(1.0)
            kf.set_min_gain(1.0)
        got, _, _ = run_packets(kp, x, counts_list, N, 'device')
        d = kp.delay_sample
        assert d == {8000: 303, 16000: 511, 48000: 1679}[rate] == DELAY[rate] + F - 1
        # the input delayed by delay_sample = D + F - 1, bit for bit: the reference is numpy's, F - 1 zeros in front of the delay by D
        want = np.concatenate([np.zeros((B, F - 1), np.int16), delayed4[cls]], axis=1)[:, :n]
        assert np.array_equal(got, want)
        if rate == 16000:  # (there the delay by D is a shift and nothing else)
            assert not got[:, :d].any() and np.array_equal(got[:, d:], x[:, :n - d])
        # and the frame handle's own pure delay behind F - 1 zeros
        want = np.concatenate([np.zeros((B, F - 1), np.int16), kf.process(x)], axis=1)[:, :n]
        assert np.array_equal(got, want)
    finally:
        kp.delete()
        kf.delete()


# ------------------------------------------------------------------------------------------------ stalls, resets, records

@pytest.mark.parametrize('rate,precision', [(16000, 'fp32'), (48000, 'bf16')])
def test_a_stalled_stream_is_not_advanced_bit_for_bit(random_model, rate, precision):
    B, N = 12, 500
    x = signal(B, rate)
    kp = packet_handle(random_model, B, N, precision, rate)
    try:
        kp.process_packets(x[:, :N], np.full(B, 333, np.int32))
        before = kp.export_state()
        counts = np.where(np.arange(B) % 3 == 0, 0, 480).astype(np.int32)
        kp.process_packets(x[:, 333:333 + N], counts)
        after = kp.export_state()
        stalled = counts == 0
        assert np.array_equal(before[stalled], after[stalled]) and not any(np.array_equal(before[b], after[b]) for b in np.flatnonzero(~stalled))
        kp.process_packets(x[:, :N], np.zeros(B, np.int32))  # every stream stalled: no work at all
        assert np.array_equal(kp.export_state(), after)
    finally:
        kp.delete()


def feed(kp, y, counts_list, N, who, restart=None):
    """the streams of `who` take y by the schedule, the others stall -> their outputs; `restart` rides on the first call"""
    B = y.shape[0]
    pos, got = np.zeros(B, int), [[] for _ in range(B)]
    for i, counts in enumerate(counts_list):
        c = np.where(who, counts, 0).astype(np.int32)
        pcm = np.zeros((B, N), np.int16)
        for b in range(B):
            pcm[b, :c[b]] = y[b, pos[b]:pos[b] + c[b]]
        out = kp.process_packets(pcm, c, restart=restart if i == 0 else None)
        for b in range(B):
            got[b].append(out[b, :c[b]])
        pos += c
    return [np.concatenate(g) for g in got]


@pytest.mark.parametrize('how', ['full', 'masked', 'restart'])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_every_reset_gives_a_fresh_stream(random_model, rate, precision, how):
    B = 9
    x, y = signal(B, rate, seed=1), signal(B, rate, frames=4, seed=2)
    counts_list, N = schedule(B, y.shape[1], '10ms', rate, seed=5)
    N = max(N, 300)
    kp, fresh = packet_handle(random_model, B, N, precision, rate), packet_handle(random_model, B, N, precision, rate)
    try:
        want, _, _ = run_packets(fresh, y, counts_list, N)
        kp.process_packets(x[:, :N], np.full(B, 217, np.int32))  # every stream mid-frame, with history
        who = np.ones(B, bool) if how == 'full' else np.arange(B) % 2 == 0
        before = kp.export_state()
        if how == 'full':
            kp.reset()
        elif how == 'masked':
            kp.reset(who.astype(np.uint8))
        # the streams that are not reset stall from here on: their records must stay what they were
        got = feed(kp, y, counts_list, N, who, restart=who.astype(np.uint8) if how == 'restart' else None)
        for b in np.flatnonzero(who):
            assert np.array_equal(got[b], want[b]), b
        assert np.array_equal(kp.export_state()[~who], before[~who])
    finally:
        kp.delete()
        fresh.delete()


@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_a_stream_moved_mid_frame_continues_sample_for_sample(random_model, rate, precision):
    F = flen(rate)
    x = signal(5, rate)
    n, at = x.shape[1], 3 * F + 101
    counts_list, N = schedule(5, n, '10ms', rate, seed=2)
    a, b, whole = (packet_handle(random_model, 5, N, precision, rate), packet_handle(random_model, 9, N + 40, precision, rate),
                   packet_handle(random_model, 5, N, precision, rate))
    try:
        want, _, _ = run_packets(whole, x, counts_list, N)
        # stream 3 of `a` up to sample `at` (mid-frame), then as stream 7 of `b`, in packets of another size
        first = []
        for t in range(0, at, N):
            c = np.zeros(5, np.int32)
            c[3] = min(N, at - t)
            pcm = np.zeros((5, N), np.int16)
            pcm[3, :c[3]] = x[3, t:t + c[3]]
            first.append(a.process_packets(pcm, c)[3, :c[3]])
        rec = a.export_state([3])
        assert rec.shape == (1, a.state_size) and int(rec[0, 4:8].view('<u4')[0]) == 3
        tail = a.state_size - (4 + 2 * (F - 1) + 15) // 16 * 16  # where the packet part begins: uint32 fill
        assert int(rec[0, tail:tail + 4].view('<u4')[0]) == at % F != 0
        b.import_state(rec, [7])
        rest, M = [], N + 40
        for t in range(at, n, M):
            c = np.zeros(9, np.int32)
            c[7] = min(M, n - t)
            pcm = np.zeros((9, M), np.int16)
            pcm[7, :c[7]] = x[3, t:t + c[7]]
            rest.append(b.process_packets(pcm, c)[7, :c[7]])
        assert np.array_equal(np.concatenate(first + rest), want[3])
    finally:
        for h in (a, b, whole):
            h.delete()


def test_records_of_another_version_or_rate_are_refused_with_the_field_named(random_model):
    a = packet_handle(random_model, 4, 320, 'fp32', 16000)
    f16 = frame_handle(random_model, 4, 1, 'fp32', 16000)
    try:
        a.process_packets(signal(4, 16000)[:, :320], np.full(4, 300, np.int32))
        good = a.export_state()

        def refused(fn, *words):
            with pytest.raises(KoalaInvalidArgumentError) as e:
                fn()
            text = ' '.join(e.value.message_stack)
            for w in words:
                assert w in text, (w, text)
            assert np.array_equal(a.export_state(), good)  # nothing was written

        for version in (1, 2):
            bad = good.copy()
            bad[2, 4:8] = np.frombuffer(np.uint32(version).tobytes(), np.uint8)
            refused(lambda: a.import_state(bad), 'record 2', 'version')
        # a frame handle's own (version 1) record, padded to the size: its header says version 1
        v1 = np.zeros((1, a.state_size), np.uint8)
        v1[0, :f16.state_size] = f16.export_state([0])[0]
        refused(lambda: a.import_state(v1, [1]), 'record 0', 'version')
        bad = good.copy()
        bad[1, 24:28] = np.frombuffer(np.uint32(48000).tobytes(), np.uint8)
        refused(lambda: a.import_state(bad), 'record 1', 'sample_rate')
        bad = good.copy()
        bad[3, f16.state_size:f16.state_size + 4] = np.frombuffer(np.uint32(256).tobytes(), np.uint8)
        refused(lambda: a.import_state(bad), 'record 3', 'fill')
        # and a frame handle keeps refusing what is not its own
        with pytest.raises(KoalaInvalidArgumentError):
            f16.import_state(good[:, :f16.state_size].copy())
        a.import_state(good)
    finally:
        a.delete()
        f16.delete()


# ------------------------------------------------------------------------------------------------ the frame report

@pytest.mark.parametrize('mode', ['host', 'device'])
@pytest.mark.parametrize('rate,precision', RATE_PREC)
def test_report_rows_are_the_frame_handles(random_model, rate, precision, mode):
    B, F = 24, flen(rate)
    x = signal(B, rate)
    counts_list, N = schedule(B, x.shape[1], 'random', rate, seed=4)
    kp, kf = packet_handle(random_model, B, N, precision, rate), frame_handle(random_model, B, FRAMES, precision, rate)
    try:
        _, want = kf.process_call(x, report=True)
        got, frames_seen, rows = run_packets(kp, x, counts_list, N, mode, report=True)
        fill = np.zeros(B, int)
        for counts, fr in zip(counts_list, frames_seen):
            k, fill = packets.frames_due(fill, counts, F)
            assert np.array_equal(fr, k)
        assert max(fr.max() for fr in frames_seen) >= 2
        got_rows = np.stack(rows)
        assert got_rows.shape == want.shape
        assert np.array_equal(got_rows[..., 0], want[..., 0]) and not got_rows[..., 3].any()
        if precision == 'fp32':
            assert np.array_equal(got_rows, want)
        else:
            nz = want[..., 1] != 0
            rel = np.abs(got_rows[..., 1].astype(np.float64)[nz] - want[..., 1][nz]) / want[..., 1][nz]
            mg = np.abs(got_rows[..., 2].astype(np.float64) - want[..., 2]) / 257.0
            print('report %d Hz: e_out max rel %.3g, mask_sum / 257 max abs %.3g' % (rate, rel.max(), mg.max()))
            assert np.array_equal(got_rows[..., 1][~nz], want[..., 1][~nz])
            assert rel.max() <= BF16_E_OUT_REL and mg.max() <= BF16_MEAN_GAIN_ABS
    finally:
        kp.delete()
        kf.delete()


# ------------------------------------------------------------------------------------------------ pointer kinds

@pytest.mark.parametrize('rate,precision', [(16000, 'bf16'), (8000, 'fp32'), (48000, 'bf16')])
def test_host_device_and_in_place_give_the_same_samples(random_model, rate, precision):
    B = 40
    x = signal(B, rate)
    counts_list, N = schedule(B, x.shape[1], 'random', rate, seed=6)
    outs = []
    for mode in ('host', 'device', 'inplace'):
        kp = packet_handle(random_model, B, N, precision, rate)
        try:
            outs.append(run_packets(kp, x, counts_list, N, mode)[0])
        finally:
            kp.delete()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and outs[0].any()


# ------------------------------------------------------------------------------------------------ refusals

def test_refused_calls_leave_all_state_unchanged(random_model):
    B, N, F = 6, 600, 256
    x = signal(B, 16000)
    kp, kf = packet_handle(random_model, B, N, 'fp32'), frame_handle(random_model, B, 2, 'fp32')
    try:
        assert kp.packet_samples == N and kp.max_frames_per_call == 3 and kf.packet_samples == 0
        is_p = ctypes.c_int32(-1)
        for h, v in ((kp, 1), (kf, 0)):
            fn = h._lib.pv_koala_batch_is_packet_handle
            fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int
            assert fn(h._handle, ctypes.byref(is_p)) == 0 and is_p.value == v
        kp.process_packets(x[:, :N], np.full(B, 250, np.int32))
        good = kp.export_state()
        pcm, out = np.ascontiguousarray(x[:, :N]), np.zeros((B, N), np.int16)
        counts, frames = np.full(B, 300, np.int32), np.zeros(B, np.int32)
        rep = np.zeros((B, 4, 4), np.float32)

        def raw(**kw):
            c = BatchPackets(ctypes.sizeof(BatchPackets), N, counts.ctypes.data, pcm.ctypes.data, out.ctypes.data, None, None, 0, frames.ctypes.data)
            for name, v in kw.items():
                setattr(c, name, v)
            return kp._lib.pv_koala_batch_process_packets(kp._handle, ctypes.byref(c))

        def refused(fn, *words):
            out[:] = 0
            with pytest.raises(KoalaInvalidArgumentError) as e:
                kp._check(fn(), 'refused')
            text = ' '.join(e.value.message_stack)
            for w in words:
                assert w in text, (w, text)
            assert np.array_equal(kp.export_state(), good) and not out.any()

        for bad in (-1, N + 1):
            c2 = counts.copy()
            c2[4] = bad
            refused(lambda: raw(counts=c2.ctypes.data), 'counts[4]')
        c3 = np.full(B, 1, np.int32)
        refused(lambda: raw(max_samples=N + 1, counts=c3.ctypes.data), 'max_samples')
        refused(lambda: raw(max_samples=0, counts=c3.ctypes.data), 'max_samples')
        refused(lambda: raw(struct_size=ctypes.sizeof(BatchPackets) - 8), 'struct_size')
        c4 = np.full(B, 600, np.int32)  # 250 + 600: three frames
        refused(lambda: raw(counts=c4.ctypes.data, report=rep.ctypes.data, report_frames=2), 'report_frames')
        # frame entry points on a packet handle
        xf = np.ascontiguousarray(x[:, :F])
        for fn in (lambda: kp.process(xf), lambda: kp.process_hold(xf, np.zeros(B, np.uint8)), lambda: kp.process_resets(xf, np.zeros((B, 1), np.uint8)),
                   lambda: kp.process_call(xf, report=True), lambda: kp.process_async(xf, np.zeros_like(xf)),
                   lambda: kp.process_async_resets(xf, np.zeros_like(xf), None)):
            with pytest.raises(KoalaInvalidArgumentError) as e:
                fn()
            assert 'packet handle' in ' '.join(e.value.message_stack)
            assert np.array_equal(kp.export_state(), good)
        # the packet call on a frame handle
        kf.process(np.ascontiguousarray(x[:, :2 * F]))
        fgood = kf.export_state()
        c = BatchPackets(ctypes.sizeof(BatchPackets), N, counts.ctypes.data, pcm.ctypes.data, out.ctypes.data, None, None, 0, frames.ctypes.data)
        kf._lib.pv_koala_batch_process_packets.argtypes = [ctypes.c_void_p, ctypes.POINTER(BatchPackets)]
        kf._lib.pv_koala_batch_process_packets.restype = PicovoiceStatuses
        with pytest.raises(KoalaInvalidArgumentError) as e:
            kf._check(kf._lib.pv_koala_batch_process_packets(kf._handle, ctypes.byref(c)), 'refused')
        assert 'frame handle' in ' '.join(e.value.message_stack) and np.array_equal(kf.export_state(), fgood)
        with pytest.raises(KoalaInvalidArgumentError):
            kf.process_packets(pcm, counts)
        # and the accepted call still works: the state is intact
        assert raw() is PicovoiceStatuses.SUCCESS and frames.tolist() == [2] * B
    finally:
        kp.delete()
        kf.delete()
