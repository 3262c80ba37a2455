"""
Output leveller (include/pv_koala_batch.h, OUTPUT LEVELLER; DESIGN.md section 2, eleventh extension) on a real MI355X: the two launches of
koala_amd/csrc/kns_level.hip behind the 16 kHz call, through every layer above it.

Every test builds a twin handle without the feature, takes E and the frame report from it and compares the levelling handle's output with
koala_amd.level.apply(E, report, ...) -- the rule sees the device's own report, so every comparison is == in both precisions.  On handles
whose samples are not the inner 16 kHz stream's (48 kHz, 8 kHz u-law, 48 kHz packets) E is not visible from outside: there the gains in
column 3 of the report and the state are held to the rule with ==, the streams that are off to the twin's samples, and the samples that
level must differ.  B = 4, calls of 3, 2, 1, 3 frames, the default model, the speech fixture at about -45 dBFS plus noise.
"""
import functools

import numpy as np
import pytest

import gpu_kit
from gpu_kit import DEV_LIB, MARK, cut, route_of, same
from koala_amd import KoalaInvalidArgumentError, channels as chan, formats, level
from level_recipe import B, FRAMES, OTHER, SEQ, SETTING, TMAX, over_calls, quiet_speech, vivid
from packet_recipe import PacketStream
from sample_rate_recipe import STAGES, Stage

pytestmark = pytest.mark.gpu

batch = functools.partial(gpu_kit.batch, lib=DEV_LIB)
call = gpu_kit.call
PRECISIONS = ['fp32', 'bf16']


@functools.lru_cache(maxsize=None)
def _input():
    x = quiet_speech()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _twin(model, precision):
    """(E, report) of the handle without the feature over the call sequence, computed once and left unchanged"""
    kb = batch(model, B, TMAX, precision)
    got = [call(kb, c, 'device', report=True) for c in cut(_input(), 16000, SEQ)]
    kb.delete()
    E, rep = np.concatenate([g[0] for g in got], axis=1), np.concatenate([g[1] for g in got], axis=1)
    assert not rep[..., 3].any()  # the reserved word of a handle that does not level
    E.setflags(write=False)
    rep.setflags(write=False)
    return E, rep


def run(kb, mode, report=True, resets=None, holds=None):
    """the call sequence on a levelling handle -> (out, report or None)"""
    outs, reps = [], []
    for i, c in enumerate(cut(_input(), 16000, SEQ)):
        got = call(kb, c, mode, report=report, reset=None if resets is None else resets[i], hold=None if holds is None else holds[i])
        outs.append(got[0] if report else got)
        reps.append(got[1] if report else None)
    return np.concatenate(outs, axis=1), np.concatenate(reps, axis=1) if report else None


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('mode,report', [('device', True), ('device', False), ('host', True), ('host', False), ('offset', True)])
def test_16k_handle_is_the_rule(gate_model, precision, mode, report):
    E, rep = _twin(gate_model, precision)
    kb = batch(gate_model, B, TMAX, precision, level=SETTING)
    assert kb.level(2) == SETTING
    out, got = run(kb, mode, report)
    state = kb.level_state()
    kb.delete()
    want, gains, wstate = over_calls(E, rep, SETTING, SEQ)
    assert vivid(rep, SETTING, gains) and (want != E).any()  # the device's own report: speech in a third of the frames, a gain of 2 somewhere
    assert same(out, want) and same(state, wstate)
    if report:
        assert same(got[..., :3], rep[..., :3]) and same(got[..., 3], gains)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_mixed_streams_and_a_switch_between_calls(gate_model, precision):
    E, rep = _twin(gate_model, precision)
    first, later = [None, SETTING, OTHER, SETTING], [None, SETTING, OTHER, None]
    kb = batch(gate_model, B, TMAX, precision)
    kb.set_level(first)
    outs, reps = [], []
    for i, c in enumerate(cut(_input(), 16000, SEQ)):
        if i == 2:
            kb.set_level(None, streams=[3])  # stream 3 off from the third call on: its state stays where it is
        o, r = call(kb, c, 'device', report=True)
        outs.append(o)
        reps.append(r)
    out, got, state = np.concatenate(outs, axis=1), np.concatenate(reps, axis=1), kb.level_state()
    kb.delete()
    want, gains, wstate = over_calls(E, rep, {0: first, 1: first, 2: later, 3: later}, SEQ)
    assert same(out, want) and same(state, wstate)
    assert same(out[0], E[0]) and same(out[3, 5 * 256:], E[3, 5 * 256:]) and (out[1] != out[2]).any()
    assert not got[0, :, 3].any() and not got[3, 5:, 3].any() and same(got[1:3, :, 3], gains[1:3]) and same(got[3, :5, 3], gains[3, :5])
    assert state[3, 1] != 1.0 and state[0, 0] == 0.0 and state[0, 1] == 1.0


@pytest.mark.parametrize('precision', PRECISIONS)
def test_hold_reset_and_masked_reset(gate_model, precision):
    x = cut(_input(), 16000, SEQ)
    hold = np.array([0, 1, 0, 0], np.uint8)
    reset = np.zeros((B, 3), np.uint8)
    reset[2, 1] = 1
    mask = np.array([0, 0, 0, 1], np.uint8)
    kb, twin = batch(gate_model, B, TMAX, precision, level=SETTING), batch(gate_model, B, TMAX, precision)
    # call 0 plain; call 1 holds stream 1; a masked reset of stream 3; call 2 plain; call 3 restarts stream 2 at its frame 1
    steps = [dict(), dict(hold=hold), dict(), dict(reset=reset)]
    state, E, rep, out = None, [], [], []
    for i, c in enumerate(x):
        if i == 2:
            kb.reset(mask)
            twin.reset(mask)
            assert same(kb.level_state([3]), level.fresh(1))
            state[3] = (0.0, 1.0)
        before = kb.level_state()
        e, r = call(twin, c, 'device', report=True, **steps[i])
        o = call(kb, c, 'device', **steps[i])
        w, _, state = level.apply(e, r, SETTING, before, steps[i].get('reset'), steps[i].get('hold'))
        after = kb.level_state()
        assert same(after, state)
        live = np.flatnonzero(steps[i].get('hold', np.zeros(B)) == 0)  # (held rows of `out` are unspecified)
        assert same(o[live], w[live])
        if i == 1:
            assert same(after[1], before[1]) and (after[0] != before[0]).any()
        out.append(o)
        E.append(e)
    kb.delete()
    twin.delete()
    assert (np.concatenate(out, axis=1) != np.concatenate(E, axis=1)).any()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_frame_call_then_several(gate_model, precision):
    x = _input()
    kb, twin = batch(gate_model, B, TMAX, precision, level=SETTING), batch(gate_model, B, TMAX, precision)
    state = None
    for t0, t1 in ((0, 3), (3, 4), (4, 7)):
        c = gpu_kit.frames(x, t0, t1)
        e, r = call(twin, c, 'device', report=True)
        o, g = call(kb, c, 'device', report=True)
        if t1 - t0 == 1:
            assert route_of(kb) == route_of(twin)  # the one-frame route of the plain handle, with the two launches behind it
        w, gains, state = level.apply(e, r, SETTING, state)
        assert same(o, w) and same(g[..., 3], gains[:, 1:]) and same(kb.level_state(), state)
    kb.delete()
    twin.delete()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_a_stream_moves_to_another_handle(gate_model, precision):
    x = _input()
    a, moved, twin = batch(gate_model, B, TMAX, precision, level=SETTING), batch(gate_model, 6, 2, precision), batch(gate_model, B, TMAX, precision, level=SETTING)
    moved.set_level(SETTING, streams=[5])
    head = gpu_kit.frames(x, 0, 3)
    call(a, head, 'device')
    call(twin, head, 'device')
    moved.import_state(a.export_state([1]), streams=[5])
    moved.set_level_state(a.level_state([1]), streams=[5])
    assert same(moved.level_state([5]), a.level_state([1])) and same(moved.level_state([0]), level.fresh(1))
    for t0, t1 in ((3, 5), (5, 6), (6, 8)):
        c = gpu_kit.frames(x, t0, t1)
        rows = np.zeros((6, c.shape[1]), np.int16)
        rows[5] = c[1]
        assert same(call(moved, rows, 'device')[5], call(twin, c, 'device')[1])
    assert same(moved.level_state([5]), twin.level_state([1]))
    for h in (a, moved, twin):
        h.delete()


def _outer(model, precision, lvl, **kw):
    return batch(model, B, TMAX, precision, level=lvl, **kw)



@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('rate,fmt', [(48000, 's16'), (8000, 'ulaw')])
def test_rate_and_format_handles(gate_model, precision, rate, fmt):
    """The handle is decode -> in-stage -> 16 kHz call -> leveller -> out-stage -> encode.  The stages are tests/sample_rate_recipe.py's (held
    to the device bit for bit by the sample-rate suite), the 16 kHz call is a twin device handle fed the recipe's in-stage output: E and
    the report are the device's own, and every sample of the levelling handle is compared with =="""
    F = gpu_kit.flen(rate)
    # (the speech at the handle's rate: every sample three times, or every second one -- crude, and the talker is still there)
    pcm = np.repeat(_input(), 3, axis=1) if rate == 48000 else formats.encode(fmt, np.ascontiguousarray(_input()[:, ::2]))
    assert pcm.shape[1] == FRAMES * F
    lvl = [None, SETTING, OTHER, SETTING]
    kb, twin = _outer(gate_model, precision, None, sample_rate=rate, sample_format=fmt), batch(gate_model, B, TMAX, precision)
    kb.set_level(lvl)
    s_in, s_out = (Stage(B, max(U, D), U, D) for U, D in STAGES[rate])
    state, differs = None, False
    for c in cut(pcm, rate, SEQ):
        y = s_in.run(formats.decode(fmt, c))
        E, r = call(twin, y, 'device', report=True)
        w, gains, state = level.apply(E, r, lvl, state)
        want = formats.encode(fmt, s_out.run(w))
        o, g = kb.process_call(c, report=True)
        assert same(o, want) and same(g[..., :3], r[..., :3]) and same(g[1:, :, 3], gains[1:, 1:]) and not g[0, :, 3].any()
        assert same(kb.level_state(), state)
        differs = differs or (w[1:] != E[1:]).any()
    kb.delete()
    twin.delete()
    assert differs and (state[1:, 1] != 1.0).all()  # (the levelled samples are not the plain handle's)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_two_channels_f32_link_off(gate_model, precision):
    x = formats.encode('f32', _input())
    kw = dict(sample_format='f32', channels=2)
    kb, twin = _outer(gate_model, precision, SETTING, **kw), batch(gate_model, B, TMAX, precision, **kw)
    state = None
    for c in cut(x, 16000, SEQ):
        inter = chan.interleave(c, 2)
        e, r = twin.process_call(inter, report=True)
        o, g = kb.process_call(inter, report=True)
        E = formats.decode('f32', chan.deinterleave(e, 2))  # (exact: an f32 sample is an int16 / 32768)
        w, gains, state = level.apply(E, r, SETTING, state)
        assert same(o, chan.interleave(formats.encode('f32', w), 2)) and same(g[..., 3], gains[:, 1:])
    assert (state[:, 1] != 1.0).any()
    kb.delete()
    twin.delete()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_48k_packets_with_a_stall_and_a_restart(gate_model, precision):
    """The packet handle in numpy around the device's own 16 kHz call: tests/packet_recipe.py's packetiser per stream, the engine's plan of
    sub-calls (frames [c0, c1) of the call, the streams with fewer frames held), tests/sample_rate_recipe.py's stages per stream, and a
    16 kHz twin device handle for E and the report.  Every sample, report row and state value of the levelling handle is compared with =="""
    rate, N, F = 48000, 960, 768
    (Ui, Di), (Uo, Do) = STAGES[rate]
    pcm = np.repeat(quiet_speech(B, 8), 3, axis=1)[:, :6 * N]
    kb = _outer(gate_model, precision, SETTING, sample_rate=rate, packet_samples=N)
    twin = batch(gate_model, B, kb.max_frames_per_call, precision)
    done = {}
    ps = [PacketStream(lambda frames, b=b: done.pop(b), F) for b in range(B)]
    s_in, s_out = [Stage(1, max(Ui, Di), Ui, Di) for _ in range(B)], [Stage(1, max(Uo, Do), Uo, Do) for _ in range(B)]
    state, moved = level.fresh(B), False
    for i in range(6):
        counts = np.full(B, N, np.int32)
        restart = np.zeros(B, np.uint8)
        if i in (2, 3):
            counts[1] = 0  # stream 1 stalls for two packets
        if i == 4:
            restart[2] = 1  # stream 2 is fresh before this packet: packetiser, stages, engine and leveller
            ps[2].reset()
            s_in[2].reset([1])
            s_out[2].reset([1])
            twin.reset(restart)
            state[2] = (0.0, 1.0)
        c = np.ascontiguousarray(pcm[:, i * N:(i + 1) * N])
        k = np.array([ps[b].frames_due(int(counts[b])) for b in range(B)])
        y = [s_in[b].run(np.concatenate([ps[b].buf[:ps[b].fill], c[b, :counts[b]]])[None, :k[b] * F]) if k[b] else None for b in range(B)]
        lev, rows = [[] for _ in range(B)], [[] for _ in range(B)]
        cuts = [0] + sorted(set(int(v) for v in k if v > 0))
        for c0, c1 in zip(cuts[:-1], cuts[1:]):  # the engine's sub-calls
            hold = (k < c1).astype(np.uint8)
            x16 = np.zeros((B, (c1 - c0) * 256), np.int16)
            for b in np.flatnonzero(hold == 0):
                x16[b] = y[b][0, c0 * 256:c1 * 256]
            E, r = call(twin, x16, 'device', report=True, hold=hold if hold.any() else None)
            w, gains, state = level.apply(E, r, SETTING, state, hold=hold)
            for b in np.flatnonzero(hold == 0):
                lev[b].append(w[b])
                rows[b].append(np.concatenate([r[b, :, :3], gains[b, 1:, None]], axis=1))
                moved = moved or (w[b] != E[b]).any()
        want = np.zeros_like(c)
        for b in range(B):
            if k[b]:
                done[b] = s_out[b].run(np.concatenate(lev[b])[None])[0]
            want[b, :counts[b]] = ps[b].push(c[b, :counts[b]])
        o, k2, g = kb.process_packets(c, counts, restart, report=True)
        assert same(k2, k.astype(np.int32)) and same(o, want) and same(kb.level_state(), state)
        for b in range(B):
            if k[b]:
                assert same(g[b, :k[b]], np.concatenate(rows[b]).astype(np.float32))
    kb.delete()
    twin.delete()
    assert moved and (state[:, 1] != 1.0).all() and not done


def _refused(kb, fn, *words):
    before = kb.level_state()
    with pytest.raises(KoalaInvalidArgumentError) as e:
        fn()
    text = str(e.value) + ' '.join(getattr(e.value, 'message_stack', []) or [])
    assert all(w in text for w in words), text
    assert same(kb.level_state(), before)


@pytest.mark.parametrize('precision', ['fp32'])
def test_refusals_leave_everything_untouched(gate_model, precision):
    x = gpu_kit.frames(_input(), 0, 1)
    # the channel link
    kb = batch(gate_model, B, TMAX, precision, channels=2, channel_link='max', level=SETTING)
    out = np.full((B // 2, 512), MARK, np.int16)
    _refused(kb, lambda: kb.process_into(chan.interleave(x, 2).reshape(B, -1), out.reshape(B, -1)), 'leveller', 'channel link')
    assert (out == MARK).all()
    kb.set_level(None)
    kb.process(chan.interleave(x, 2))
    kb.delete()
    # the high-band carry
    kb = batch(gate_model, B, TMAX, precision, sample_rate=48000, high_band='carry', level=SETTING)
    big = np.zeros((B, 768), np.int16)
    out = np.full_like(big, MARK)
    _refused(kb, lambda: kb.process_into(big, out), 'leveller', 'high-band carry')
    assert (out == MARK).all()
    kb.delete()
    # the asynchronous entry points
    kb = batch(gate_model, B, TMAX, precision, level=SETTING)
    a, b = kb.alloc_host(1), kb.alloc_host(1)
    a[:] = x
    b[:] = MARK
    _refused(kb, lambda: kb.process_async(a, b), 'leveller', 'asynchronous')
    assert (b == MARK).all()
    kb.delete()
    # 44 100 Hz
    kb = batch(gate_model, B, 1, precision, sample_rate=44100, packet_samples=441, level=SETTING)
    pk = np.zeros((B, 441), np.int16)
    out = np.full_like(pk, MARK)
    _refused(kb, lambda: kb._packets(441, np.full(B, 441, np.int32), pk.ctypes.data, out.ctypes.data, None, None, 0), 'leveller', '44100')
    assert (out == MARK).all()
    kb.delete()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_case_off_is_parent(gate_model, precision):
    """a handle with every stream off gives the bits and the route numbers of a handle that never heard of the feature"""
    E, rep = _twin(gate_model, precision)
    kb = batch(gate_model, B, TMAX, precision, level=SETTING)
    kb.set_level(None)  # every stream off again, and one explicit all-off table
    kb.set_level([None] * B)
    plain = batch(gate_model, B, TMAX, precision)
    outs, reps = [], []
    for c in cut(_input(), 16000, SEQ):
        o, r = call(kb, c, 'device', report=True)
        call(plain, c, 'device', report=True)
        assert route_of(kb) == route_of(plain)
        outs.append(o)
        reps.append(r)
    assert same(np.concatenate(outs, axis=1), E) and same(np.concatenate(reps, axis=1), rep)
    for mode in ('host', 'device'):  # and the host routes: the sub-chunk pipeline and the one-frame graph stay the plain handle's
        for t0, t1 in ((0, 3), (3, 4)):
            c = gpu_kit.frames(_input(), t0, t1)
            assert same(call(kb, c, mode), call(plain, c, mode)) and route_of(kb) == route_of(plain)
    assert same(kb.level_state(), level.fresh(B))
    kb.delete()
    plain.delete()


@pytest.mark.parametrize('precision', ['fp32'])
def test_single_stream_handle(gate_model, precision):
    """Koala.set_level: the one-stream handle of the reference's ABI, frame by frame on host memory, is stream 0 of the batch handle"""
    import koala_amd
    x = np.array(_input()[:1])  # (a writable copy: the device modes hand it to torch)
    k = koala_amd.create('key', model_path=gate_model, library_path=DEV_LIB)
    k.set_level(SETTING)
    assert k.level() == SETTING
    kb = batch(gate_model, 1, 1, precision, level=SETTING)
    got = np.concatenate([np.array(k.process(x[0, t * 256:(t + 1) * 256]), np.int16) for t in range(FRAMES)])
    want = np.concatenate([call(kb, gpu_kit.frames(x, t, t + 1), 'device') for t in range(FRAMES)], axis=1)[0]
    plain = batch(gate_model, 1, 1, precision)
    E = np.concatenate([call(plain, gpu_kit.frames(x, t, t + 1), 'device') for t in range(FRAMES)], axis=1)[0]
    k.delete()
    kb.delete()
    plain.delete()
    assert same(got, want) and (got != E).any()
