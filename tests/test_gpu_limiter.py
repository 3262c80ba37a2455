"""
Peak limiter (include/pv_koala_batch.h, PEAK LIMITER; DESIGN.md section 2, thirteenth extension) on a real MI355X: limit_kernel of
koala_amd/csrc/kns_limit.hip behind the 16 kHz call, in level_apply_kernel's place, through every layer above it.

The level suite's twin method: a twin handle without the feature gives E and the frame report, and the limiting handle's output is compared
with koala_amd.limiter.apply (behind koala_amd.level.track where the stream levels) -- the rule sees the device's own samples and report,
so every comparison is == in both precisions.  The ceiling comes from the twin, c_b = max|E_b| // 4, so every stream engages; delta is
1/1024, so releases cross frame and call boundaries.  Every parity test first asserts on the rule's own output that its case is vivid
(tests/limiter_recipe.py, vivid).  On handles whose samples are not the inner 16 kHz stream's (48 kHz, 8 kHz u-law, 48 kHz packets) E is not
visible from outside: there the streams that are off are held to a twin of the same kind, the limited ones must differ, some g is below 1,
and with c = 32767 and no leveller the whole output is the twin's.  B = 4, calls of 3, 2, 1, 3 frames, the level recipe's input.
"""
import functools

import numpy as np
import pytest

import gpu_kit
from gpu_kit import DEV_LIB, MARK, cut, same
from koala_amd import KoalaInvalidArgumentError, channels as chan, formats, level, limiter
from level_recipe import B, FRAMES, SEQ, TMAX, quiet_speech
from limiter_recipe import over_calls, setting, vivid

pytestmark = pytest.mark.gpu

batch = functools.partial(gpu_kit.batch, lib=DEV_LIB)
call = gpu_kit.call
PRECISIONS = ['fp32', 'bf16']
F32 = np.float32
# the leveller in front of the limiter: 30 dB of boost towards a target near full scale, every frame with energy classed as speech, no
# smoothing -- the gain is at its bound from the second frame on
BOOST = level.settings(target_dbfs=-3.0, max_boost_db=30.0, attack_ms=0.0, slew_ms=0.0, theta=0.0, floor_dbfs=-200.0)
# The input of the leveller-and-limiter test is the level recipe's, four times as loud: at the recipe's -45 dBFS the largest sample the default
# model lets through is 1009, and 30 dB of boost (x 31.62) takes that to 31 907 -- the product cannot pass 32767, which that test has to assert
LOUD = 4


@functools.lru_cache(maxsize=None)
def _input(rows=B, loud=1):
    x = np.clip(quiet_speech(rows).astype(np.int64) * loud, -32768, 32767).astype(np.int16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _twin(model, precision, rows=B, loud=1):
    """(E, report) of the handle without the feature over the call sequence, computed once and left unchanged"""
    kb = batch(model, rows, TMAX, precision)
    got = [call(kb, c, 'device', report=True) for c in cut(_input(rows, loud), 16000, SEQ)]
    kb.delete()
    E, rep = np.concatenate([g[0] for g in got], axis=1), np.concatenate([g[1] for g in got], axis=1)
    E.setflags(write=False)
    rep.setflags(write=False)
    return E, rep


def ceilings(E):
    """one setting per stream, c_b = max|E_b| // 4"""
    c = np.abs(E.astype(np.int64)).max(axis=1) // 4
    assert (c >= 1).all()
    return [setting(v) for v in c]


def run(kb, x, mode='device', report=False, before=None):
    """the call sequence -> (out, report or None); before(i): what happens in front of call i"""
    outs, reps = [], []
    for i, c in enumerate(cut(x, 16000, SEQ)):
        if before:
            before(i)
        got = call(kb, c, mode, report=report)
        outs.append(got[0] if report else got)
        reps.append(got[1] if report else None)
    return np.concatenate(outs, axis=1), np.concatenate(reps, axis=1) if report else None


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('mode,report', [('device', True), ('device', False), ('host', True), ('host', False), ('offset', True), ('offset', False)])
def test_limiter_alone_is_the_rule(gate_model, precision, mode, report):
    E, rep = _twin(gate_model, precision)
    lim = ceilings(E)
    want, G, ends, wstate, _, _ = over_calls(E, lim, SEQ)
    assert vivid(G, ends) and (want != E).any()
    kb = batch(gate_model, B, TMAX, precision)
    kb.set_limiter(lim)
    assert kb.limiter(2) == lim[2] and same(kb.limiter_state(), limiter.fresh(B))
    out, got = run(kb, _input(), mode, report)
    state = kb.limiter_state()
    kb.delete()
    assert same(out, want) and same(state, wstate)
    assert (np.abs(out.astype(np.int64)).max(axis=1) <= [s.ceiling for s in lim]).all()
    if report:
        assert same(got, rep)  # untouched: column 3 stays the leveller's, 0 on a handle that does not level


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('mode', ['device', 'host', 'offset'])
def test_leveller_and_limiter_together(gate_model, precision, mode):
    E, rep = _twin(gate_model, precision, B, LOUD)
    lim = ceilings(E)
    want, G, ends, wstate, wlevel, gains = over_calls(E, lim, SEQ, rep, BOOST)
    start, end, _, _ = level.track(rep, BOOST)
    v = np.abs(E.reshape(B, FRAMES, 256).astype(np.float64)) * np.minimum(start, end)[:, :, None]
    print('max |v| at least %.0f, largest leveller gain %.2f' % (v.max(), gains.max()))
    assert v.max() > 32767  # the product passes the rails: what the limiter holds back, saturation would have clipped
    saturated, _, _ = level.apply(E, rep, BOOST)
    assert vivid(G, ends) and (want != saturated).any()
    kb = batch(gate_model, B, TMAX, precision, level=BOOST, limiter=None)
    kb.set_limiter(lim)
    out, got = run(kb, _input(B, LOUD), mode, True)
    state, lstate = kb.limiter_state(), kb.level_state()
    kb.delete()
    assert same(out, want) and same(state, wstate) and same(lstate, wlevel)
    assert (np.abs(out.astype(np.int64)).max(axis=1) <= [s.ceiling for s in lim]).all()
    assert same(got[..., :3], rep[..., :3]) and same(got[..., 3], gains)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_mixed_streams_and_a_switch_between_calls(gate_model, precision):
    """streams {off, limiter, leveller, both}; stream 3's limiter is switched off from the third call on, and its g stays"""
    E, rep = _twin(gate_model, precision, B, LOUD)
    c = ceilings(E)
    lev = [None, None, BOOST, BOOST]
    first, later = [None, c[1], None, c[3]], [None, c[1], None, None]
    want, G, ends, wstate, wlevel, gains = over_calls(E, {0: first, 1: first, 2: later, 3: later}, SEQ, rep, lev)
    assert vivid(G, ends) and ends[1, 3] < 1
    kb = batch(gate_model, B, TMAX, precision)
    kb.set_level(lev)
    kb.set_limiter(first)
    out, got = run(kb, _input(B, LOUD), 'device', True, before=lambda i: kb.set_limiter(None, streams=[3]) if i == 2 else None)
    state, lstate = kb.limiter_state(), kb.level_state()
    kb.delete()
    assert same(out, want) and same(state, wstate) and same(lstate, wlevel)
    assert same(out[0], E[0]) and state[0] == 1 and state[2] == 1 and state[3] == ends[1, 3]
    levelled, _, _ = level.apply(E, rep, lev)
    assert same(out[2], levelled[2]) and same(out[3, 5 * 256:], levelled[3, 5 * 256:]) and (out[3, :5 * 256] != levelled[3, :5 * 256]).any()
    assert same(got[..., 3], np.where(np.array([0, 0, 1, 1])[:, None] != 0, gains, F32(0)).astype(F32))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_five_streams_a_ragged_last_workgroup(gate_model, precision):
    E, rep = _twin(gate_model, precision, 5)
    lim = ceilings(E)
    want, G, ends, wstate, _, _ = over_calls(E, lim, SEQ)
    assert vivid(G, ends)
    kb = batch(gate_model, 5, TMAX, precision)
    kb.set_limiter(lim)
    out, _ = run(kb, _input(5))
    state = kb.limiter_state()
    kb.delete()
    assert same(out, want) and same(state, wstate)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_hold_resets_and_state_that_travels(gate_model, precision):
    x = cut(_input(), 16000, SEQ)
    E, _ = _twin(gate_model, precision)
    lim = ceilings(E)
    hold = np.array([0, 1, 0, 0], np.uint8)
    reset = np.zeros((B, 3), np.uint8)
    reset[2, 1] = 1
    mask = np.array([0, 0, 0, 1], np.uint8)
    kb, twin, other = batch(gate_model, B, TMAX, precision), batch(gate_model, B, TMAX, precision), batch(gate_model, 6, TMAX, precision)
    stayed = batch(gate_model, B, TMAX, precision)  # (a second twin that runs calls 0 and 1 with nothing held: E of the stream that moves)
    kb.set_limiter(lim)
    other.set_limiter(lim[1], streams=[5])
    # call 0 plain; call 1 holds stream 1; a masked reset of stream 3; call 2 plain; call 3 restarts stream 2 at its frame 1
    steps = [dict(), dict(hold=hold), dict(), dict(reset=reset)]
    state, below = limiter.fresh(B), False
    for i, c in enumerate(x):
        if i == 2:
            assert kb.limiter_state([3])[0] < 1
            kb.reset(mask)
            twin.reset(mask)
            assert same(kb.limiter_state([3]), limiter.fresh(1))
            state[3] = 1.0
        e = call(twin, c, 'device', **steps[i])
        o = call(kb, c, 'device', **steps[i])
        w, state = limiter.apply(e, lim, None, None, state, steps[i].get('reset'), steps[i].get('hold'))
        after = kb.limiter_state()
        live = np.flatnonzero(steps[i].get('hold', np.zeros(B)) == 0)  # (held rows of `out` are unspecified)
        assert same(after, state) and same(o[live], w[live])
        below = below or (state < 1).any()
        if i == 0:  # stream 1 moves to slot 5 of another handle -- the record and the limiter's four bytes -- and continues there ==
            other.import_state(kb.export_state([1]), streams=[5])
            other.set_limiter_state(kb.limiter_state([1]), streams=[5])
            assert same(other.limiter_state([5]), state[1:2]) and same(other.limiter_state([0]), limiter.fresh(1)) and state[1] < 1
            rows = np.zeros((6, x[1].shape[1]), np.int16)
            rows[5] = x[1][1]
            moved = call(other, rows, 'device')[5]
            call(stayed, c, 'device')
            w1, s1 = limiter.apply(call(stayed, x[1], 'device')[1:2], lim[1], state=state[1:2])
            assert same(moved, w1[0]) and same(other.limiter_state([5]), s1) and (w1 != 0).any()
        if i == 1:
            assert after[1] == state[1] < 1  # held: g stays where call 0 left it
    for h in (kb, twin, other, stayed):
        h.delete()
    assert below


@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_frame_call_between_longer_ones(gate_model, precision):
    x = _input()
    E, _ = _twin(gate_model, precision)
    lim = ceilings(E)
    kb, twin = batch(gate_model, B, TMAX, precision), batch(gate_model, B, TMAX, precision)
    kb.set_limiter(lim)
    state, below = None, False
    for t0, t1 in ((0, 3), (3, 4), (4, 7)):
        c = gpu_kit.frames(x, t0, t1)
        e = call(twin, c, 'device')
        w, state = limiter.apply(e, lim, state=state)
        assert same(call(kb, c, 'device'), w) and same(kb.limiter_state(), state)
        below = below or (t1 - t0 == 1 and (state < 1).any())
    for t0, t1 in ((7, 8), (8, 9)):  # ... and on host memory, where a plain handle would take the one-frame graph
        c = gpu_kit.frames(x, t0, t1)
        w, state = limiter.apply(call(twin, c, 'host'), lim, state=state)
        assert same(call(kb, c, 'host'), w) and same(kb.limiter_state(), state)
    kb.delete()
    twin.delete()
    assert below


@pytest.mark.parametrize('precision', PRECISIONS)
def test_two_channels_the_full_rule(gate_model, precision):
    E, _ = _twin(gate_model, precision)
    lim = ceilings(E)
    kb, twin = batch(gate_model, B, TMAX, precision, channels=2), batch(gate_model, B, TMAX, precision, channels=2)
    kb.set_limiter(lim)
    state, Gs, ends = None, [], []
    for c in cut(_input(), 16000, SEQ):
        inter = chan.interleave(c, 2)
        e = chan.deinterleave(twin.process(inter), 2)
        w, state, G = limiter.apply(e, lim, state=state, return_gain=True)
        assert same(kb.process(inter), chan.interleave(w, 2)) and same(kb.limiter_state(), state)
        Gs.append(G)
        ends.append(state)
    kb.delete()
    twin.delete()
    assert vivid(np.concatenate(Gs, axis=1), np.array(ends))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_16k_packets_the_full_rule(gate_model, precision):
    """A 16 kHz packet handle delivers the inner stream late by delay_sample - 256 more samples and in other pieces; the rule is causal, so
    what has come out of the twin so far, cut into frames (the last one padded), gives every sample the limiting handle has delivered"""
    N, calls = 200, 11
    x = _input()
    E, _ = _twin(gate_model, precision)
    lim = ceilings(E)
    kb, twin = batch(gate_model, B, TMAX, precision, packet_samples=N), batch(gate_model, B, TMAX, precision, packet_samples=N)
    kb.set_limiter(lim)
    late = kb.delay_sample - 256
    assert 0 < late < 256 and calls * N <= x.shape[1]
    counts = np.full(B, N, np.int32)
    got = np.concatenate([kb.process_packets(np.ascontiguousarray(x[:, i * N:(i + 1) * N]), counts) for i in range(calls)], axis=1)
    plain = np.concatenate([twin.process_packets(np.ascontiguousarray(x[:, i * N:(i + 1) * N]), counts) for i in range(calls)], axis=1)
    g = kb.limiter_state()
    kb.delete()
    twin.delete()
    inner = plain[:, late:]
    n = inner.shape[1]
    padded = np.concatenate([inner, np.zeros((B, -n % 256), np.int16)], axis=1)
    want, _, G = limiter.apply(padded, lim, return_gain=True)
    assert not plain[:, :late].any() and not got[:, :late].any()
    assert same(got[:, late:], want[:, :n]) and (want[:, :n] != inner).any() and (G < 1).any() and (g < 1).any()


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('kind', ['48k', '8k-ulaw', '48k-packets'])
def test_outer_layers(gate_model, precision, kind):
    """off streams == a twin of the same kind, limited streams differ, some g < 1; with c = 32767 and no leveller the whole output == the twin's"""
    if kind == '48k':
        kw, pcm = dict(sample_rate=48000), np.repeat(_input(), 3, axis=1)
    elif kind == '8k-ulaw':
        kw, pcm = dict(sample_rate=8000, sample_format='ulaw'), formats.encode('ulaw', np.ascontiguousarray(_input()[:, ::2]))
    else:
        kw, pcm = dict(sample_rate=48000, packet_samples=960), np.repeat(_input(), 3, axis=1)[:, :6 * 960]
    E, _ = _twin(gate_model, precision)
    c = ceilings(E)
    tables = ([None, c[1], None, c[3]], [setting(32767)] * B)

    def through(kb):
        if kind == '48k-packets':
            return np.concatenate([kb.process_packets(np.ascontiguousarray(pcm[:, i * 960:(i + 1) * 960]), np.full(B, 960, np.int32)) for i in range(6)], axis=1)
        return np.concatenate([kb.process(p) for p in cut(pcm, kw['sample_rate'], SEQ)], axis=1)

    twin = batch(gate_model, B, TMAX, precision, **kw)
    plain = through(twin)
    twin.delete()
    for i, table in enumerate(tables):
        kb = batch(gate_model, B, TMAX, precision, **kw)
        kb.set_limiter(table)
        out, g = through(kb), kb.limiter_state()
        kb.delete()
        if i == 0:
            assert same(out[0], plain[0]) and same(out[2], plain[2]) and (out[1] != plain[1]).any() and (out[3] != plain[3]).any()
            assert g[0] == 1 and g[2] == 1 and (g[[1, 3]] < 1).any()
        else:
            assert same(out, plain) and same(g, limiter.fresh(B))  # identity through every layer


@pytest.mark.parametrize('precision', ['fp32'])
def test_single_stream_handle(gate_model, precision):
    """Koala.set_limiter: the one-stream handle of the reference's ABI, frame by frame on host memory, against the rule"""
    import koala_amd
    x = np.array(_input()[:1])
    plain = batch(gate_model, 1, 1, precision)
    E = np.concatenate([call(plain, gpu_kit.frames(x, t, t + 1), 'device') for t in range(FRAMES)], axis=1)
    plain.delete()
    lim = ceilings(E)[0]
    want, G, ends, _, _, _ = over_calls(E, lim, (1,) * FRAMES)
    assert vivid(G, ends)
    k = koala_amd.create('key', model_path=gate_model, library_path=DEV_LIB)
    k.set_limiter(lim)
    assert k.limiter() == lim
    got = np.concatenate([np.array(k.process(x[0, t * 256:(t + 1) * 256]), np.int16) for t in range(FRAMES)])
    k.delete()
    assert same(got, want[0]) and (got != E[0]).any()


def _refused(kb, fn, *words):
    before = kb.limiter_state()
    with pytest.raises(KoalaInvalidArgumentError) as e:
        fn()
    text = str(e.value) + ' '.join(getattr(e.value, 'message_stack', []) or [])
    assert all(w in text for w in words), text
    assert same(kb.limiter_state(), before)


@pytest.mark.parametrize('precision', ['fp32'])
def test_refusals_leave_everything_untouched(gate_model, precision):
    x = gpu_kit.frames(_input(), 0, 1)
    on = setting(1000)
    # the channel link
    kb = batch(gate_model, B, TMAX, precision, channels=2, channel_link='max', limiter=on)
    out = np.full((B // 2, 512), MARK, np.int16)
    _refused(kb, lambda: kb.process_into(chan.interleave(x, 2).reshape(B, -1), out.reshape(B, -1)), 'peak limiter', 'channel link')
    assert (out == MARK).all()
    kb.set_limiter(None)
    kb.process(chan.interleave(x, 2))  # a plain call afterwards still works
    kb.delete()
    # the high-band carry
    kb = batch(gate_model, B, TMAX, precision, sample_rate=48000, high_band='carry', limiter=on)
    big = np.zeros((B, 768), np.int16)
    out = np.full_like(big, MARK)
    _refused(kb, lambda: kb.process_into(big, out), 'peak limiter', 'high-band carry')
    assert (out == MARK).all()
    kb.set_limiter(None)
    kb.process(big)
    kb.delete()
    # the asynchronous entry points
    kb = batch(gate_model, B, TMAX, precision, limiter=on)
    a, b = kb.alloc_host(1), kb.alloc_host(1)
    a[:] = x
    b[:] = MARK
    _refused(kb, lambda: kb.process_async(a, b), 'peak limiter', 'asynchronous')
    assert (b == MARK).all()
    kb.set_limiter(None)
    kb.process_async(a, b)
    kb.synchronize()
    assert not (b == MARK).all()
    kb.delete()
    # 44 100 Hz
    kb = batch(gate_model, B, 1, precision, sample_rate=44100, packet_samples=441, limiter=on)
    pk = np.zeros((B, 441), np.int16)
    out = np.full_like(pk, MARK)
    _refused(kb, lambda: kb._packets(441, np.full(B, 441, np.int32), pk.ctypes.data, out.ctypes.data, None, None, 0), 'peak limiter', '44100')
    assert (out == MARK).all()
    kb.set_limiter(None)
    kb._packets(441, np.full(B, 441, np.int32), pk.ctypes.data, out.ctypes.data, None, None, 0)
    kb.delete()
