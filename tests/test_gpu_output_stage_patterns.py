"""
The output kernels (limit_kernel of koala_amd/csrc/kns_limit.hip, level_track_kernel and level_apply_kernel of koala_amd/csrc/kns_level.hip) on
samples chosen one by one, on a real MI355X.  tests/test_gpu_limiter.py and tests/test_gpu_level.py hold them to the numpy rules on quiet
speech behind the default model; here the unity-mask model makes a 16 kHz handle a pure delay, bit for bit in both precisions, so E is
gpu_kit.delayed(x) for the rows of tests/output_stage_recipe.py: lone peaks at every envelope distance, the rails, exact ties, a frame whose
only over sits in lane 0 or lane 63, whole frames of release with no over, silence, full-scale cut -- under the library's default release
and six other limiter settings, as one batch of 175 streams (ragged last workgroup, ragged last table tile) over calls of 3, 2, 1, 2 frames.

Every comparison is gpu_kit.same: no tolerance anywhere.  tests/test_output_stage_patterns.py shows on the CPU that the rule itself notices
the faults these rows were written for, and records the one change they do not notice.
"""
import functools

import numpy as np
import pytest

import gpu_kit
import level_recipe
from gpu_kit import DEV_LIB, cut, delayed, same
from koala_amd import formats, level, limiter
from limiter_recipe import over_calls
from output_stage_recipe import DEFAULT_RELEASE, LEVELS, SEQ, SETTINGS, T, TMAX, grid, products, rows, setting, stream, thirds
from packet_recipe import PacketStream
from sample_rate_recipe import STAGES, Delay256, Stage

pytestmark = pytest.mark.gpu

batch = functools.partial(gpu_kit.batch, lib=DEV_LIB)
call = gpu_kit.call
PRECISIONS = ['fp32', 'bf16']
F32 = np.float32
R = 25  # rows per limiter setting


@functools.lru_cache(maxsize=None)
def _grid():
    x, lim, names = grid()
    x.setflags(write=False)
    return x, lim, names


@functools.lru_cache(maxsize=None)
def _twin(model, precision):
    """THE PREMISE, asserted where it is made: a handle without any output stage returns the grid one frame late, exactly -> (E, report)"""
    x, _, _ = _grid()
    kb = batch(model, x.shape[0], TMAX, precision)
    got = [call(kb, c, 'device', report=True) for c in cut(x, 16000, SEQ)]
    kb.delete()
    E, rep = np.concatenate([g[0] for g in got], axis=1), np.concatenate([g[1] for g in got], axis=1)
    assert same(E, delayed(x)), 'the unity-mask handle is not a pure delay'
    E.setflags(write=False)
    rep.setflags(write=False)
    return E, rep


@functools.lru_cache(maxsize=None)
def _limited(model, precision):
    """the rule on the grid over the calls, once per precision"""
    E, _ = _twin(model, precision)
    return over_calls(E, _grid()[1], SEQ)


def run(kb, x, mode, report=False):
    """the calls -> (out, report or None, the limiter's state behind every call, the leveller's behind the last)"""
    outs, reps, ends = [], [], []
    for c in cut(x, 16000, SEQ):
        got = call(kb, c, mode, report=report)
        outs.append(got[0] if report else got)
        reps.append(got[1] if report else None)
        ends.append(kb.limiter_state())
    return np.concatenate(outs, axis=1), np.concatenate(reps, axis=1) if report else None, np.array(ends), kb.level_state()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_premise_the_twin_is_a_pure_delay(unity_model, precision):
    E, rep = _twin(unity_model, precision)
    assert (rep[..., 2] == 257).all() and not rep[..., 3].any()  # a mask of exactly 1 in every bin, and the reserved word
    assert E.shape[0] == R * len(SETTINGS) and E.shape[0] % 4 and E.shape[0] % 16 and E.shape[1] == T * 256


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('mode', ['device', 'offset', 'inplace', 'host'])
def test_limiter_alone(unity_model, precision, mode):
    """limit_kernel: every envelope distance on its own (peak@p), the far deep peak, both rails, c = 1, a non-integer c, delta = 1 and
    2^-30, the default release fl(1/800) whose additions round; no over with g < 1 (tail), the only over in lane 0 / lane 63, nothing stored
    (flat); 'offset': the sample-by-sample loads and stores; 175 streams: a last workgroup of three waves"""
    x, lim, names = _grid()
    E, _ = _twin(unity_model, precision)
    want, G, ends, wstate, _, _ = _limited(unity_model, precision)
    c = np.array([s.ceiling for s in lim])
    engaged = (G < 1).any(axis=1).reshape(len(SETTINGS), R)
    assert engaged[:, :R - 1].any(axis=1).all() and (ends < 1).any(axis=1).all() and (want != E).any()  # (the rule's own output is vivid)
    kb = batch(unity_model, len(lim), TMAX, precision)
    kb.set_limiter(lim)
    out, _, states, _ = run(kb, x, mode)  # ('offset': gpu_kit.call asserts the guard zones around `enhanced` untouched)
    kb.delete()
    assert same(states, ends) and same(states[-1], wstate)
    assert same(out, want)
    whole = c == np.floor(c)
    assert (np.abs(out.astype(np.int64)).max(axis=1)[whole] <= c[whole]).all()
    flat = np.array([n.startswith('flat/') for n in names]) & (c >= 100)
    assert flat.sum() == len(SETTINGS) - 1 and same(out[flat], E[flat])
    r = stream(names, 'dc-', 3)
    assert (out[r, 256:] == -32767).all()  # E = -32768 under c = 32767


@pytest.mark.parametrize('precision', PRECISIONS)
def test_an_entering_state(unity_model, precision):
    """g = 1/4 in front of the streams whose release is 2^-30 -- the gain does not come back within the test -- and g = 2^-20 in front of
    a lone peak: h alone decides G, across every call boundary"""
    x, lim, names = _grid()
    E, _ = _twin(unity_model, precision)
    state = limiter.fresh(len(lim))
    slow = np.flatnonzero(np.array([s.release for s in lim]) == 2.0 ** -30)
    peak = stream(names, 'peak@5', 1)
    state[slow], state[peak] = 0.25, 2.0 ** -20
    want, G, ends, wstate, _, _ = over_calls(E, lim, SEQ, state=state.copy())
    assert len(slow) == R and (wstate[slow] < 0.2501).all() and (G[slow] < 0.2501).all() and G[peak, 0] == F32(2.0 ** -20) + F32(DEFAULT_RELEASE)
    kb = batch(unity_model, len(lim), TMAX, precision)
    kb.set_limiter(lim)
    kb.set_limiter_state(state)
    assert same(kb.limiter_state(), state)
    out, _, states, _ = run(kb, x, 'device')
    kb.delete()
    assert same(states, ends) and same(out, want)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_resets_and_a_hold(unity_model, precision):
    """the reset flag on the frame directly behind the peak's (the first frame of the second call) on every third stream, and on the frame
    behind that one on their neighbours; the third call holds every fifth stream.  A reset restarts the engine's stream too, so E is a
    twin's that gets the same flags"""
    x, lim, names = _grid()
    B = len(lim)
    reset = np.zeros((B, SEQ[1]), np.uint8)
    reset[0::3, 0] = 1
    reset[1::3, 1] = 1
    hold = (np.arange(B) % 5 == 0).astype(np.uint8)
    steps = [dict(), dict(reset=reset), dict(hold=hold), dict()]
    kb, twin = batch(unity_model, B, TMAX, precision), batch(unity_model, B, TMAX, precision)
    kb.set_limiter(lim)
    state, seen = limiter.fresh(B), []
    for i, c in enumerate(cut(x, 16000, SEQ)):
        e = call(twin, c, 'device', **steps[i])
        o = call(kb, c, 'device', **steps[i])
        before = state
        w, state = limiter.apply(e, lim, None, None, state, steps[i].get('reset'), steps[i].get('hold'))
        live = np.flatnonzero(steps[i].get('hold', np.zeros(B)) == 0)  # (held rows of `enhanced` are unspecified)
        assert same(kb.limiter_state(), state) and same(o[live], w[live]), i
        seen.append((before, state))
    kb.delete()
    twin.delete()
    (_, after0), (_, after1), (before2, after2), _ = seen
    assert (after0[0::3] < 1).any() and (after0[1::3] < 1).any()  # gains that the resets had to lift ...
    _, plain = limiter.apply(np.zeros((B, SEQ[1] * 256), np.int16), lim, state=after0)
    assert (after1[0::3] > plain[0::3]).any() and (after1[1::3] > plain[1::3]).any()  # ... and did, where a release alone had not
    held = hold != 0
    assert same(after2[held], before2[held]) and (before2[held] < 1).any()


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('mode', ['device', 'offset'])
def test_the_tracker_on_chosen_energies(unity_model, precision, mode):
    """level_track_kernel: the clamps at max_boost and at max_cut, lvl == 0 over silent frames, a_down on falling energy, theta = 1.0;
    level_apply_kernel: products past both rails, and in 'offset' its lane-consecutive unaligned path"""
    x, lim, names = _grid()
    E, rep = _twin(unity_model, precision)
    B = len(lim)
    lev = thirds(B)
    want, gains, wstate = level_recipe.over_calls(E, rep, lev, SEQ)
    start, end, spoke, _ = level.track(rep, lev)
    v = products(E, start, end)
    assert ((want == 32767) & (v > 32767.5)).any() and ((want == -32768) & (v < -32768.5)).any()  # saturation made these samples
    assert (gains[0::3] == F32(LEVELS['BOOST'].max_boost)).any() and (gains[1::3] == F32(LEVELS['CUT'].max_cut)).any()
    ramp = [b for b, n in enumerate(names) if n.startswith('ramp/')]
    assert (gains[ramp, :2] == 1).all() and (gains[ramp, 3:] != 1).all() and spoke[2::3].any()
    kb = batch(unity_model, B, TMAX, precision)
    kb.set_level(lev)
    out, got, _, state = run(kb, x, mode, report=True)
    kb.delete()
    assert same(got[..., :3], rep[..., :3]) and same(got[..., 3], gains) and same(state, wstate)
    assert same(out, want)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('mode', ['device', 'offset'])
def test_leveller_and_limiter_at_the_rails(unity_model, precision, mode):
    """BOOST and CUT on alternate streams in front of the grid's limiter settings: products of several hundred thousand under every (c, delta)"""
    x, lim, names = _grid()
    E, rep = _twin(unity_model, precision)
    B = len(lim)
    lev = [LEVELS['BOOST'] if b % 2 == 0 else LEVELS['CUT'] for b in range(B)]
    want, G, ends, wstate, wlevel, gains = over_calls(E, lim, SEQ, rep, lev)
    start, end, _, _ = level.track(rep, lev)
    peak = float(np.abs(products(E, start, end)).max())
    print('largest |v| of the rule: %.0f' % peak)
    assert peak > 1e5
    saturated, _, _ = level.apply(E, rep, lev)
    assert (want != saturated).any() and (G < 1).any()
    kb = batch(unity_model, B, TMAX, precision)
    kb.set_level(lev)
    kb.set_limiter(lim)
    out, got, states, lstate = run(kb, x, mode, report=True)
    kb.delete()
    assert same(states, ends) and same(lstate, wlevel) and same(got[..., 3], gains)
    assert same(out, want)
    c = np.array([s.ceiling for s in lim])
    whole = c == np.floor(c)
    assert (np.abs(out.astype(np.int64)).max(axis=1)[whole] <= c[whole]).all()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_nine_streams_eight_frames_in_one_call(unity_model, precision):
    """three workgroups, the last with one wave, and the longest walk of the frame loop with its prefetch"""
    x, names = rows()
    pick = ['noise', 'far_deep', 'dc-', 'peak@255', 'tie', 'tail', 'nyquist', 'lane63', 'ramp']  # (c = 32767 on the two rail rows)
    x = np.ascontiguousarray(x[[names.index(n) for n in pick]])
    lim = [setting(*SETTINGS[1 + b % 4]) for b in range(len(pick))]
    kb = batch(unity_model, len(pick), T, precision)
    kb.set_limiter(lim)
    out = call(kb, x, 'device')
    state = kb.limiter_state()
    kb.delete()
    want, wstate, G = limiter.apply(delayed(x), lim, return_gain=True)
    assert (G < 1).any(axis=1).all() and (wstate < 1).any()
    assert same(state, wstate) and same(out, want)


def _outer_input(kind, x):
    if kind.startswith('48k'):
        return np.repeat(x, 3, axis=1)
    if kind == '24k':
        return np.ascontiguousarray(np.repeat(x, 3, axis=1)[:, ::2])
    return formats.encode('ulaw', np.ascontiguousarray(x[:, ::2]))


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('kind', ['48k', '24k', '8k-ulaw'])
def test_outer_layers_exact(unity_model, precision, kind):
    """The handle is decode -> in-stage -> the pure delay -> limiter -> out-stage -> encode: tests/sample_rate_recipe.py's Recipe(None, ...)
    taken apart, with the rule between its delay and its out-stage.  Every row once with the limiter and once without (the second copy
    of the rows shifts the alternation), every sample and limiter_state() == after every call"""
    rate, fmt = {'48k': (48000, 's16'), '24k': (24000, 's16'), '8k-ulaw': (8000, 'ulaw')}[kind]
    x, names = rows()
    pcm = _outer_input(kind, np.concatenate([x, x]))
    B = pcm.shape[0]
    on = setting(14000.0, DEFAULT_RELEASE)
    lim = [on if b % 2 else None for b in range(B)]
    assert B == 2 * len(names) and B % 4 and all((lim[r] is None) != (lim[len(names) + r] is None) for r in range(len(names)))
    kb = batch(unity_model, B, TMAX, precision, sample_rate=rate, sample_format=fmt)
    kb.set_limiter(lim)
    s_in, s_out = (Stage(B, max(U, D), U, D) for U, D in STAGES[rate])
    inner, state, moved, below = Delay256(B), None, False, False
    for c in cut(pcm, rate, SEQ):
        e = inner.process(s_in.run(formats.decode(fmt, c)))
        w, state = limiter.apply(e, lim, state=state)
        want = formats.encode(fmt, s_out.run(w))
        assert same(kb.process(c), want) and same(kb.limiter_state(), state)
        moved, below = moved or (w[1::2] != e[1::2]).any(), below or (state[1::2] < 1).any()
        assert same(w[0::2], e[0::2]) and (state[0::2] == 1).all()
    kb.delete()
    assert moved and below


@pytest.mark.parametrize('precision', PRECISIONS)
def test_48k_packets_exact(unity_model, precision):
    """tests/packet_recipe.py's packetiser per stream around the same chain: packets of 960 samples against frames of 768"""
    N, F, calls = 960, 768, 6
    x, names = rows()
    pick = [names.index(n) for n in ('peak@3', 'far_deep', 'dc-', 'nyquist', 'noise')]
    pcm = _outer_input('48k', np.concatenate([x[pick], x[pick]]))
    B = pcm.shape[0]
    on = setting(14000.0, DEFAULT_RELEASE)
    lim = [on if b % 2 else None for b in range(B)]
    (Ui, Di), (Uo, Do) = STAGES[48000]
    s_in, s_out = [Stage(1, max(Ui, Di), Ui, Di) for _ in range(B)], [Stage(1, max(Uo, Do), Uo, Do) for _ in range(B)]
    inner, g = [Delay256(1) for _ in range(B)], limiter.fresh(B)

    def chain(frames, b):
        w, g[b:b + 1] = limiter.apply(inner[b].process(s_in[b].run(frames[None])), lim[b], state=g[b:b + 1])
        return s_out[b].run(w)[0]

    ps = [PacketStream(functools.partial(chain, b=b), F) for b in range(B)]
    kb = batch(unity_model, B, TMAX, precision, sample_rate=48000, packet_samples=N)
    kb.set_limiter(lim)
    below = False
    for i in range(calls):
        c = np.ascontiguousarray(pcm[:, i * N:(i + 1) * N])
        want = np.stack([ps[b].push(c[b]) for b in range(B)])
        assert same(kb.process_packets(c, np.full(B, N, np.int32)), want) and same(kb.limiter_state(), g), i
        below = below or (g[1::2] < 1).any()
    kb.delete()
    assert below and (g[0::2] == 1).all()
