"""
The engine's own kernels (kns_stft.hip, kns_stft_synthesis.inc, kns_gemm.hip, kns_gru.hip, kns_gruq.hip) against the oracle on edge inputs, on
a real MI355X: DC at either rail, the rails alternating at Nyquist, full-range noise, a full-scale impulse and step, +-1 LSB dither, digital
silence, speech after silence, speech driven into the rails, a full-scale square wave (tests/edge_recipe.py) -- on every route of
Engine::run_device's dispatch table, the route read back from the developer library after every call.

No bar is new.  fp32 is ==, for every input and every model.  bf16 is held to the suite's existing bars (gpu_kit.check_pcm) on the pairs of
edge_recipe.BF16_ASSERTED -- the pairs on which two valid bf16 implementations agree within 1 LSB (tests/test_edge_inputs.py) -- and everywhere
else to what is exact: two handles agree, replicas agree, silence is silence; the distance to the oracle is printed beside the oracle's own
jitter there.  The fixed-mask models (a brick wall: mask exactly 1 or about 1e-13) put the synthesis kernel's clamp to work together with a
mask that is not 1 everywhere: where the float64 statement of the filter leaves the int16 range, the device output sits on the rail.

The twelve rows are tiled over the B slots (slot i holds row i % 12): the oracle runs on 12 streams per case, the first 12 slots are compared
with it and every other slot with its row.  A device run is made once per (model, case) and shared by the tests that read it.
"""
import collections

import numpy as np
import pytest

import koala_amd
from edge_recipe import (BF16_ASSERTED, FIXED, MODELS, NAMES, PASSBANDS, ROWS, SILENCE, asserted_rows, beyond, edge_streams, jitter_figures,
                         model_path, unclamped)
from frame_report_recipe import ReportRecipe
from gpu_kit import (DEV_LIB, ROUTE_CHUNKED, ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_RESETS, ROUTE_SMALL, ROUTE_WAVE, batch, call, check_pcm, cut,
                     delayed, lsb, oracle_prec, replicas, route_of, tiled)
from oracle import oracle

pytestmark = pytest.mark.gpu

# the smallest shape that reaches each route (tests/test_gpu_parity.py::test_dispatch_routes); every case makes at least two calls, so
# that state crosses a call boundary.  `flagged`: the reset flag is set on frame 2 of every call on every third stream.
Case = collections.namedtuple('Case', 'precision name route B T calls mode flagged')
CASES = [
    Case('fp32', 'small', ROUTE_SMALL, 16, 1, 6, 'host', False),
    Case('fp32', 'wavefront', ROUTE_WAVE, 64, 2, 2, 'device', False),
    Case('fp32', 'chunked', ROUTE_CHUNKED, 4112, 2, 2, 'device', False),
    Case('fp32', 'resets', ROUTE_RESETS, 64, 4, 2, 'device', True),
    Case('bf16', 'small', ROUTE_SMALL, 16, 1, 6, 'host', False),
    Case('bf16', 'quad', ROUTE_QUAD1, 960, 1, 6, 'device', False),
    Case('bf16', 'wavefront', ROUTE_WAVE, 64, 4, 2, 'device', False),
    Case('bf16', 'chunked', ROUTE_CHUNKED, 1040, 2, 2, 'device', False),
    Case('bf16', 'pipelined', ROUTE_PIPELINED, 784, 32, 2, 'device', False),
    Case('bf16', 'resets', ROUTE_RESETS, 64, 4, 2, 'device', True),
]
FP32 = [c for c in CASES if c.precision == 'fp32']
BF16 = [c for c in CASES if c.precision == 'bf16']


def cid(c):
    return '%s-%s-%dx%dx%d' % (c.precision, c.name, c.B, c.T, c.calls)


def pairs(cases, models=MODELS):
    """(model, case), the five-frame front-end on the small and the wavefront route only"""
    return [pytest.param(m, c, id='%s-%s' % (m, cid(c))) for m in models for c in cases if m != 'random5' or c.name in ('small', 'wavefront')]


@pytest.fixture(scope='module')
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp('edge_models')
    return {m: model_path(d, m) for m in MODELS}


# ---------------------------------------------------------------------------------------------------- expected and delivered samples, made once

def reset_flags(c):
    """[ROWS, T] of one call"""
    f = np.zeros((ROWS, c.T), np.uint8)
    if c.flagged:
        f[::3, 2] = 1
    return f


_want, _got, _jitter = {}, {}, {}


def want(models, model, c):
    """the oracle's samples of the twelve rows, int16 [12, calls * T * 256]"""
    key = (model, c.precision, c.T * c.calls, c.T if c.flagged else 0)
    if key not in _want:
        o = oracle.Oracle(models[model], ROWS, oracle_prec(c.precision))
        out = []
        for xc in cut(edge_streams(c.T * c.calls)[0], 16000, [c.T] * c.calls):
            if c.flagged:  # a reset right before frame 2 of the call
                out += [o.process(np.ascontiguousarray(xc[:, :512]))]
                o.reset(reset_flags(c)[:, 2])
                out += [o.process(np.ascontiguousarray(xc[:, 512:]))]
            else:
                out.append(o.process(xc))
        _want[key] = np.concatenate(out, axis=1)
        _want[key].setflags(write=False)
    return _want[key]


def run(models, model, c, mode=None, bypass=False):
    """one handle through the case's calls -> the first twelve slots, int16 [12, calls * T * 256]; asserts the route after every call and
    that every other slot equals its row.  `bypass`: an attenuation limit of 0 dB (minimum gain 1) on every stream."""
    kb = batch(models[model], c.B, c.T, c.precision, DEV_LIB)
    if bypass:
        kb.set_attenuation_limit(0.0)
        assert (kb.min_gain() == 1.0).all()
    out = []
    flags = tiled(reset_flags(c), c.B) if c.flagged else None
    for n, xc in enumerate(cut(edge_streams(c.T * c.calls)[0], 16000, [c.T] * c.calls)):
        y = call(kb, tiled(xc, c.B), mode or c.mode, reset=flags)
        assert route_of(kb) == c.route, (cid(c), n, route_of(kb))
        assert replicas(y, ROWS), (cid(c), n)
        out.append(y[:ROWS])
    kb.delete()
    return np.concatenate(out, axis=1)


def got(models, model, c):
    """the first run of (model, case), shared by the tests that read it"""
    key = (model, cid(c))
    if key not in _got:
        _got[key] = run(models, model, c)
        _got[key].setflags(write=False)
    return _got[key]


def jitter(models, model, frames):
    """the oracle's own jitter on the twelve rows over `frames` frames (CPU)"""
    key = (model, frames)
    if key not in _jitter:
        _jitter[key] = jitter_figures(models[model], edge_streams(frames)[0])
    return _jitter[key]


def differing(y, ref):
    return {NAMES[r]: int((y[r] != ref[r]).sum()) for r in range(ROWS) if (y[r] != ref[r]).any()}


# ---------------------------------------------------------------------------------------------------- a. fp32 == oracle

@pytest.mark.parametrize('model,c', pairs(FP32))
def test_fp32_equals_the_oracle(models, model, c):
    y, ref = got(models, model, c), want(models, model, c)
    assert np.array_equal(y, ref), (differing(y, ref), int(lsb(y, ref).max()))
    assert not y[SILENCE].any()


@pytest.mark.parametrize('mode', ['inplace', 'offset'])
def test_fp32_equals_the_oracle_in_place_and_off_alignment(models, mode):
    """64 x 2 on the wavefront route: `enhanced` == `pcm`, and both pointers one element behind an aligned address (guard zones: gpu_kit.call)"""
    c = CASES[1]
    y, ref = run(models, 'random', c, mode=mode), want(models, 'random', c)
    assert np.array_equal(y, ref), (differing(y, ref), int(lsb(y, ref).max()))


# ---------------------------------------------------------------------------------------------------- b. fp32 stage taps at the rails

@pytest.mark.parametrize('model', ['random', 'adaptive'])
def test_fp32_stage_taps_at_the_rails(models, monkeypatch, model):
    """spectrum, features, embedding, mask, hidden state and samples == Oracle.process_tap on the twelve rows (B = 12, T = 3, two calls)"""
    monkeypatch.setenv('KOALA_AMD_DEBUG_TAPS', '1')
    T, calls = 3, 2
    x = edge_streams(T * calls)[0]
    kb = batch(models[model], ROWS, T, 'fp32', DEV_LIB)
    streams = [oracle.Oracle(models[model]) for _ in range(ROWS)]
    for n, xc in enumerate(cut(x, 16000, [T] * calls)):
        y = kb.process(xc)
        taps = {k: kb.debug_read(k, T) for k in ('spectrum', 'features', 'embed', 'mask')}
        hidden = kb.debug_read('hidden', T)
        for b in range(ROWS):
            for t in range(T):
                ref, tp = streams[b].process_tap(xc[b, t * 256:(t + 1) * 256])
                for k in ('spectrum', 'features', 'embed', 'mask'):
                    assert np.array_equal(taps[k][t, b], tp[k]), (k, NAMES[b], n, t, float(np.abs(taps[k][t, b] - tp[k]).max()))
                assert np.array_equal(ref, y[b, t * 256:(t + 1) * 256]), (NAMES[b], n, t)
            assert np.array_equal(hidden[:, b], tp['hidden']), (NAMES[b], n)
        assert np.isfinite(taps['features']).all()
    kb.delete()


# ---------------------------------------------------------------------------------------------------- c. bf16 features

def _round_bf16(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize('T,calls', [(3, 1), (1, 3)])
def test_bf16_features_are_the_oracles_bits_at_the_rails(models, monkeypatch, T, calls):
    """power 0 (silence, the frames before the impulse and the step) and the largest power there is (DC and Nyquist at the rails) through
    kns_log_fast: the engine's bf16 feature operands == the oracle's features rounded to bf16, on all twelve rows"""
    monkeypatch.setenv('KOALA_AMD_DEBUG_TAPS', '1')
    x = edge_streams(3)[0]
    kb = batch(models['random'], ROWS, T, 'bf16', DEV_LIB)
    streams = [oracle.Oracle(models['random'], 1, oracle.PREC_BF16) for _ in range(ROWS)]
    for n, xc in enumerate(cut(x, 16000, [T] * calls)):
        kb.process(xc)
        feat = kb.debug_read('features', T)
        for b in range(ROWS):
            for t in range(T):
                _, tp = streams[b].process_tap(xc[b, t * 256:(t + 1) * 256])
                assert np.array_equal(feat[t, b], _round_bf16(tp['features'])), (NAMES[b], n, t)
    kb.delete()


# ---------------------------------------------------------------------------------------------------- d. bf16, the asserted pairs

@pytest.mark.parametrize('model,c', pairs(BF16))
def test_bf16_asserted_pairs_meet_the_suites_bars(models, model, c):
    y, ref = got(models, model, c), want(models, model, c)
    rows = asserted_rows(model)
    if model in FIXED:  # a recorded figure: the mask is exactly 0 or 1 on both sides
        print('%s %s: == the bf16 oracle: %s %s' % (model, cid(c), 'yes' if np.array_equal(y, ref) else 'no', differing(y, ref)))
    check_pcm(y[rows], ref[rows], 'bf16', '%s %s, %d asserted rows' % (model, cid(c), len(rows)))


# ---------------------------------------------------------------------------------------------------- e. bf16, every pair, what is exact

@pytest.mark.parametrize('model,c', pairs(BF16))
def test_bf16_every_pair_is_reproducible_and_silence_is_silence(models, model, c):
    y = got(models, model, c)
    again = run(models, model, c)  # a second handle, the same calls (replicas in other slots: asserted by `run`)
    assert np.array_equal(y, again), differing(y, again)
    assert not y[SILENCE].any()
    open_rows = [r for r in range(ROWS) if (model, NAMES[r]) not in BF16_ASSERTED]
    if open_rows:
        d = lsb(y, want(models, model, c))
        jmax, jwithin = jitter(models, model, c.T * c.calls)
        for r in open_rows:  # recorded, not asserted: two valid bf16 implementations differ by as much here
            print('%s %s %-14s recorded: max %2d LSB, %.4f within 1 | the oracle against its own jitter: max %2d LSB, %.4f within 1' %
                  (model, cid(c), NAMES[r], int(d[r].max()), float((d[r] <= 1).mean()), int(jmax[r]), float(jwithin[r])))


# ---------------------------------------------------------------------------------------------------- f. a pure delay at the rails

def delay_of(c):
    """the twelve rows one frame late; a restarted stream starts from silence, so the frame in front of a reset never comes out"""
    expect = delayed(edge_streams(c.T * c.calls)[0]).copy()
    if c.flagged:
        for n in range(c.calls):
            a = (n * c.T + 2) * 256
            expect[::3, a:a + 256] = 0
    return expect


@pytest.mark.parametrize('c', CASES, ids=cid)
def test_unity_mask_is_a_pure_delay_at_the_rails(models, c):
    y = got(models, 'unity', c)
    assert np.array_equal(y, delay_of(c)) and (y == 32767).any() and (y == -32768).any()


@pytest.mark.parametrize('c', CASES, ids=cid)
def test_an_attenuation_limit_of_0_db_is_a_pure_delay_at_the_rails(models, c):
    """the kMinGain arm of the synthesis kernel at gain 1 on the random-weight model: whatever the network says, the input comes back"""
    y = run(models, 'random', c, bypass=True)
    assert np.array_equal(y, delay_of(c)) and (y == 32767).any() and (y == -32768).any()


# ---------------------------------------------------------------------------------------------------- g. saturation with a real mask

@pytest.mark.parametrize('model,c', pairs([c for c in CASES if not c.flagged], ['highpass8', 'lowpass64']))
def test_brick_wall_filters_sit_on_the_rail_where_the_filter_leaves_the_range(models, model, c):
    """the positions come from the float64 statement of the filter (edge_recipe.unclamped), never from the device"""
    y, ref = got(models, model, c), want(models, model, c)
    if c.precision == 'fp32':
        assert np.array_equal(y, ref), differing(y, ref)
    else:
        check_pcm(y, ref, 'bf16', '%s %s' % (model, cid(c)))
    x = edge_streams(c.T * c.calls)[0]
    above, below = beyond(unclamped(x, PASSBANDS[model]))
    row = NAMES.index('noise' if model == 'highpass8' else 'square')
    print('%s %s: %d samples above, %d below the range (row %s: %d, %d)' % (model, cid(c), above.sum(), below.sum(), NAMES[row], above[row].sum(), below[row].sum()))
    assert above[row].any() and below[row].any()
    assert (y[above] == 32767).all() and (y[below] == -32768).all()
    assert (y[row] != delayed(x)[row]).any()  # (not the identity)


# ---------------------------------------------------------------------------------------------------- h. report rows

@pytest.mark.parametrize('model', ['random', 'highpass8'])
def test_fp32_report_rows_at_the_rails(models, model):
    c = CASES[1]
    kb, rec = batch(models[model], c.B, c.T, 'fp32', DEV_LIB), ReportRecipe(models[model], ROWS, 'fp32')
    for n, xc in enumerate(cut(edge_streams(c.T * c.calls)[0], 16000, [c.T] * c.calls)):
        y, rep = call(kb, tiled(xc, c.B), 'device', report=True)
        assert route_of(kb) == c.route
        rows = rec.process(xc)
        assert np.array_equal(rep[:ROWS], rows), (n, [NAMES[r] for r in range(ROWS) if not np.array_equal(rep[r], rows[r])])
        assert replicas(rep, ROWS) and replicas(y, ROWS)
        assert (rep[SILENCE, :, 0] == 0).all() and (rep[SILENCE, :, 1] == 0).all()  # e_in of silence: exactly 0
    kb.delete()


# ---------------------------------------------------------------------------------------------------- i. the single-stream ABI

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('model', ['adaptive', 'highpass8'])
def test_single_stream_abi_on_edge_inputs(models, monkeypatch, model, precision):
    """pv_koala_init / pv_koala_process, one frame per call through the captured graph, each of the twelve rows for 24 frames"""
    monkeypatch.setenv('KOALA_AMD_PRECISION', precision)
    frames = 24
    x = edge_streams(frames)[0]
    ref = oracle.Oracle(models[model], ROWS, oracle_prec(precision)).process(x)
    k = koala_amd.create('key', model_path=models[model], device='gpu:0')
    y = np.zeros_like(x)
    for r in range(ROWS):
        k.reset()
        y[r] = np.concatenate([np.array(k.process(x[r, t * 256:(t + 1) * 256]), np.int16) for t in range(frames)])
    k.delete()
    if precision == 'fp32':
        assert np.array_equal(y, ref), differing(y, ref)
    else:
        rows = asserted_rows(model)
        check_pcm(y[rows], ref[rows], 'bf16', '%s single stream, %d asserted rows' % (model, len(rows)))
        d = lsb(y, ref)
        for r in range(ROWS):
            if r not in rows:
                print('%s single stream %-14s recorded: max %d LSB, %.4f within 1' % (model, NAMES[r], int(d[r].max()), float((d[r] <= 1).mean())))
    assert not y[SILENCE].any()
