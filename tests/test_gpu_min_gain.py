"""
Per-stream attenuation limit (include/pv_koala_batch.h: pv_koala_batch_set_min_gain, pv_koala_set_min_gain) on
a real MI355X: the kMinGain arm of koala_amd/csrc/kns_stft.hip's synthesis kernel under every route of the dispatch table.

The expected samples of a limited stream are built from the oracle's stage functions (tests/min_gain_recipe.py).  fp32 comparisons are ==
(FP32_TOL = 0); bf16 within the suite's bars (BF16_TOL, BF16_WITHIN_1 of tests/gpu_kit.py).  Two consequences hold exactly in both
precisions and are tested with ==: gain 0 is the plain engine, gain 1 is the input delayed by delay_sample.

Streams are independent, so large batches are filled with copies of a few CLASSES of stream (a signal and a sequence of gains), scattered
over the slots at random -- neighbouring rows of an m-tile carry different gains: the oracle runs once per class, every stream is compared.

Every call goes through the older entry points (process, process_resets, process_hold and their device and asynchronous forms).
"""
import functools

import numpy as np
import pytest

import gpu_kit
import koala_amd
from conftest import synth_streams
from gpu_kit import DEV_LIB, ROUTE_RESETS, check_pcm as check, classes, delayed, frames, route_of
from min_gain_recipe import GAINS, NCLS, SHAPES, Recipe
from stream_state_recipe import OFF_H, OFF_TAIL

pytestmark = pytest.mark.gpu

batch = functools.partial(gpu_kit.batch, lib=DEV_LIB)
call = functools.partial(gpu_kit.call, entry='classic')


# ------------------------------------------------------------------------------------------------ 7. mixed gains, every route

@pytest.mark.parametrize('precision,B,Tmax,calls,routes', SHAPES, ids=['%s-%dx%d' % (s[0], s[1], s[2]) for s in SHAPES])
def test_mixed_gains_match_the_recipe(random_model, precision, B, Tmax, calls, routes):
    if any(m != 'host' and m != 'async' for _, m in calls):
        pytest.importorskip('torch')
    total = sum(T for T, _ in calls)
    xc = synth_streams(NCLS, total, seed=21)
    cls = classes(B, B, NCLS)
    x = xc[cls]
    kb, plain = batch(random_model, B, Tmax, precision), batch(random_model, B, Tmax, precision)
    rec = Recipe(random_model, NCLS, precision)
    assert not kb.min_gain().any()
    taken, t0, differs = set(), 0, 0
    for n, (T, mode) in enumerate(calls):
        gc = np.roll(GAINS, n)  # changed between the calls
        kb.set_min_gain(gc[cls])
        assert np.array_equal(kb.min_gain(), gc[cls])
        xn = frames(x, t0, t0 + T)
        got = call(kb, xn, mode)
        taken.add(route_of(kb))
        base = call(plain, xn, mode)
        want = rec.process(frames(xc, t0, t0 + T), gc)
        check(got, want[cls], precision, 'call %d (%d frames, %s)' % (n, T, mode))
        # a stream without a limit in this call, next to limited ones: the plain engine's samples from the second frame on (the first
        # frame overlap-adds a tail made under the previous call's gain) -- in the first call, all of them
        zero = gc[cls] == 0
        skip = 256 if n else 0
        assert np.array_equal(got[zero][:, skip:], base[zero][:, skip:]), n
        differs += int((got[~zero] != base[~zero]).sum())
        t0 += T
    assert differs > 0  # (the limit does something)
    kb.delete()
    plain.delete()
    for r in routes:
        assert r in taken, (taken, routes)


# ------------------------------------------------------------------------------------------------ 5. back to zero = the plain handle

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,T', [(21, 4), (1024, 32)])
def test_zero_gains_after_a_limit_are_the_plain_handle(random_model, precision, B, T):
    seq = [1, T, 1, 1, T]
    x0, x1 = synth_streams(B, sum(seq), seed=3), synth_streams(B, sum(seq), seed=4)
    kb, plain = batch(random_model, B, T, precision), batch(random_model, B, T, precision)
    kb.set_min_gain(np.resize(GAINS[1:], B))
    t0 = 0
    for n in seq:  # one-frame calls among them: the captured frames of the limited form
        kb.process(frames(x0, t0, t0 + n))
        plain.process(frames(x0, t0, t0 + n))
        t0 += n
    kb.set_min_gain(0.0)
    assert not kb.min_gain().any()
    # without a reset: the state the mask network sees never knew of the limit; only the first output frame carries the old tail
    first = kb.process(frames(x1, 0, T))
    want = plain.process(frames(x1, 0, T))
    assert np.array_equal(first[:, 256:], want[:, 256:]) and not np.array_equal(first[:, :256], want[:, :256])
    # after a reset: a fresh plain handle, whatever the call length and pointer kind
    kb.reset()
    fresh = batch(random_model, B, T, precision)
    t0 = 0
    for n in seq:
        xn = frames(x1, t0, t0 + n)
        assert np.array_equal(kb.process(xn), fresh.process(xn)), n
        assert route_of(kb) == route_of(fresh)
        t0 += n
    for h in (kb, plain, fresh):
        h.delete()


# ------------------------------------------------------------------------------------------------ 6. gain 1 = a pure delay

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('kind', ['random', 'default', 'random5'])
def test_unit_gain_is_a_pure_delay(random_model, gate_model, random5_model, kind, precision):
    model = {'random': random_model, 'default': gate_model, 'random5': random5_model}[kind]
    for B, T, seq in ((21, 4, [1, 4, 1, 1, 3]), (1024, 32, [32, 1, 32])):
        x = synth_streams(B, sum(seq), seed=8)
        kb = batch(model, B, T, precision)
        kb.set_min_gain(1.0)
        outs, t0 = [], 0
        for n in seq:
            outs.append(kb.process(frames(x, t0, t0 + n)))
            t0 += n
        kb.delete()
        assert np.array_equal(np.concatenate(outs, axis=1), delayed(x)), (kind, precision, B)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_unit_gain_is_a_pure_delay_from_device_memory(random_model, precision):
    pytest.importorskip('torch')
    B, T = 4100, 4
    x = synth_streams(64, 2 * T + 1, seed=9)[np.random.default_rng(1).integers(0, 64, B)]
    kb = batch(random_model, B, T, precision)
    kb.set_attenuation_limit(0.0)
    outs = [call(kb, frames(x, 0, T), 'device'), call(kb, frames(x, T, T + 1), 'device'), call(kb, frames(x, T + 1, 2 * T + 1), 'inplace')]
    kb.delete()
    assert np.array_equal(np.concatenate(outs, axis=1), delayed(x))


# ------------------------------------------------------------------------------------------------ 8. resets, held streams, stream records

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('mode', ['host', 'inplace', 'async'])
def test_per_frame_resets_under_a_limit(random_model, precision, mode):
    if mode == 'inplace':
        pytest.importorskip('torch')
    B, T = 40, 8
    xc = synth_streams(NCLS, 2 * T + 1, seed=13)
    cls = classes(B, 5, NCLS)
    rng = np.random.default_rng(6)
    rc = [(rng.random((NCLS, T)) < 0.2).astype(np.uint8) for _ in range(2)]
    rc[0][2, 0] = rc[0][2, 1] = rc[1][3, T - 1] = 1  # frame 0, adjacent frames, the last frame
    kb = batch(random_model, B, T, precision)
    rec = Recipe(random_model, NCLS, precision)
    kb.set_min_gain(GAINS[cls])
    for n in range(2):
        xn = frames(xc, n * T, (n + 1) * T)
        got = call(kb, xn[cls], mode, reset=np.ascontiguousarray(rc[n][cls]))
        assert route_of(kb) == ROUTE_RESETS
        check(got, rec.process_resets(xn, GAINS, rc[n])[cls], precision, 'resets, call %d (%s)' % (n, mode))
        assert np.array_equal(kb.min_gain(), GAINS[cls])  # a reset is no change of configuration
    # a one-frame call that restarts streams at frame 0: the reset kernel in front of the captured frame
    r0 = np.zeros((NCLS, 1), np.uint8)
    r0[[1, 4]] = 1
    xn = frames(xc, 2 * T, 2 * T + 1)
    got = kb.process_resets(xn[cls], np.ascontiguousarray(r0[cls]))
    check(got, rec.process_resets(xn, GAINS, r0)[cls], precision, 'resets, one frame')
    kb.reset()
    assert np.array_equal(kb.min_gain(), GAINS[cls])
    kb.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_held_streams_keep_their_limit_and_state(random_model, precision):
    B, T = 40, 4
    xc = synth_streams(NCLS, 3 * T, seed=17)
    cls = classes(B, 7, NCLS)
    hold = (np.random.default_rng(8).random(B) < 0.4).astype(np.uint8)
    hold[0], hold[1] = 1, 0
    kb = batch(random_model, B, T, precision)
    full, skip = Recipe(random_model, NCLS, precision), Recipe(random_model, NCLS, precision)
    kb.set_min_gain(GAINS[cls])
    x = [frames(xc, n * T, (n + 1) * T) for n in range(3)]
    check(kb.process(x[0][cls]), full.process(x[0], GAINS)[cls], precision, 'hold, call 0')
    skip.process(x[0], GAINS)
    before = kb.export_state()
    got = kb.process_hold(x[1][cls], hold)
    free = hold == 0
    check(got[free], full.process(x[1], GAINS)[cls][free], precision, 'hold, call 1 (streams not held)')
    assert np.array_equal(kb.min_gain(), GAINS[cls])
    assert np.array_equal(kb.export_state()[hold != 0], before[hold != 0])  # state bit for bit what it was
    got = kb.process(x[2][cls])
    want = np.where((hold != 0)[:, None], skip.process(x[2], GAINS)[cls], full.process(x[2], GAINS)[cls])
    check(got, want, precision, 'hold, call 2')
    kb.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_records_do_not_carry_the_limit(random_model, precision):
    B, T = 48, 4
    x = synth_streams(B, 2 * T + 2, seed=19)
    gains = np.resize(GAINS, B)
    a, plain = batch(random_model, B, T, precision), batch(random_model, B, T, precision)
    a.set_min_gain(gains)
    for h in (a, plain):
        h.process(frames(x, 0, T))
        h.process(frames(x, T, T + 1))
    ra, rp = a.export_state(), plain.export_state()
    # the mask network never sees its own output: everything but the overlap-add tail is the unlimited run's, and a stream with gain 0
    # has the unlimited run's record in full
    assert np.array_equal(ra[:, :OFF_TAIL], rp[:, :OFF_TAIL]) and np.array_equal(ra[:, OFF_H:], rp[:, OFF_H:])
    zero = gains == 0
    assert np.array_equal(ra[zero], rp[zero])
    assert all(not np.array_equal(ra[b, OFF_TAIL:OFF_H], rp[b, OFF_TAIL:OFF_H]) for b in np.flatnonzero(~zero))
    # into another handle, other slots: the limit stays behind (the caller sets it at the destination), the stream continues
    c = batch(random_model, B + 16, T, precision)
    dst = np.random.default_rng(2).permutation(B + 16)[:B]
    c.set_min_gain(0.5)
    c.import_state(ra, dst)
    assert np.array_equal(c.min_gain(), np.full(B + 16, 0.5, np.float32))
    c.set_min_gain(0.0)
    c.set_min_gain(gains, dst)
    for t0, n in ((T + 1, T), (2 * T + 1, 1)):
        xn = frames(x, t0, t0 + n)
        xcn = np.zeros((B + 16, n * 256), np.int16)
        xcn[dst] = xn
        assert np.array_equal(c.process(xcn)[dst], a.process(xn)), (t0, n)
    for h in (a, plain, c):
        h.delete()


# ------------------------------------------------------------------------------------------------ 9. the single-stream ABI

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_single_stream_handle_changes_its_limit_between_frames(random_model, precision, monkeypatch):
    """one frame per call: the hipGraph path.  The limit is set after the plain frame has been captured, changed in value, and taken away."""
    monkeypatch.setenv('KOALA_AMD_PRECISION', precision)
    phases = [0.0, 0.25, 0.6, 1.0, 0.0]
    per = 4
    x = synth_streams(1, per * len(phases), seed=23)
    k, plain = koala_amd.create('key', model_path=random_model), koala_amd.create('key', model_path=random_model)
    rec = Recipe(random_model, 1, precision)
    assert k.min_gain() == 0.0
    for p, g in enumerate(phases):
        if p:
            k.set_min_gain(g)
        assert k.min_gain() == np.float32(g)
        xn = frames(x, p * per, (p + 1) * per)
        got = np.array([k.process(xn[0, t * 256:(t + 1) * 256]) for t in range(per)], np.int16).reshape(1, -1)
        base = np.array([plain.process(xn[0, t * 256:(t + 1) * 256]) for t in range(per)], np.int16).reshape(1, -1)
        check(got, rec.process(xn, [g]), precision, 'single stream, phase %d (gain %g)' % (p, g))
        if g == 0.0:  # the plain handle's samples (after a limit: from the second frame on, the first carries the old tail)
            assert np.array_equal(got[:, 256 if p else 0:], base[:, 256 if p else 0:])
        elif g == 1.0:
            assert np.array_equal(got[:, 256:], xn[:, :-256])
        else:
            assert not np.array_equal(got, base)
    k.set_attenuation_limit(12.0)
    assert k.min_gain() == np.float32(10.0 ** (-12.0 / 20.0))
    k.reset()
    assert k.min_gain() == np.float32(10.0 ** (-12.0 / 20.0))
    k.delete()
    plain.delete()
