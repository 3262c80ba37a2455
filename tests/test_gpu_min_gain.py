"""
Per-stream attenuation limit (include/pv_koala_batch.h: pv_koala_batch_set_min_gain, pv_koala_set_min_gain) on
a real MI355X: the kMinGain arm of koala_amd/csrc/kns_stft.hip's synthesis kernel under every route of the dispatch table.

The expected samples of a limited stream are built from the oracle's stage functions (`Recipe` below): `Oracle.process_with_mask` gives every
frame's mask m, `Oracle.analysis` its spectrum, numpy float32 forms m' = g + (1 - g) m (one subtraction, one product, one sum, each rounded
to float32) and `oracle.synthesis` makes the samples.  fp32 comparisons are == (FP32_TOL = 0); bf16 within the suite's bars (BF16_TOL,
BF16_WITHIN_1 of tests/test_gpu_parity.py).  Two consequences hold exactly in both precisions and are tested with ==: gain 0 is the plain
engine, gain 1 is the input delayed by delay_sample.

Streams are independent, so large batches are filled with copies of a few CLASSES of stream (a signal and a sequence of gains), scattered
over the slots at random -- neighbouring rows of an m-tile carry different gains: the oracle runs once per class, every stream is compared.
"""
import numpy as np
import pytest

import koala_amd
from conftest import synth_streams
from oracle import oracle
from test_stream_state import OFF_H, OFF_TAIL

pytestmark = pytest.mark.gpu

BF16_TOL, BF16_WITHIN_1, FP32_TOL = 5, 0.99, 0  # tests/test_gpu_parity.py
DEV_LIB = koala_amd.developer_library_path()
# kns_engine.cpp, enum Route
ROUTE_CHUNKED, ROUTE_SMALL, ROUTE_SMALL_STEPS, ROUTE_QUAD1, ROUTE_WAVE, ROUTE_PIPELINED, ROUTE_RESETS = 0, 1, 2, 3, 4, 5, 6
NCLS = 8
# per class: 0 (no limit), 1 (bypass) and values in between; a call's gains are this list rotated by the call's number
GAINS = np.array([0.0, 1.0, 0.25, 0.5, 0.1, 0.9, 0.031622775, 0.70710677], np.float32)


def oracle_prec(precision):
    return oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32


def frames(x, t0, t1):
    return np.ascontiguousarray(x[:, t0 * 256:t1 * 256])


def delayed(x):
    """the input delayed by delay_sample = one frame"""
    return np.concatenate([np.zeros((x.shape[0], 256), np.int16), x[:, :-256]], axis=1)


def batch(model, B, T, precision, lib=DEV_LIB):
    return koala_amd.create_batch('key', B, T, precision, model_path=model, library_path=lib)


def route_of(kb):
    return int(kb.debug_read('route', 1)[0])


def check(got, want, precision, what):
    """fp32: the recipe's samples; bf16: the suite's bars.  Prints the figures before it asserts."""
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print('%s %s: max |engine - recipe| = %d LSB, %.4f %% within 1, %d samples' % (what, precision, int(d.max()), 100.0 * (d <= 1).mean(), d.size))
    if precision == 'bf16':
        assert d.max() <= BF16_TOL and (d <= 1).mean() >= BF16_WITHIN_1, (what, int(d.max()), float((d <= 1).mean()))
    else:
        assert d.max() <= FP32_TOL, (what, int(d.max()))


class Recipe:
    """n streams of the spec with a minimum gain, from the oracle's stages (the module's docstring)"""

    def __init__(self, model, n, precision):
        self.o = oracle.Oracle(model, n, oracle_prec(precision))
        self.n = n
        self.hist = np.zeros((n, 256), np.int16)
        self.tail = np.zeros((n, 256), np.float32)

    def reset(self, rows):
        rows = np.asarray(rows, bool)
        if rows.any():
            self.o.reset(rows.astype(np.uint8))
            self.hist[rows] = 0
            self.tail[rows] = 0

    def process(self, x, gains):
        x = np.ascontiguousarray(x, np.int16)
        T = x.shape[1] // 256
        _, mask = self.o.process_with_mask(x)
        out = np.empty_like(x)
        for b in range(self.n):
            g = np.float32(gains[b])
            u = np.float32(1.0) - g
            for t in range(T):
                fr = x[b, t * 256:(t + 1) * 256]
                spec, _ = self.o.analysis(self.hist[b], fr)
                m = mask[t, b].astype(np.float32)
                mp = (g + (u * m).astype(np.float32)).astype(np.float32)
                out[b, t * 256:(t + 1) * 256] = oracle.synthesis(spec, mp, self.tail[b])
                self.hist[b] = fr
        return out

    def process_resets(self, x, gains, reset):
        """per-frame stream resets [n, T]: frame by frame, a reset right before its frame"""
        T = x.shape[1] // 256
        outs = []
        for t in range(T):
            self.reset(reset[:, t] != 0)
            outs.append(self.process(frames(x, t, t + 1), gains))
        return np.concatenate(outs, axis=1)


def call(kb, x, mode, reset=None):
    """one call: 'host' (pageable), 'device', 'inplace' (device, enhanced == pcm), 'async' (page-locked, asynchronous, waited for)"""
    T = x.shape[1] // 256
    if mode == 'host':
        return kb.process(x) if reset is None else kb.process_resets(x, reset)
    if mode == 'async':
        a, b = kb.alloc_host(T), kb.alloc_host(T)
        a[:] = x
        if reset is None:
            kb.process_async(a, b)
        else:
            kb.process_async_resets(a, b, reset)
        kb.synchronize()
        return b.copy()
    import torch
    xd = torch.from_numpy(x).cuda()
    yd = xd if mode == 'inplace' else torch.zeros_like(xd)
    torch.cuda.synchronize()
    if reset is None:
        kb.process_device(T, xd.data_ptr(), yd.data_ptr())
    else:
        kb.process_device_resets(T, xd.data_ptr(), yd.data_ptr(), reset)
    kb.synchronize()
    return yd.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 7. mixed gains, every route

# (precision, streams, max frames, [(frames, mode)], routes that must have been taken)
SHAPES = [
    ('fp32', 21, 4, [(1, 'host'), (4, 'host'), (1, 'host'), (1, 'host'), (4, 'inplace')], (ROUTE_SMALL, ROUTE_WAVE)),
    ('bf16', 21, 4, [(1, 'host'), (1, 'host'), (4, 'host'), (1, 'device'), (4, 'inplace')], (ROUTE_SMALL, ROUTE_WAVE)),
    ('bf16', 1024, 48, [(48, 'device'), (1, 'device'), (32, 'device'), (1, 'host'), (8, 'inplace')],
     (ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_CHUNKED)),
    # host calls of 16 MiB: sub-chunks of 4 12 12 4 frames on three streams (each takes the route of a call of its length); asynchronous: whole
    ('bf16', 1024, 32, [(32, 'host'), (32, 'async'), (32, 'host')], (ROUTE_PIPELINED,)),
    ('bf16', 4100, 4, [(4, 'device'), (1, 'device'), (4, 'inplace')], (ROUTE_CHUNKED,)),  # resident8; 257 m-tiles, the last one ragged
    ('fp32', 4100, 2, [(2, 'device'), (1, 'device'), (2, 'inplace')], (ROUTE_CHUNKED,)),  # fp32 chunked (more than 256 m-tiles)
    ('fp32', 512, 4, [(4, 'device'), (1, 'host'), (4, 'host')], (ROUTE_WAVE, ROUTE_SMALL)),
]


@pytest.mark.parametrize('precision,B,Tmax,calls,routes', SHAPES, ids=['%s-%dx%d' % (s[0], s[1], s[2]) for s in SHAPES])
def test_mixed_gains_match_the_recipe(random_model, precision, B, Tmax, calls, routes):
    if any(m != 'host' and m != 'async' for _, m in calls):
        pytest.importorskip('torch')
    total = sum(T for T, _ in calls)
    xc = synth_streams(NCLS, total, seed=21)
    cls = np.random.default_rng(B).integers(0, NCLS, B)
    cls[:NCLS] = np.arange(NCLS)  # (every class somewhere)
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
    cls = np.random.default_rng(5).integers(0, NCLS, B)
    cls[:NCLS] = np.arange(NCLS)
    rng = np.random.default_rng(6)
    rc = [(rng.random((NCLS, T)) < 0.2).astype(np.uint8) for _ in range(2)]
    rc[0][2, 0] = rc[0][2, 1] = rc[1][3, T - 1] = 1  # frame 0, adjacent frames, the last frame
    kb = batch(random_model, B, T, precision)
    rec = Recipe(random_model, NCLS, precision)
    kb.set_min_gain(GAINS[cls])
    for n in range(2):
        xn = frames(xc, n * T, (n + 1) * T)
        got = call(kb, xn[cls], mode, np.ascontiguousarray(rc[n][cls]))
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
    cls = np.random.default_rng(7).integers(0, NCLS, B)
    cls[:NCLS] = np.arange(NCLS)
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
