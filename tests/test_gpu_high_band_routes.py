"""
The high-band carry (include/pv_koala_batch.h: HIGH-BAND CARRY; DESIGN.md section 2, ninth extension) on a real MI355X, at the sizes and
inputs tests/test_gpu_high_band.py (B = 4, T <= 3, noise of peak 20000) does not reach: every route of Engine::run_device's dispatch table
under the carry, with the route of the inner 16 kHz call read back from the developer library, and inputs at and near full scale.

Every comparison is ==.  Handle A is plain and asked for its report, handle B carries and gets the same call; B's samples must equal
tests/high_band_recipe.HighBand(x, A's samples, A's mask_sum, the gains) -- in both precisions, since high_band_kernel<R> sees int16 samples
and the float report only -- and B's report, when it is asked for one, must be A's bit for bit (a call that asks for none has its rows
written to the engine's own d_hb_rep_).  What this pins of the engine block (kns_engine.cpp, run_call_rate): that every route leaves the
in-stage's rows in d_in_ as they are, that the report rows of every route (inside the quad kernel's synthesis launch, per slice of the
layer pipeline) are complete when the carry's kernel reads them, and the copy of the input kept in d_hb_in_ where the out-stage writes
over it.

A batch holds 16 distinct streams -- white noise up to Nyquist, every stream its own, the last one digital silence -- tiled over all B
slots: the first replica is compared with the recipe, every other replica must equal the first.

Routes.  A handle with a rate hands its inner call to run_call as a device-pointer call from d_in_ to d_out_ with the caller's T, so it takes
the row of test_dispatch_routes (tests/test_gpu_parity.py) of its (precision, B, T): no route is out of its reach, and every route of the
table below is asserted from the read-back after every call.  The call that carries frame-0 reset flags (B = 4100, the one-frame call) took
route 0, the chunked route, at both rates: flags on frame 0 alone are a masked reset in front of the call, not ROUTE_RESETS (6).
"""
import numpy as np
import pytest

from conftest import model_file
from gpu_kit import (DEV_LIB, ROUTE_CHUNKED, ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_SMALL, ROUTE_WAVE, batch, call, cut, replicas, route_info,
                     route_of, same, tiled)
from high_band_recipe import EDGE_GAINS, EDGE_SEQ, RATES, HighBand, edge_conditions, edge_streams
from koala_amd import formats
from koala_amd.channels import deinterleave, interleave

pytestmark = pytest.mark.gpu

R = 16  # distinct streams of a batch
GAINS = np.array([0.0, 0.25, 1.0, 0.0, 0.5, 0.25, 0.0, 0.1, 0.25, 0.0, 0.0, 1.0, 0.7, 0.0, 0.25, 0.5], np.float32)
FLAGGED = (2, 7, 11)  # the streams whose frame 0 carries a reset flag in the flagged call


def make(B, Tmax, rate, precision, carry, **kw):
    return batch(model_file('random'), B, Tmax, precision, DEV_LIB, sample_rate=rate, high_band='carry' if carry else None, **kw)


def noise(rate, frames, seed, peak=20000):
    """white noise (flat to Nyquist), every stream its own; the last stream is digital silence"""
    x = np.random.default_rng(seed).integers(-peak, peak + 1, size=(R, frames * rate * 256 // 16000)).astype(np.int16)
    x[R - 1] = 0
    return x


# ------------------------------------------------------------------------------------------------ 1. routes

Q, W, P, C0, S = ROUTE_QUAD1, ROUTE_WAVE, ROUTE_PIPELINED, ROUTE_CHUNKED, ROUTE_SMALL
# (precision, rate, streams, max frames, [(frames, mode, ask B for a report, the inner call's route)], the call with frame-0 flags)
SHAPES = [
    # one-step quad kernel on the one-frame calls: the state spans three of them, then a call that makes the history row-internal, then a
    # one-frame call that reads 48 y and all x history from state
    ('bf16', 48000, 960, 4, [(1, 'device', True, Q), (1, 'inplace', False, Q), (1, 'device', False, Q), (4, 'inplace', True, W), (1, 'device', True, Q)], None),
    # chunked: 257 m-tiles, the last one ragged (Bpad_ != B_)
    ('bf16', 32000, 4100, 2, [(2, 'device', True, C0), (1, 'inplace', False, C0), (2, 'inplace', True, C0)], 1),
    ('bf16', 48000, 4100, 2, [(2, 'device', True, C0), (1, 'inplace', False, C0), (2, 'inplace', True, C0)], 1),
    # layer pipeline on the 32-frame calls, the second without a report (the rows come from d_hb_rep_); chunked on the 5-frame call
    ('bf16', 32000, 784, 32, [(32, 'device', True, P), (32, 'inplace', False, P), (5, 'device', True, C0)], None),
    ('bf16', 48000, 784, 32, [(32, 'device', True, P), (32, 'inplace', False, P), (5, 'device', True, C0)], None),
    ('fp32', 48000, 256, 32, [(32, 'device', False, W), (1, 'host', True, S)], None),  # wavefront on a long call
    ('fp32', 32000, 4112, 2, [(2, 'inplace', False, C0), (1, 'device', True, C0)], None),
]


@pytest.mark.parametrize('precision,rate,B,Tmax,calls,flagged', SHAPES, ids=['%s-%d-%dx%d' % s[:4] for s in SHAPES])
def test_every_route_equals_the_recipe_over_the_plain_handle(precision, rate, B, Tmax, calls, flagged):
    ka, kb, ref = make(B, Tmax, rate, precision, False), make(B, Tmax, rate, precision, True), HighBand(R, rate)
    x16 = cut(noise(rate, sum(c[0] for c in calls), 61), rate, [c[0] for c in calls])
    gain, taken = GAINS, []
    for h in (ka, kb):
        h.set_min_gain(tiled(gain, B))
    for n, (T, mode, ask, route) in enumerate(calls):
        if n == 1:
            gain = np.roll(GAINS, 3)
            for h in (ka, kb):
                h.set_min_gain(tiled(gain, B))
        kw = {}
        if n == flagged:
            flags = np.zeros((R, T), np.uint8)
            flags[list(FLAGGED), 0] = 1
            kw = {'reset': tiled(flags, B)}
            ref.reset(flags[:, 0])
        x = tiled(x16[n], B)
        e, rep = call(ka, x, mode, report=True, **kw)
        taken.append(route_of(ka))
        got = call(kb, x, mode, report=ask, **kw)
        taken.append(route_of(kb))
        y, rep_b = got if ask else (got, None)
        print(n, T, mode, ask, 'routes (A, B):', taken[-2:])
        assert taken[-2:] == [route, route], (n, taken)
        want = ref.process(x16[n], e[:R], rep[:R, :, 2], gain)
        assert np.array_equal(y[:R], want), (n, mode, int((y[:R] != want).sum()), sorted(set(np.nonzero(y[:R] != want)[0].tolist())))
        assert replicas(y, R), (n, mode)
        assert rep_b is None or same(rep_b, rep), (n, mode)
        # a band was added on every stream but the silent one -- once a stream is older than D, which is longer than a frame: not in a first
        # call, and not on the streams that a one-frame call's flags have just made fresh
        old = [b for b in range(R - 1) if n > 0 and not (n == flagged and T == 1 and b in FLAGGED)]
        assert (y[old] != e[old]).any(axis=1).all(), (n, mode)
        assert not y[R - 1].any()
    ka.delete(), kb.delete()


def test_six_one_frame_calls_on_the_quad_route_equal_one_six_frame_call():
    """samples and report rows, both handles carrying: the carry's state across one-frame calls (x history over two calls, y history, the pair
    of gains) against the same frames row-internal"""
    B, K, rate = 960, 6, 32000
    x = tiled(noise(rate, K, 62), B)
    k1, kt = make(B, K, rate, 'bf16', True), make(B, K, rate, 'bf16', True)
    for h in (k1, kt):
        h.set_min_gain(tiled(GAINS, B))
    ys, reps = [], []
    for t, p in enumerate(cut(x, rate, [1] * K)):
        y, rep = call(k1, p, 'inplace' if t % 2 else 'device', report=True)
        info = route_info(k1)
        assert int(info[0]) == ROUTE_QUAD1 and info[2] == 1, (t, info)  # the route, and the mask head rode in the synthesis launch
        ys.append(y), reps.append(rep)
    yt, rt = call(kt, x, 'device', report=True)
    assert route_of(kt) != ROUTE_QUAD1
    y1 = np.concatenate(ys, axis=1)
    assert np.array_equal(y1, yt), int((y1 != yt).sum())
    assert same(np.concatenate(reps, axis=1), rt)
    assert replicas(yt, R) and (yt[:R - 1, -512:] != 0).any(axis=1).all()
    k1.delete(), kt.delete()


def test_formats_channels_and_the_link_stay_outside_at_a_chunked_shape():
    """case 5 of tests/test_gpu_high_band.py (float32 samples, interleaved channels, linked masks, 48 kHz, its call sequence) at B = 4104 with
    C = 8: the group's max runs over 8 report rows, and the call -- in place on the handle's own rows, whatever the caller's pointers are --
    keeps its input in d_hb_in_ on the chunked route (257 m-tiles, the last one a single group)"""
    rate, C, B = 48000, 8, 4104
    kw = dict(sample_format='f32', channels=C, channel_link='max')
    ka, kb, ref = make(B, 3, rate, 'bf16', False, **kw), make(B, 3, rate, 'bf16', True, **kw), HighBand(R, rate, channels=C)
    for h in (ka, kb):
        h.set_min_gain(tiled(GAINS, B))
    x = noise(rate, sum(EDGE_SEQ), 63)
    x[R - 1] = x[0] // 2  # (every channel a signal: the group max is taken over unequal masks)
    for i, p in enumerate(cut(x, rate, EDGE_SEQ)):
        xf = formats.encode('f32', interleave(tiled(p, B), C))
        mode = 'inplace' if i % 2 else 'device'
        e, rep = call(ka, xf, mode, report=True)
        y = call(kb, xf, mode)
        assert route_of(ka) == ROUTE_CHUNKED and route_of(kb) == ROUTE_CHUNKED, i
        want = ref.process(p, deinterleave(formats.decode('f32', e), C)[:R], rep[:R, :, 2], GAINS)
        assert same(y, formats.encode('f32', interleave(tiled(want, B), C))), (i, mode)
        assert len(set(rep[:C, 0, 2].tolist())) == C  # (the channels' own masks differ: the max over all eight matters)
    ka.delete(), kb.delete()


# ------------------------------------------------------------------------------------------------ 2. inputs at and near full scale

@pytest.mark.parametrize('mode', ['device', 'inplace'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('rate', RATES)
def test_inputs_at_the_rails_equal_the_recipe_over_the_plain_handle(rate, precision, mode):
    """tests/high_band_recipe.edge_streams (DC at either rail, the rails alternating at Nyquist in either phase, full-range noise, an impulse on
    a call's last sample, a step, +-1 dither; each with g = 0 and with g = 1) through test_gpu_high_band's call sequence at B = 16: Lf leaves
    the int16 range, E has been saturated by the out-stage, the sum saturates again -- all three asserted from the recipe and A alone."""
    ka, kb = make(R, 3, rate, precision, False), make(R, 3, rate, precision, True)
    ref, probe = HighBand(R, rate), HighBand(R, rate)
    for h in (ka, kb):
        h.set_min_gain(EDGE_GAINS)
    lf, es, wants = [], [], []
    for i, x in enumerate(cut(edge_streams(rate), rate, EDGE_SEQ)):
        e, rep = call(ka, x, mode, report=True)
        if i % 2:
            y, rep_b = call(kb, x, mode, report=True)
            assert same(rep_b, rep), i
        else:
            y = call(kb, x, mode)
        lf.append(probe.parts(x, rep[:, :, 2], EDGE_GAINS)[1])
        want = ref.process(x, e, rep[:, :, 2], EDGE_GAINS)
        assert np.array_equal(y, want), (i, int((y != want).sum()), sorted(set(np.nonzero(y != want)[0].tolist())))
        es.append(e), wants.append(want)
    held = edge_conditions(np.concatenate(lf, axis=1), np.concatenate(es, axis=1), np.concatenate(wants, axis=1))
    print(held)
    assert all(held.values()), held
    ka.delete(), kb.delete()
