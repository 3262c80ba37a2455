"""
Band profile (include/pv_koala_batch.h: pv_koala_batch_set_band_profile, pv_koala_set_band_profile; DESIGN.md section 2, tenth extension)
on a real MI355X: the kProfile arm of koala_amd/csrc/kns_stft.hip's synthesis kernels under every route of the dispatch table.

The expected samples come from the oracle's stage functions under the rule (tests/band_profile_recipe.py).  fp32 comparisons are ==;
bf16 within the suite's bars (tests/gpu_kit.py), against the bf16 oracle under the same rule.  The rule's exact consequences are tested
with == in both precisions.  16 distinct streams, tiled over larger batches; T <= 3 unless a route needs more.
"""
import functools

import numpy as np
import pytest

import gpu_kit
import koala_amd
from band_profile_recipe import GAINS, K, ProfileRecipe, profiles
from gpu_kit import (DEV_LIB, MARK, ROUTE_CHUNKED, ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_SMALL, ROUTE_WAVE, check_pcm, delayed, frames, replicas,
                     route_of, same, streams, tiled)
from koala_amd import bands

pytestmark = pytest.mark.gpu

batch = functools.partial(gpu_kit.batch, lib=DEV_LIB)
call = gpu_kit.call
N = 16  # distinct streams
PRECISIONS = ['fp32', 'bf16']


def mixed(n=N, seed=0):
    """(floor, ceiling, gains) of n streams: tests/band_profile_recipe.py's profiles, g of 0, 0.25 and 1 among the gains"""
    lo, hi = profiles(n, seed)
    return lo, hi, np.resize(GAINS, n)


def configure(kb, lo, hi, g):
    B = kb.num_streams
    kb.set_band_profile(tiled(lo, B), tiled(hi, B))
    kb.set_min_gain(tiled(g[:, None], B)[:, 0])


# ------------------------------------------------------------------------------------------------ 1. recipe parity

@pytest.mark.parametrize('precision', PRECISIONS)
def test_a_profile_per_stream_matches_the_recipe(random_model, precision):
    lo, hi, g = mixed()
    x = streams(N, 6 * 256, seed=31)
    kb = batch(random_model, N, 3, precision)
    configure(kb, lo, hi, g)
    for b in range(N):
        flo, fhi = kb.band_profile(b)
        assert same(flo, lo[b]) and same(fhi, hi[b])
    rec = ProfileRecipe(random_model, N, precision)
    got = np.concatenate([call(kb, frames(x, 0, 3), 'host'), call(kb, frames(x, 3, 4), 'host'), call(kb, frames(x, 4, 6), 'host')], axis=1)
    kb.delete()
    want = rec.process(x, g, lo, hi)
    check_pcm(got, want, precision, 'profile per stream')
    plain = ProfileRecipe(random_model, N, precision).process(x, g)
    assert (want != plain).any()  # (the profile does something)


# ------------------------------------------------------------------------------------------------ 2. exact properties

@pytest.mark.parametrize('precision', PRECISIONS)
def test_neutral_profile_is_the_handle_without(random_model, precision):
    x = streams(N, 5 * 256, seed=32)
    kb, plain = batch(random_model, N, 3, precision), batch(random_model, N, 3, precision)
    lo, hi, g = mixed()
    configure(kb, lo, hi, 0 * g)
    kb.process(frames(x, 0, 1))
    plain.process(frames(x, 0, 1))
    kb.set_band_profile()  # back to neutral: the plain routes and kernels, and from the second frame on the plain samples
    for t0, t1 in ((1, 2), (2, 5)):
        a, b = kb.process(frames(x, t0, t1)), plain.process(frames(x, t0, t1))
        assert route_of(kb) == route_of(plain)
        assert same(a[:, 256 if t0 == 1 else 0:], b[:, 256 if t0 == 1 else 0:])
    fresh = batch(random_model, N, 3, precision)
    fresh.set_band_profile(np.zeros(K, np.float32), np.ones(K, np.float32))
    fresh2 = batch(random_model, N, 3, precision)
    for t0, t1 in ((0, 1), (1, 4)):
        assert same(fresh.process(frames(x, t0, t1)), fresh2.process(frames(x, t0, t1))) and route_of(fresh) == route_of(fresh2)
    for h in (kb, plain, fresh, fresh2):
        h.delete()


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('kind', ['random', 'default'])
def test_all_ones_is_a_pure_delay(random_model, gate_model, kind, precision):
    x = streams(N, 5 * 256, seed=33)
    kb = batch(random_model if kind == 'random' else gate_model, N, 3, precision)
    kb.set_band_profile(np.ones(K, np.float32), np.ones(K, np.float32))
    got = np.concatenate([kb.process(frames(x, 0, 1)), kb.process(frames(x, 1, 4)), kb.process(frames(x, 4, 5))], axis=1)
    kb.delete()
    assert same(got, delayed(x))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_zero_ceiling_is_silence_from_the_second_frame(random_model, precision):
    x = streams(N, 5 * 256, seed=34)
    kb = batch(random_model, N, 3, precision)
    kb.process(frames(x, 0, 1))
    kb.set_band_profile(None, np.zeros(K, np.float32))
    y1, r1 = kb.process_call(frames(x, 1, 4), report=True)
    y2, r2 = kb.process_call(frames(x, 4, 5), report=True)
    kb.delete()
    assert not r1[:, :, 1].any() and not r2[:, :, 1].any() and r1[:, :, 0].all()  # e_out == 0 in every frame, e_in is not
    assert y1[:, :256].any() and not y1[:, 256:].any() and not y2.any()  # (the first frame carries the tail made under the old profile)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_the_network_never_sees_its_own_output(random_model, precision):
    lo, hi, g = mixed()
    x = streams(N, 4 * 256, seed=35)
    kb, plain = batch(random_model, N, 3, precision), batch(random_model, N, 3, precision)
    configure(kb, lo, hi, g)
    differs = False
    for t0, t1 in ((0, 3), (3, 4)):
        (ya, ra), (yb, rb) = kb.process_call(frames(x, t0, t1), report=True), plain.process_call(frames(x, t0, t1), report=True)
        assert same(ra[:, :, 0], rb[:, :, 0]) and same(ra[:, :, 2], rb[:, :, 2])  # e_in, mask_sum
        differs = differs or not same(ra[:, :, 1], rb[:, :, 1])
        assert same(kb.debug_read('hidden', t1 - t0), plain.debug_read('hidden', t1 - t0))
    assert differs  # (e_out is of the shaped mask)
    # records: everything but the overlap-add tail, which is made of the samples -- equal where the profile is neutral (stream 3 of `profiles`, g = 0)
    ra, rb = kb.export_state(), plain.export_state()
    from stream_state_recipe import OFF_TAIL
    tail = slice(OFF_TAIL, OFF_TAIL + 1024)
    keep = np.ones(ra.shape[1], bool)
    keep[tail] = False
    assert same(ra[:, keep], rb[:, keep]) and same(ra[3], rb[3]) and not same(ra[:, tail], rb[:, tail])
    assert kb.state_size == plain.state_size
    kb.delete()
    plain.delete()


# ------------------------------------------------------------------------------------------------ 3. every route

# the smallest (precision, B, T) row of tests/test_gpu_parity.py::test_dispatch_routes that reaches each route, and a ragged last m-tile
ROUTES = [('bf16', 16, 1, ROUTE_SMALL), ('bf16', 960, 1, ROUTE_QUAD1), ('bf16', 64, 4, ROUTE_WAVE), ('bf16', 1040, 2, ROUTE_CHUNKED),
          ('bf16', 784, 32, ROUTE_PIPELINED), ('fp32', 256, 1, ROUTE_SMALL), ('fp32', 64, 2, ROUTE_WAVE), ('fp32', 4112, 1, ROUTE_CHUNKED),
          ('fp32', 21, 3, None), ('bf16', 3093, 1, None)]


@pytest.mark.parametrize('precision,B,T,route', ROUTES, ids=['%s-%dx%d' % r[:3] for r in ROUTES])
def test_every_route(random_model, precision, B, T, route):
    pytest.importorskip('torch')
    lo, hi, g = mixed()
    x16 = streams(N, 2 * T * 256, seed=36)
    kb, plain = batch(random_model, B, T, precision), batch(random_model, B, T, precision)
    configure(kb, lo, hi, g)
    rec = ProfileRecipe(random_model, N, precision)
    for c in range(2):
        xn = tiled(frames(x16, c * T, (c + 1) * T), B)
        got = call(kb, xn, 'device')
        taken = route_of(kb)
        call(plain, xn, 'device')
        assert taken == route_of(plain) and (route is None or taken == route), (taken, route)
        assert replicas(got, N)
        check_pcm(got[:N], rec.process(frames(x16, c * T, (c + 1) * T), g, lo, hi), precision, 'route %d call %d' % (taken, c))
    kb.delete()
    plain.delete()


# ------------------------------------------------------------------------------------------------ 4. some streams, changed between calls

@pytest.mark.parametrize('precision', PRECISIONS)
def test_resets_and_held_streams_under_a_changing_profile(random_model, precision):
    pytest.importorskip('torch')
    lo, hi, g = mixed()
    nlo, nhi = bands.neutral()
    some = np.arange(0, N, 2)  # the profile on every other stream only
    lo[1::2], hi[1::2] = nlo, nhi
    x = streams(N, 6 * 256, seed=37)
    reset = np.zeros((N, 3), np.uint8)
    reset[[1, 2, 5], [1, 2, 1]] = 1
    kb = batch(random_model, N, 3, precision)
    kb.set_min_gain(g)
    kb.set_band_profile(lo[some], hi[some], streams=some)
    rec = ProfileRecipe(random_model, N, precision)
    check_pcm(call(kb, frames(x, 0, 3), 'device', reset=reset), rec.process_resets(frames(x, 0, 3), g, reset, lo, hi), precision, 'resets')
    # changed: the two halves swap; streams 4 .. 7 are held in the next call and continue in the one after
    lo2, hi2 = np.roll(lo, 1, axis=0), np.roll(hi, 1, axis=0)
    kb.set_band_profile(lo2, hi2)
    hold = np.zeros(N, np.uint8)
    hold[4:8] = 1
    run = hold == 0
    got = call(kb, frames(x, 3, 4), 'host', hold=hold)
    held = ProfileRecipe(random_model, N, precision)  # (the held streams' expectation: a second recipe that skips the call)
    held.process_resets(frames(x, 0, 3), g, reset, lo, hi)
    want4 = rec.process(frames(x, 3, 4), g, lo2, hi2)
    check_pcm(got[run], want4[run], precision, 'hold: the running streams')
    got5 = call(kb, frames(x, 4, 5), 'host')
    want_run, want_held = rec.process(frames(x, 4, 5), g, lo2, hi2), held.process(frames(x, 4, 5), g, lo2, hi2)
    check_pcm(got5[run], want_run[run], precision, 'after hold: the running streams')
    check_pcm(got5[~run], want_held[~run], precision, 'after hold: the held streams')
    kb.delete()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_an_asynchronous_call_keeps_the_profile_it_was_issued_under(random_model, precision):
    lo, hi, g = mixed()
    x = streams(N, 4 * 256, seed=38)
    kb = batch(random_model, N, 2, precision)
    kb.set_min_gain(g)
    kb.set_band_profile(lo, hi)
    a, ya, b, yb = (kb.alloc_host(2) for _ in range(4))
    a[:], b[:] = frames(x, 0, 2), frames(x, 2, 4)
    lo2, hi2 = np.roll(lo, 3, axis=0), np.roll(hi, 3, axis=0)
    kb.process_async(a, ya)
    kb.set_band_profile(lo2, hi2)  # at once: the call in flight shows A, the next one B
    kb.process_async(b, yb)
    kb.synchronize()
    rec = ProfileRecipe(random_model, N, precision)
    check_pcm(ya, rec.process(frames(x, 0, 2), g, lo, hi), precision, 'in flight: profile A')
    check_pcm(yb, rec.process(frames(x, 2, 4), g, lo2, hi2), precision, 'next: profile B')
    kb.delete()


# ------------------------------------------------------------------------------------------------ 5. single-stream ABI

def test_single_stream_frames_are_the_batch_call(random_model):
    lo, hi = profiles(2, seed=5)
    x = streams(1, 6 * 256, seed=39)
    kb = batch(random_model, 1, 6, 'fp32')
    kb.set_band_profile(lo[:1], hi[:1])
    want, wrep = kb.process_call(x, report=True)
    kb.delete()
    k = koala_amd.create('key', model_path=random_model, library_path=DEV_LIB)
    k.set_band_profile(lo[0], hi[0])
    flo, fhi = k.band_profile()
    assert same(flo, lo[0]) and same(fhi, hi[0])
    got = []
    for t in range(6):  # the one-frame graph path, alternating calls with and without a report
        fr = np.ascontiguousarray(x[0, t * 256:(t + 1) * 256])
        if t & 1:
            y, rep = k.process_with_report(fr)
            assert same(rep, wrep[0, t])
        else:
            y = k.process(fr)
        got.append(np.array(y, np.int16))
    k.delete()
    assert same(np.concatenate(got)[None], want)


# ------------------------------------------------------------------------------------------------ 6. outer layers

class _Inner:
    """a 16 kHz planar handle under the same configuration as the inner engine of a layer's numpy transform"""

    def __init__(self, model, n, T, lo, hi, g):
        self.kb = batch(model, n, T, 'fp32')
        self.kb.set_min_gain(g)
        self.kb.set_band_profile(lo, hi)

    def process(self, x):
        return self.kb.process(np.ascontiguousarray(x, np.int16))


def test_a_48_khz_frame_handle(random_model):
    from sample_rate_recipe import Recipe as RateRecipe
    lo, hi, g = mixed(4)
    x = streams(4, 2 * 768, seed=40)
    kb = batch(random_model, 4, 2, 'fp32', sample_rate=48000)
    kb.set_min_gain(g)
    kb.set_band_profile(lo, hi)
    rec = RateRecipe(None, 4, 'fp32', 48000)
    rec.o = _Inner(random_model, 4, 2, lo, hi, g)
    assert same(kb.process(x), rec.process(x))
    rec.o.kb.delete()
    kb.delete()


def test_an_8_khz_ulaw_handle(random_model):
    from sample_format_recipe import ULAW, decode, encode
    from sample_rate_recipe import Recipe as RateRecipe
    lo, hi, g = mixed(4)
    x = encode(ULAW, streams(4, 3 * 128, seed=41))
    kb = batch(random_model, 4, 3, 'fp32', sample_rate=8000, sample_format='ulaw')
    kb.set_min_gain(g)
    kb.set_band_profile(lo, hi)
    rec = RateRecipe(None, 4, 'fp32', 8000)
    rec.o = _Inner(random_model, 4, 3, lo, hi, g)
    assert same(kb.process(x), encode(ULAW, rec.process(decode(ULAW, x))))
    rec.o.kb.delete()
    kb.delete()


def test_a_two_channel_handle(random_model):
    from koala_amd.channels import deinterleave, interleave
    lo, hi, g = mixed(4)
    x = streams(2, 3 * 512, seed=42)
    kb = batch(random_model, 4, 3, 'fp32', channels=2)
    kb.set_min_gain(g)
    kb.set_band_profile(lo, hi)
    inner = _Inner(random_model, 4, 3, lo, hi, g)
    assert same(kb.process(x), interleave(inner.process(deinterleave(x, 2)), 2))
    inner.kb.delete()
    kb.delete()


def test_a_packet_handle_with_ragged_counts(random_model):
    from packet_recipe import PacketStream
    lo, hi, g = mixed(4)
    counts = np.array([[300, 0, 512, 77], [212, 256, 1, 435], [256, 500, 255, 0]], np.int32)
    x = streams(4, 512 * 3, seed=43)
    kb = batch(random_model, 4, 1, 'fp32', packet_samples=512)
    kb.set_min_gain(g)
    kb.set_band_profile(lo, hi)
    recs = [ProfileRecipe(random_model, 1, 'fp32') for _ in range(4)]
    ps = [PacketStream(lambda fr, b=b: recs[b].process(fr[None], g[b:b + 1], lo[b:b + 1], hi[b:b + 1])[0], 256) for b in range(4)]
    pos = np.zeros(4, int)
    for c in counts:
        pcm = np.zeros((4, 512), np.int16)
        for b in range(4):
            pcm[b, :c[b]] = x[b, pos[b]:pos[b] + c[b]]
        got = kb.process_packets(pcm, c)
        for b in range(4):
            assert same(got[b, :c[b]], ps[b].push(x[b, pos[b]:pos[b] + c[b]])), (b, c)
            pos[b] += c[b]
    kb.delete()


# ------------------------------------------------------------------------------------------------ 7. the two refusals

@pytest.mark.parametrize('what', ['link', 'carry'])
def test_refused_with_the_link_or_the_carry_on(random_model, what):
    pytest.importorskip('torch')
    kw = dict(channels=2, channel_link='max') if what == 'link' else dict(sample_rate=48000, high_band='carry')
    F = 768 if what == 'carry' else 256
    B, T = 4, 2
    kb, twin = batch(random_model, B, T, 'fp32', **kw), batch(random_model, B, T, 'fp32', **kw)
    x = streams(B, 2 * T * F, seed=44).reshape(B // (2 if what == 'link' else 1), -1)
    half = x.shape[1] // 2
    x0, x1 = np.ascontiguousarray(x[:, :half]), np.ascontiguousarray(x[:, half:])
    assert same(call(kb, x0, 'device'), call(twin, x0, 'device'))
    kb.set_band_profile(None, bands.highpass(90.0))
    with pytest.raises(koala_amd.KoalaInvalidArgumentError) as e:
        call(kb, x1, 'device')  # (gpu_kit.call: `enhanced` lies between guard zones)
    assert 'band profile' in str(e.value) and ('channel link' if what == 'link' else 'high-band carry') in str(e.value)
    import torch
    out = torch.full((x1.size,), MARK, dtype=torch.int16, device='cuda')
    src = torch.from_numpy(x1.reshape(-1)).cuda()
    with pytest.raises(koala_amd.KoalaInvalidArgumentError):
        kb.process_device(T, src.data_ptr(), out.data_ptr())
    kb.synchronize()
    assert (out.cpu().numpy() == MARK).all()  # nothing processed
    kb.set_band_profile()  # neutral again: the next call continues where the stream was
    assert same(call(kb, x1, 'device'), call(twin, x1, 'device'))
    kb.delete()
    twin.delete()
