"""
Comfort noise (include/pv_koala_batch.h: pv_koala_batch_set_comfort_noise; DESIGN.md section 2, twelfth extension) on a real MI355X: the
kComfort arm of koala_amd/csrc/kns_stft.hip's synthesis kernels and the counter's launch (kns_comfort.hip) under every route of the
dispatch table.

The expected samples come from the oracle's stage functions under the rule (tests/comfort_recipe.py).  fp32 comparisons are ==; bf16 within
the suite's bars (tests/gpu_kit.py), against the bf16 oracle under the same rule.  The rule's exact consequences are tested with == in both
precisions.  16 distinct streams, tiled over larger batches; T <= 4 unless a route needs more.
"""
import functools

import numpy as np
import pytest

import gpu_kit
import koala_amd
from band_profile_recipe import GAINS, profiles
from comfort_recipe import K, ComfortRecipe, curves
from frame_report_recipe import BF16_E_OUT_REL
from gpu_kit import DEV_LIB, MARK, check_pcm, delayed, frames, replicas, route_of, same, streams, tiled
from test_gpu_band_profile import ROUTES

pytestmark = pytest.mark.gpu

batch = functools.partial(gpu_kit.batch, lib=DEV_LIB)
call = gpu_kit.call
N = 16  # distinct streams
PRECISIONS = ['fp32', 'bf16']
F32 = np.float32


def mixed(n=N, seed=0):
    """(floor, ceiling, gains, curves, seeds, on) of n streams: the profiles and gains of tests/band_profile_recipe.py, a curve and a seed
    per stream, every fifth stream off"""
    lo, hi = profiles(n, seed)
    on = np.arange(n) % 5 != 4
    return lo, hi, np.resize(GAINS, n), curves(n, seed + 1), (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(7)), on


def configure(kb, lo, hi, g, amp, seeds, on):
    B = kb.num_streams
    col = lambda v: tiled(np.asarray(v)[:, None], B)[:, 0]
    kb.set_band_profile(tiled(lo, B), tiled(hi, B))
    kb.set_min_gain(col(g))
    kb.set_comfort_noise(tiled(amp, B), col(seeds))
    off = np.flatnonzero(~col(on))
    if off.size:
        kb.set_comfort_noise(None, col(seeds)[off], streams=off, on=False)


def plainly(kb, amp, seeds=None):
    """comfort noise on every stream of a handle without gains or a profile"""
    B = kb.num_streams
    kb.set_comfort_noise(tiled(amp, B), seeds)


# ------------------------------------------------------------------------------------------------ 1. recipe parity

@pytest.mark.parametrize('precision', PRECISIONS)
def test_settings_per_stream_match_the_recipe(random_model, precision):
    B, T = 21, 3
    lo, hi, g, amp, seeds, on = mixed(B)
    x = streams(B, 2 * T * 256, seed=51)
    kb = batch(random_model, B, T, precision)
    configure(kb, lo, hi, g, amp, seeds, on)
    for b in (0, 4, 20):
        fon, fseed, famp = kb.comfort_noise(b)
        assert fon == bool(on[b]) and fseed == int(seeds[b]) and same(famp, amp[b])
    # off and on again without a seed: the stream keeps the seed it was given, and its curve
    kb.set_comfort_noise(streams=[3], on=False)
    assert kb.comfort_noise(3)[:2] == (False, int(seeds[3]))
    kb.set_comfort_noise(streams=[3])
    fon, fseed, famp = kb.comfort_noise(3)
    assert fon and fseed == int(seeds[3]) and same(famp, amp[3])
    rec = ComfortRecipe(random_model, B, precision)
    got = np.concatenate([call(kb, frames(x, 0, T), 'host'), call(kb, frames(x, T, 2 * T), 'device')], axis=1)
    assert same(kb.comfort_state(), rec.count + np.where(on, 2 * T, 0).astype(np.uint32))
    kb.delete()
    want = rec.process(x, g, lo, hi, amp, seeds, on)
    check_pcm(got, want, precision, 'comfort noise per stream')
    plain = ComfortRecipe(random_model, B, precision).process(x, g, lo, hi, amp, seeds, np.zeros(B, bool))
    assert (want[on] != plain[on]).any() and same(want[~on], plain[~on])  # (the fill does something, and only where it is on)


# ------------------------------------------------------------------------------------------------ 2. every route

@pytest.mark.parametrize('precision,B,T,route', ROUTES, ids=['%s-%dx%d' % r[:3] for r in ROUTES])
def test_every_route(random_model, precision, B, T, route):
    pytest.importorskip('torch')
    lo, hi, g, amp, seeds, on = mixed()
    x16 = streams(N, 2 * T * 256, seed=52)
    kb, plain = batch(random_model, B, T, precision), batch(random_model, B, T, precision)
    configure(kb, lo, hi, g, amp, seeds, on)
    rec = ComfortRecipe(random_model, N, precision)
    for c in range(2):  # (two calls: the counter crosses a call boundary)
        xn = tiled(frames(x16, c * T, (c + 1) * T), B)
        got = call(kb, xn, 'device')
        taken = route_of(kb)
        call(plain, xn, 'device')
        assert taken == route_of(plain) and (route is None or taken == route), (taken, route)
        assert replicas(got, N)
        check_pcm(got[:N], rec.process(frames(x16, c * T, (c + 1) * T), g, lo, hi, amp, seeds, on), precision, 'route %d call %d' % (taken, c))
    kb.delete()
    plain.delete()


# ------------------------------------------------------------------------------------------------ 3. exact consequences

@pytest.mark.parametrize('precision', PRECISIONS)
def test_min_gain_one_is_still_the_pure_delay(random_model, precision):
    x = streams(N, 5 * 256, seed=53)
    kb = batch(random_model, N, 3, precision)
    plainly(kb, curves(N, 3) + F32(0.01))
    kb.set_min_gain(np.ones(N, F32))
    got = np.concatenate([kb.process(frames(x, 0, 1)), kb.process(frames(x, 1, 4)), kb.process(frames(x, 4, 5))], axis=1)
    kb.delete()
    assert same(got, delayed(x))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_a_zero_curve_is_off_and_nothing_upstream_moves(random_model, precision):
    x = streams(N, 4 * 256, seed=54)
    amp = curves(N, 4) + F32(0.01)
    amp[::2] = 0  # (every other stream: a zero curve)
    kb, plain = batch(random_model, N, 3, precision), batch(random_model, N, 3, precision)
    plainly(kb, amp)
    rec = ComfortRecipe(random_model, N, precision)
    zero = np.zeros(N, F32)
    for t0, t1 in ((0, 3), (3, 4)):
        (ya, ra), (yb, rb) = kb.process_call(frames(x, t0, t1), report=True), plain.process_call(frames(x, t0, t1), report=True)
        assert same(ya[::2], yb[::2]) and not same(ya[1::2], yb[1::2])
        assert same(ra[:, :, 0], rb[:, :, 0]) and same(ra[:, :, 2], rb[:, :, 2])  # e_in, mask_sum
        assert same(kb.debug_read('hidden', t1 - t0), plain.debug_read('hidden', t1 - t0))
        rec.process(frames(x, t0, t1), zero, None, None, amp, np.arange(N), None)
        # e_out is that of Y: the recipe's, bit for bit in fp32; in bf16 the engine's mask differs from the bf16 oracle's in the last bit now and
        # then (tests/gpu_kit.py), so the suite's bar for e_out holds -- tests/frame_report_recipe.py's, made for m' X: the fill changes Y by
        # (m_engine - m_oracle) (X - A z), and |A z| < 0.04 is far below |X| on these streams.  (The fixed-mask case below is exact in bf16 too.)
        rel = np.abs(ra[:, :, 1].astype(np.float64) - rec.e_out) / rec.e_out
        print('%s e_out against the recipe: max relative distance %.3e' % (precision, rel.max()))
        assert same(ra[:, :, 1], rec.e_out) if precision == 'fp32' else rel.max() <= BF16_E_OUT_REL
        assert not same(ra[1::2, :, 1], rb[1::2, :, 1])
    assert kb.state_size == plain.state_size
    kb.delete()
    plain.delete()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_a_fixed_mask_puts_the_noise_in_the_stop_bins_only(tmp_path, precision):
    """tests/edge_recipe.py's `comb`: the mask is exactly 1 on the even bins and sigmoid(-30) (fp16: 0) on the odd ones in every precision, so
    samples and e_out are the recipe's bit for bit in bf16 as well -- a slip in the hash or in a bin's index cannot hide behind the mask.
    (The `spectrum` debug tap holds X, not Y: the check is on the samples and on e_out.)  Stream 0 is silence: X = 0, so its samples are the
    fill alone -- the recipe's w = 0 on the passband bins and w = 1 - sigmoid(-30) on the others -- and any noise on a passband bin, or the
    wrong variate on a stop bin, moves them."""
    from edge_recipe import model_path
    model = model_path(tmp_path, 'comb')
    amp = curves(N, 6) + F32(0.01)
    seeds = np.arange(N, dtype=np.uint32) + np.uint32(1000)
    x = streams(N, 6 * 256, seed=65)
    x[0] = 0  # silence: X = 0, Y is the fill alone
    kb = batch(model, N, 3, precision)
    kb.set_comfort_noise(amp, seeds)
    rec = ComfortRecipe(model, N, precision)
    zero = np.zeros(N, F32)
    for t0, t1, mode in ((0, 3, 'host'), (3, 6, 'device')):
        y, rep = call(kb, frames(x, t0, t1), mode, report=True)
        want = rec.process(frames(x, t0, t1), zero, None, None, amp, seeds, None)
        assert same(y, want) and same(rep[:, :, 1], rec.e_out), (precision, t0)
        assert y[0, 256:].any() and (rep[0, :, 0] == 0).all() and (rep[0, :, 1] > 0).all()  # (silence in, the fill out)
    kb.delete()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_equal_seeds_give_equal_rows_and_different_seeds_do_not(random_model, precision):
    x = tiled(streams(1, 3 * 256, seed=55), 4)
    kb = batch(random_model, 4, 3, precision)
    kb.set_comfort_noise(curves(1, 5)[0] + F32(0.01), np.array([9, 9, 10, 9], np.uint32))
    got = kb.process(x)
    kb.delete()
    assert same(got[0], got[1]) and same(got[0], got[3]) and not same(got[0], got[2])


# ------------------------------------------------------------------------------------------------ 4. state

@pytest.mark.parametrize('precision', PRECISIONS)
def test_resets_holds_and_the_counter(random_model, precision):
    pytest.importorskip('torch')
    T = 4
    lo, hi, g, amp, seeds, on = mixed()
    x = streams(N, 11 * 256, seed=56)
    reset = np.zeros((N, T), np.uint8)
    reset[[1, 2, 5, 9], [0, 1, T - 1, 1]] = 1  # frames 0, 1 and T - 1 (stream 9 is off)
    kb = batch(random_model, N, T, precision)
    configure(kb, lo, hi, g, amp, seeds, on)
    rec = ComfortRecipe(random_model, N, precision)
    args = (lo, hi, amp, seeds, on)
    check_pcm(call(kb, frames(x, 0, 4), 'device', reset=reset), rec.process_resets(frames(x, 0, 4), g, reset, *args), precision, 'resets')
    assert same(kb.comfort_state(), rec.count)
    # a masked reset
    m = np.zeros(N, np.uint8)
    m[[0, 3]] = 1
    kb.reset(m)
    rec.reset(m != 0)
    assert same(kb.comfort_state(), rec.count)
    # hold, T = 1 then T = 4: streams 4 .. 7 stand still and continue sample for sample afterwards
    hold = np.zeros(N, np.uint8)
    hold[4:8] = 1
    run = hold == 0
    held = ComfortRecipe(random_model, N, precision)
    held.process_resets(frames(x, 0, 4), g, reset, *args)
    held.reset(m != 0)
    for t0, t1 in ((4, 5), (5, 9)):
        got = call(kb, frames(x, t0, t1), 'device', hold=hold)
        check_pcm(got[run], rec.process(frames(x, t0, t1), g, *args)[run], precision, 'hold: the running streams')
    count = np.where(run, rec.count, held.count)
    assert same(kb.comfort_state(), count)
    got = call(kb, frames(x, 9, 11), 'host')
    want_run, want_held = rec.process(frames(x, 9, 11), g, *args), held.process(frames(x, 9, 11), g, *args)
    check_pcm(got[run], want_run[run], precision, 'after hold: the running streams')
    check_pcm(got[~run], want_held[~run], precision, 'after hold: the held streams')
    kb.delete()


def test_a_stream_moves_with_its_record_and_its_counter(random_model):
    lo, hi, g, amp, seeds, on = mixed(4)
    on[:] = True
    x = streams(4, 5 * 256, seed=57)
    a, b = batch(random_model, 4, 3, 'fp32'), batch(random_model, 4, 3, 'fp32')
    configure(a, lo, hi, g, amp, seeds, on)
    rec, stay = ComfortRecipe(random_model, 4, 'fp32'), ComfortRecipe(random_model, 4, 'fp32')
    assert same(a.process(frames(x, 0, 3)), rec.process(frames(x, 0, 3), g, lo, hi, amp, seeds, on))
    stay.process(frames(x, 0, 3), g, lo, hi, amp, seeds, on)  # (a second recipe for what stays on `a`)
    # stream 1 of `a` goes to slot 3 of `b`: its record, its counter, and its configuration
    assert same(b.comfort_state(), np.zeros(4, np.uint32))  # (a handle that never filled)
    b.import_state(a.export_state([1]), [3])
    b.set_comfort_state(a.comfort_state([1]), [3])
    b.set_min_gain(np.array([0, 0, 0, g[1]], F32))
    b.set_band_profile(lo[1:2], hi[1:2], streams=[3])
    b.set_comfort_noise(amp[1], seeds[1], streams=[3])
    y = np.zeros((4, 2 * 256), np.int16)
    y[3] = x[1, 3 * 256:]
    want = rec.process(frames(x, 3, 5), g, lo, hi, amp, seeds, on)
    assert same(b.process(y)[3], want[1])
    # off and on again: no frame counts while a stream is off, and the count continues from where it stood
    a.set_comfort_noise(on=False)
    off = np.zeros(4, bool)
    assert same(a.process(frames(x, 3, 4)), stay.process(frames(x, 3, 4), g, lo, hi, amp, seeds, off))
    assert same(a.comfort_state(), np.full(4, 3, np.uint32))
    a.set_comfort_noise()
    assert same(a.process(frames(x, 4, 5)), stay.process(frames(x, 4, 5), g, lo, hi, amp, seeds, on)) and same(stay.count, np.full(4, 4, np.uint32))
    a.delete()
    b.delete()


# ------------------------------------------------------------------------------------------------ 5. outer layers

class _Inner:
    """a 16 kHz planar handle under the same configuration as the inner engine of a layer's numpy transform"""

    def __init__(self, model, n, T, cfg, **kw):
        self.kb = batch(model, n, T, 'fp32', **kw)
        configure(self.kb, *cfg)

    def process(self, x):
        return self.kb.process(np.ascontiguousarray(x, np.int16))


def test_an_8_khz_ulaw_handle(random_model):
    from sample_format_recipe import ULAW, decode, encode
    from sample_rate_recipe import Recipe as RateRecipe
    cfg = mixed(4)
    x = encode(ULAW, streams(4, 3 * 128, seed=58))
    kb = batch(random_model, 4, 3, 'fp32', sample_rate=8000, sample_format='ulaw')
    configure(kb, *cfg)
    rec = RateRecipe(None, 4, 'fp32', 8000)
    rec.o = _Inner(random_model, 4, 3, cfg)
    assert same(kb.process(x), encode(ULAW, rec.process(decode(ULAW, x))))
    rec.o.kb.delete()
    kb.delete()


def test_a_48_khz_two_channel_handle(random_model):
    from koala_amd.channels import deinterleave, interleave
    from sample_rate_recipe import Recipe as RateRecipe
    cfg = mixed(4)
    x = streams(2, 2 * 2 * 768, seed=59)
    kb = batch(random_model, 4, 2, 'fp32', sample_rate=48000, channels=2)
    configure(kb, *cfg)
    rec = RateRecipe(None, 4, 'fp32', 48000)
    rec.o = _Inner(random_model, 4, 2, cfg)
    assert same(kb.process(x), interleave(rec.process(deinterleave(x, 2)), 2))
    rec.o.kb.delete()
    kb.delete()


def test_a_packet_handle_with_ragged_counts_a_stall_and_a_restart(random_model):
    from packet_recipe import PacketStream
    lo, hi, g, amp, seeds, on = mixed(4)
    counts = np.array([[300, 0, 512, 77], [212, 256, 1, 435], [256, 500, 255, 0], [256, 256, 256, 256]], np.int32)
    restart = np.zeros((4, 4), np.uint8)
    restart[3, 2] = 1
    x = streams(4, 512 * 4, seed=60)
    kb = batch(random_model, 4, 1, 'fp32', packet_samples=512)
    configure(kb, lo, hi, g, amp, seeds, on)
    recs = [ComfortRecipe(random_model, 1, 'fp32') for _ in range(4)]
    one = lambda b: (g[b:b + 1], lo[b:b + 1], hi[b:b + 1], amp[b:b + 1], seeds[b:b + 1], on[b:b + 1])
    mk = lambda b: PacketStream(lambda fr: recs[b].process(fr[None], *one(b))[0], 256)
    ps = [mk(b) for b in range(4)]
    pos = np.zeros(4, int)
    for c, r in zip(counts, restart):
        pcm = np.zeros((4, 512), np.int16)
        for b in range(4):
            pcm[b, :c[b]] = x[b, pos[b]:pos[b] + c[b]]
            if r[b]:
                recs[b].reset(np.ones(1, bool))
                ps[b] = mk(b)
        got, _ = gpu_kit.packet_call(kb, pcm, c, r if r.any() else None, mode='host')
        for b in range(4):
            assert same(got[b, :c[b]], ps[b].push(x[b, pos[b]:pos[b] + c[b]])), (b, c)
            pos[b] += c[b]
    assert same(kb.comfort_state(), np.concatenate([r.count for r in recs]))
    kb.delete()


def test_the_leveller_sees_the_noise(random_model):
    from koala_amd import level
    lo, hi, g, amp, seeds, on = mixed(4)
    x = streams(4, 3 * 256, seed=61)
    s = level.settings(theta=0.0, floor_dbfs=-90.0)
    kb, ref = batch(random_model, 4, 3, 'fp32'), batch(random_model, 4, 3, 'fp32')
    configure(kb, lo, hi, g, amp, seeds, on)
    configure(ref, lo, hi, g, amp, seeds, on)
    kb.set_level(s)
    E, rep = ref.process_call(x, report=True)
    want, _, _ = level.apply(E, rep, s)
    assert same(kb.process(x), want)
    kb.delete()
    ref.delete()


def test_the_single_stream_handle_through_host_pointers(random_model):
    amp = curves(1, 9)[0] + F32(0.01)
    x = streams(1, 4 * 256, seed=62)
    rec = ComfortRecipe(random_model, 1, 'fp32')
    want = rec.process(x, np.zeros(1, F32), None, None, amp[None], np.array([77], np.uint32))
    k = koala_amd.create('key', model_path=random_model, library_path=DEV_LIB)
    k.set_comfort_noise(amp, 77)
    fon, fseed, famp = k.comfort_noise()
    assert fon and fseed == 77 and same(famp, amp)
    got = [np.array(k.process(np.ascontiguousarray(x[0, t * 256:(t + 1) * 256])), np.int16) for t in range(4)]
    k.delete()
    assert same(np.concatenate(got)[None], want)


# ------------------------------------------------------------------------------------------------ 6. the refusals

@pytest.mark.parametrize('what', ['link', 'carry', 'async', '44100'])
def test_refusals_touch_nothing(random_model, what):
    pytest.importorskip('torch')
    import torch
    amp = curves(1, 11)[0] + F32(0.01)
    if what == '44100':
        kb = batch(random_model, 2, 1, 'fp32', sample_rate=44100, packet_samples=441)
        kb.set_comfort_noise(amp)
        pcm, c = streams(2, 441, seed=63), np.array([441, 441], np.int32)
        out = np.full_like(pcm, MARK)
        with pytest.raises(koala_amd.KoalaInvalidArgumentError) as e:
            kb._packets(441, c, pcm.ctypes.data, out.ctypes.data, None, None, 0)
        assert 'Comfort noise' in str(e.value) and '44100' in str(e.value)
        assert (out == MARK).all()  # nothing processed
        kb.set_comfort_noise(on=False)
        twin = batch(random_model, 2, 1, 'fp32', sample_rate=44100, packet_samples=441)
        assert same(gpu_kit.packet_call(kb, pcm, c, mode='host')[0], gpu_kit.packet_call(twin, pcm, c, mode='host')[0])
        kb.delete()
        twin.delete()
        return
    kw = dict(channels=2, channel_link='max') if what == 'link' else dict(sample_rate=48000, high_band='carry') if what == 'carry' else {}
    F = 768 if what == 'carry' else 256
    B, T = 4, 2
    kb, twin = batch(random_model, B, T, 'fp32', **kw), batch(random_model, B, T, 'fp32', **kw)
    x = streams(B, 2 * T * F, seed=64).reshape(B // (2 if what == 'link' else 1), -1)
    half = x.shape[1] // 2
    x0, x1 = np.ascontiguousarray(x[:, :half]), np.ascontiguousarray(x[:, half:])
    assert same(call(kb, x0, 'device'), call(twin, x0, 'device'))
    kb.set_comfort_noise(amp)
    name = {'link': 'channel link', 'carry': 'high-band carry', 'async': 'asynchronous'}[what]
    if what == 'async':
        a, b = kb.alloc_host(T), kb.alloc_host(T)
        a[:], b[:] = x1, MARK
        with pytest.raises(koala_amd.KoalaInvalidArgumentError) as e:
            kb.process_async(a, b)
        kb.synchronize()
        assert (b == MARK).all()
    else:
        out = torch.full((x1.size,), MARK, dtype=torch.int16, device='cuda')
        src = torch.from_numpy(x1.reshape(-1)).cuda()
        with pytest.raises(koala_amd.KoalaInvalidArgumentError) as e:
            kb.process_device(T, src.data_ptr(), out.data_ptr())
        kb.synchronize()
        assert (out.cpu().numpy() == MARK).all()  # nothing processed
    assert 'Comfort noise' in str(e.value) and name in str(e.value)
    assert same(kb.comfort_state(), np.zeros(B, np.uint32))
    if what == 'async':
        # the synchronous call that follows, comfort noise still on, is the recipe's: the refused call moved nothing
        rec, g = ComfortRecipe(random_model, B, 'fp32'), np.zeros(B, F32)
        rec.process(x0, g, on=np.zeros(B, bool))
        assert same(call(kb, x1, 'device'), rec.process(x1, g, None, None, tiled(amp[None], B), np.arange(B)))
        assert same(kb.comfort_state(), rec.count)
    else:
        # (no call with comfort noise on can follow on these handles, and a linked or carried stretch has no recipe without its feature:
        # off again, the next call continues where the twin is)
        kb.set_comfort_noise(on=False)
        assert same(call(kb, x1, 'device'), call(twin, x1, 'device'))
    kb.delete()
    twin.delete()
