"""
Linked channels (include/pv_koala_batch.h: LINKED CHANNELS; DESIGN.md section 2, eighth extension) on a real MI355X: the kLink arm of the
synthesis kernels (koala_amd/csrc/kns_stft_synthesis.inc) through the product library, with device pointers between guard zones
(tests/gpu_kit.call), every channel its own signal, the `random` model.

B = 24 streams are two mask tiles, the second ragged (8 rows); C = 8 makes groups that span a wave pair.  fp32 is compared with == against
tests/channel_link_recipe.LinkRecipe (the oracle's stages and the rule in numpy).  In bf16 the GPU's raw masks are not the oracle's, so
the linked handle L is compared with == against oracle.synthesis(spectrum, link_masks(the mask tap of an unlinked twin U), tail) per stream
from a reset: the synthesis stage is fp32 and exact in both precisions.  The one-frame bf16 route forms its mask inside the synthesis launch
(kMaskIn), where it never leaves LDS and no tap serves it: that route is covered with distinct channels by
tests/test_gpu_channel_link_routes.py (one-frame calls == one long call that is held to the tapped-mask reference, on the small and the quad
route), which also walks the other routes, segment lengths and packet phases this module's one size does not reach.  A handle with channels runs on device rows whatever the caller's pointers are, so its one-frame
calls never take the host route's graph.
"""
import numpy as np
import pytest

import koala_amd
from channel_link_recipe import LinkRecipe
from conftest import model_file, synth_streams
from frame_report_recipe import applied_mask
from gpu_kit import call, frames, same
from koala_amd import KoalaError, KoalaInvalidArgumentError
from koala_amd.channels import deinterleave, interleave, link_masks
from oracle import oracle

pytestmark = pytest.mark.gpu

SHAPES = [(2, 24), (4, 24), (8, 24)]
T = 3


def make(B, C, precision, link, **kw):
    return koala_amd.create_batch('key', B, T, precision, model_path=model_file('random'), channels=C, channel_link='max' if link else None, **kw)


def calls(B, C, seed):
    """the call list of tests 1 and 2: (planar samples, mode, per-frame resets, gains)"""
    x = synth_streams(B, 4 * T + 2, seed)
    rs = np.zeros((B, T), np.uint8)
    rs[0, 1] = rs[C - 1, 2] = rs[B - 1, 0] = rs[17, 1] = 1  # (differing within their groups)
    g = np.tile(np.array([0.0, 0.25, 1.0, 0.0, 1.0, 0.25, 0.0, 0.0], np.float32), B // 8 + 1)[:B]
    return [(frames(x, 0, T), 'device', None, None), (frames(x, T, 2 * T), 'inplace', None, None),
            (frames(x, 2 * T, 2 * T + 1), 'device', None, None), (frames(x, 2 * T + 1, 2 * T + 2), 'inplace', None, None),
            (frames(x, 2 * T + 2, 3 * T + 2), 'device', rs, None), (frames(x, 3 * T + 2, 4 * T + 2), 'device', None, g)]


def run(kb, C, x, mode, rs, g):
    if g is not None:
        kb.set_min_gain(g)
    kw = {} if rs is None else {'reset': rs}
    return call(kb, interleave(x, C), mode, report=True, **kw)


@pytest.mark.parametrize('C,B', SHAPES)
def test_fp32_every_form_equals_the_recipe(C, B):
    """multi-frame out of place (recomputed spectrum) and in place (stored), one-frame calls, per-frame resets and gains that differ within a
    group: samples and report rows == the recipe's"""
    kl = make(B, C, 'fp32', True)
    assert kl.channel_link == 'max'
    ref = LinkRecipe(model_file('random'), B, C)
    for i, (x, mode, rs, g) in enumerate(calls(B, C, 11)):
        y, rep = run(kl, C, x, mode, rs, g)
        want, wrep = ref.process(x, g, rs)
        assert np.array_equal(y, interleave(want, C)), (i, mode)
        assert same(rep, wrep), (i, mode, np.abs(rep - wrep).max())
    kl.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('C,B', SHAPES)
def test_output_is_the_synthesis_of_the_twins_tapped_masks_linked(C, B, precision):
    """every frame route, both precisions: L's samples == oracle.synthesis(X, m'(link_masks(mask tap of U)), tail) per stream, the tail
    kept here from the reset on.  X is the oracle's analysis of the same samples (the analysis stage is exact in both precisions; where
    the engine stored its spectrum -- the in-place calls -- the tap must equal it).  The one-frame calls come last: in bf16 their mask is
    formed inside the launch and the tap refuses, which ends the comparison (see the module's docstring)."""
    kl, ku = make(B, C, precision, True), make(B, C, precision, False)
    an = oracle.Oracle(model_file('random'), 1)
    hist, tail, gain = np.zeros((B, 256), np.int16), np.zeros((B, 256), np.float32), np.zeros(B, np.float32)
    cs = calls(B, C, 12)
    compared = 0
    for i, (x, mode, rs, g) in enumerate(cs[:2] + cs[4:] + cs[2:4]):
        (yl, _), _ = run(kl, C, x, mode, rs, g), run(ku, C, x, mode, rs, g)
        gain = gain if g is None else g
        n = x.shape[1] // 256
        try:
            m = ku.debug_read('mask', n)  # [n, B, 257]
        except KoalaError:
            assert precision == 'bf16' and n == 1, (i, mode)
            break
        stored = ku.debug_read('spectrum', n) if mode == 'inplace' and n > 1 else None
        want = np.empty_like(x)
        for t in range(n):
            if rs is not None:
                hist[rs[:, t] != 0] = 0
                tail[rs[:, t] != 0] = 0
            ml = link_masks(m[t], C)
            for b in range(B):
                fr = x[b, t * 256:(t + 1) * 256]
                spec, _ = an.analysis(hist[b], fr)
                if stored is not None:
                    assert same(stored[t, b], spec), (i, t, b)
                want[b, t * 256:(t + 1) * 256] = oracle.synthesis(spec, applied_mask(ml[b], gain[b]), tail[b])
                hist[b] = fr
        assert np.array_equal(yl, interleave(want, C)), (i, mode)
        compared += 1
    assert compared >= 4
    kl.delete(), ku.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('C,B', SHAPES)
def test_state_records_e_in_and_mask_sum_are_the_unlinked_handles(C, B, precision):
    """the network never sees its own output: e_in and mask_sum of every frame are U's bit for bit while the samples differ (every channel
    has its own signal); and after one more frame with the link off on both -- the overlap-add tail is the one part of a record that
    follows the samples, and a frame rewrites it -- the stream records of L == U's, every byte"""
    kl, ku = make(B, C, precision, True), make(B, C, precision, False)
    assert kl.state_size == ku.state_size
    differ = False
    for i, (x, mode, rs, g) in enumerate(calls(B, C, 12)):
        (yl, rl), (yu, ru) = run(kl, C, x, mode, rs, g), run(ku, C, x, mode, rs, g)
        assert same(rl[..., [0, 2, 3]], ru[..., [0, 2, 3]]), (i, mode)
        differ = differ or not np.array_equal(yl, yu)
    assert differ
    assert not np.array_equal(kl.export_state(), ku.export_state())  # (the tails)
    kl.set_channel_link(None)
    x = synth_streams(B, 1, 13)
    run(kl, C, x, 'device', None, None), run(ku, C, x, 'device', None, None)
    assert np.array_equal(kl.export_state(), ku.export_state())
    kl.delete(), ku.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('C,B', SHAPES)
def test_identical_channels_give_exactly_the_unlinked_output(C, B, precision):
    """every route: a wrong lane or word in the partner fetch would pick up another group's mask"""
    kl, ku = make(B, C, precision, True), make(B, C, precision, False)
    for i, (x, mode, rs, g) in enumerate(calls(B, C, 14)):
        x = np.repeat(x[::C], C, axis=0)  # (every group: its first channel's samples in all channels)
        if rs is not None:
            rs = np.repeat(rs[::C], C, axis=0)  # (equal state needs equal resets)
        if g is not None:
            g = np.repeat(g[::C], C)
        (yl, rl), (yu, ru) = run(kl, C, x, mode, rs, g), run(ku, C, x, mode, rs, g)
        assert np.array_equal(yl, yu) and same(rl, ru), (i, mode)
    kl.delete(), ku.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('n', [1, T])
def test_toggling_the_link_between_calls(n, precision):
    """one handle goes off, off, on, on, off, off, on beside a never-linked and an always-linked twin; all three get the same calls and
    nothing else (no record moves between them).  The streams evolve alike under either setting but for the overlap-add tail, which a
    frame rewrites: a call whose predecessor ran under the same setting == the twin's of that setting in every sample, and a call right
    behind a switch == that twin's from its second frame on.  Toggling leaves no residue."""
    C, B = 2, 24
    k, off, on = make(B, C, precision, False), make(B, C, precision, False), make(B, C, precision, True)
    seq = [None, None, 'max', 'max', None, None, 'max']
    x = synth_streams(B, len(seq) * n, 15)
    prev = None
    for i, link in enumerate(seq):
        xi = interleave(frames(x, i * n, (i + 1) * n), C)
        k.set_channel_link(link)
        assert k.channel_link == link and off.channel_link is None and on.channel_link == 'max'
        got, a, b = call(k, xi, 'device'), call(off, xi, 'device'), call(on, xi, 'device')
        want, other = (b, a) if link else (a, b)
        assert not np.array_equal(a, b), i
        if link == prev:
            assert np.array_equal(got, want), (i, link)
        else:
            assert np.array_equal(got[:, 256 * C:], want[:, 256 * C:]), (i, link)
            assert n == 1 or not np.array_equal(got[:, 256 * C:], other[:, 256 * C:]), (i, link)
        prev = link
    for h in (k, off, on):
        h.delete()


def test_unequal_hold_is_refused_and_changes_nothing():
    C, B = 2, 24
    kl, twin = make(B, C, 'fp32', True), make(B, C, 'fp32', True)
    x = synth_streams(B, 2 * T, 16)
    first = interleave(frames(x, 0, T), C)
    assert np.array_equal(kl.process(first), twin.process(first))
    hold = np.zeros(B, np.uint8)
    hold[5] = 1  # (stream 5 is channel 1 of group 2; its partner, stream 4, is not held)
    before = kl.export_state()
    with pytest.raises(KoalaInvalidArgumentError) as e:
        kl.process_hold(interleave(frames(x, T, 2 * T), C), hold)
    text = str(e.value) + ' '.join(getattr(e.value, 'message_stack', []) or [])
    assert 'group 2' in text and 'streams 4 and 5' in text and 'hold' in text, text
    assert np.array_equal(kl.export_state(), before)
    hold[4] = 1  # the group as a whole: legal
    second = interleave(frames(x, T, 2 * T), C)
    a, b = kl.process_hold(second, hold), twin.process_hold(second, hold)
    keep = np.ones(B // C, bool)
    keep[2] = False  # (a held group's elements are unspecified)
    assert np.array_equal(a[keep], b[keep])
    assert np.array_equal(kl.export_state(), twin.export_state())
    kl.delete(), twin.delete()


# ------------------------------------------------------------------------------------------------ another rate and a format

def test_a_48_khz_f32_handle_is_the_composition_around_the_linked_16_khz_call():
    """== encode(out-stage(linked 16 kHz call(in-stage(decode(x))))): tests/sample_rate_recipe.Recipe with the linked recipe as its inner
    engine, tests/sample_format_recipe around it"""
    import sample_format_recipe as sf
    import sample_rate_recipe as srr
    C, B, rate = 2, 6, 48000
    F = rate * 256 // 16000
    kl = make(B, C, 'fp32', True, sample_rate=rate, sample_format='f32')
    rec = srr.Recipe(model_file('random'), B, 'fp32', rate)
    link = LinkRecipe(model_file('random'), B, C)

    class Inner:
        def process(self, x16):
            return link.process(x16)[0]
    rec.o = Inner()
    x = (synth_streams(B, 2 * T * 3, 17)[:, :2 * T * F].astype(np.float32) / np.float32(32768)).astype(np.float32)
    for k in range(2):
        part = np.ascontiguousarray(x[:, k * T * F:(k + 1) * T * F])
        got = call(kl, interleave(part, C), 'device' if k == 0 else 'inplace')
        want = sf.encode(sf.F32, rec.process(sf.decode(sf.F32, part)))
        assert same(got, interleave(want, C)), k
    kl.delete()


# ------------------------------------------------------------------------------------------------ packet handles

def packet_handle(B, C, n, rate=16000, link=True):
    return koala_amd.create_batch('key', B, 1, 'fp32', model_path=model_file('random'), sample_rate=rate, packet_samples=n, channels=C,
                                  channel_link='max' if link else None)


def test_a_16_khz_packet_handle_is_the_frame_recipe_behind_the_packet_delay():
    """160-sample packets, C = 2: the concatenated output == the linked frame recipe's, frame_length - 1 samples later"""
    C, B, n, packets = 2, 4, 160, 8
    kp = packet_handle(B, C, n)
    x = synth_streams(B, 5, 18)  # 8 x 160 = 5 frames
    out = [deinterleave(kp.process_packets(interleave(np.ascontiguousarray(x[:, k * n:(k + 1) * n]), C), [n] * B), C) for k in range(packets)]
    got = np.concatenate(out, axis=1)
    want, _ = LinkRecipe(model_file('random'), B, C).process(x)
    assert not got[:, :255].any() and np.array_equal(got[:, 255:], want[:, :packets * n - 255])
    plain, _ = LinkRecipe(model_file('random'), B, C, link=False).process(x)
    assert not np.array_equal(got[:, 255:], plain[:, :packets * n - 255])
    kp.delete()


def test_a_44100_hz_packet_handle_is_the_fractional_stages_around_the_linked_16_khz_packet_call():
    """C = 2 at 44 100 Hz: per stream tests/fractional_rate_recipe's in-stage and out-stage in numpy, and between them the linked 16 kHz
    packet handle of the test above, given every call's inner samples of all streams together (the same cuts the engine makes)"""
    import fractional_rate_recipe as frr
    C, B, rate, n = 2, 4, 44100, 882
    k44, k16 = packet_handle(B, C, n, rate), packet_handle(B, C, int(frr.inner_samples(n, rate)) + 1)
    st = [frr.Stream(rate, None) for _ in range(B)]
    x = synth_streams(B, 12, 19)
    at = 0
    for count in (882, 441, 700, 1, 882):
        part = np.ascontiguousarray(x[:, at:at + count])
        at += count
        row = np.zeros((B, n), np.int16)
        row[:, :count] = part
        got = deinterleave(k44.process_packets(interleave(row, C), [count] * B), C)[:, :count]
        y = np.stack([s.in_stage(part[b]) for b, s in enumerate(st)])
        m = y.shape[1]
        v = deinterleave(k16.process_packets(interleave(y, C), [m] * B), C) if m else y
        want = np.stack([s.out_stage(v[b], count) for b, s in enumerate(st)])
        for s in st:
            s.phase = (s.phase + count) % frr.D
        assert np.array_equal(got, want), count
    k44.delete(), k16.delete()


# ------------------------------------------------------------------------------------------------ refusals of a packet call

def refused(call):
    with pytest.raises(KoalaInvalidArgumentError) as e:
        call()
    return str(e.value)


@pytest.mark.parametrize('rate,n', [(16000, 160), (44100, 441)])
def test_unequal_restart_and_a_group_out_of_phase_are_refused_and_change_nothing(rate, n):
    C, B = 2, 4
    kl, twin = packet_handle(B, C, n, rate), packet_handle(B, C, n, rate)
    x = synth_streams(B, 12, 20)  # (six packets of n <= 441 samples)
    part = lambda k, m=n: interleave(np.ascontiguousarray(x[:, k * n:k * n + m]), C)
    full = [n] * B
    assert np.array_equal(kl.process_packets(part(0), full), twin.process_packets(part(0), full))
    # restart that differs within group 1 (streams 2 and 3)
    text = refused(lambda: kl.process_packets(part(1), full, restart=[0, 0, 0, 1]))
    assert 'restart' in text and 'group 1' in text and 'streams 2 and 3' in text, text
    assert np.array_equal(kl.process_packets(part(1), full), twin.process_packets(part(1), full))  # (nothing had changed)
    # a whole group restarting is legal
    r = [1, 1, 0, 0]
    assert np.array_equal(kl.process_packets(part(2), full, restart=r), twin.process_packets(part(2), full, restart=r))
    # a masked reset of one channel leaves group 0 out of phase: legal per stream, reported by the packet call
    mask = np.array([1, 0, 0, 0], np.uint8)
    kl.reset(mask)
    text = refused(lambda: kl.process_packets(part(3), full))
    assert 'out of phase' in text and 'group 0' in text and 'streams 0 and 1' in text, text
    text = refused(lambda: kl.process_packets(part(3), full))  # (still: the refused call moved nothing)
    assert 'out of phase' in text
    # a reset of the whole group cures it; the twin never saw the refused calls
    whole = np.array([1, 1, 0, 0], np.uint8)
    kl.reset(whole), twin.reset(whole)
    for k in (3, 4):
        assert np.array_equal(kl.process_packets(part(k), full), twin.process_packets(part(k), full)), k
    # with the link off the same de-phased group is today's handle: accepted
    kl.reset(mask)
    kl.set_channel_link(None)
    kl.process_packets(part(5), full)
    kl.delete(), twin.delete()
