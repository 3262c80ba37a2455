"""
Linked channels (include/pv_koala_batch.h: LINKED CHANNELS; DESIGN.md section 2, eighth extension) on a real MI355X, at the sizes
tests/test_gpu_channel_link.py (B = 24 streams, T = 3 frames) does not reach: every route of Engine::run_device's dispatch table with the
route read back from the developer library, synthesis segments longer than one frame, the one-frame bf16 route (the mask formed inside the
synthesis launch, kMaskIn, the partners read from LDS) with distinct channels, and packet handles whose groups are out of phase.

Every comparison is ==, on samples and on report rows.  fp32: tests/channel_link_recipe.LinkRecipe.  bf16: the synthesis stage is fp32 and
exact, so a linked handle L == oracle.synthesis(X, m'(link_masks(the mask tap of an unlinked twin U)), tail) per stream from a reset on
(`Tapped` below; the construction of test_gpu_channel_link's twin test), and a route that no tap serves is tied to that reference through
a handle that was given the same frames in another grouping.

Every channel carries its own signal.  A batch holds R = 16 distinct streams -- 16 / C whole groups -- tiled over all B slots in whole
groups (the last replica of B = 24, 40 and 4104 is cut at a group boundary): the first replica is compared with the reference, every other
replica must equal the first bit for bit.

What a handle with channels can and cannot reach: its call runs in place on the handle's own rows (Channels), so at
16 kHz / s16 every multi-frame linked call reads the STORED spectrum, whatever the caller's pointers are.  The recomputing linked kernels
(report forms only; a call without a report gives the report's descriptor no range) run where another stage stands between the rows and the
call: a sample format, a rate, the packetiser.  Hence the 'f32' handles below: the slices of the layer pipeline (t0c > 0: the mask offset,
the previous frame in the PCM) and the segment test's recomputing linked arms.

Segments: synthesis_slice (kns_engine.cpp, seg_auto) starts from min(T, 4) frames for calls of up to four and halves while
m-tiles x segments < 512.  B = 4104 x T = 4 is 257 m-tiles: seg 4 -> 257 x 1 < 512 -> seg 2 -> 257 x 2 = 514: the engine itself chooses
seg = 2 there, two frames behind one replayed frame per workgroup.  B = 1024 x T = 48 (64 m-tiles): 24 -> 12 -> 6, eight segments of six.
KOALA_AMD_SYNTH_SEG (developer library) forces any length at any size: test_segment_length_* below, for every arm of the kernel.
"""
import functools

import numpy as np
import pytest

from channel_link_recipe import LinkRecipe
from conftest import model_file, synth_streams
from frame_report_recipe import applied_mask, report_rows, row_sum
from gpu_kit import (DEV_LIB, ROUTE_CHUNKED, ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_RESETS, ROUTE_SMALL, ROUTE_WAVE, batch, call, frames, replicas,
                     route_info, route_of, same, streams, tiled)
from koala_amd.channels import deinterleave, interleave, link_masks
from oracle import oracle

pytestmark = pytest.mark.gpu

R = 16  # distinct streams of a batch: NG = 16 / C groups
GAINS = np.array([0.0, 0.25, 1.0, 0.0, 0.5, 0.25, 0.0, 0.1, 0.25, 0.0, 0.0, 1.0, 0.7, 0.0, 0.25, 0.5], np.float32)  # (differ within every group)
SEG_ENV = 'KOALA_AMD_SYNTH_SEG'


def make(B, C, T, precision, link=True, **kw):
    return batch(model_file('random'), B, T, precision, DEV_LIB, channels=C, channel_link='max' if link else None, **kw)


def as_f32(s):
    """int16 samples as the 'f32' format's (exact: 16 bits times a power of two)"""
    return (np.asarray(s, np.int16).astype(np.float32) / np.float32(32768)).astype(np.float32)


class Tapped:
    """n streams from a reset on: samples and report rows of a linked handle from raw masks tapped off an unlinked twin -- the oracle's
    analysis and synthesis, the rule in numpy, the tail kept here"""

    def __init__(self, n, C):
        self.n, self.C = n, C
        self.an = oracle.Oracle(model_file('random'), 1)
        self.hist, self.tail = np.zeros((n, 256), np.int16), np.zeros((n, 256), np.float32)

    def process(self, x, m, gain, stored=None):
        """x int16 [n, T * 256], m raw masks [T, n, 257], gain [n]; stored: the engine's spectrum tap [T, n, 257, 2] where it kept one, which
        must be the oracle's analysis"""
        T = x.shape[1] // 256
        want, rep = np.empty_like(x), np.zeros((self.n, T, 4), np.float32)
        for t in range(T):
            ml = link_masks(m[t], self.C)
            for b in range(self.n):
                fr = x[b, t * 256:(t + 1) * 256]
                spec, _ = self.an.analysis(self.hist[b], fr)
                if stored is not None:
                    assert same(stored[t, b], spec), (t, b)
                want[b, t * 256:(t + 1) * 256] = oracle.synthesis(spec, applied_mask(ml[b], gain[b]), self.tail[b])
                rep[b, t] = report_rows(spec, ml[b], gain[b])
                rep[b, t, 2] = row_sum(m[t, b])
                self.hist[b] = fr
        return want, rep


def where(got, want, C):
    """for a failing ==: (stream, frame) pairs of the first replica that differ, and how many samples"""
    d = np.asarray(got) != np.asarray(want)
    rows, cols = np.nonzero(d)
    return {'streams': sorted(set(rows.tolist())), 'frames': sorted(set((cols // 256).tolist())), 'samples': int(d.sum()), 'C': C}


# ------------------------------------------------------------------------------------------------ 1. routes, fp32: the recipe

# (precision, channels, streams, max frames, [(frames, mode)], routes that must have been taken)
FP32_SHAPES = [
    ('fp32', 2, 512, 4, [(4, 'device'), (1, 'device'), (4, 'inplace'), (1, 'inplace')], (ROUTE_WAVE, ROUTE_SMALL)),
    ('fp32', 4, 4104, 2, [(2, 'device'), (1, 'device'), (2, 'inplace')], (ROUTE_CHUNKED,)),  # 257 m-tiles, the last one 8 rows = two groups
]
BF16_SHAPES = [
    ('bf16', 2, 1024, 48, [(48, 'device'), (32, 'inplace'), (8, 'device')], (ROUTE_PIPELINED, ROUTE_CHUNKED)),
    ('bf16', 8, 4104, 4, [(4, 'device'), (4, 'inplace')], (ROUTE_CHUNKED,)),  # resident8; seg = 2 by the engine's own choice; ragged tile
    ('bf16', 4, 784, 8, [(4, 'device'), (8, 'inplace'), (3, 'device')], (ROUTE_WAVE, ROUTE_CHUNKED)),  # 49 m-tiles: wavefront up to 4 frames
]


def ids(shapes):
    return ['%s-c%d-%dx%d' % s[:4] for s in shapes]


@pytest.mark.parametrize('precision,C,B,Tmax,calls,routes', FP32_SHAPES, ids=ids(FP32_SHAPES))
def test_fp32_routes_equal_the_recipe(precision, C, B, Tmax, calls, routes):
    """samples and report rows of the first replica == LinkRecipe's; gains differ within every group and the second call brings a new table"""
    x1 = synth_streams(R, sum(T for T, _ in calls), 31)
    kl, ref = make(B, C, Tmax, precision), LinkRecipe(model_file('random'), R, C)
    gain = GAINS
    kl.set_min_gain(tiled(gain, B))
    taken, t0 = [], 0
    for n, (T, mode) in enumerate(calls):
        if n == 1:
            gain = np.roll(GAINS, 3)
            kl.set_min_gain(tiled(gain, B))
        xn = frames(x1, t0, t0 + T)
        y, rep = call(kl, interleave(tiled(xn, B), C), mode, report=True)
        taken.append(route_of(kl))
        yp = deinterleave(y, C)
        want, wrep = ref.process(xn, gain)
        assert np.array_equal(yp[:R], want), (n, mode, where(yp[:R], want, C))
        assert same(rep[:R], wrep), (n, mode)
        assert replicas(yp, R) and replicas(rep, R), (n, mode)
        t0 += T
    kl.delete()
    for r in routes:
        assert r in taken, (taken, routes)


# ------------------------------------------------------------------------------------------------ 2. routes, bf16: multi-frame calls

@pytest.mark.parametrize('precision,C,B,Tmax,calls,routes', BF16_SHAPES, ids=ids(BF16_SHAPES))
def test_bf16_routes_equal_the_synthesis_of_the_twins_tapped_masks(precision, C, B, Tmax, calls, routes):
    """L and its unlinked twin U get the same calls; the first replica of L == Tapped(the mask tap of U) in samples and report rows, U's
    stored spectrum == the oracle's analysis, and e_in / mask_sum of L are U's"""
    x1 = synth_streams(R, sum(T for T, _ in calls), 32)
    kl, ku, ref = make(B, C, Tmax, precision), make(B, C, Tmax, precision, link=False), Tapped(R, C)
    tables = [np.zeros(R, np.float32), GAINS, np.roll(GAINS, 5)]  # the first call runs without a limit
    taken, t0 = [], 0
    for n, (T, mode) in enumerate(calls):
        gain = tables[n]
        for h in (kl, ku):
            h.set_min_gain(tiled(gain, B))
        xn = frames(x1, t0, t0 + T)
        xi = interleave(tiled(xn, B), C)
        yl, rl = call(kl, xi, mode, report=True)
        taken.append(route_of(kl))
        yu, ru = call(ku, xi, mode, report=True)
        info = route_info(ku)
        assert int(info[0]) == taken[-1] and info[2] == 0, (n, info)  # the twin took the same route, its masks are in memory
        m = ku.debug_read('mask', T)[:, :R]
        stored = ku.debug_read('spectrum', T)[:, :R] if info[3] else None
        assert stored is not None  # (a handle with channels runs in place on its own rows: the module's docstring)
        want, wrep = ref.process(xn, m, gain, stored)
        yp = deinterleave(yl, C)
        assert np.array_equal(yp[:R], want), (n, mode, where(yp[:R], want, C))
        assert same(rl[:R], wrep), (n, mode)
        assert same(rl[..., [0, 2, 3]], ru[..., [0, 2, 3]]), (n, mode)
        assert replicas(yp, R) and replicas(rl, R), (n, mode)
        assert not np.array_equal(yl, yu), n
        t0 += T
    kl.delete(), ku.delete()
    for r in routes:
        assert r in taken, (taken, routes)


def test_bf16_pipeline_slices_recompute_linked_with_and_without_a_report():
    """B = 1024 x T = 48 through an 'f32' handle: the format stage stands between the handle's rows and the call, so the call is out of place,
    recomputes its spectrum, and the layer pipeline cuts its synthesis into two slices of 24 frames (t0c = 24: the mask offset, the previous
    frame in the PCM, the report rows offset), three frames a segment.  Its samples and rows == the s16 handle's of the same calls -- which
    the test above holds to the tapped-mask reference at this shape -- scaled by 2^-15; the first call asks for no report: the recomputing
    linked kernel with no report rows in range."""
    C, B, T = 2, 1024, 48
    x1 = synth_streams(R, 2 * T, 33)
    kf, ks = make(B, C, T, 'bf16', sample_format='f32'), make(B, C, T, 'bf16')
    for h in (kf, ks):
        h.set_min_gain(tiled(GAINS, B))
    for n in range(2):
        xi = interleave(tiled(frames(x1, n * T, (n + 1) * T), B), C)
        ys, rs = call(ks, xi, 'device', report=True)
        got = call(kf, as_f32(xi), 'device', report=n == 1)
        info = route_info(kf)
        assert int(info[0]) == ROUTE_PIPELINED and info[3] == 0, info  # pipelined, no spectrum stored
        assert route_of(ks) == ROUTE_PIPELINED
        yf, rf = got if n == 1 else (got, None)
        assert same(yf, as_f32(ys)), (n, where(deinterleave(yf, C)[:R], deinterleave(as_f32(ys), C)[:R], C))
        assert rf is None or same(rf, rs), n
    kf.delete(), ks.delete()


# ------------------------------------------------------------------------------------------------ 3. bf16 one-frame calls: the mask formed in the launch

@pytest.mark.parametrize('C,B,route', [(2, 24, ROUTE_SMALL), (4, 960, ROUTE_QUAD1), (8, 4096, ROUTE_QUAD1)])
def test_bf16_one_frame_calls_equal_one_long_call_linked_and_distinct(C, B, route):
    """K one-frame calls (the mask head inside the synthesis launch, the partners' values out of LDS) == one K-frame call, first unlinked
    -- the grouping alone -- then linked, in every sample and report row; and the K-frame linked call == Tapped(the unlinked K-frame
    call's masks), which pins the one-frame route to the oracle's synthesis without a tap"""
    K = 6
    x1 = synth_streams(R, K, 34)
    x = tiled(x1, B)
    out = {}
    for link in (False, True):
        k1, kt = make(B, C, K, 'bf16', link), make(B, C, K, 'bf16', link)
        for h in (k1, kt):
            h.set_min_gain(tiled(GAINS, B))
        ys, reps = [], []
        for t in range(K):
            y, rep = call(k1, interleave(frames(x, t, t + 1), C), 'inplace' if t % 2 else 'device', report=True)
            got = route_info(k1)
            assert int(got[0]) == route and got[2] == 1, (link, t, got)  # the route, and the mask head rode in the synthesis launch
            ys.append(deinterleave(y, C))
            reps.append(rep)
        y1, r1 = np.concatenate(ys, axis=1), np.concatenate(reps, axis=1)
        yt, rt = call(kt, interleave(x, C), 'device', report=True)
        yt = deinterleave(yt, C)
        assert np.array_equal(y1, yt), (link, where(y1, yt, C))
        assert same(r1, rt), link
        out[link] = (yt, rt, None if link else kt.debug_read('mask', K)[:, :R])
        k1.delete(), kt.delete()
    (yu, ru, m), (yl, rl, _) = out[False], out[True]
    want, wrep = Tapped(R, C).process(x1, m, GAINS)
    assert np.array_equal(yl[:R], want), where(yl[:R], want, C)
    assert same(rl[:R], wrep)
    assert replicas(yl, R) and replicas(rl, R) and not np.array_equal(yl, yu)


# ------------------------------------------------------------------------------------------------ 4. segment length, every arm

SEG_T = 7
ARMS = ('plain', 'min_gain', 'report', 'linked', 'linked_gains_report', 'linked_gains', 'linked_gains_report_f32', 'linked_gains_f32')


def seg_resets(C):
    """[R, SEG_T]: frame 0, the last frame, adjacent frames; they differ within their groups"""
    rs = np.zeros((R, SEG_T), np.uint8)
    rs[0, 1] = rs[3, 1] = rs[C - 1, 4] = rs[9, 6] = rs[14, 0] = rs[15, 5] = rs[6, 2] = rs[6, 3] = 1
    return rs


def run_arms(precision, B, C):
    """the three calls -- out of place, in place, per-frame resets that differ within a group -- through every arm, each on a handle of its
    own made under the environment as it is now -> arm: ([(samples, report or None)], records).  The planar arms recompute their spectrum
    out of place and store it in place; a linked s16 handle stores it in either mode, a linked 'f32' handle recomputes it in either mode
    (the module's docstring)."""
    x1 = synth_streams(R, 3 * SEG_T, 35)
    rs = tiled(seg_resets(C), B)
    gains = tiled(GAINS, B)
    seq = [('device', None), ('inplace', None), ('device', rs)]
    out = {}
    for arm in ARMS:
        linked, f32 = arm.startswith('linked'), arm.endswith('f32')
        kw = {'sample_format': 'f32'} if f32 else {}
        kb = make(B, C if linked else 1, SEG_T, precision, linked, **kw)
        if 'gain' in arm:
            kb.set_min_gain(gains)
        got = []
        for n, (mode, reset) in enumerate(seq):
            x = tiled(frames(x1, n * SEG_T, (n + 1) * SEG_T), B)
            x = interleave(x, C) if linked else x
            r = call(kb, as_f32(x) if f32 else x, mode, report='report' in arm, **({} if reset is None else {'reset': reset}))
            if reset is not None:
                assert route_of(kb) == ROUTE_RESETS, arm
            got.append(r if 'report' in arm else (r, None))
        out[arm] = (got, kb.export_state())
        kb.delete()
    return out


@functools.lru_cache(maxsize=None)
def unset_run(precision, B, C):
    """run_arms with the engine's own segment length: computed once per shape, shared by the tests below, left unchanged"""
    return run_arms(precision, B, C)


SEG_SHAPES = [(24, 8), (40, 2)]


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,C', SEG_SHAPES)
def test_segment_length_unset_arms_agree_and_fp32_is_the_recipe(B, C, precision, monkeypatch):
    monkeypatch.delenv(SEG_ENV, raising=False)
    base = unset_run(precision, B, C)
    calls = lambda arm: base[arm][0]
    for n in range(3):
        # a linked call without a report == with one, stored and recomputed; the 'f32' handle == the s16 handle, scaled
        assert same(calls('linked_gains')[n][0], calls('linked_gains_report')[n][0]), n
        assert same(calls('linked_gains_f32')[n][0], calls('linked_gains_report_f32')[n][0]), n
        assert same(calls('linked_gains_report_f32')[n][0], as_f32(calls('linked_gains_report')[n][0])), n
        assert same(calls('linked_gains_report_f32')[n][1], calls('linked_gains_report')[n][1]), n
        assert same(calls('report')[n][0], calls('plain')[n][0]), n
        assert not np.array_equal(calls('linked')[n][0], interleave(calls('plain')[n][0], C)), n
        for arm in ARMS:
            y = calls(arm)[n][0]
            assert replicas(deinterleave(y, C) if arm.startswith('linked') else y, R), (arm, n)
    if precision == 'fp32':
        x1, rs = synth_streams(R, 3 * SEG_T, 35), seg_resets(C)
        ref = LinkRecipe(model_file('random'), R, C)
        for n in range(3):
            want, wrep = ref.process(frames(x1, n * SEG_T, (n + 1) * SEG_T), GAINS, rs if n == 2 else None)
            y, rep = calls('linked_gains_report')[n]
            assert np.array_equal(deinterleave(y, C)[:R], want), (n, where(deinterleave(y, C)[:R], want, C))
            assert same(rep[:R], wrep), n


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,C', SEG_SHAPES)
@pytest.mark.parametrize('seg', [1, 2, 3, 5, 7])
def test_segment_length_changes_nothing_in_any_arm(seg, B, C, precision, monkeypatch):
    """T = 7 in segments of 1 (every frame behind its replayed predecessor), 2, 3, 5 (a ragged last segment) and 7 (one): samples, report
    rows and stream records of every arm == those under the engine's own choice"""
    monkeypatch.delenv(SEG_ENV, raising=False)
    base = unset_run(precision, B, C)
    monkeypatch.setenv(SEG_ENV, str(seg))
    forced = run_arms(precision, B, C)
    for arm in ARMS:
        for n, ((y, rep), (y0, rep0)) in enumerate(zip(forced[arm][0], base[arm][0])):
            assert same(y, y0), (arm, n, int((y != y0).sum()))
            assert rep0 is None or same(rep, rep0), (arm, n)
        assert np.array_equal(forced[arm][1], base[arm][1]), arm
    for n in range(3):
        assert same(forced['linked_gains'][0][n][0], forced['linked_gains_report'][0][n][0]), n
        assert same(forced['linked_gains_f32'][0][n][0], forced['linked_gains_report_f32'][0][n][0]), n


# ------------------------------------------------------------------------------------------------ 5. packet handles, groups out of phase

PACKET = 400
# counts per call and group, equal inside a group: group 1 is stalled in calls 1-3; no group has a frame due in call 3, group 1 alone in
# call 4; calls 5, 7, 9 and 11 are cut into two sub-calls, in the second of which the groups with one frame due are held
SCHEDULE = np.array([[400, 160, 1, 256], [400, 0, 255, 160], [256, 0, 400, 1], [160, 0, 1, 1], [1, 255, 1, 0], [255, 400, 160, 400],
                     [0, 256, 400, 255], [400, 1, 0, 256], [160, 400, 256, 0], [256, 160, 400, 1], [1, 0, 255, 400], [400, 255, 160, 400]], np.int32)


def frames_due(schedule, F=256):
    """[calls, groups]: the frames each group completes in each call of a 16 kHz packet handle (fill + count) // F"""
    fill, due = np.zeros(schedule.shape[1], np.int64), []
    for row in schedule:
        due.append((fill + row) // F)
        fill = (fill + row) % F
    return np.array(due)


def test_the_schedule_has_the_phases_it_claims():
    due = frames_due(SCHEDULE)
    assert set(SCHEDULE.ravel().tolist()) == {0, 1, 160, 255, 256, 400}
    assert not SCHEDULE[1:4, 1].any() and SCHEDULE[3].any()
    assert not due[3].any() and due[4].tolist() == [0, 1, 0, 0]
    assert any(len(set(d.tolist()) - {0}) == 2 for d in due)  # (sub-calls in which a group with fewer frames due is held)


def packet_handle(B, C, rate=16000):
    return batch(model_file('random'), B, 1, 'fp32', DEV_LIB, sample_rate=rate, packet_samples=PACKET, channels=C, channel_link='max')


def run_schedule(C, G, rate, seed):
    """all G groups on one handle against every group alone on a handle of its own (B = C) that sees only its own packets: samples,
    frame counts and report rows.  -> per group: (the samples it was fed, the samples it got), planar and concatenated"""
    B = G * C
    kp, lone = packet_handle(B, C, rate), [packet_handle(C, C, rate) for _ in range(G)]
    fed, out = [[] for _ in range(G)], [[] for _ in range(G)]
    for k, per_group in enumerate(SCHEDULE[:, :G]):
        planar = streams(B, PACKET, seed=seed + k)
        counts = np.repeat(per_group, C)
        got, fr, rep = kp.process_packets(interleave(planar, C), counts, report=True)
        for g, n in enumerate(per_group):
            rows = slice(g * C, (g + 1) * C)
            assert not got[g, n * C:].any(), (k, g)
            if n == 0:  # a stalled group is given no packet
                assert not fr[rows].any(), (k, g)
                continue
            want, wfr, wrep = lone[g].process_packets(interleave(planar[rows], C), [n] * C, report=True)
            assert np.array_equal(got[g, :n * C], want[0, :n * C]), (k, g, int((got[g, :n * C] != want[0, :n * C]).sum()))
            assert np.array_equal(fr[rows], wfr), (k, g)
            assert same(rep[rows, :int(wfr[0])], wrep[:, :int(wfr[0])]), (k, g)
            fed[g].append(planar[rows, :n])
            out[g].append(deinterleave(got[g:g + 1, :n * C], C))
    for h in [kp] + lone:
        h.delete()
    return [(np.concatenate(fed[g], axis=1), np.concatenate(out[g], axis=1)) for g in range(G)]


@pytest.mark.parametrize('C', [2, 8])
def test_packet_groups_out_of_phase_equal_every_group_alone(C):
    """... and one group directly: the linked frame recipe of its samples, frame_length - 1 samples later"""
    per_group = run_schedule(C, 4, 16000, 200)
    x, got = per_group[2]
    n = x.shape[1]
    want, _ = LinkRecipe(model_file('random'), C, C).process(np.ascontiguousarray(x[:, :n // 256 * 256]))
    assert not got[:, :255].any() and np.array_equal(got[:, 255:], want[:, :n - 255])
    plain, _ = LinkRecipe(model_file('random'), C, C, link=False).process(np.ascontiguousarray(x[:, :n // 256 * 256]))
    assert not np.array_equal(got[:, 255:], plain[:, :n - 255])


def test_packet_groups_out_of_phase_at_44100_hz_equal_every_group_alone():
    """two groups of two whose positions in the 441-sample period and fills differ from call to call; group 1 stalled for three calls"""
    run_schedule(2, 2, 44100, 300)


# ------------------------------------------------------------------------------------------------ 6. one more rate and format

def test_an_8_khz_ulaw_handle_is_the_composition_around_the_linked_16_khz_call():
    """== encode(out-stage(linked 16 kHz call(in-stage(decode(x))))): tests/sample_rate_recipe.Recipe with the linked recipe as its inner
    engine, tests/sample_format_recipe around it (test_gpu_channel_link's 48 kHz / f32 composition at another rate, format and C)"""
    import sample_format_recipe as sf
    import sample_rate_recipe as srr
    C, B, rate, T = 4, 8, 8000, 3
    F = rate * 256 // 16000
    kl = make(B, C, T, 'fp32', sample_rate=rate, sample_format='ulaw')
    rec = srr.Recipe(model_file('random'), B, 'fp32', rate)
    link = LinkRecipe(model_file('random'), B, C)

    class Inner:
        def process(self, x16):
            return link.process(x16)[0]
    rec.o = Inner()
    x = sf.encode(sf.ULAW, streams(B, 2 * T * F, seed=36))
    for k in range(2):
        part = np.ascontiguousarray(x[:, k * T * F:(k + 1) * T * F])
        got = call(kl, interleave(part, C), 'device' if k == 0 else 'inplace')
        want = sf.encode(sf.ULAW, rec.process(sf.decode(sf.ULAW, part)))
        assert same(got, interleave(want, C)), k
    kl.delete()
