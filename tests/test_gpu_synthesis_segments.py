"""
Time segments of the STFT kernels under the two newest kernel families, on a real MI355X: synthesis_profile_kernel and
synthesis_comfort_kernel (koala_amd/csrc/kns_stft_synthesis.inc) at segments longer than one frame, and the analysis kernel at segments the
engine only ever chooses near 4096 streams.

A synthesis workgroup walks `seg` frames; every segment but the first replays frame t0 - 1 in full to rebuild its overlap-add tail, under
that frame's own mask, gain, clamp, counter value and reset, and inside a segment the stored-spectrum profile forms request the next frame's
operands behind m', the recomputing comfort forms fetch the mask behind the forward FFT.  None of that runs at seg = 1, which is what the
engine chooses at every shape of tests/test_gpu_band_profile.py and tests/test_gpu_comfort.py.  Here the length is forced
(KOALA_AMD_SYNTH_SEG, KOALA_AMD_ANALYSIS_SEG; developer library) at B = 24 x T = 7, and chosen by the engine itself at the smallest shapes
at which it chooses more than one frame; either way it is read back (gpu_kit.segments_of) and asserted, with the route and whether the
spectrum was stored.

The reference is tests/segment_recipe.py: the handle's own `mask` tap, then numpy float32 and the oracle's analysis and synthesis.  The
synthesis stage is float32 in both configurations, so every comparison with it is ==, in bf16 too: samples, report rows, counters.  On top
of that fp32 == tests/comfort_recipe.py's ComfortRecipe driven by the oracle alone, and bf16 meets the suite's bars against it.

R = 16 distinct streams tiled over all B slots; the first replica is compared with the reference, every other one must equal the first.
"""
import functools

import numpy as np
import pytest

from comfort_recipe import ComfortRecipe
from conftest import model_file, synth_streams
from gpu_kit import (DEV_LIB, ROUTE_CHUNKED, ROUTE_PIPELINED, ROUTE_RESETS, ROUTE_WAVE, batch, call, check_pcm, frames, oracle_prec,
                     replicas, route_info, same, segments_of, tiled)
from min_gain_recipe import Recipe
from oracle import oracle
from segment_recipe import SegmentRecipe, mixed, round_bf16

pytestmark = pytest.mark.gpu

R, B, T = 16, 24, 7  # 16 distinct streams over 24 slots: the second m-tile is ragged, 8 rows
SEGS = [1, 2, 3, 5, 7]  # 1: every frame behind its replayed predecessor (the control); 5: a ragged last segment; 7: one segment, no replay
PRECISIONS = ['fp32', 'bf16']
SYNTH_ENV, ANALYSIS_ENV, TAPS_ENV, CHUNK_ENV = 'KOALA_AMD_SYNTH_SEG', 'KOALA_AMD_ANALYSIS_SEG', 'KOALA_AMD_DEBUG_TAPS', 'KOALA_AMD_PIPE_CHUNK'
SETTINGS = mixed(R)  # (floor, ceiling, gains, curves, seeds, on): per stream, every fifth stream off, stream 2 with a zero curve
ARMS = ('profile', 'profile_report', 'comfort', 'comfort_report', 'profile_f32', 'profile_report_f32', 'comfort_f32', 'comfort_report_f32')


def as_f32(s):
    """int16 samples as the 'f32' format's (exact: 16 bits times a power of two)"""
    return (np.asarray(s, np.int16).astype(np.float32) / np.float32(32768)).astype(np.float32)


def make(arm, n, frames_max, precision):
    """a handle of arm `arm` under the environment as it is now (the engine reads its switches when it is created)"""
    lo, hi, g, amp, seeds, on = SETTINGS
    kb = batch(model_file('random'), n, frames_max, precision, DEV_LIB, **({'sample_format': 'f32'} if arm.endswith('f32') else {}))
    col = lambda v: tiled(np.asarray(v)[:, None], n)[:, 0]
    kb.set_band_profile(tiled(lo, n), tiled(hi, n))
    kb.set_min_gain(col(g))
    if arm.startswith('comfort'):
        kb.set_comfort_noise(tiled(amp, n), col(seeds))
        off = np.flatnonzero(~col(on))
        kb.set_comfort_noise(None, col(seeds)[off], streams=off, on=False)
    return kb


def settings(arm):
    """the recipe's arguments behind the mask: comfort noise on no stream in the profile arms"""
    lo, hi, g, amp, seeds, on = SETTINGS
    return (g, lo, hi, amp, seeds, on if arm.startswith('comfort') else np.zeros(R, bool))


def seg_resets():
    """[R, T]: frame 0 and the last frame; the first frame of a segment (2: seg 2; 3: seg 3; 5: seg 5; 6: seg 2 and 3) and the replayed frame
    in front of one (1, 2, 4, 5); two adjacent frames (stream 6); off streams (4, 9, 14); the stream with the zero curve (2); and every
    stream below 8 is also a row of the ragged tile"""
    rs = np.zeros((R, T), np.uint8)
    for b, t in ((0, 0), (8, 6), (5, 6), (6, 2), (6, 3), (4, 1), (9, 4), (14, 5), (1, 4), (2, 5), (3, 1), (15, 5), (10, 2), (13, 3), (7, 0), (7, 6)):
        rs[b, t] = 1
    return rs


def where(got, want, per=256):
    """for a failing ==: the rows that differ, the frames (`per` values of a row each), and how many values"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return got.shape, want.shape
    d = (got != want).reshape(got.shape[0], -1)
    rows, cols = np.nonzero(d)
    return {'rows': sorted(set(rows.tolist())), 'frames': sorted(set((cols // per).tolist())), 'values': int(d.sum())}


def clean(monkeypatch):
    """none of the switches this module sets is on"""
    for env in (SYNTH_ENV, ANALYSIS_ENV, TAPS_ENV, CHUNK_ENV):
        monkeypatch.delenv(env, raising=False)


class Got:
    """what one call of one arm gave, first replica and all"""

    def __init__(self, kb, y, rep, frames_in, tap):
        self.y, self.rep, self.info = y, rep, route_info(kb)
        self.route, self.stored = int(self.info[0]), bool(self.info[3])
        self.segs = segments_of(kb)
        self.count = kb.comfort_state()
        self.mask = kb.debug_read('mask', frames_in)[:, :R] if tap else None


def run_calls(arm, kb, x1, seq):
    """the calls of `seq` [(mode, resets [R, T] or None)] of consecutive frames of x1 through one handle -> [Got]"""
    n, f32, rep = kb.num_streams, arm.endswith('f32'), 'report' in arm
    out, t0 = [], 0
    Tc = x1.shape[1] // 256 // len(seq)
    for mode, reset in seq:
        x = tiled(frames(x1, t0, t0 + Tc), n)
        r = call(kb, as_f32(x) if f32 else x, mode, report=rep, **({} if reset is None else {'reset': tiled(reset, n)}))
        y, rows = r if rep else (r, None)
        out.append(Got(kb, y, rows, Tc, tap=not f32))
        t0 += Tc
    return out


def check_against_the_recipe(arm, got, x1, seq, oracle_only=None, precision=None):
    """samples, report rows and counters of the first replica == SegmentRecipe on the arm's own mask tap, every other replica == the first"""
    rec = SegmentRecipe(model_file('random'), R)
    Tc = x1.shape[1] // 256 // len(seq)
    for n, ((mode, reset), g) in enumerate(zip(seq, got)):
        want, wrep = rec.process(frames(x1, n * Tc, (n + 1) * Tc), g.mask, *settings(arm), reset=reset)
        assert same(g.y[:R], want), (arm, n, mode, where(g.y[:R], want))
        assert g.rep is None or same(g.rep[:R], wrep), (arm, n, mode, where(g.rep[:R], wrep, 4))
        assert same(g.count[:R], rec.count), (arm, n, g.count[:R], rec.count)
        assert replicas(g.y, R) and replicas(g.count[:, None], R) and (g.rep is None or replicas(g.rep, R)), (arm, n)
        if oracle_only is not None:
            check_pcm(g.y[:R], oracle_only[n], precision, '%s call %d against the oracle alone' % (arm, n))


# ------------------------------------------------------------------------------------------------ 1. synthesis, forced lengths

SEQ = [('device', None), ('inplace', None), ('device', seg_resets())]


def x_forced():
    return synth_streams(R, 3 * T, 81)


def run_arms(precision):
    """three consecutive 7-frame calls -- out of place, in place, per-frame resets -- through every arm, each on a handle of its own
    -> arm: ([Got], records)"""
    out = {}
    for arm in ARMS:
        kb = make(arm, B, T, precision)
        out[arm] = (run_calls(arm, kb, x_forced(), SEQ), kb.export_state())
        kb.delete()
    return out


@functools.lru_cache(maxsize=None)
def unset_run(precision):
    """run_arms under the engine's own choice: once per precision, shared, left unchanged"""
    return run_arms(precision)


@functools.lru_cache(maxsize=None)
def oracle_alone(precision):
    """ComfortRecipe driven by the oracle, no tap: 'profile' / 'comfort' -> the samples of the three calls.  Once per precision."""
    out = {}
    for arm in ('profile', 'comfort'):
        g, lo, hi, amp, seeds, on = settings(arm)
        rec, x1 = ComfortRecipe(model_file('random'), R, precision), x_forced()
        ys = []
        for n, (_, reset) in enumerate(SEQ):
            xn = frames(x1, n * T, (n + 1) * T)
            ys.append(rec.process(xn, g, lo, hi, amp, seeds, on) if reset is None else rec.process_resets(xn, g, reset, lo, hi, amp, seeds, on))
        out[arm] = ys
    return out


def check_forms(run, seg):
    """which form ran in every arm and call, stated not supposed: the route, whether the spectrum was stored, the segment lengths.  An s16
    handle recomputes its spectrum out of place and stores it in place; an 'f32' handle's call is always out of place behind the format
    stage and recomputes; the reset call takes the reset route, the others the wavefront route (two m-tiles), whose STFT launches take
    their segments like any other's."""
    for arm in ARMS:
        for n, ((mode, reset), g) in enumerate(zip(SEQ, run[arm][0])):
            assert g.route == (ROUTE_RESETS if reset is not None else ROUTE_WAVE), (arm, n, g.info)
            assert g.stored == (mode == 'inplace' and not arm.endswith('f32')), (arm, n, mode, g.info)
            assert g.segs == (1, seg, 1), (arm, n, g.segs)  # (analysis: two m-tiles, one frame a workgroup)


def test_the_reset_table_has_the_frames_it_claims():
    rs = seg_resets()
    on = SETTINGS[5]
    assert rs[:, 0].any() and rs[:, T - 1].any() and (rs[:, :-1] & rs[:, 1:]).any()
    for seg in (2, 3, 5):
        assert rs[:, seg].any() and rs[:, seg - 1].any()  # the first frame of the second segment, and the frame it replays
    assert rs[~on].any() and rs[:B - R].any() and rs[2].any() and not SETTINGS[3][2].any()
    assert (~on).sum() == 3 and all((~on[4 * w:4 * w + 4]).sum() <= 1 for w in range(4))  # on and off rows inside a wave's four


@pytest.mark.parametrize('precision', PRECISIONS)
def test_unset_the_engine_runs_one_frame_a_segment_here(precision, monkeypatch):
    """... which is why this module exists: at B = 24 x T = 7 the engine's own choice is seg = 1 in both kernels"""
    clean(monkeypatch)
    check_forms(unset_run(precision), 1)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('seg', SEGS)
def test_synthesis_segments_of_every_length_equal_the_recipe(seg, precision, monkeypatch):
    """fp32 figures against the oracle alone: 0 LSB at every length.  bf16: the bars of tests/gpu_kit.py."""
    clean(monkeypatch)
    base = unset_run(precision)
    monkeypatch.setenv(SYNTH_ENV, str(seg))
    run = run_arms(precision)
    check_forms(run, seg)
    alone = oracle_alone(precision)
    for arm in ('profile_report', 'comfort_report'):
        check_against_the_recipe(arm, run[arm][0], x_forced(), SEQ, alone[arm.split('_')[0]], precision)
    for kind in ('profile', 'comfort'):
        plain, rep, plain32, rep32 = (run[kind + s][0] for s in ('', '_report', '_f32', '_report_f32'))
        for n in range(3):
            # without a report == with one (the same mask went in); the 'f32' handle == the s16 handle, scaled
            assert same(plain[n].mask, rep[n].mask) and same(plain[n].y, rep[n].y), (kind, n, where(plain[n].y, rep[n].y))
            assert same(plain[n].count, rep[n].count) and same(plain32[n].count, rep[n].count) and same(rep32[n].count, rep[n].count), (kind, n)
            assert same(rep32[n].y, as_f32(rep[n].y)), (kind, n, where(rep32[n].y, as_f32(rep[n].y)))
            assert same(rep32[n].rep, rep[n].rep), (kind, n, where(rep32[n].rep, rep[n].rep, 4))
            assert same(plain32[n].y, rep32[n].y), (kind, n, where(plain32[n].y, rep32[n].y))
            assert replicas(plain32[n].y, R) and replicas(rep32[n].y, R) and replicas(rep32[n].rep, R), (kind, n)
    for n in range(3):  # (the fill does something, and only where it is on and the curve is not zero: stream 2)
        quiet = ~SETTINGS[5]
        quiet[2] = True
        a, b = run['comfort_report'][0][n].y[:R], run['profile_report'][0][n].y[:R]
        assert same(a[quiet], b[quiet]) and all((a[r] != b[r]).any() for r in np.flatnonzero(~quiet)), n
    for arm in ARMS:  # the stream records, and with them everything else, are those under the engine's own choice
        assert np.array_equal(run[arm][1], base[arm][1]), arm
        for n in range(3):
            assert same(run[arm][0][n].y, base[arm][0][n].y), (arm, n, where(run[arm][0][n].y, base[arm][0][n].y))
            assert run[arm][0][n].rep is None or same(run[arm][0][n].rep, base[arm][0][n].rep), (arm, n)


# ------------------------------------------------------------------------------------------------ 2. analysis, forced lengths

def run_analysis(precision):
    """a plain handle with the debug taps on, the three calls of SEQ -> ([(samples, spectrum, features, info, segs)], records)"""
    kb = batch(model_file('random'), B, T, precision, DEV_LIB)
    x1, out = x_forced(), []
    for n, (mode, reset) in enumerate(SEQ):
        y = call(kb, tiled(frames(x1, n * T, (n + 1) * T), B), mode, **({} if reset is None else {'reset': tiled(reset, B)}))
        out.append((y, kb.debug_read('spectrum', T), kb.debug_read('features', T), route_info(kb), segments_of(kb)))
    rec = kb.export_state()
    kb.delete()
    return out, rec


@functools.lru_cache(maxsize=None)
def unset_analysis(precision):
    return run_analysis(precision)


@functools.lru_cache(maxsize=None)
def analysis_wanted(precision):
    """the oracle's samples, spectra and features of the three calls; bf16 features: the oracle's rounded to bf16"""
    x1 = x_forced()
    rec = Recipe(model_file('random'), R, precision)
    an = oracle.Oracle(model_file('random'), 1, oracle_prec(precision))
    hist, zero, out = np.zeros((R, 256), np.int16), np.zeros(R, np.float32), []
    for n, (_, reset) in enumerate(SEQ):
        xn = frames(x1, n * T, (n + 1) * T)
        spec, feat = np.empty((T, R, 257, 2), np.float32), np.empty((T, R, 257), np.float32)
        for t in range(T):
            if reset is not None:
                hist[reset[:, t] != 0] = 0
            for b in range(R):
                spec[t, b], f = an.analysis(hist[b], xn[b, t * 256:(t + 1) * 256])
                feat[t, b] = round_bf16(f) if precision == 'bf16' else f
                hist[b] = xn[b, t * 256:(t + 1) * 256]
        out.append((rec.process(xn, zero) if reset is None else rec.process_resets(xn, zero, reset), spec, feat))
    return out


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('seg', SEGS)
def test_analysis_segments_of_every_length_equal_the_oracle(seg, precision, monkeypatch):
    """a ragged last analysis segment (5: the history written from its last frame, the clamped prefetch) and resets in the middle of short
    segments: the `spectrum` and `features` taps == Oracle.analysis, the samples == the oracle's in fp32 and within the bars in bf16, the
    stream records == those under the engine's own choice (one frame)"""
    clean(monkeypatch)
    monkeypatch.setenv(TAPS_ENV, '1')
    base, base_rec = unset_analysis(precision)
    monkeypatch.setenv(ANALYSIS_ENV, str(seg))
    got, rec = run_analysis(precision)
    for n, ((mode, reset), (y, spec, feat, info, segs), (wy, wspec, wfeat)) in enumerate(zip(SEQ, got, analysis_wanted(precision))):
        assert segs == (seg, 1, 1) and base[n][4] == (1, 1, 1), (n, segs, base[n][4])
        assert bool(info[3]) and int(info[0]) == int(base[n][3][0]) and (reset is None or int(info[0]) == ROUTE_RESETS), (n, info)
        assert same(spec[:, :R], wspec), (n, where(spec[:, :R], wspec, 514))  # (rows: frames; frames: streams)
        assert same(feat[:, :R], wfeat), (n, where(feat[:, :R], wfeat, 257))
        assert replicas(spec.transpose(1, 0, 2, 3), R) and replicas(feat.transpose(1, 0, 2), R) and replicas(y, R), n
        check_pcm(y[:R], wy, precision, 'analysis seg %d call %d' % (seg, n))
        assert same(y, base[n][0]) and same(spec, base[n][1]) and same(feat, base[n][2]), n
    assert np.array_equal(rec, base_rec)


# ------------------------------------------------------------------------------------------------ 3. the lengths the engine chooses

def chosen_resets(frames_in):
    """[R, 4] for seg = 2: frame 0, frame 2 (the first of the second segment), frame 1 (the one it replays), the last, 1 and 2 of one stream,
    an off stream"""
    rs = np.zeros((R, frames_in), np.uint8)
    for b, t in ((0, 0), (1, 2), (3, 1), (8, 3), (6, 1), (6, 2), (4, 2), (9, 1), (2, 3)):
        rs[b, t] = 1
    return rs


# (id, precision, streams, frames, forced synthesis segment, frames per pipeline chunk, arms, [(mode, resets)], route of the first call,
#  (analysis seg, synthesis seg, synthesis launches of an out-of-place call))
CHOSEN = [
    # 256 m-tiles: synthesis 4 -> 256 x 2 = 512 workgroups, segments of 4 and 3; analysis 7 -> 4 -> 2 (256 x 4 = 1024): 2, 2, 2, 1
    ('4096x7', 'bf16', 4096, 7, None, None, ('comfort', 'comfort_report', 'profile_report'), [('device', None), ('inplace', None)], ROUTE_CHUNKED, (2, 4, 1)),
    # 257 m-tiles, the last one 8 rows: synthesis 4 -> 2 (257 x 2 = 514); analysis one frame
    ('4104x4-bf16', 'bf16', 4104, 4, None, None, ('comfort_report', 'profile_report'), [('device', None), ('device', chosen_resets(4))], ROUTE_CHUNKED, (1, 2, 1)),
    ('4104x4-fp32', 'fp32', 4104, 4, None, None, ('comfort_report', 'profile_report'), [('device', None), ('device', chosen_resets(4))], ROUTE_CHUNKED, (1, 2, 1)),
    # the layer pipeline, 49 m-tiles.  At 32 frames a call the engine runs the STFT stages as whole-call launches (it slices them from 48
    # frames on: kns_engine.cpp, stft_sliced): segments 5 5 5 5 5 5 2 ...
    ('784x32-whole', 'bf16', 784, 32, 5, None, ('comfort', 'comfort_report', 'profile_report'), [('device', None), ('inplace', None)], ROUTE_PIPELINED, (1, 5, 1)),
    # ... and with the pipeline's chunk length given, two slices of 16 frames (t0c = 16: the mask offset, the previous frame in the PCM,
    # comfort_n + t0c, the report rows offset) with segments 5 5 5 1 inside each; the second call stores its spectrum and is not sliced
    ('784x32-sliced', 'bf16', 784, 32, 5, 16, ('comfort', 'comfort_report', 'profile_report'), [('device', None), ('device', None), ('inplace', None)], ROUTE_PIPELINED, (1, 5, 2)),
]


@pytest.mark.parametrize('case', CHOSEN, ids=[c[0] for c in CHOSEN])
def test_segments_the_engine_chooses_equal_the_recipe(case, monkeypatch):
    _, precision, n, frames_in, seg, chunk, arms, seq, route, segs = case
    clean(monkeypatch)
    for env, v in ((SYNTH_ENV, seg), (CHUNK_ENV, chunk)):
        if v is not None:
            monkeypatch.setenv(env, str(v))
    x1 = synth_streams(R, len(seq) * frames_in, 82)
    runs = {}
    for arm in arms:
        kb = make(arm, n, frames_in, precision)
        runs[arm] = run_calls(arm, kb, x1, seq)
        kb.delete()
        for k, ((mode, reset), g) in enumerate(zip(seq, runs[arm])):
            assert g.route == (ROUTE_RESETS if reset is not None else route), (arm, k, g.info)
            assert g.stored == (mode == 'inplace'), (arm, k, g.info)
            assert g.segs == segs[:2] + (segs[2] if mode == 'device' and reset is None else 1,), (arm, k, g.segs)
        if 'report' in arm:
            check_against_the_recipe(arm, runs[arm], x1, seq)
    if 'comfort' in arms:
        for k, (a, b) in enumerate(zip(runs['comfort'], runs['comfort_report'])):
            assert same(a.mask, b.mask) and same(a.y, b.y) and same(a.count, b.count), (k, where(a.y, b.y))
