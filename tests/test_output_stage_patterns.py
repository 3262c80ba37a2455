"""
The pattern rows of tests/output_stage_recipe.py held to the numpy rules alone (koala_amd/limiter.py, koala_amd/level.py), without a GPU:
what tests/test_gpu_output_stage_patterns.py compares the kernels with must itself notice the faults the rows were written for -- a missing
envelope level, another order of the envelope's additions, another tie rule in to_pcm, a wrong rail -- and the leveller's settings must reach
the tracker's clamps and branches.  Conditions on the rule, not measurements; where the rows do NOT notice a change, that is asserted too.
"""
import functools

import numpy as np
import pytest

from conftest import model_file
from frame_report_recipe import ReportRecipe
from koala_amd import level, limiter
from koala_amd.level import FRAME, fma32, to_pcm
from output_stage_recipe import DEFAULT_RELEASE, LEVELS, PEAK_AT, SETTINGS, T, delayed, grid, rows, setting

F32 = np.float32
DELTAS = [1.0 / 1024.0, DEFAULT_RELEASE]


@functools.lru_cache(maxsize=None)
def _rows():
    x, names = rows()
    E = delayed(x)
    E.setflags(write=False)
    return E, tuple(names)


def variant(E, s, skip=None, recursive=False, unfused=False):
    """limiter.apply without a leveller, with one change to limiter.gains: envelope level `skip` left out; the envelope formed by the plain
    per-sample recursion m[n] = min(q[n], m[n - 1] + delta) in float32; h = g + (n + 1) * delta as a product and a sum, each rounded.
    With no change it is the rule (asserted in every test that uses it).  -> (out, g, G)"""
    n_rows = E.shape[0]
    c, delta = F32(s.ceiling), F32(s.release)
    g = limiter.fresh(n_rows)
    out, Gs = np.empty_like(E), np.empty(E.shape, F32)
    n1 = np.arange(1, FRAME + 1, dtype=F32)
    for t in range(E.shape[1] // FRAME):
        v = E[:, t * FRAME:(t + 1) * FRAME].astype(F32)
        mag = np.abs(v)
        m = np.where(mag <= c, F32(1.0), (c / np.where(mag <= c, F32(1.0), mag)).astype(F32)).astype(F32)
        if recursive:
            for n in range(1, FRAME):
                m[:, n] = np.minimum(m[:, n], (m[:, n - 1] + delta).astype(F32))
        else:
            for j in range(8):
                if j == skip:
                    continue
                k = 1 << j
                nxt = m.copy()
                nxt[:, k:] = np.minimum(m[:, k:], (m[:, :-k] + F32(F32(k) * delta)).astype(F32))
                m = nxt
        if unfused:
            h = ((n1 * delta).astype(F32)[None, :] + g[:, None]).astype(F32)
        else:
            h = fma32(np.broadcast_to(n1, v.shape), np.full(v.shape, delta, F32), np.broadcast_to(g[:, None], v.shape))
        G = np.minimum(F32(1.0), np.minimum(m, h)).astype(F32)
        out[:, t * FRAME:(t + 1) * FRAME] = to_pcm((v * G).astype(F32))
        Gs[:, t * FRAME:(t + 1) * FRAME] = G
        g = G[:, -1].copy()
    return out, g, Gs


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_the_recipe_is_what_the_issue_lists():
    E, names = _rows()
    assert len(names) == 25 and len(set(names)) == 25 and E.shape == (25, T * FRAME) and not E[:, :FRAME].any()
    x, lim, gnames = grid()
    assert x.shape[0] == 25 * len(SETTINGS) == len(lim) and x.shape[0] % 4 and x.shape[0] % 16
    assert [(s.ceiling, s.release) for s in lim[::25]] == [tuple(float(F32(v)) if i else v for i, v in enumerate(cd)) for cd in SETTINGS]
    assert lim[25].release == limiter.settings().release == float(F32(1.0 / 800.0))
    for s in lim:
        limiter.check(s)
    for s in LEVELS.values():
        level.check(s)


@pytest.mark.parametrize('delta', DELTAS)
def test_every_envelope_level_shows_on_a_lone_peak(delta):
    """for each j the rule without level j differs from the rule on a peak@p row: sample p + 2^j can only be reached through level j"""
    E, names = _rows()
    peaks = [names.index('peak@%d' % p) for p in PEAK_AT]
    s = setting(14000.0, delta)
    want, g = limiter.apply(E[peaks], s)
    out, g0, _ = variant(E[peaks], s)
    assert np.array_equal(out, want) and np.array_equal(bits(g0), bits(g))
    for j in range(8):
        out, gj, _ = variant(E[peaks], s, skip=j)
        differs = (out != want).any(axis=1) | (bits(gj) != bits(g))
        print('delta %g, level %d left out: %d of %d peak rows differ' % (delta, j, int(differs.sum()), len(peaks)))
        assert differs.any(), j


def test_the_order_of_additions_shows_with_the_default_release_only():
    """delta = fl(1/800): the per-sample recursion and the rule's doubling round differently, in the bits of G or g, on some row;
    delta = 1/1024: the same bits on every row -- the release every earlier GPU test used could not see the order"""
    E, _ = _rows()
    for delta, shows in ((DEFAULT_RELEASE, True), (1.0 / 1024.0, False)):
        s = setting(14000.0, delta)
        _, g, G = limiter.apply(E, s, return_gain=True)
        _, gr, Gr = variant(E, s, recursive=True)
        rows_that_differ = (bits(G) != bits(Gr)).any(axis=1) | (bits(g) != bits(gr))
        print('delta %r: %d of %d rows differ in the bits of G or g' % (delta, int(rows_that_differ.sum()), E.shape[0]))
        assert rows_that_differ.any() == shows


def test_the_tie_row_separates_the_two_roundings():
    E, names = _rows()
    r = names.index('tie')
    out, _, G = limiter.apply(E[r:r + 1], setting(14000.0, 1.0 / 1024.0), return_gain=True)
    p = E[r].astype(np.float64) * G[0].astype(np.float64)  # exact: 3000 (897 + n) / 1024
    assert np.array_equal((E[r].astype(F32) * G[0]).astype(np.float64), p)
    tie = (p - np.floor(p) == 0.5) & (np.floor(p) % 2 == 0)  # half away: up; half even: down
    assert tie.any() and np.array_equal(out[0][tie], (np.floor(p[tie]) + 1).astype(np.int16))
    n = 2 * FRAME + 63  # (one frame late: sample 319 of the input's frames)
    assert tie[n] and p[n] == 2812.5 and out[0, n] == 2813


def test_the_rails():
    E, names = _rows()
    r = names.index('dc-')
    for c, delta in SETTINGS:
        if c == 32767.0:
            out, g = limiter.apply(E[r:r + 1], setting(c, delta))
            assert (out[0, FRAME:] == -32767).all() and not out[0, :FRAME].any() and g[0] == F32(32767.0) / F32(32768.0)


@functools.lru_cache(maxsize=None)
def _report():
    x, names = rows()
    rep = ReportRecipe(model_file('unity'), len(names), 'fp32').process(x)
    rep.setflags(write=False)
    return rep


def test_the_tracker_settings_reach_their_branches():
    rep, names = _report(), _rows()[1]
    tab = {k: level.track(rep, s) for k, s in LEVELS.items()}
    # the clamps, from the second value of the frame's pair (no smoothing: g_t is `want`)
    assert (tab['BOOST'][1] == F32(LEVELS['BOOST'].max_boost)).any()
    for r in ('dc-', 'nyquist', 'ramp'):
        assert (tab['CUT'][1][names.index(r)] == F32(LEVELS['CUT'].max_cut)).any(), r
    # silence first: lvl == 0 and a gain of 1 for the silent frames, then it moves
    r = names.index('ramp')
    for k in LEVELS:
        start, end, spoke, _ = tab[k]
        silent = int(np.flatnonzero(spoke[r])[0])
        assert silent >= 2 and (end[r, :silent] == 1).all() and (end[r, silent:] != 1).all(), k
        _, _, _, state = level.track(rep[r:r + 1, :silent], LEVELS[k])
        assert state[0, 0] == 0 and state[0, 1] == 1
    # falling energy on a speech frame: a_down
    for k in ('BOOST', 'SLOW'):
        s, fell = LEVELS[k], False
        for r in range(len(names)):
            lvl = F32(0)
            for t in range(rep.shape[1]):
                _, _, spoke, state = level.track(rep[r:r + 1, t:t + 1], s, np.array([[lvl, 1.0]], F32))
                fell = fell or bool(spoke[0, 0] and lvl != 0 and rep[r, t, 1] < lvl)
                lvl = state[0, 0]
        assert fell, k
    # theta = 1.0: the unity mask's mean, 257 * fl(1 / 257), passes the gate -- and one ulp less would not
    m = F32(rep[0, 0, 2]) * (F32(1.0) / F32(257.0))
    assert rep[0, 0, 2] == 257 and m == F32(1.0) and tab['SLOW'][2].any()


def test_not_detected_the_fused_h():
    """RECORDED AS NOT COVERED: h[n] = fma(n + 1, delta, g) formed as a product and a sum, each rounded, gives the same samples and the
    same g as the rule on every row under both c = 14000 settings of the GPU suite's main grid -- 256 delta is exact or a rounding of h
    moves G by one ulp, which rarely moves an int16.  The pattern tests therefore do not claim to detect a kernel that contracts or
    splits that one operation; if this assertion ever fails, the rows have begun to see it and this note goes."""
    E, _ = _rows()
    for delta in DELTAS:
        s = setting(14000.0, delta)
        want, g = limiter.apply(E, s)
        out, gu, _ = variant(E, s, unfused=True)
        assert np.array_equal(out, want) and np.array_equal(bits(gu), bits(g))
