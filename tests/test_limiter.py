"""
Peak limiter (include/pv_koala_batch.h, PEAK LIMITER; DESIGN.md section 2, thirteenth extension) without a GPU: the numpy rule
koala_amd/limiter.py on synthetic E held to its consequences -- the ceiling, the identity, cut invariance, the distance from the per-sample
recursion, a case worked by hand, resets and holds -- the settings, and the C ABI through a stand-alone driver under the sanitizers.
"""
import math

import numpy as np
import pytest

import sanitized_build
from conftest import model_file
from koala_amd import level, limiter
from limiter_recipe import BOUND, RELEASE, over_calls, recursion, setting

F32 = np.float32
ROWS, T = 4, 9


def noise(rows=ROWS, frames=T, seed=11):
    """full-scale noise with stretches of quiet, so the gain comes all the way back now and then"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (rows, frames * 256))
    x[:, 256:700] //= 64
    x[:, 1500:1900] //= 300
    return x.astype(np.int16)


def ramp_to(top, rows=ROWS, frames=T):
    """leveller pairs that climb from 1 to `top` over the frames"""
    g = np.linspace(1.0, top, frames + 1).astype(F32)
    return np.tile(g[:-1], (rows, 1)), np.tile(g[1:], (rows, 1))


@pytest.mark.parametrize('c', [1, 1000, 29205, 32767])
def test_ceiling(c):
    E = noise()
    start, end = ramp_to(8.0)
    out, g, G = limiter.apply(E, setting(c), start, end, return_gain=True)
    peak = int(np.abs(out.astype(np.int64)).max())
    print('c = %d: max |out| = %d, min G = %g' % (c, peak, G.min()))
    assert peak <= c and (G < 1).any()
    assert (np.abs(E[:, -256:].astype(np.float64)) * 7 > 32767).any()  # (the ramped product is far over the rails)
    out1, _ = limiter.apply(E, setting(c))  # and without the leveller
    assert int(np.abs(out1.astype(np.int64)).max()) <= c


def test_identity_where_nothing_is_above_the_ceiling():
    E = (noise() // 8).astype(np.int16)  # |E| <= 4096
    out, g, G = limiter.apply(E, setting(4096), return_gain=True)
    assert np.array_equal(out, E) and (G == 1).all() and (g == 1).all()
    # behind the leveller: the leveller's samples bit for bit, through level.apply's own ramp
    rep = np.zeros((ROWS, T, 4), F32)
    rep[..., 1], rep[..., 2] = 20.0, 200.0
    lev = level.settings(theta=0.25, floor_dbfs=-90.0, max_boost_db=6.0)
    want, gains, _ = level.apply(E, rep, lev)
    start, end, _, _ = level.track(rep, lev)
    assert gains.max() > 1.5 and (want != E).any() and np.abs(want.astype(int)).max() < 32767
    out, g = limiter.apply(E, setting(32767), start, end)
    assert np.array_equal(out, want) and (g == 1).all()
    # a stream that is off: the leveller's output (or E), and its state stays
    out, g = limiter.apply(E, None, start, end, state=np.full(ROWS, 0.5, F32))
    assert np.array_equal(out, want) and (g == F32(0.5)).all()


def test_cut_invariance():
    E = noise()
    start, end = ramp_to(3.0)
    whole, gw, Gw = limiter.apply(E, setting(5000), start, end, return_gain=True)
    outs, state, t0 = [], None, 0
    for n in (3, 2, 1, 3):
        o, state = limiter.apply(E[:, t0 * 256:(t0 + n) * 256], setting(5000), start[:, t0:t0 + n], end[:, t0:t0 + n], state)
        outs.append(o)
        t0 += n
    assert np.array_equal(np.concatenate(outs, axis=1), whole) and np.array_equal(state, gw)
    f = Gw.reshape(ROWS, T, 256)
    assert ((f[:, 1:, 0] < 1) & (f[:, 1:, 0] > f[:, :-1, -1])).any()  # a release crossed a frame boundary


@pytest.mark.parametrize('c,release', [(1000, RELEASE), (20000, 1.0 / 800.0), (300, 1.0 / 3.0), (12000, 1.0)])
def test_exact_recursion(c, release):
    E = noise()
    start, end = ramp_to(2.0)
    w = (np.arange(256, dtype=F32) / F32(256)).astype(F32)
    out, g, G = limiter.apply(E, setting(c, release), start, end, return_gain=True)
    s = setting(c, release)
    worst = 0.0
    for b in range(ROWS):
        ramp = level.fma32(np.tile(w, T), np.repeat((end[b] - start[b]).astype(F32), 256), np.repeat(start[b], 256))
        v = (E[b].astype(F32) * ramp).astype(F32)
        want = recursion(v, float(F32(s.ceiling)), float(F32(s.release)))
        worst = max(worst, float(np.abs(G[b].astype(np.float64) - want).max()))
    print('c = %d, delta = %g: max |G - recursion| = %.3g (bound %.3g)' % (c, release, worst, BOUND))
    assert worst <= BOUND and (G < 1).any()


def test_two_frames_by_hand():
    """c = 14000, delta = 1/1024.  Frame 0 is 100 everywhere but a peak of 16000 at its last sample: q[255] = 14000 / 16000 = 7/8 exactly,
    every other q is 1, so m_8[255] = 7/8, h[255] = 1 + 256/1024 and G[255] = 7/8: out[255] = 14000, g = 7/8.  Frame 1 is 1000 everywhere:
    q = m_8 = 1, h[n] = 7/8 + (n + 1)/1024 -- exact -- reaches 1 at n = 127, so G[n] = (897 + n)/1024 for n < 127 and 1 from there on; the
    product 1000 (897 + n)/1024 is exact in float32 and to_pcm rounds it half away from zero.  The release ends in frame 1: g = 1."""
    E = np.full((1, 512), 100, np.int16)
    E[0, 255] = 16000
    E[0, 256:] = 1000
    out, g, G = limiter.apply(E, setting(14000, 1.0 / 1024.0), return_gain=True)
    want = np.full(512, 100, np.int64)
    want[255] = 14000
    n = np.arange(256)
    want[256:] = np.where(n < 127, (2 * 1000 * (897 + n) + 1024) // 2048, 1000)
    assert want[256] == 876 and want[256 + 126] == 999 and want[256 + 127] == 1000
    assert np.array_equal(out[0].astype(np.int64), want)
    assert np.array_equal(G[0, :255], np.ones(255, F32)) and G[0, 255] == F32(0.875)
    assert np.array_equal(G[0, 256:], np.minimum(1.0, (897 + n) / 1024.0).astype(F32)) and g[0] == 1
    _, g0 = limiter.apply(E[:, :256], setting(14000, 1.0 / 1024.0))
    assert g0[0] == F32(0.875)
    # the same peak under a leveller ramp from 1 to 2: r[255] = fma(255/256, 1, 1) = 511/256, v = 31937.5, q = fl(14000 / 31937.5)
    out, g = limiter.apply(E[:, :256], setting(14000, 1.0 / 1024.0), np.ones((1, 1), F32), np.full((1, 1), 2.0, F32))
    q = F32(14000.0) / F32(31937.5)
    assert g[0] == q and out[0, 255] == int(math.floor(float(F32(31937.5) * q) + 0.5)) and out[0, 254] == int(math.floor(100 * 510 / 256 + 0.5))


def test_reset_and_hold():
    E = noise()
    E[:, :100] //= 64  # (a quiet start: the gain a stream enters with shows)
    s = setting(2000)
    entering = np.array([0.25, 0.25, 0.25, 0.25], F32)
    reset = np.zeros((ROWS, T), np.uint8)
    reset[1, 0] = 1  # stream 1 restarts at frame 0, stream 2 at frame 4
    reset[2, 4] = 1
    hold = np.array([0, 0, 0, 1], np.uint8)
    out, g = limiter.apply(E, s, state=entering, reset=reset, hold=hold)
    plain, gp = limiter.apply(E, s, state=entering)
    fresh, gf = limiter.apply(E, s)
    assert np.array_equal(out[0], plain[0]) and g[0] == gp[0]
    assert np.array_equal(out[1], fresh[1]) and not np.array_equal(out[1], plain[1])  # a reset at frame 0 is a fresh stream
    tail, gt = limiter.apply(E[2:3, 4 * 256:], s)
    assert np.array_equal(out[2, :4 * 256], plain[2, :4 * 256]) and np.array_equal(out[2, 4 * 256:], tail[0]) and g[2] == gt[0]
    assert np.array_equal(out[3], E[3]) and g[3] == F32(0.25)  # held: the samples and g stay
    # a reset of a stream that is off, or held, leaves its g alone
    reset[:] = 1
    _, g = limiter.apply(E, [None, s, s, s], state=entering, reset=reset, hold=hold)
    assert g[0] == F32(0.25) and g[3] == F32(0.25)
    assert np.array_equal(limiter.fresh(3), np.ones(3, F32))


def test_settings_and_check():
    s = limiter.settings()
    assert s == limiter.Setting(1, float(math.floor(32767 * 10 ** (-1 / 20))), float(F32(1.0 / 800.0)))
    assert limiter.settings(ceiling_dbfs=0.0).ceiling == 32767.0 and limiter.settings(release_ms=1.0 / 16.0).release == 1.0
    assert limiter.settings(ceiling_dbfs=-3.0, on=False).on == 0
    assert limiter.OFF.on == 0
    limiter.check(limiter.OFF)
    limiter.check(limiter.Setting(1, 1.0, 1e-30))
    for bad in (dict(ceiling_dbfs=0.1), dict(ceiling_dbfs=-100.0), dict(ceiling_dbfs=float('nan')), dict(release_ms=0.0), dict(release_ms=-5.0),
                dict(release_ms=1.0 / 32.0), dict(release_ms=float('inf')), dict(ceiling_dbfs=float('-inf'))):
        with pytest.raises(ValueError):
            limiter.settings(**bad)
    for bad in (limiter.Setting(2, 1000.0, 0.5), limiter.Setting(1, 0.5, 0.5), limiter.Setting(1, 32768.0, 0.5), limiter.Setting(1, float('nan'), 0.5),
                limiter.Setting(1, 1000.0, 0.0), limiter.Setting(1, 1000.0, 1.5), limiter.Setting(1, 1000.0, float('nan')), limiter.Setting(1, float('inf'), 0.5)):
        with pytest.raises(ValueError):
            limiter.check(bad)
    with pytest.raises(ValueError):
        limiter.apply(np.zeros((2, 256), np.int16), [limiter.OFF])  # one setting for two streams


def test_abi_under_sanitizers(tmp_path):
    """tests/abi_limiter/driver.cpp (with koala_amd/csrc/pv_limiter.cpp) against koala_amd/csrc/pv_api*.cpp and the engine double: a
    stand-alone program with the sanitizers linked in, run as it is; nothing is loaded into python"""
    run = sanitized_build.run(sanitized_build.build_abi_driver('abi_limiter', tmp_path), model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
