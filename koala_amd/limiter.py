"""
The rule of the peak limiter (include/pv_koala_batch.h, PEAK LIMITER; DESIGN.md section 2, thirteenth extension) in numpy float32: what a
handle delivers while a stream's limiter is on, given what the same handle delivers without it at 16 kHz (E, int16) and, where the stream
also levels, the leveller's gain pair of every frame (koala_amd.level.track).

Per stream a setting (`Setting`; `settings()` builds one from dBFS and milliseconds): the ceiling c in sample units, 1 <= c <= 32767, and
the release delta, the gain recovered per 16 kHz sample, 0 < delta <= 1; and one float32 value of state, g, the gain behind the stream's
last sample; fresh: g = 1.  For every frame t, n = 0 .. 255:

    r[n]   = fma(n / 256, g_t - g_{t-1}, g_{t-1})          the leveller's ramp (1 where the stream does not level)
    v[n]   = float(E[256 t + n]) * r[n]                     the leveller's own product, before to_pcm
    q[n]   = 1 if |v[n]| <= c else c / |v[n]|
    m_0    = q
    m_{j+1}[n] = min(m_j[n], m_j[n - 2^j] + 2^j delta)      for n >= 2^j, else m_j[n];  j = 0 .. 7
    h[n]   = fma(float(n + 1), delta, g)                    g: the state entering this frame
    G[n]   = min(1, min(m_8[n], h[n]))
    out[256 t + n] = to_pcm(v[n] * G[n]);   g = G[255]

Every operation is one float32 operation, in this order; `fma32` and `to_pcm` are the leveller's.  m_8 is the lower envelope
min_k (q[n - k] + k delta) inside the frame -- instant attack, linear release -- and h carries the release over the frame boundary, so the
result does not depend on how frames are cut into calls, and G is within 9 * 2^-23 of the per-sample recursion min(1, q[n], g[n-1] + delta).
G <= q: for an integer c no output sample is above c in magnitude.  A reset sets g = 1 before its frame, a held stream keeps g and its
samples, a stream that is off delivers the leveller's output (or E) and its g does not move.  Self-contained: numpy only.
"""
import math
from collections import namedtuple

import numpy as np

from .level import FRAME, fma32, to_pcm

F32 = np.float32
SAMPLE_RATE_KHZ = 16.0

Setting = namedtuple('Setting', 'on ceiling release')
FIELDS = Setting._fields[1:]
OFF = Setting(0, 32767.0, 1.0)  # what a new handle holds for every stream


def settings(ceiling_dbfs=-1.0, release_ms=50.0, on=True):
    """A `Setting` from physical units: no sample above `ceiling_dbfs` (dB against the int16 full scale 32767, rounded down to a whole
    sample value), and a gain that recovers linearly, from 0 to 1 in `release_ms`: delta = 1 / (16 release_ms)."""
    if not (isinstance(ceiling_dbfs, (int, float)) and math.isfinite(ceiling_dbfs)) or not (isinstance(release_ms, (int, float)) and math.isfinite(release_ms)):
        raise ValueError("`ceiling_dbfs` and `release_ms` are finite numbers")
    if release_ms <= 0:
        raise ValueError("`release_ms` %r is not > 0" % (release_ms,))
    s = Setting(1 if on else 0, float(F32(math.floor(32767.0 * 10.0 ** (ceiling_dbfs / 20.0)))), float(F32(1.0 / (SAMPLE_RATE_KHZ * release_ms))))
    check(s)
    return s


def check(s):
    """ValueError unless `s` is a setting the library accepts"""
    if s.on not in (0, 1):
        raise ValueError("`on` %r is not 0 or 1" % (s.on,))
    ok = (('ceiling', 1 <= s.ceiling <= 32767), ('release', 0 < s.release <= 1))
    for name, good in ok:
        if not good or not math.isfinite(getattr(s, name)):
            raise ValueError("`%s` %r is outside its range" % (name, getattr(s, name)))


def _table(setting, rows):
    """one Setting, None (off) or a list of them, one per row -> float32 ceiling [rows], release [rows] and on [rows]"""
    each = list(setting) if isinstance(setting, (list, tuple)) and not isinstance(setting, Setting) else [setting] * rows
    if len(each) != rows:
        raise ValueError("%d settings for %d streams" % (len(each), rows))
    each = [OFF if s is None else s for s in each]
    for s in each:
        check(s)
    return np.array([s.ceiling for s in each], F32), np.array([s.release for s in each], F32), np.array([s.on for s in each], bool)


def fresh(rows):
    """the state of `rows` fresh streams, float32 [rows] = g"""
    return np.ones(rows, F32)


def gains(v, ceiling, release, g):
    """One frame of the rule.  v: float32 [rows, 256], the products; ceiling, release, g: float32 [rows] -> G float32 [rows, 256]"""
    c, delta = ceiling[:, None], release[:, None]
    mag = np.abs(v)
    with np.errstate(divide='ignore', invalid='ignore'):
        m = np.where(mag <= c, F32(1.0), (c / np.where(mag <= c, F32(1.0), mag)).astype(F32)).astype(F32)
    for j in range(8):
        k = 1 << j
        step = (F32(k) * delta).astype(F32)
        nxt = m.copy()
        nxt[:, k:] = np.minimum(m[:, k:], (m[:, :-k] + step).astype(F32))
        m = nxt
    n1 = np.arange(1, FRAME + 1, dtype=F32)
    h = fma32(np.broadcast_to(n1, v.shape), np.broadcast_to(delta, v.shape), np.broadcast_to(g[:, None], v.shape))
    return np.minimum(F32(1.0), np.minimum(m, h)).astype(F32)


def apply(E, setting, level_start=None, level_end=None, state=None, reset=None, hold=None, return_gain=False):
    """THE RULE.  E: int16 [rows, T * 256], what the 16 kHz call delivers; setting: a Setting, None (off) or one per row; level_start,
    level_end: float32 [rows, T], the leveller's pair (g_{t-1}, g_t) of every frame (koala_amd.level.track's `start` and `end`: 1 and 1
    for rows that do not level or are held) or None: no stream levels; state: float32 [rows] = g in front of the call (None: fresh);
    reset: [rows, T] or None, the call's per-frame resets; hold: [rows] or None, its held streams (their rows come back as E).
    -> (out int16 like E, state' float32 [rows]) and, with return_gain, G float32 [rows, T * 256] (1 where the limiter did not run)"""
    E = np.asarray(E, np.int16)
    rows = E.shape[0]
    T = E.shape[1] // FRAME
    ceiling, release, on = _table(setting, rows)
    g = fresh(rows) if state is None else np.array(state, F32).reshape(rows).copy()
    held = np.zeros(rows, bool) if hold is None else np.asarray(hold).reshape(rows) != 0
    live = on & ~held
    reset = np.zeros((rows, T), bool) if reset is None else np.asarray(reset).reshape(rows, T) != 0
    start = np.ones((rows, T), F32) if level_start is None else np.asarray(level_start, F32).reshape(rows, T)
    end = np.ones((rows, T), F32) if level_end is None else np.asarray(level_end, F32).reshape(rows, T)
    w = (np.arange(FRAME, dtype=F32) / F32(FRAME)).astype(F32)
    out = np.empty((rows, T, FRAME), np.int16)
    Gs = np.ones((rows, T, FRAME), F32)
    frames = E.reshape(rows, T, FRAME)
    for t in range(T):
        g = np.where(live & reset[:, t], F32(1.0), g).astype(F32)
        ramp = fma32(np.broadcast_to(w, (rows, FRAME)), np.broadcast_to((end[:, t] - start[:, t]).astype(F32)[:, None], (rows, FRAME)),
                     np.broadcast_to(start[:, t][:, None], (rows, FRAME)))
        v = (frames[:, t].astype(F32) * ramp).astype(F32)
        G = np.where(live[:, None], gains(v, ceiling, release, g), F32(1.0)).astype(F32)
        out[:, t] = to_pcm((v * G).astype(F32))
        Gs[:, t] = G
        g = np.where(live, G[:, -1], g).astype(F32)
    out = out.reshape(E.shape)
    return (out, g, Gs.reshape(rows, T * FRAME)) if return_gain else (out, g)


__all__ = ['Setting', 'OFF', 'FIELDS', 'settings', 'check', 'fresh', 'gains', 'apply']
