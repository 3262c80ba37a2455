"""
The rule of the output leveller (include/pv_koala_batch.h, OUTPUT LEVELLER; DESIGN.md section 2, eleventh extension) in numpy float32: what
a handle delivers while a stream's leveller is on, given what the same handle delivers without it at 16 kHz (E, int16) and its frame report.

Per stream a setting (`Setting`; `settings()` builds one from dBFS and milliseconds) and two float32 values of state, lvl (the tracked
speech energy) and gain; fresh: lvl = 0, gain = 1.  For every frame t, with e_out and mask_sum of the stream's report row:

    speech  = mask_sum * (1/257) >= theta  and  e_out > e_floor
    if speech:  lvl = e_out                                   if lvl == 0
                lvl = lvl + a * (e_out - lvl)                 a = a_up if e_out > lvl else a_down
    want    = 1                                               if lvl == 0
            = min(max_boost, max(max_cut, sqrt(target / lvl)))
    g_t     = gain + slew * (want - gain);   gain = g_t
    out[256 t + n] = to_pcm(E[256 t + n] * fma(n / 256, g_t - g_{t-1}, g_{t-1}))      n = 0 .. 255

Every operation is one float32 operation, in this order; `fma32` is an exact float32 fused multiply-add; to_pcm rounds half away from zero
and saturates; a ceiling below the rails, and a gain that gives way before the product clips, is the peak limiter's
(koala_amd.limiter), which takes this product before to_pcm.  A reset makes the state fresh before its frame (the ramp then starts from 1), a held
stream keeps its state, a stream that is off delivers E and its state does not move.  Self-contained: numpy only.
"""
import math
from collections import namedtuple

import numpy as np

F32 = np.float32
FRAME = 256
BINS = 257
FRAME_MS = 16.0
# e_out of a stationary signal whose RMS is full scale (1.0): the report's energies are sums of |X[k]|^2 over the one-sided spectrum of a
# 512-sample block of samples / 32768 under the sqrt-Hann window w[n] = sin(pi n / 512) (no scaling in the
# FFT).  Parseval: sum_k |X[k]|^2 (one-sided, DC and Nyquist half-counted) = 256 sum_n (w[n] x[n])^2, and sum_n w[n]^2 = 256, so a signal of
# mean square P reads 256 * 256 * P.
ENERGY_AT_FULL_SCALE = 65536.0

Setting = namedtuple('Setting', 'on target max_boost max_cut theta e_floor a_up a_down slew')
FIELDS = Setting._fields[1:]
OFF = Setting(0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0)  # what a new handle holds for every stream


def energy(dbfs):
    """e_out of a stationary signal whose RMS is `dbfs` dB relative to full scale"""
    return ENERGY_AT_FULL_SCALE * 10.0 ** (dbfs / 10.0)


def rms_dbfs(e):
    """the RMS, in dBFS, of a stationary signal whose frames report the energy `e`"""
    with np.errstate(divide='ignore'):
        return 10.0 * np.log10(np.asarray(e, np.float64) / ENERGY_AT_FULL_SCALE)


def coefficient(ms):
    """the one-pole coefficient per 16 ms frame of a time constant in milliseconds (0: 1, no smoothing)"""
    return 1.0 if ms <= 0 else 1.0 - math.exp(-FRAME_MS / ms)


def settings(target_dbfs=-23.0, max_boost_db=18.0, max_cut_db=12.0, attack_ms=50.0, release_ms=400.0, slew_ms=100.0, theta=0.5,
             floor_dbfs=-60.0, on=True):
    """A `Setting` from physical units: speech frames are brought to an RMS of `target_dbfs`, by at most `max_boost_db` up and `max_cut_db`
    down; the tracked level follows rising energy with `attack_ms` and falling energy with `release_ms`, the gain follows with `slew_ms`;
    a frame is speech when its mean mask is at least `theta` and its output is above `floor_dbfs`."""
    s = Setting(1 if on else 0, float(F32(energy(target_dbfs))), float(F32(10.0 ** (max_boost_db / 20.0))), float(F32(10.0 ** (-max_cut_db / 20.0))),
                float(F32(theta)), float(F32(energy(floor_dbfs))), float(F32(coefficient(attack_ms))), float(F32(coefficient(release_ms))),
                float(F32(coefficient(slew_ms))))
    check(s)
    return s


def check(s):
    """ValueError unless `s` is a setting the library accepts"""
    ok = (('target', s.target > 0), ('max_boost', s.max_boost >= 1), ('max_cut', 0 < s.max_cut <= 1), ('theta', 0 <= s.theta <= 1),
          ('e_floor', s.e_floor >= 0), ('a_up', 0 < s.a_up <= 1), ('a_down', 0 < s.a_down <= 1), ('slew', 0 < s.slew <= 1))
    if s.on not in (0, 1):
        raise ValueError("`on` %r is not 0 or 1" % (s.on,))
    for name, good in ok:
        if not good or not math.isfinite(getattr(s, name)):
            raise ValueError("`%s` %r is outside its range" % (name, getattr(s, name)))


def fma32(a, b, c):
    """round_to_float32(a * b + c), exactly: the product is exact in float64, the float64 sum is made round-to-odd with TwoSum's error
    term, and the rounding to float32 is then the single rounding of the exact value"""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    even = (bits & 1) == 0
    up = np.where(s < 0, err < 0, err > 0)
    down = np.where(s < 0, err > 0, err < 0)
    bits = np.where(even & up, bits + 1, np.where(even & down, bits - 1, bits))
    return bits.view(np.float64).astype(F32)


def to_pcm(acc):
    """clip(round_half_away(acc)) -> int16"""
    acc = np.asarray(acc)
    r = np.sign(acc) * np.floor(np.abs(acc.astype(np.float64)) + 0.5)
    return np.clip(r, -32768, 32767).astype(np.int16)


def _table(setting, rows):
    """one Setting, None (off) or a list of them, one per row -> float32 [rows, 8] and on [rows]"""
    each = list(setting) if isinstance(setting, (list, tuple)) and not isinstance(setting, Setting) else [setting] * rows
    if len(each) != rows:
        raise ValueError("%d settings for %d streams" % (len(each), rows))
    each = [OFF if s is None else s for s in each]
    for s in each:
        check(s)
    return np.array([s[1:] for s in each], F32).reshape(rows, 8), np.array([s.on for s in each], bool)


def fresh(rows):
    """the state of `rows` fresh streams, float32 [rows, 2] = lvl, gain"""
    return np.tile(np.array([0.0, 1.0], F32), (rows, 1))


def track(report, setting, state=None, reset=None, hold=None):
    """The gains alone.  report: float32 [rows, T, 4]; setting: a Setting, None or one per row; state: float32 [rows, 2] (None: fresh);
    reset: [rows, T] or None; hold: [rows] or None -> (start, end, speech, state'): float32 [rows, T] each of g_{t-1} as frame t's ramp
    begins with it and of g_t (1 and 1 for rows that are off or held), bool [rows, T], float32 [rows, 2]"""
    report = np.asarray(report, F32)
    rows, T = report.shape[:2]
    tab, on = _table(setting, rows)
    target, max_boost, max_cut, theta, e_floor, a_up, a_down, slew = (tab[:, i] for i in range(8))
    state = fresh(rows) if state is None else np.array(state, F32).reshape(rows, 2)
    live = on & ~(np.zeros(rows, bool) if hold is None else np.asarray(hold).reshape(rows) != 0)
    reset = np.zeros((rows, T), bool) if reset is None else np.asarray(reset).reshape(rows, T) != 0
    lvl, gain = state[:, 0].copy(), state[:, 1].copy()
    start, end, spoke = np.ones((rows, T), F32), np.ones((rows, T), F32), np.zeros((rows, T), bool)
    one = F32(1.0)
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        for t in range(T):
            r = reset[:, t]
            lvl, gain = np.where(r, F32(0.0), lvl), np.where(r, one, gain)
            e, m = report[:, t, 1], (report[:, t, 2] * (one / F32(BINS))).astype(F32)
            speech = (m >= theta) & (e > e_floor)
            moved = (lvl + (np.where(e > lvl, a_up, a_down) * (e - lvl).astype(F32)).astype(F32)).astype(F32)
            lvl = np.where(speech, np.where(lvl == 0, e, moved), lvl).astype(F32)
            safe = np.where(lvl == 0, one, lvl)
            want = np.minimum(max_boost, np.maximum(max_cut, np.sqrt((target / safe).astype(F32)).astype(F32)))
            want = np.where(lvl == 0, one, want).astype(F32)
            g = (gain + (slew * (want - gain).astype(F32)).astype(F32)).astype(F32)
            start[:, t], end[:, t], spoke[:, t] = np.where(live, gain, one), np.where(live, g, one), speech & live
            gain = g
    new = np.stack([lvl, gain], axis=1).astype(F32)
    return start, end, spoke, np.where(live[:, None], new, state).astype(F32)


def apply(E, report, setting, state=None, reset=None, hold=None):
    """THE RULE.  E: int16 [rows, T * 256], what the 16 kHz call delivers; report: its frame report, float32 [rows, T, 4]; setting: a
    Setting, None (off) or one per row; state: float32 [rows, 2] = lvl, gain in front of the call (None: fresh); reset: [rows, T] or None,
    the call's per-frame resets; hold: [rows] or None, its held streams (their rows come back as E).
    -> (out int16 like E, gains float32 [rows, T + 1]: the gain in front of the call and g_t of every frame, state' float32 [rows, 2])"""
    E = np.asarray(E, np.int16)
    rows = E.shape[0]
    T = E.shape[1] // FRAME
    state = fresh(rows) if state is None else np.array(state, F32).reshape(rows, 2)
    start, end, _, new = track(report, setting, state, reset, hold)
    w = (np.arange(FRAME, dtype=F32) / F32(FRAME)).astype(F32)
    ramp = fma32(np.broadcast_to(w, (rows, T, FRAME)), np.broadcast_to((end - start).astype(F32)[:, :, None], (rows, T, FRAME)),
                 np.broadcast_to(start[:, :, None], (rows, T, FRAME)))
    out = to_pcm((E.reshape(rows, T, FRAME).astype(F32) * ramp).astype(F32)).reshape(E.shape)
    gains = np.concatenate([state[:, 1:2], end], axis=1).astype(F32)
    return out, gains, new


__all__ = ['Setting', 'OFF', 'FIELDS', 'ENERGY_AT_FULL_SCALE', 'energy', 'rms_dbfs', 'coefficient', 'settings', 'check', 'fma32', 'to_pcm', 'fresh',
           'track', 'apply']
