"""
The rule of the high-band carry (include/pv_koala_batch.h, HIGH-BAND CARRY; DESIGN.md section 2, ninth extension) in numpy float32, for
whole streams that begin fresh: what a frame handle at 32 000 or 48 000 Hz made with `high_band='carry'` delivers, given what the same
handle delivers without it (E) and its frame report's mask_sum.

    R = rate / 16000, D = delay_sample = 304 R
    y      = in_stage(x)                         int16 at 16 kHz (third extension)
    Lf[n]  = out_stage_sum(y delayed by 256)     the out-stage's fmaf chain, NOT rounded to int16
    s'[t]  = g + (1 - g) (mask_sum[t] / 257)     (linked channels: the max over the group first); 0 in front of the stream
    G[n]   = fmaf(w, s'[t] - s'[t-1], s'[t-1])   j = floor((n - 24 R) / R), t = floor(j / 256), w = (j - 256 t) / 256
    out[n] = to_pcm(fmaf(G[n], (float) x[n - D] - Lf[n], (float) E[n]))

Every operation is one float32 operation, in this order; `fma32` is an exact float32 fused multiply-add.  Self-contained: numpy only.
"""
import math

import numpy as np

F32 = np.float32
RATES = (32000, 48000)
Y_HIST = 256 + 48  # in-stage samples the rule looks back over: one engine frame and the out-stage's history


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


def delay_sample(rate):
    return Y_HIST * (rate // 16000)


def prototype(K):
    """the stages' low-pass of K = R in double: a Blackman-Harris windowed sinc of 48 K + 1 taps, cut-off 0.94 / K, unit sum"""
    L, c = 48 * K + 1, 24 * K
    g0 = []
    for i in range(L):
        px = math.pi * 0.94 * (i - c) / K
        sinc = 1.0 if i == c else math.sin(px) / px
        w = (0.35875 - 0.48829 * math.cos(2.0 * math.pi * i / (L - 1)) + 0.14128 * math.cos(4.0 * math.pi * i / (L - 1)) -
             0.01168 * math.cos(6.0 * math.pi * i / (L - 1)))
        g0.append(sinc * w)
    total = 0.0
    for v in g0:
        total += v
    return np.array([v / total for v in g0], np.float64)


def _chain(a, first, step, count, taps):
    """sum over the taps, ascending, of fmaf(tap_j, a[first - j + step * q], acc), q = 0 .. count - 1, acc = 0 first -> float32 [rows, count]"""
    acc = np.zeros((a.shape[0], count), F32)
    for j, h in enumerate(taps):
        lo = first - j
        acc = fma32(np.full(acc.shape, h, F32), a[:, lo:lo + step * (count - 1) + 1:step], acc)
    return acc


def in_stage(x, rate):
    """x int16 [rows, N] at `rate`, N a multiple of R, streams that begin fresh -> y int16 [rows, N / R] at 16 kHz"""
    R = rate // 16000
    h = prototype(R).astype(F32)
    H = 48 * R
    a = np.concatenate([np.zeros((x.shape[0], H), F32), np.asarray(x, np.int16).astype(F32)], axis=1)
    return to_pcm(_chain(a, H, R, x.shape[1] // R, h))


def low_band(y, rate):
    """Lf: y int16 [rows, Q] -> float32 [rows, R Q], the out-stage's sums over y delayed by one engine frame (256 samples)"""
    R = rate // 16000
    h = (R * prototype(R)).astype(F32)
    Q = y.shape[1]
    a = np.concatenate([np.zeros((y.shape[0], Y_HIST), F32), np.asarray(y, np.int16).astype(F32)], axis=1)[:, :Q + 48]
    out = np.empty((y.shape[0], R * Q), F32)
    for p in range(R):
        out[:, p::R] = _chain(a, 48, 1, Q, h[p::R])
    return out


def gains(mask_sum, min_gain=None, channels=1):
    """s': mask_sum float32 [rows, T] (the frame report's third value), min_gain [rows] or [rows, T] in [0, 1] (the limit in force in the call
    that processed the frame; None: 0), channels: of a linked group (1: no link) -> float32 [rows, T]"""
    s = np.asarray(mask_sum, F32) * F32(1.0 / 257.0)
    if channels > 1:
        grouped = s.reshape(s.shape[0] // channels, channels, -1)
        s = np.ascontiguousarray(np.broadcast_to(grouped.max(axis=1, keepdims=True), grouped.shape)).reshape(s.shape)
    g = np.zeros(s.shape, F32) if min_gain is None else np.broadcast_to(np.asarray(min_gain, F32).reshape(s.shape[0], -1), s.shape)
    return (g + ((F32(1.0) - g) * s).astype(F32)).astype(F32)


def ramp(sp, rate):
    """G: s' float32 [rows, T] -> float32 [rows, T 256 R], the overlap-add's cross-fade between consecutive frames' gains, delayed by the
    out-stage's 24 samples at 16 kHz"""
    R = rate // 16000
    rows, T = sp.shape
    s = np.concatenate([np.zeros((rows, 2), F32), sp], axis=1)  # s'[-2], s'[-1] = 0
    j = np.arange(T * 256 * R) // R - 24
    t = j // 256
    w = ((j - 256 * t).astype(F32) / F32(256.0)).astype(F32)
    hi, lo = s[:, t + 2], s[:, t + 1]
    return fma32(np.broadcast_to(w, hi.shape), (hi - lo).astype(F32), lo)


def carry(x, enhanced, mask_sum, rate, min_gain=None, channels=1):
    """x, enhanced int16 [rows, T 256 R] from the streams' beginning; mask_sum [rows, T] -> int16, what the handle with the carry delivers"""
    if rate not in RATES:
        raise ValueError("the high-band carry is defined at 32000 and 48000 Hz, not at %r" % (rate,))
    x = np.asarray(x, np.int16)
    D = delay_sample(rate)
    xd = np.concatenate([np.zeros((x.shape[0], D), np.int16), x], axis=1)[:, :x.shape[1]].astype(F32)
    hb = (xd - low_band(in_stage(x, rate), rate)).astype(F32)
    G = ramp(gains(mask_sum, min_gain, channels), rate)
    return to_pcm(fma32(G, hb, np.asarray(enhanced, np.int16).astype(F32)))


__all__ = ['RATES', 'delay_sample', 'in_stage', 'low_band', 'gains', 'ramp', 'carry']
