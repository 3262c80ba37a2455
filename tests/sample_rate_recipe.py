"""
The sample-rate stages of DESIGN.md section 2 (third extension) restated in numpy float32, from the text: the prototype in double, the two
tables rounded once, and every tap one exact float32 fma (fma32 below: tests/frame_report_recipe.py's, for operands of any sign) in the
spec's order.  Shared by tests/test_sample_rate.py (CPU) and tests/test_gpu_sample_rate.py; not a test module.

`Recipe` is a whole handle at 8, 32 or 48 kHz: in-stage -> oracle.Oracle.process -> out-stage, with streaming state, every kind of
reset and stream records of the stages' part.
"""
import math

import numpy as np

from oracle import oracle

F32 = np.float32
RATES = (8000, 32000, 48000)


def fma32(a, b, c):
    """round_to_float32(a * b + c) for float32 arrays of ANY sign, exactly -- tests/frame_report_recipe.py's fma32 (non-negative addends)
    with the direction of its round-to-odd step taken from the sum's sign: a * b is exact in float64, the float64 sum is made
    round-to-odd with TwoSum's error term, after which the rounding to float32 is the single rounding of the exact value."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    even = (bits & 1) == 0
    up = np.where(s < 0, err < 0, err > 0)    # the exact value lies further from zero than s
    down = np.where(s < 0, err > 0, err < 0)  # ... nearer to zero (s != 0 wherever err != 0)
    bits = np.where(even & up, bits + 1, np.where(even & down, bits - 1, bits))
    return bits.view(np.float64).astype(F32)


def ratio(rate):
    return 3 if rate == 48000 else 2


def frame_length(rate):
    return rate * 256 // 16000


def delay_sample(rate):
    """at the handle's rate: the engine's frame and 24 R high-rate samples per stage"""
    return frame_length(rate) + (48 if rate < 16000 else 48 * ratio(rate))


def prototype(R):
    """-> (g float64 [L], hd float32 [L], hi float32 [L]); math.sin / math.cos: the C library's, as the engine's host code uses"""
    L, c = 48 * R + 1, 24 * R
    g0 = []
    for i in range(L):
        x = 0.94 * (i - c) / R
        px = math.pi * x
        sinc = 1.0 if i == c else math.sin(px) / px
        w = (0.35875 - 0.48829 * math.cos(2.0 * math.pi * i / (L - 1)) + 0.14128 * math.cos(4.0 * math.pi * i / (L - 1)) -
             0.01168 * math.cos(6.0 * math.pi * i / (L - 1)))
        g0.append(sinc * w)
    total = 0.0
    for v in g0:
        total += v
    g = np.array([v / total for v in g0], np.float64)
    return g, g.astype(F32), (R * g).astype(F32)


def to_pcm(acc):
    """clip(round_half_away(acc)) -> int16"""
    r = np.sign(acc) * np.floor(np.abs(acc.astype(np.float64)) + 0.5)
    return np.clip(r, -32768, 32767).astype(np.int16)


def interpolate(hist, a, R, hi):
    """hist int16 [n, 48] (the samples in front of a), a int16 [n, N] -> int16 [n, R N]"""
    n, N = a.shape
    x = np.concatenate([hist, a], axis=1).astype(F32)
    out = np.empty((n, N * R), np.int16)
    for p in range(R):
        acc = np.zeros((n, N), F32)
        j = 0
        while p + R * j <= 48 * R:
            acc = fma32(np.full((n, N), hi[p + R * j], F32), x[:, 48 - j:48 - j + N], acc)
            j += 1
        out[:, p::R] = to_pcm(acc)
    return out


def decimate(hist, a, R, hd):
    """hist int16 [n, 48 R], a int16 [n, R N] -> int16 [n, N]"""
    n, M = a.shape
    N, H = M // R, 48 * R
    x = np.concatenate([hist, a], axis=1).astype(F32)
    acc = np.zeros((n, N), F32)
    for i in range(H + 1):
        acc = fma32(np.full((n, N), hd[i], F32), x[:, H - i:H - i + M:R], acc)
    return to_pcm(acc)


class Stage:
    """one direction for n streams, streaming: keeps the last 48 (interpolator) or 48 R (decimator) input samples"""

    def __init__(self, n, R, up):
        self.n, self.R, self.up = n, R, up
        _, self.hd, self.hi = prototype(R)
        self.hist = np.zeros((n, 48 if up else 48 * R), np.int16)

    def reset(self, rows):
        self.hist[np.asarray(rows, bool)] = 0

    def run(self, a):
        a = np.ascontiguousarray(a, np.int16)
        out = interpolate(self.hist, a, self.R, self.hi) if self.up else decimate(self.hist, a, self.R, self.hd)
        H = self.hist.shape[1]
        self.hist = np.concatenate([self.hist, a], axis=1)[:, -H:].copy()
        return out

    def abs_tap_sum(self):
        """largest sum of |tap| over an output phase: how far one LSB of every input can move an output"""
        if self.up:
            return max(float(np.abs(self.hi[p::self.R].astype(np.float64)).sum()) for p in range(self.R))
        return float(np.abs(self.hd.astype(np.float64)).sum())


class Delay256:
    """the engine under a unity mask: its input one frame later"""

    def __init__(self, n):
        self.prev = np.zeros((n, 256), np.int16)

    def reset(self, rows):
        self.prev[np.asarray(rows, bool)] = 0

    def process(self, x):
        y = np.concatenate([self.prev, x], axis=1)
        self.prev = y[:, -256:].copy()
        return np.ascontiguousarray(y[:, :-256])


class Recipe:
    """n streams of a handle at `rate`: in-stage -> inner 16 kHz engine -> out-stage.  `model` None: the inner engine is the pure
    delay (a unity mask, or min_gain = 1); else oracle.Oracle on that model."""

    def __init__(self, model, n, precision, rate):
        self.n, self.rate, self.R, self.fl = n, rate, ratio(rate), frame_length(rate)
        self.s_in = Stage(n, self.R, up=rate < 16000)
        self.s_out = Stage(n, self.R, up=rate > 16000)
        self.o = Delay256(n) if model is None else oracle.Oracle(model, n, oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32)

    def reset(self, rows=None):
        rows = np.ones(self.n, bool) if rows is None else np.asarray(rows, bool)
        if rows.any():
            self.s_in.reset(rows)
            self.s_out.reset(rows)
            if isinstance(self.o, Delay256):
                self.o.reset(rows)
            else:
                self.o.reset(rows.astype(np.uint8))

    def inner(self, x):
        """the in-stage alone: what the inner 16 kHz engine is fed"""
        return self.s_in.run(x)

    def process(self, x):
        """x int16 [n, T * frame_length] -> enhanced, same shape"""
        return self.s_out.run(np.ascontiguousarray(self.o.process(self.s_in.run(x))))

    def process_resets(self, x, reset):
        """per-frame stream resets [n, T]: the call cut at its frames, a reset right before its frame"""
        out = []
        for t in range(x.shape[1] // self.fl):
            self.reset(reset[:, t] != 0)
            out.append(self.process(np.ascontiguousarray(x[:, t * self.fl:(t + 1) * self.fl])))
        return np.concatenate(out, axis=1)

    def rs_state(self):
        """the stages' part of the version-2 stream records: rs_in, rs_out, int16, zero-padded to 16-byte words -> uint8 [n, bytes]"""
        s = np.concatenate([self.s_in.hist, self.s_out.hist], axis=1)
        pad = (-s.shape[1] * 2) % 16
        return np.concatenate([np.ascontiguousarray(s).view(np.uint8), np.zeros((self.n, pad), np.uint8)], axis=1)
