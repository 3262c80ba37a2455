"""
The high-band carry of DESIGN.md section 2 (ninth extension) restated in numpy float32 on top of tests/sample_rate_recipe.py (prototype /
table, fma32, to_pcm, the in-stage), STREAMING: call by call, with exactly the per-stream state the text lists -- the last D input samples
(int16), the last 256 + 48 in-stage outputs (int16) and s' of the last two frames (float32).  Shared by tests/test_high_band.py (CPU) and
tests/test_gpu_high_band.py; not a test module.  koala_amd/highband.py states the same rule for whole streams, independently.
"""
import numpy as np

import sample_rate_recipe as srr
from sample_rate_recipe import F32, fma32, to_pcm

RATES = (32000, 48000)
Y_HIST = 256 + 48


def stage_sum(hist, a, U, table):
    """the sum of sample_rate_recipe.stage for a stage "up U, down 1", kept as float32: hist [rows, 48], a [rows, Q] -> [rows, U Q]"""
    rows, Q = a.shape
    L, H = len(table), (len(table) - 1) // U
    assert hist.shape == (rows, H)
    x = np.concatenate([hist, a], axis=1).astype(F32)
    out = np.empty((rows, U * Q), F32)
    for p in range(U):
        acc = np.zeros((rows, Q), F32)
        i, j = p, 0
        while i < L:
            acc = fma32(np.full((rows, Q), table[i], F32), x[:, H - j:H - j + Q], acc)
            i, j = i + U, j + 1
        out[:, p::U] = acc
    return out


class HighBand:
    """n streams of the carry at `rate`; `channels`: of a linked group (1: no link).  process() takes what the plain handle gave for the
    same call -- E and the report's mask_sum -- and the attenuation limit in force in that call."""

    def __init__(self, n, rate, channels=1):
        assert rate in RATES and n % channels == 0
        self.n, self.rate, self.R, self.C = n, rate, rate // 16000, channels
        self.D = srr.delay_sample(rate)
        assert self.D == Y_HIST * self.R
        (ui, di), (uo, do) = srr.STAGES[rate]
        self.s_in = srr.Stage(n, max(ui, di), ui, di)  # the handle's own in-stage: y is its output
        self.table = srr.table(max(uo, do), uo)        # the out-stage's taps
        self.x_hist = np.zeros((n, self.D), np.int16)
        self.y_hist = np.zeros((n, Y_HIST), np.int16)
        self.sp = np.zeros((n, 2), F32)  # s'[t-1], s'[t-2] of the next call's frame 0

    def reset(self, rows=None):
        rows = np.ones(self.n, bool) if rows is None else np.asarray(rows, bool)
        self.s_in.reset(rows)
        self.x_hist[rows], self.y_hist[rows], self.sp[rows] = 0, 0, 0

    def gains(self, mask_sum, g):
        s = (np.asarray(mask_sum, F32) * F32(1.0 / 257.0)).astype(F32)
        if self.C > 1:
            grp = s.reshape(self.n // self.C, self.C, -1)
            s = np.ascontiguousarray(np.broadcast_to(grp.max(axis=1, keepdims=True), grp.shape)).reshape(s.shape)
        g = np.broadcast_to(np.asarray(g, F32).reshape(self.n, 1), s.shape)
        return (g + ((F32(1.0) - g).astype(F32) * s).astype(F32)).astype(F32)

    def parts(self, x, mask_sum, g):
        """one call -> (x delayed by D as float32, Lf, G), and the state moves on"""
        x = np.ascontiguousarray(x, np.int16)
        R, T = self.R, x.shape[1] // (256 * self.R)
        assert x.shape == (self.n, T * 256 * R) and np.shape(mask_sum) == (self.n, T)
        y = self.s_in.run(x)
        ycat = np.concatenate([self.y_hist, y], axis=1)
        Lf = stage_sum(ycat[:, :48], ycat[:, 48:48 + T * 256], R, self.table)
        xcat = np.concatenate([self.x_hist, x], axis=1)
        xd = xcat[:, :x.shape[1]].astype(F32)
        s = np.concatenate([self.sp[:, ::-1], self.gains(mask_sum, g)], axis=1)  # s'[-2], s'[-1], s'[0] ...
        j = np.arange(T * 256 * R) // R - 24
        t = j // 256
        w = ((j - 256 * t).astype(F32) / F32(256.0)).astype(F32)
        assert np.array_equal(w.astype(np.float64) * 256.0, (j - 256 * t).astype(np.float64))  # w is exact
        hi, lo = s[:, t + 2], s[:, t + 1]
        G = fma32(np.broadcast_to(w, hi.shape), (hi - lo).astype(F32), lo)
        self.x_hist, self.y_hist = xcat[:, -self.D:].copy(), ycat[:, -Y_HIST:].copy()
        self.sp = np.ascontiguousarray(s[:, :-3:-1])
        return xd, Lf, G

    def process(self, x, enhanced, mask_sum, g=0.0):
        """x, enhanced int16 [n, T F]; mask_sum [n, T]; g: scalar or [n] -> int16 [n, T F]"""
        xd, Lf, G = self.parts(x, mask_sum, np.broadcast_to(np.asarray(g, F32), (self.n,)))
        hb = (xd - Lf).astype(F32)
        return to_pcm(fma32(G, hb, np.ascontiguousarray(enhanced, np.int16).astype(F32)))
