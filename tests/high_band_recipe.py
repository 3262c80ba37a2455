"""
The high-band carry of DESIGN.md section 2 (ninth extension) restated in numpy float32 on top of tests/sample_rate_recipe.py (prototype /
table, fma32, to_pcm, the in-stage), STREAMING: call by call, with exactly the per-stream state the text lists -- the last D input samples
(int16), the last 256 + 48 in-stage outputs (int16) and s' of the last two frames (float32).  Shared by tests/test_high_band.py (CPU),
tests/test_gpu_high_band.py and tests/test_gpu_high_band_routes.py; not a test module.  koala_amd/highband.py states the same rule for whole streams, independently.
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


# ------------------------------------------------------------------------------------------------ inputs at and near full scale

EDGE_SEQ = (1, 1, 1, 3, 2, 1)  # frames per call
EDGE_GAINS = np.tile(np.array([0.0, 1.0], F32), 8)
EDGE_DITHER = (14, 15)


def edge_streams(rate, seed=1):
    """int16 [16, 9 frames]: eight inputs, each on two streams (the even one with g = 0, the odd one with g = 1): DC at +32767, DC at -32768,
    the rails alternating at the handle's Nyquist in either phase, uniform noise over the whole int16 range, one full-scale impulse on the
    last sample of frame 5 (the last of EDGE_SEQ's 3-frame call), two frames of silence and then a full-scale step, +-1 LSB dither"""
    F = rate * 256 // 16000
    N, rng = sum(EDGE_SEQ) * F, np.random.default_rng(seed)
    n = np.arange(N)
    alt = np.where(n % 2 == 0, 32767, -32768)
    impulse, step = np.zeros(N, int), np.zeros(N, int)
    impulse[6 * F - 1] = 32767
    step[2 * F:] = 32767
    rows = [np.full(N, 32767), np.full(N, -32768), alt, alt[::-1] if N % 2 == 0 else -alt - 1, rng.integers(-32768, 32768, N), impulse, step,
            rng.choice([-1, 1], N)]
    assert rows[3][0] == -32768 and rows[3][1] == 32767
    return np.ascontiguousarray(np.repeat(np.array(rows), 2, axis=0).astype(np.int16))


def edge_conditions(Lf, e, want):
    """what keeps a run over edge_streams from being vacuous, from the recipe's Lf (HighBand.parts), the plain handle's samples and the
    expected output of the whole run -- never from the carrying handle's own output"""
    d = list(EDGE_DITHER)
    return {'Lf leaves the int16 range': bool((Lf > 32767).any() and (Lf < -32768).any()),
            'E reaches a rail': bool((e == 32767).any() or (e == -32768).any()),
            'the output reaches +32767': bool((want == 32767).any()), 'the output reaches -32768': bool((want == -32768).any()),
            'the dither streams leave E': bool((want[d] != e[d]).any(axis=1).all())}
