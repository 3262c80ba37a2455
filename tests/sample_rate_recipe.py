"""
The sample-rate stages of DESIGN.md section 2 (third extension) restated in numpy float32, from the text: one stage "up U, down D" over the
prototype of K = max(U, D) in double, its table rounded once, every tap one exact float32 fma (fma32 below: tests/frame_report_recipe.py's,
for operands of any sign) in ascending tap order, then to_pcm.  The constants restate koala_amd/csrc/kns_kernels.h (rs_stage_in,
rs_stage_hist, rs_delay, rs_record_bytes).  Shared by tests/test_sample_rate.py and tests/test_rational_rate.py (CPU),
tests/sample_rate_cases.py and the two GPU modules that call it; not a test module.

`Recipe` is a whole handle at 8, 12, 24, 32 or 48 kHz: in-stage -> oracle.Oracle.process -> out-stage, with streaming state, every kind
of reset and stream records of the stages' part.
"""
import math

import numpy as np

from oracle import oracle

F32 = np.float32
RATES = (8000, 12000, 24000, 32000, 48000)
# rate -> (in-stage, out-stage), each (U, D); a stage's prototype is that of K = max(U, D)
STAGES = {8000: ((2, 1), (1, 2)), 12000: ((4, 3), (3, 4)), 24000: ((2, 3), (3, 2)), 32000: ((1, 2), (2, 1)), 48000: ((1, 3), (3, 1))}


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


def frame_length(rate):
    return rate * 256 // 16000


def hist_length(K, U):
    """the input samples a stage keeps: (L - 1) / U"""
    return 48 * K // U


def delay_sample(rate):
    """at the handle's rate: the engine's frame and, for both stages together, the in-stage's history"""
    U, D = STAGES[rate][0]
    return frame_length(rate) + hist_length(max(U, D), U)


def record_tail(rate):
    """bytes of the stages' part of a version-2 stream record: rs_in, rs_out, int16, in whole 16-byte words"""
    return (sum(hist_length(max(U, D), U) for U, D in STAGES[rate]) * 2 + 15) // 16 * 16


def prototype(K):
    """-> g float64 [L], L = 48 K + 1; math.sin / math.cos: the C library's, as the engine's host code uses"""
    L, c = 48 * K + 1, 24 * K
    g0 = []
    for i in range(L):
        x = 0.94 * (i - c) / K
        px = math.pi * x
        sinc = 1.0 if i == c else math.sin(px) / px
        w = (0.35875 - 0.48829 * math.cos(2.0 * math.pi * i / (L - 1)) + 0.14128 * math.cos(4.0 * math.pi * i / (L - 1)) -
             0.01168 * math.cos(6.0 * math.pi * i / (L - 1)))
        g0.append(sinc * w)
    total = 0.0
    for v in g0:
        total += v
    return np.array([v / total for v in g0], np.float64)


def table(K, U):
    """h_U[i] = (float) (U g[i]) over the prototype of K, L = 48 K + 1 values"""
    return (U * prototype(K)).astype(F32)


def to_pcm(acc):
    """clip(round_half_away(acc)) -> int16"""
    r = np.sign(acc) * np.floor(np.abs(acc.astype(np.float64)) + 0.5)
    return np.clip(r, -32768, 32767).astype(np.int16)


def stage(hist, a, U, D, table):
    """out[n] = to_pcm(sum over i = D n mod U, + U, ... < L, ascending, of fmaf(h_U[i], (float) a[(D n - i) / U], acc)), acc = 0 first.
    hist int16 [rows, (L - 1) / U] (the samples in front of a), a int16 [rows, D Q] -> int16 [rows, U Q]"""
    rows, M = a.shape
    L = len(table)
    H = (L - 1) // U
    assert hist.shape == (rows, H) and M % D == 0
    Q = M // D
    x = np.concatenate([hist, a], axis=1).astype(F32)
    out = np.empty((rows, U * Q), np.int16)
    for p in range(U):  # the outputs n = p + U q, q = 0 ... Q - 1: D n = U (D q + e) + r
        e, r = divmod(D * p, U)
        acc = np.zeros((rows, Q), F32)
        i, j = r, 0
        while i < L:
            first = H + e - j  # a[(D n - i) / U] = a[D q + e - j]
            acc = fma32(np.full((rows, Q), table[i], F32), x[:, first:first + D * (Q - 1) + 1:D], acc)
            i, j = i + U, j + 1
        out[:, p::U] = to_pcm(acc)
    return out


class Stage:
    """one stage for n streams, streaming: keeps its last (L - 1) / U input samples"""

    def __init__(self, n, K, U, D):
        self.n, self.U, self.D = n, U, D
        self.table = table(K, U)
        self.hist = np.zeros((n, hist_length(K, U)), np.int16)

    def reset(self, rows):
        self.hist[np.asarray(rows, bool)] = 0

    def run(self, a):
        a = np.ascontiguousarray(a, np.int16)
        out = stage(self.hist, a, self.U, self.D, self.table)
        H = self.hist.shape[1]
        self.hist = np.concatenate([self.hist, a], axis=1)[:, -H:].copy()
        return out

    def abs_tap_sum(self):
        """largest sum of |tap| over an output phase: how far one LSB of every input can move an output"""
        t = np.abs(self.table.astype(np.float64))
        return max(float(t[r::self.U].sum()) for r in range(self.U))


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
        self.n, self.rate, self.fl = n, rate, frame_length(rate)
        self.s_in, self.s_out = (Stage(n, max(U, D), U, D) for U, D in STAGES[rate])
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
        s = np.ascontiguousarray(np.concatenate([self.s_in.hist, self.s_out.hist], axis=1)).view(np.uint8)
        return np.concatenate([s, np.zeros((self.n, -s.shape[1] % 16), np.uint8)], axis=1)

    def set_rs_state(self, blob):
        """the inverse of rs_state: a record's stages' part -> the two histories"""
        v = np.ascontiguousarray(blob).view(np.int16)
        hi, ho = self.s_in.hist.shape[1], self.s_out.hist.shape[1]
        self.s_in.hist, self.s_out.hist = v[:, :hi].copy(), v[:, hi:hi + ho].copy()
