"""
The rational sample-rate stages of DESIGN.md section 2 (third extension, generalised) restated in numpy float32, from the text: one stage
"up U, down D" over the prototype of K = max(U, D), every tap one exact float32 fma (sample_rate_recipe.fma32) in ascending tap order, then
sample_rate_recipe.to_pcm.  Shared by tests/test_rational_rate.py (CPU) and tests/test_gpu_rational_rate.py; not a test module.

`Recipe` is a whole handle at 12 or 24 kHz: in-stage -> oracle.Oracle.process -> out-stage, with streaming state, every kind of reset and
stream records of the stages' part.
"""
import numpy as np

import sample_rate_recipe as srr
from oracle import oracle

F32 = np.float32
RATES = (12000, 24000)
COMMON = 48000
STAGES = {12000: ((4, 3), (3, 4)), 24000: ((2, 3), (3, 2))}  # rate -> (in-stage, out-stage), each (U, D)


def common_k(rate):
    return COMMON // min(rate, 16000)


def frame_length(rate):
    return rate * 256 // 16000


def delay_sample(rate):
    """at the handle's rate: the engine's frame and 24 K samples at 48 kHz per stage"""
    return frame_length(rate) + 2 * (24 * common_k(rate) * rate // COMMON)


def table(K, U):
    """h_U[i] = (float) (U g[i]) over the prototype of K, L = 48 K + 1 values"""
    return (U * srr.prototype(K)[0]).astype(F32)


def hist_length(K, U):
    return 48 * K // U


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
            acc = srr.fma32(np.full((rows, Q), table[i], F32), x[:, first:first + D * (Q - 1) + 1:D], acc)
            i, j = i + U, j + 1
        out[:, p::U] = srr.to_pcm(acc)
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


class Recipe:
    """n streams of a handle at `rate`: in-stage -> inner 16 kHz engine -> out-stage.  `model` None: the inner engine is the pure
    delay (a unity mask, or min_gain = 1); else oracle.Oracle on that model."""

    def __init__(self, model, n, precision, rate):
        self.n, self.rate, self.fl, K = n, rate, frame_length(rate), common_k(rate)
        (ui, di), (uo, do) = STAGES[rate]
        self.s_in, self.s_out = Stage(n, K, ui, di), Stage(n, K, uo, do)
        self.o = srr.Delay256(n) if model is None else oracle.Oracle(model, n, oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32)

    def reset(self, rows=None):
        rows = np.ones(self.n, bool) if rows is None else np.asarray(rows, bool)
        if rows.any():
            self.s_in.reset(rows)
            self.s_out.reset(rows)
            if isinstance(self.o, srr.Delay256):
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

    def set_rs_state(self, blob):
        """the inverse of rs_state: a record's stages' part -> the two histories"""
        v = np.ascontiguousarray(blob).view(np.int16)
        hi, ho = self.s_in.hist.shape[1], self.s_out.hist.shape[1]
        self.s_in.hist, self.s_out.hist = v[:, :hi].copy(), v[:, hi:hi + ho].copy()
