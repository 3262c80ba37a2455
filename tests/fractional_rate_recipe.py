"""
Packet handles at 44 100 and 22 050 Hz (sixth extension) restated in numpy float32, from the text: the prototype of
K = 441 in double (sample_rate_recipe.prototype), the two tables rounded once, every tap one exact float32 fma (sample_rate_recipe.fma32) in
ascending tap order, then sample_rate_recipe.to_pcm.  Shared by tests/test_fractional_rate.py (CPU) and tests/test_gpu_fractional_rate.py;
not a test module.

`Stream` is ONE stream of such a handle, streaming, with the state the text lists and no more: N mod 441, the in-stage's last input samples,
the out-stage's last inner output samples.  Its inner path is any stateful callable  samples int16 [m] -> int16 [m]  (m >= 0): a 16 kHz
packet stream around the oracle (`oracle_inner`), or a pure delay by 511 samples (`DelayInner`).
"""
import numpy as np

import packet_recipe as pr
import sample_rate_recipe as srr

F32 = np.float32
RATES = (44100, 22050)
D = 441
L = 48 * D + 1
INNER_DELAY = 511
UP = {44100: 160, 22050: 320}
H_OUT = 49  # inner output samples the out-stage keeps: its taps reach 48 samples back from an index that can lie one before the newest


def shift(rate):
    """c: the smallest non-negative integer that makes (246 519 + c) / U whole"""
    return (-(24 * D + INNER_DELAY * D + 24 * D)) % UP[rate]


def delay_sample(rate):
    return (24 * D + INNER_DELAY * D + 24 * D + shift(rate)) // UP[rate]


def in_taps(rate):
    """the most taps of one in-stage output, which is also the input samples the in-stage keeps: 133 / 67"""
    return -(-L // UP[rate])


def inner_samples(n, rate):
    """M(N): inner samples that exist once a stream has received n samples in total = floor((U n - 1) / 441) + 1, M(0) = 0"""
    n = np.asarray(n, np.int64)
    return (UP[rate] * n - 1) // D + 1


_tables = {}


def tables(rate):
    """(h_in, h_out) float32 [L]: (float) (U g[i]) and (float) (441 g[i])"""
    if rate not in _tables:
        g = srr.prototype(D)
        assert g.shape == (L,)
        _tables[rate] = ((UP[rate] * g).astype(F32), (D * g).astype(F32))
    return _tables[rate]


def chain(table, first, step, taps, x, newest):
    """acc[k] = the ascending chain over j = 0 .. taps - 1 of fmaf(table[first[k] + step j], x[newest[k] - j], acc[k]) from 0, a tap index
    at or beyond L ending the chain (such a tap does not exist)"""
    acc = np.zeros(first.shape, F32)
    for j in range(taps):
        i = first + step * j
        live = i < L
        if not live.any():
            break
        at = newest - j
        assert at[live].min() >= 0
        new = srr.fma32(table[np.minimum(i, L - 1)], x[np.maximum(at, 0)], acc)
        acc = np.where(live, new, acc)
    return srr.to_pcm(acc)


class DelayInner(object):
    """the 16 kHz packet handle under a unity mask: its input 511 samples later"""

    def __init__(self):
        self.buf = np.zeros(INNER_DELAY, np.int16)

    def __call__(self, y):
        cat = np.concatenate([self.buf, np.asarray(y, np.int16)])
        self.buf = cat[cat.size - INNER_DELAY:].copy()
        return cat[:cat.size - INNER_DELAY]


def oracle_inner(model, precision):
    """a 16 kHz packet stream around one oracle stream"""
    ps = pr.PacketStream(pr.oracle_stream(model, precision), 256)
    return ps.push


class Stream(object):
    def __init__(self, rate, inner):
        self.rate, self.U, self.c, self.inner = rate, UP[rate], shift(rate), inner
        self.h_in, self.h_out = tables(rate)
        self.t_in = in_taps(rate)
        self.phase = 0                                  # N mod 441
        self.hist_in = np.zeros(self.t_in, np.int16)    # the in-stage's last input samples
        self.hist_out = np.zeros(H_OUT, np.int16)       # the out-stage's last inner output samples
        self.fed = []                                   # what the inner path was given, call by call (tests read it)

    def due(self, count):
        """inner samples a call with `count` samples feeds the inner path"""
        return int(inner_samples(self.phase + count, self.rate) - inner_samples(self.phase, self.rate))

    def in_stage(self, x):
        U, ph, H = self.U, self.phase, self.t_in
        m0, m1 = int(inner_samples(ph, self.rate)), int(inner_samples(ph + x.size, self.rate))
        xs = np.concatenate([self.hist_in, x]).astype(F32)  # sample e (counted from the cycle's start: N - N mod 441) at [H + e - ph]
        t = D * np.arange(m0, m1, dtype=np.int64)
        y = chain(self.h_in, t % U, U, self.t_in, xs, H + t // U - ph)
        self.hist_in = np.concatenate([self.hist_in, x])[-H:].copy()
        return y

    def out_stage(self, v, count):
        U, ph = self.U, self.phase
        m0 = int(inner_samples(ph, self.rate))
        vs = np.concatenate([self.hist_out, v]).astype(F32)  # inner sample e (counted from the cycle's start) at [H_OUT + e - m0]
        p = U * np.arange(ph, ph + count, dtype=np.int64) - self.c
        e = p // D  # (floor: the mathematical modulus below)
        assert count == 0 or (H_OUT + e.max() - m0) < vs.size
        z = chain(self.h_out, p - D * e, D, 49, vs, H_OUT + e - m0)
        self.hist_out = np.concatenate([self.hist_out, v])[-H_OUT:].copy()
        return z

    def push(self, samples):
        """the next len(samples) output samples; len 0: nothing changes"""
        x = np.asarray(samples, np.int16)
        if x.size == 0:
            return np.zeros(0, np.int16)
        y = self.in_stage(x)
        assert y.size == self.due(x.size)
        self.fed.append(y)
        v = np.asarray(self.inner(y), np.int16)
        assert v.size == y.size
        z = self.out_stage(v, x.size)
        self.phase = (self.phase + x.size) % D
        return z


def out_abs_tap_sum(rate):
    """the out-stage's largest per-phase sum of |tap|: how far one LSB of every inner sample can move an output"""
    t = np.abs(tables(rate)[1].astype(np.float64))
    return max(float(t[r::D].sum()) for r in range(D))
