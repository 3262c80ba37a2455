"""
The switch model: a KNS1 model every gate of which saturates, its inputs, and an integer reference of what the network must compute --
shared by tests/test_switch_recipe.py (CPU) and tests/test_gpu_switch_model.py; not a test module.

With every gate saturated the bf16 network is a digital circuit ("Network kernels: the switch model"): r and z are
exactly 0 or 1, n is exactly -1 or +1, h' = fma(z, h - n, n) stays in {-1, 0, +1}, the heads are exactly 0 or 1 -- all exact as bf16
operands and as the fp16 mask -- and a last-bit difference in a pre-activation of magnitude several hundred changes nothing.  The correct
output is then an integer computation, and the engine can be held to it with == on every route.

Saturation, derived from the code.  The bf16 gates (kns_device.hpp gate_block_bf16 / gate_elem_bf16 / fast_sigmoid, kns_gru.hip through them;
oracle/kns_oracle.c gru_block and the head epilogue of frame_block) are q(y) = 1 / (1 + 2^y) on PRE-SCALED operands: y = -log2(e) x for r, z
and the heads, y = 2 log2(e) x for n = 1 - 2 q(y).
  * y >= 128: 2^y is above the largest float32 and becomes +inf (v_exp_f32 and (float) exp2((double) y) alike), 1 + inf = inf, 1 / inf = +0.
  * y <= -25: 2^y <= 2^-25 is below half an ulp of 1, so 1 + 2^y == 1 whatever the last bit of 2^y is, and 1 / 1 = 1.
The saturation point is therefore |y| = 128 (the larger of the two), and the margin the recipe keeps is twice that: every scaled
pre-activation the integer reference ever sees has |y| >= 256 (tests/test_switch_recipe.py asserts it).

The constants.  LOG2E = 1.44269504088896341f is the engine's constant (scale_gates / gate_scaled: one float32 multiplication BEFORE the
weights are rounded to bf16).  G = float32(512 ln 2) = 354.89..., so a dense r / z weight +-G becomes -+512 (1 + 1e-7) and rounds to the
bf16 value 512 exactly; the n columns carry +-G/2, which the n scale 2 log2(e) turns into the same 512.  In the quantum U = G/4 (scaled: 128
for r / z, 256 for n):
  r, z   weights +-4U; b_ih = 0, b_hh = U (4m + 2), an odd multiple of G/2; the pre-activation is U (4k + 4m + 2), k the integer sum over
         h in {-1, 0, 1} and y in {0, 1}: never closer to zero than 2U = G/2 -- scaled 256.
  n      weights +-2U; b_ih = U (the G/4 offset of gi_n), b_hh = 2U m with m = +-1 (the G/2 offset of gh_n); gi_n + r gh_n is
         U (2 k_i + 1 + r (2 k_h + 2m)), an odd multiple of U for r = 0 and for r = 1: never closer to zero than U = G/4 -- scaled 256.
         (With n weights +-G the same offsets would hold the same margin at twice the gi: |gi_n| = 1024 |k| leaves fp16 at |k| = 64, and the
         sum of 271 random signs gets there; +-G/2 keeps the margin and |gi| = 512 |k| + 256 <= 65 280 up to |k| = 127, 7.7 sigma.)
  heads  weights +-GH, GH = 512 (a bf16 value as it is; the head matrices are rounded but not scaled), b_head = GH (m + 1/2), m in {-1, 0}:
         |x| >= 256, scaled by log2(e) 369.
  gi is exact in fp16: 512 k (+ 256) has at most 8 significant bits; |gi| < 65 504, the fp16 maximum, is asserted on what the reference sees.
  A biased hidden-state row b_lo = bf16(b - bf16(b)) of the packed W_hh is 1e-5 here; it cannot decide anything (what remains uncovered).

Features are real numbers, so in every layer A a block of F = 64 "input units" does the thresholding: all three gates of input unit u have
W_hh = 0, b_hh = 0 and read ONE feature bin (and one tap of a five-frame front-end) through w_in (a single 1, embedding channel u) and the
e rows of W_ih: gi = s GF (f_k - THETA) for r, s GF/2 (f_k - THETA) for n, s = +-1 per gate, GF = float32(1024 ln 2): scaled
+-1024 (f_k - THETA), which stays a single entry of the folded matrix.  The z gate reads the same bin as -GF (f_k - THETA_Z) with
THETA_Z = -36, below every feature (ln 1e-10 = -23.03): z = 0 in every frame, so the unit's state is s_n (2 [f_k > THETA] - 1), the
bin's bit of THIS frame (with a z that switched on the bit a unit would keep the first value it ever took).  mean = 0, scale = 1, THETA = -12 (|X|^2 = 6e-6: far
above the rounding noise of integer samples, ln P about -17.7, far below any tone).  The inputs are chosen so that every bin of every frame
of every stream has |f - THETA| >= 0.3125 in both precisions: 0.25 for the margin 256 / 1024, 0.0625 for the rounding of a feature below 32
to bf16.  |gi| <= 1024 (11.1 + 36) = 48 230 there (a full-scale sine has ln P = 11.1).  The other units of layer A read no feature: dense over h (the input units' included) and y.
The block sits at units 0-63, 96-159 or 200-263 for seed % 3 = 0, 1, 2: every column of every matrix is dense in two models of three.

fp32: kns_exp clamps its argument to [-87, 88], so kns_sigmoid(-x) is 1 / (1 + e^88) = 6e-39, not 0: r, z and the heads saturate to
{6e-39, 1}; kns_tanh is exactly +-1 (e^-87 vanishes beside 1).  The hidden state is still exactly {-1, 0, 1} (z (h - n) = 1e-38 vanishes
beside n) and the samples are the reference's, but the mask is not bit for bit 0: tests/test_switch_recipe.py records it, and the fp32
engine is held to its own oracle, as everywhere.

Inputs.  Sixteen streams of 64 frames: runs of 2-5 frames of either digital silence or a sum of one to three tones at HALF-bin frequencies
(k0 + 1/2) / 512 -- under the sqrt-Hann window such a tone is exactly the two lines k0 and k0 + 1, so a steady frame sets a few bins, a frame
in which a run begins or ends splatters over all of them, and a silent frame sets none.  Every stream was drawn until it met the
feature condition (SUBSEEDS: the accepted draws, found on the CPU by running this file from the repository root, fixed here).
"""
import os

import numpy as np

from koala_amd import params
from oracle import oracle

H, BINS, G3, HEADS = params.HIDDEN, params.BINS, params.G3, params.HEADS
LOG2E = np.float32(1.44269504088896341)
G = np.float32(512.0 * np.log(2.0))
U = np.float32(G / np.float32(4))
GH = np.float32(512.0)
GF = np.float32(1024.0 * np.log(2.0))
THETA = -12.0
THETA_Z = -36.0             # an input unit's z gate reads its bin against a threshold no feature reaches: z = 0, the unit follows its bin
F = 64
SATURATION = 128.0          # |y| from which 2^y = inf (and beyond which, negative, 1 + 2^y == 1): see above
MARGIN = 2 * SATURATION     # the smallest scaled |pre-activation| the recipe allows
FEATURE_GAP = MARGIN / 1024.0 + 0.0625
FP16_MAX = 65504.0
SEEDS = (1, 2, 3)
ROWS, FRAMES = 16, 64
SILENT_FEATURE = float(np.log(1e-10))


def round_bf16(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------------- the circuit and its KNS1 file

class Circuit:
    """the model in integers.  Per layer l = 2 stage + (0: A, 1: B): wi [d, 813] over the layer's dense input (A: y_prev, B: layer A's h),
    wh [271, 813], entries -1 / 0 / +1 (times 4U in the r and z columns, 2U in the n columns); bh [813] in U; per stage head [271, d_out]
    in +-1 and mh [d_out] (b_head = GH (mh + 1/2)).  Input units: block p0 .. p0 + F - 1 of every layer A, bin[i], tap[i], sign [4][F][3]."""

    def __init__(self, seed, front_taps=1):
        rng = np.random.default_rng([20240, seed])
        self.seed, self.front_taps = seed, front_taps
        self.p0 = (0, 96, 200)[seed % 3]
        self.bin = (7 * seed + 4 * np.arange(F) + 1) % BINS
        self.tap = np.arange(F) % front_taps
        self.sign = rng.choice([-1, 1], size=(4, F, 3))
        blk = np.arange(self.p0, self.p0 + F)
        self.cols = np.concatenate([blk, H + blk, 2 * H + blk])  # the input units' gate columns
        self.wi, self.wh, self.bh, self.head, self.mh = [], [], [], [], []
        for s in range(4):
            d_in = HEADS[s - 1] if s else 0
            for layer_b in (0, 1):
                wi = rng.choice([-1, 1], size=(H if layer_b else d_in, G3))
                wh = rng.choice([-1, 1], size=(H, G3))
                bh = np.concatenate([4 * rng.integers(-2, 2, 2 * H) + 2, 2 * rng.choice([-1, 1], H)])
                if not layer_b:
                    wi[:, self.cols] = 0
                    wh[:, self.cols] = 0
                    bh[self.cols] = 0
                self.wi.append(wi), self.wh.append(wh), self.bh.append(bh)
            self.head.append(rng.choice([-1, 1], size=(H, HEADS[s])))
            self.mh.append(rng.integers(-1, 1, HEADS[s]))

    def tensors(self):
        """the KNS1 tensors (koala_amd.params.tensor_order)"""
        t = {name: np.zeros(shape, np.float32) for name, shape in params.tensor_order(self.front_taps)}
        t['scale'][:] = 1.0
        blk = np.arange(self.p0, self.p0 + F)
        t['w_in'][self.tap * BINS + self.bin, blk] = 1.0
        gate = np.concatenate([np.full(2 * H, 4.0), np.full(H, 2.0)]).astype(np.float32) * U  # |weight| per column: G, G, G/2
        for s in range(4):
            d_in = HEADS[s - 1] if s else 0
            a, b = 2 * s, 2 * s + 1
            w = np.zeros((d_in + H, G3), np.float32)
            w[:d_in] = self.wi[a] * gate
            bi = np.zeros(G3, np.float32)
            bi[2 * H:] = U                       # gi_n: G/4
            for g in range(3):
                c = g * H + blk
                gf = GF if g < 2 else GF / np.float32(2)
                sign, theta = (-1, THETA_Z) if g == 1 else (self.sign[s, :, g], THETA)
                w[d_in + blk, c] = sign * gf
                bi[c] = sign * gf * np.float32(-theta)
            t['s%d.w_ih_a' % s][:] = w
            t['s%d.b_ih_a' % s][:] = bi
            t['s%d.w_hh_a' % s][:] = self.wh[a] * gate
            t['s%d.b_hh_a' % s][:] = self.bh[a] * U
            t['s%d.w_ih_b' % s][:] = self.wi[b] * gate
            t['s%d.b_ih_b' % s][2 * H:] = U
            t['s%d.w_hh_b' % s][:] = self.wh[b] * gate
            t['s%d.b_hh_b' % s][:] = self.bh[b] * U
            t['s%d.w_head' % s][:] = self.head[s] * GH
            t['s%d.b_head' % s][:] = (self.mh[s] + 0.5) * GH
        return t


def model_path(directory, seed, front_taps=1):
    path = os.path.join(str(directory), 'switch_%d_%d.kns' % (seed, front_taps))
    if not os.path.exists(path):
        params.write_params(path, Circuit(seed, front_taps).tensors())
    return path


# ---------------------------------------------------------------------------------------------------- inputs

# the accepted draw of every row (running this file prints this line)
SUBSEEDS = (0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 0)


def draw(row, sub, frames=FRAMES):
    """one candidate stream: int16 [frames * 256]"""
    rng = np.random.default_rng([977, row, sub])
    x = np.zeros(frames * 256)
    t = 0
    while t < frames:
        run = int(rng.integers(2, 6))
        if rng.random() >= (0.5 if t == 0 and row % 4 == 3 else 0.3):
            n = np.arange(t * 256, min(frames, t + run) * 256)
            for k0 in rng.choice(np.arange(3, 250), size=int(rng.integers(1, 4)), replace=False):
                x[n] += rng.integers(2000, 9000) * np.cos(2 * np.pi * (k0 + 0.5) * n / 512 + rng.uniform(0, 2 * np.pi))
        t += run
    return np.rint(x).astype(np.int16)


_streams = {}


def switch_streams(frames=FRAMES):
    """int16 [ROWS, frames * 256]: the first `frames` frames of the sixteen streams (read-only)"""
    if 'x' not in _streams:
        _streams['x'] = np.stack([draw(r, SUBSEEDS[r]) for r in range(ROWS)])
        _streams['x'].setflags(write=False)
    return _streams['x'][:, :frames * 256]


class Analysis:
    """the oracle's spectrum and features of [rows, T * 256] samples, frame by frame with the history it keeps; `reset` [rows, T]"""

    def __init__(self, model, rows, precision):
        self.o = oracle.Oracle(model, 1, oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32)
        self.hist = np.zeros((rows, 256), np.int16)

    def process(self, x, reset=None):
        rows, T = x.shape[0], x.shape[1] // 256
        spec, feat = np.empty((T, rows, BINS, 2), np.float32), np.empty((T, rows, BINS), np.float32)
        for b in range(rows):
            for t in range(T):
                if reset is not None and reset[b, t]:
                    self.hist[b] = 0
                fr = np.ascontiguousarray(x[b, t * 256:(t + 1) * 256])
                spec[t, b], feat[t, b] = self.o.analysis(self.hist[b], fr)
                self.hist[b] = fr
        return spec, feat


def feature_gap(x, model):
    """the smallest |f - THETA| over every bin and frame of the rows of x, in either precision (the bf16 operand is the feature rounded)"""
    gaps = []
    for precision in ('fp32', 'bf16'):
        feat = Analysis(model, x.shape[0], precision).process(x)[1]
        gaps.append(np.abs(feat - THETA).min())
        gaps.append(np.abs(round_bf16(feat) - THETA).min() + 0.0625)
    return float(min(gaps))


# ---------------------------------------------------------------------------------------------------- the integer reference

class Reference:
    """`rows` streams through the circuit: thresholds the oracle's features, runs eight layers and four heads as sign tests of integer sums
    (float64 matrix products of small integers are exact), and synthesises the samples from the oracle's spectrum and the 0 / 1 mask.
    Nothing of the oracle's network code is used.  Keeps, over everything it has processed: `min_pre` (the smallest scaled |pre-activation|),
    `max_gi` (the largest scaled |gi|), `min_gap` (the smallest |f - THETA| of a bin an input unit read)."""

    def __init__(self, circuit, model, rows, precision):
        self.c, self.rows, self.precision = circuit, rows, precision
        self.an = Analysis(model, rows, precision)
        self.h = np.zeros((8, rows, H))
        self.tail = np.zeros((rows, 256), np.float32)
        self.ctx = np.full((circuit.front_taps, rows, BINS), SILENT_FEATURE)  # the last feature frames, oldest first
        self.min_pre, self.max_gi, self.min_gap = np.inf, 0.0, np.inf
        self.dense = np.ones(G3, bool)
        self.dense[circuit.cols] = False
        self.z_seen = np.zeros(2, bool)

    def _restart(self, rows):
        rows = np.asarray(rows, bool)
        self.h[:, rows] = 0
        self.tail[rows] = 0
        self.ctx[:, rows] = SILENT_FEATURE

    def reset(self, rows):
        """a masked reset between calls (a per-frame flag does the same in front of its frame: `process`)"""
        self._restart(rows)
        self.an.hist[np.asarray(rows, bool)] = 0

    def _layer(self, l, x, bits):
        """x [rows, d] the dense input, bits [rows, F] or None -> the layer's new hidden state"""
        c, h = self.c, self.h[l]
        weight = np.concatenate([np.full(2 * H, 4.0), np.full(H, 2.0)])      # in U: r, z 4U per unit of k, n 2U
        offset = np.concatenate([np.zeros(2 * H), np.ones(H)])               # b_ih in U: the G/4 of gi_n
        scale = np.concatenate([np.full(2 * H, 128.0), np.full(H, 256.0)])   # U scaled: r, z by log2 e, n by 2 log2 e
        gi = weight * (x @ c.wi[l]) + offset
        gh = weight * (h @ c.wh[l]) + c.bh[l]
        self.max_gi = max(self.max_gi, float(np.abs(gi * scale)[:, self.dense].max()))
        if bits is not None:  # the input units: gi = s 1024 (f - THETA) scaled, standing for the sign alone here
            s = c.sign[l // 2]
            for g in range(3):
                gi[:, g * H + c.p0:g * H + c.p0 + F] = -1e6 if g == 1 else s[:, g] * (2.0 * bits - 1.0) * 1e6
        pr, pz = gi[:, :H] + gh[:, :H], gi[:, H:2 * H] + gh[:, H:2 * H]
        r, z = pr > 0, pz > 0
        pn = gi[:, 2 * H:] + r * gh[:, 2 * H:]
        pre = np.abs(np.concatenate([pr, pz, pn], axis=1) * scale)[:, self.dense]
        self.min_pre = min(self.min_pre, float(pre.min()))
        self.z_seen[0] |= bool((~z).any())
        self.z_seen[1] |= bool(z.any())
        self.h[l] = np.where(z, h, np.where(pn > 0, 1.0, -1.0))
        return self.h[l]

    def frame(self, feat):
        """one frame of every stream from its features [rows, 257] -> (mask [rows, 257] of 0.0 / 1.0, [y1, y2, y3])"""
        c = self.c
        self.ctx = np.concatenate([self.ctx[1:], feat[None].astype(np.float64)])
        read = self.ctx[c.tap, :, c.bin].T  # [rows, F]
        operand = round_bf16(read) if self.precision == 'bf16' else read
        self.min_gap = min(self.min_gap, float(np.abs(operand - THETA).min()))
        bits = operand > THETA
        y, ys = np.zeros((self.rows, 0)), []
        for s in range(4):
            ha = self._layer(2 * s, y, bits)
            hb = self._layer(2 * s + 1, ha, None)
            pre = hb @ c.head[s] + c.mh[s] + 0.5
            self.min_pre = min(self.min_pre, float(np.abs(pre).min() * 512.0 * float(LOG2E)))
            y = (pre > 0).astype(np.float64)
            ys.append(y)
        return y.astype(np.float32), ys[:3]

    def process(self, x, reset=None):
        """x int16 [rows, T * 256], reset [rows, T] or None -> dict: pcm int16 [rows, T * 256], mask float32 [T, rows, 257],
        hidden int8 [T, 8, rows, 271] (the state behind every frame), spectrum, features"""
        T = x.shape[1] // 256
        spec, feat = self.an.process(x, reset)
        out ={'pcm': np.empty_like(x), 'mask': np.empty((T, self.rows, BINS), np.float32), 'hidden': np.empty((T, 8, self.rows, H), np.int8),
               'spectrum': spec, 'features': feat}
        for t in range(T):
            if reset is not None and reset[:, t].any():
                self._restart(reset[:, t])
            out['mask'][t], _ = self.frame(feat[t])
            out['hidden'][t] = self.h
            for b in range(self.rows):
                out['pcm'][b, t * 256:(t + 1) * 256] = oracle.synthesis(spec[t, b], out['mask'][t, b], self.tail[b])
        return out


def first_difference(got, want, names):
    """the first index at which two arrays differ, as 'name = value' for every axis, or None"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return 'shapes %s and %s' % (got.shape, want.shape)
    ne = np.argwhere(got != want)
    if not len(ne):
        return None
    i = tuple(ne[0])
    return '%d differ, first at %s: got %r, want %r' % (len(ne), ', '.join('%s %d' % p for p in zip(names, i)), got[i].item(), want[i].item())


if __name__ == '__main__':  # the search behind SUBSEEDS: per row the first draw whose every bin of every frame keeps FEATURE_GAP
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        model, found = model_path(d, SEEDS[0]), []
        for row in range(ROWS):
            sub = 0
            while feature_gap(draw(row, sub)[None], model) < FEATURE_GAP:
                sub += 1
            found.append(sub)
        print('SUBSEEDS = (%s)' % ', '.join(str(s) for s in found))
