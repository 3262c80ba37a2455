"""
The frame report of DESIGN.md section 2 (step 4, second extension) restated in numpy float32, from the text: every product, every fma and
every add of the spec is one explicit float32 operation here, in the spec's order.  Shared by tests/test_frame_report.py (CPU) and
tests/test_gpu_frame_report.py; not a test module.

Inputs are the oracle's stages: `Oracle.analysis(hist, frame)` for the spectrum X, `Oracle.process_with_mask` for the network's mask m (bf16:
the fp16 value widened), and m' = g + (1 - g) m as in tests/min_gain_recipe.py's Recipe.
"""
import numpy as np

from oracle import oracle

F32 = np.float32

# The bf16 bars of the report rows on the GPU.  profiles/r10_frame_report.txt (tools/frame_report_bars.py, CPU): the largest distance between
# the plain and the jittered bf16 recipe over every bf16 input of tests/test_gpu_frame_report.py was 1.449e-3 relative in e_out and 5.320e-5
# absolute in mask_sum / 257; the bars are 4 x those (the jitter probe has under-predicted the device by about 2 x before, DESIGN.md
# section 5: one factor of 2 on top of that).
BF16_E_OUT_REL = 4 * 1.449e-3
BF16_MEAN_GAIN_ABS = 4 * 5.320e-5


def fma32(a, b, c):
    """round_to_float32(a * b + c) for float32 arrays, exactly: a * b is exact in float64; the float64 sum is made round-to-odd with the
    error term of TwoSum, after which the rounding to float32 is the single rounding of the exact value (53 >= 2 * 24 + 2)."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    even = (bits & 1) == 0
    # (s > 0 wherever err != 0 here: both addends are non-negative)
    bits = np.where(even & (err > 0), bits + 1, np.where(even & (err < 0), bits - 1, bits))
    return bits.view(np.float64).astype(F32)


def row_sum(term):
    """term float32 [..., 257] -> float32 [...]: the spec's column chains and tree, plain float32 adds"""
    term = np.asarray(term, F32)
    P = []
    for c in range(16):
        p = term[..., c]
        for k2 in range(1, 16):
            p = (p + term[..., c + 16 * k2]).astype(F32)
        if c == 0:
            p = (p + term[..., 256]).astype(F32)
        P.append(p)
    Q = [(P[0] + P[8]).astype(F32)] + [(P[j] + P[16 - j]).astype(F32) for j in range(1, 8)]
    R = [(Q[2 * i] + Q[2 * i + 1]).astype(F32) for i in range(4)]
    S = [(R[2 * i] + R[2 * i + 1]).astype(F32) for i in range(2)]
    return (S[0] + S[1]).astype(F32)


def energy_terms(spec):
    """spec float32 [..., 257, 2] -> a[k]: fma(re, re, im * im) for k = 1 .. 255, re * re for the real bins 0 and 256"""
    re, im = np.asarray(spec[..., 0], F32), np.asarray(spec[..., 1], F32)
    a = fma32(re, re, (im * im).astype(F32))
    a[..., 0] = (re[..., 0] * re[..., 0]).astype(F32)
    a[..., 256] = (re[..., 256] * re[..., 256]).astype(F32)
    return a


def applied_mask(m, g):
    """m' = g + (1 - g) m: a subtraction, a product, a sum, each rounded (m float32 [..., 257], g scalar)"""
    g = F32(g)
    u = F32(F32(1.0) - g)
    return (g + (u * np.asarray(m, F32)).astype(F32)).astype(F32)


def report_rows(spec, m, g):
    """spec [..., 257, 2], raw mask m [..., 257], minimum gain g -> float32 [..., 4]"""
    spec = np.asarray(spec, F32)
    mp = applied_mask(m, g)
    y = np.stack([(mp * spec[..., 0]).astype(F32), (mp * spec[..., 1]).astype(F32)], axis=-1)
    y[..., 0, 1] = 0  # (bins 0 and 256 are real)
    y[..., 256, 1] = 0
    out = np.zeros(spec.shape[:-2] + (4,), F32)
    out[..., 0] = row_sum(energy_terms(spec))
    out[..., 1] = row_sum(energy_terms(y))
    out[..., 2] = row_sum(np.asarray(m, F32))
    return out


def sum64(term):
    """float64 sum of the same float32 terms"""
    return np.asarray(term, np.float64).sum(axis=-1)


class ReportRecipe:
    """n streams of the spec: the report rows of every frame, from the oracle's stages.  Keeps what `X` needs -- the previous frame --
    beside the oracle's own state."""

    def __init__(self, model, n, precision):
        self.o = oracle.Oracle(model, n, oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32)
        self.n = n
        self.hist = np.zeros((n, 256), np.int16)

    def reset(self, rows):
        rows = np.asarray(rows, bool)
        if rows.any():
            self.o.reset(rows.astype(np.uint8))
            self.hist[rows] = 0

    def stages(self, x):
        """x int16 [n, T * 256] -> (spectrum [n, T, 257, 2], raw mask [n, T, 257]); advances the streams"""
        x = np.ascontiguousarray(x, np.int16)
        T = x.shape[1] // 256
        _, mask = self.o.process_with_mask(x)
        spec = np.empty((self.n, T, 257, 2), F32)
        for b in range(self.n):
            for t in range(T):
                fr = x[b, t * 256:(t + 1) * 256]
                spec[b, t], _ = self.o.analysis(self.hist[b], fr)
                self.hist[b] = fr
        return spec, np.ascontiguousarray(mask.transpose(1, 0, 2))

    def process(self, x, gains=None):
        """-> report float32 [n, T, 4] under per-stream minimum gains (None: no limit)"""
        spec, m = self.stages(x)
        gains = np.zeros(self.n, F32) if gains is None else gains
        return np.stack([report_rows(spec[b], m[b], gains[b]) for b in range(self.n)])

    def process_resets(self, x, gains, reset):
        """per-frame stream resets [n, T]: frame by frame, a reset right before its frame"""
        T = x.shape[1] // 256
        rows = []
        for t in range(T):
            self.reset(reset[:, t] != 0)
            rows.append(self.process(np.ascontiguousarray(x[:, t * 256:(t + 1) * 256]), gains))
        return np.concatenate(rows, axis=1)
