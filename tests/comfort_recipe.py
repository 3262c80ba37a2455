"""
What a stream with comfort noise must deliver (include/pv_koala_batch.h: pv_koala_batch_set_comfort_noise), from the oracle's stage
functions, the way tests/band_profile_recipe.py is built on them.  Shared by tests/test_comfort.py and tests/test_gpu_comfort.py; not a test
module.

Per frame `Oracle.analysis` gives the spectrum X and `Oracle.process_with_mask` the mask m; numpy float32 forms m' (band_profile_recipe's
`shaped`) and Y = (m' X) + (((1 - m') A) z), every operation rounded to float32, z the hash of (seed, n, k); `oracle.synthesis(Y, ones, tail)`
makes the samples -- the product by 1.0 is exact.  The rule is written out here on its own, not imported from koala_amd.comfort: the
package's statement is one of the things under test.  The counter, the resets and the holds live in the recipe.
"""
import numpy as np

from band_profile_recipe import ProfileRecipe, shaped
from frame_report_recipe import energy_terms, row_sum
from oracle import oracle

K = 257
F32 = np.float32
U32 = np.uint32
ONES = np.ones(K, F32)


def hashed(seed, n):
    """the hashed words v[k], uint32 [257], of one frame"""
    k = np.arange(K, dtype=np.uint64)
    M = np.uint64(0xFFFFFFFF)
    v = (np.uint64(seed) ^ ((np.uint64(n) * np.uint64(0x9E3779B9)) & M)) ^ ((k * np.uint64(0x85EBCA6B)) & M)
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x7FEB352D)) & M
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x846CA68B)) & M
    v = v ^ (v >> np.uint64(16))
    return v.astype(U32)


def noise(seed, n):
    """(z_re, z_im) float32 [257] of one frame"""
    v = hashed(seed, n)
    z_re = ((v & U32(0xFFFF)).astype(F32) - F32(32767.5)) * F32(1.0 / 32768.0)
    z_im = ((v >> U32(16)).astype(F32) - F32(32767.5)) * F32(1.0 / 32768.0)
    z_im[0] = z_im[K - 1] = 0
    return z_re.astype(F32), z_im.astype(F32)


def filled(spec, mp, amp, seed, n):
    """Y float32 [257, 2] of one frame"""
    z_re, z_im = noise(seed, n)
    w = (F32(1.0) - mp).astype(F32)
    a = (w * amp.astype(F32)).astype(F32)
    y = np.empty((K, 2), F32)
    y[:, 0] = ((mp * spec[:, 0]).astype(F32) + (a * z_re).astype(F32)).astype(F32)
    y[:, 1] = ((mp * spec[:, 1]).astype(F32) + (a * z_im).astype(F32)).astype(F32)
    y[0, 1] = y[K - 1, 1] = 0  # (bins 0 and 256 are real)
    return y


def curves(n, seed=0):
    """n amplitude curves [n, 257] that differ per stream: random levels around 1e-2 (some 30 LSB RMS), a zero curve at row 2"""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, K), dtype=F32) * F32(0.03)).astype(F32)
    if n > 2:
        a[2] = 0
    return np.ascontiguousarray(a)


class ComfortRecipe(ProfileRecipe):
    """n streams of the spec under a minimum gain, a band profile and comfort noise: the samples, e_out of every frame, and the counters"""

    def __init__(self, model, n, precision):
        super().__init__(model, n, precision)
        self.count = np.zeros(n, U32)
        self.e_out = None

    def reset(self, rows):
        super().reset(rows)
        self.count[np.asarray(rows, bool)] = 0

    def process(self, x, gains, floor=None, ceiling=None, amp=None, seeds=None, on=None):
        x = np.ascontiguousarray(x, np.int16)
        T = x.shape[1] // 256
        lo = np.zeros((self.n, K), F32) if floor is None else np.asarray(floor, F32)
        hi = np.ones((self.n, K), F32) if ceiling is None else np.asarray(ceiling, F32)
        on = np.ones(self.n, bool) if on is None else np.asarray(on, bool)
        _, mask = self.o.process_with_mask(x)
        out = np.empty_like(x)
        self.e_out = np.empty((self.n, T), F32)
        for b in range(self.n):
            for t in range(T):
                fr = x[b, t * 256:(t + 1) * 256]
                spec, _ = self.o.analysis(self.hist[b], fr)
                mp = shaped(mask[t, b], gains[b], lo[b], hi[b])
                if on[b]:
                    y = filled(spec, mp, amp[b], seeds[b], self.count[b])
                    self.count[b] += U32(1)
                else:
                    y = np.stack([(mp * spec[:, 0]).astype(F32), (mp * spec[:, 1]).astype(F32)], axis=-1)
                    y[0, 1] = y[K - 1, 1] = 0
                self.e_out[b, t] = row_sum(energy_terms(y))
                out[b, t * 256:(t + 1) * 256] = oracle.synthesis(y, ONES, self.tail[b])
                self.hist[b] = fr
        return out

    def process_resets(self, x, gains, reset, floor=None, ceiling=None, amp=None, seeds=None, on=None):
        """per-frame stream resets [n, T]: frame by frame, a reset right before its frame"""
        T = x.shape[1] // 256
        outs, es = [], []
        for t in range(T):
            self.reset(reset[:, t] != 0)
            outs.append(self.process(np.ascontiguousarray(x[:, t * 256:(t + 1) * 256]), gains, floor, ceiling, amp, seeds, on))
            es.append(self.e_out)
        self.e_out = np.concatenate(es, axis=1)
        return np.concatenate(outs, axis=1)
