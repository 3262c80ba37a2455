"""
What a stream under a band profile must deliver (include/pv_koala_batch.h: pv_koala_batch_set_band_profile), from the oracle's stage
functions, the way tests/min_gain_recipe.py is built on them.  Shared by tests/test_band_profile.py and tests/test_gpu_band_profile.py; not a
test module.

`Oracle.process_with_mask` gives every frame's mask m, `Oracle.analysis` its spectrum; numpy float32 forms m1 = g + (1 - g) m (one
subtraction, one product, one sum, each rounded to float32) and m' = min(ceiling, max(floor, m1)) (exact), and `oracle.synthesis` makes
the samples.  The rule is written out here on its own, not imported from koala_amd.bands: the package's statement is one of the things under test.
"""
import numpy as np

from koala_amd import bands
from min_gain_recipe import Recipe
from oracle import oracle

K = 257
F32 = np.float32


def shaped(m, g, floor, ceiling):
    """m' of one frame: float32 [257] each, g a float32 scalar"""
    g = F32(g)
    u = F32(1.0) - g
    m1 = (g + (u * m.astype(F32)).astype(F32)).astype(F32)
    return np.minimum(ceiling.astype(F32), np.maximum(floor.astype(F32), m1))


def profiles(n, seed=0):
    """n profiles (floor [n, 257], ceiling [n, 257]) that differ per stream: random pairs, a high-pass, a band-pass, neutral, all ones, an
    all-zero ceiling, a depth limit, then random pairs again"""
    rng = np.random.default_rng(seed)
    a, b = rng.random((n, K), dtype=F32), rng.random((n, K), dtype=F32)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    fixed = [(np.zeros(K, F32), bands.highpass(90.0)), (np.zeros(K, F32), bands.bandpass(300.0, 3400.0)), (np.zeros(K, F32), np.ones(K, F32)),
             (np.ones(K, F32), np.ones(K, F32)), (np.zeros(K, F32), np.zeros(K, F32)), (bands.depth_limit_db([(0, 6), (300, 18)]), np.ones(K, F32))]
    for i, (f, c) in enumerate(fixed):
        if 1 + i < n:
            lo[1 + i], hi[1 + i] = f, c
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


# per-stream minimum gains that go with them (0, 0.25 and 1 among them), cycled over the streams
GAINS = np.array([0.0, 0.25, 1.0, 0.0, 0.5, 0.0, 0.25, 0.1], F32)


class ProfileRecipe(Recipe):
    """n streams of the spec under a minimum gain and a band profile: the samples"""

    def process(self, x, gains, floor=None, ceiling=None):
        x = np.ascontiguousarray(x, np.int16)
        T = x.shape[1] // 256
        lo = np.zeros((self.n, K), F32) if floor is None else np.asarray(floor, F32)
        hi = np.ones((self.n, K), F32) if ceiling is None else np.asarray(ceiling, F32)
        _, mask = self.o.process_with_mask(x)
        out = np.empty_like(x)
        for b in range(self.n):
            for t in range(T):
                fr = x[b, t * 256:(t + 1) * 256]
                spec, _ = self.o.analysis(self.hist[b], fr)
                out[b, t * 256:(t + 1) * 256] = oracle.synthesis(spec, shaped(mask[t, b], gains[b], lo[b], hi[b]), self.tail[b])
                self.hist[b] = fr
        return out

    def process_resets(self, x, gains, reset, floor=None, ceiling=None):
        """per-frame stream resets [n, T]: frame by frame, a reset right before its frame"""
        T = x.shape[1] // 256
        outs = []
        for t in range(T):
            self.reset(reset[:, t] != 0)
            outs.append(self.process(np.ascontiguousarray(x[:, t * 256:(t + 1) * 256]), gains, floor, ceiling))
        return np.concatenate(outs, axis=1)
