"""
What the synthesis stage must deliver given the network's mask, under a minimum gain, a band profile and comfort noise -- exactly, in both
precisions.  Shared by tests/test_segment_recipe.py (CPU) and tests/test_gpu_synthesis_segments.py; not a test module.

tests/test_gpu_channel_link_routes.py's `Tapped`, carried over to the rules of tests/band_profile_recipe.py (`shaped`) and
tests/comfort_recipe.py (`filled`): the raw mask m comes from outside -- the engine's own `mask` tap, or `Oracle.process_with_mask` -- and
everything behind it is float32 in the fp32 and in the bf16 configuration alike: `Oracle.analysis` gives the spectrum X,
numpy float32 forms m' and Y = m' X (+ the fill), `oracle.synthesis(Y, ones, tail)` makes the samples, and tests/frame_report_recipe.py the
report rows: e_in from X, mask_sum from the raw mask, e_out from Y.  So a comparison with this recipe is ==, on samples, report rows and
counters, whatever the precision of the network that made the mask.  The history, the overlap-add tail and the counter live here; a
per-frame reset zeroes the three right before its frame, as ComfortRecipe.process_resets does.
"""
import numpy as np

from band_profile_recipe import GAINS, profiles, shaped
from comfort_recipe import K, ONES, curves, filled
from frame_report_recipe import energy_terms, row_sum
from oracle import oracle

F32 = np.float32
U32 = np.uint32


def mixed(n=16, seed=0):
    """(floor, ceiling, gains, curves, seeds, on) of n streams, as tests/test_gpu_comfort.py's `mixed`: the profiles and gains of
    tests/band_profile_recipe.py (non-neutral), a curve (row 2: all zero) and a seed per stream, every fifth stream off"""
    lo, hi = profiles(n, seed)
    on = np.arange(n) % 5 != 4
    return lo, hi, np.resize(GAINS, n), curves(n, seed + 1), (np.arange(n, dtype=U32) * U32(2654435761) + U32(7)), on


def round_bf16(a):
    """float32 -> the nearest bf16 (ties to even), widened again"""
    u = np.ascontiguousarray(a, F32).view(U32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(U32).view(F32)


class SegmentRecipe:
    """n streams from a reset on: samples, report rows and counters from raw masks handed in"""

    def __init__(self, model, n):
        self.n = n
        self.an = oracle.Oracle(model, 1)  # (the analysis alone: its spectrum is float32 in either precision)
        self.hist, self.tail, self.count = np.zeros((n, 256), np.int16), np.zeros((n, 256), F32), np.zeros(n, U32)

    def reset(self, rows):
        rows = np.asarray(rows, bool)
        self.hist[rows], self.tail[rows], self.count[rows] = 0, 0, 0

    def process(self, x, m, gains, floor=None, ceiling=None, amp=None, seeds=None, on=None, reset=None, stored=None):
        """x int16 [n, T * 256], m raw masks [T, n, 257], gains [n], floor / ceiling / amp [n, 257], seeds [n], on [n] (None: no comfort
        noise), reset [n, T] or None; stored: the engine's spectrum tap [T, n, 257, 2] where it kept one, which must be the oracle's analysis
        -> (samples int16 [n, T * 256], report rows float32 [n, T, 4])"""
        x = np.ascontiguousarray(x, np.int16)
        T = x.shape[1] // 256
        lo = np.zeros((self.n, K), F32) if floor is None else np.asarray(floor, F32)
        hi = np.ones((self.n, K), F32) if ceiling is None else np.asarray(ceiling, F32)
        on = np.zeros(self.n, bool) if on is None else np.asarray(on, bool)
        out, rep = np.empty_like(x), np.zeros((self.n, T, 4), F32)
        for t in range(T):
            if reset is not None:
                self.reset(np.asarray(reset)[:, t] != 0)
            for b in range(self.n):
                fr = x[b, t * 256:(t + 1) * 256]
                spec, _ = self.an.analysis(self.hist[b], fr)
                if stored is not None:
                    assert np.array_equal(stored[t, b].view(U32), spec.view(U32)), (t, b)
                raw = np.asarray(m[t, b], F32)
                mp = shaped(raw, gains[b], lo[b], hi[b])
                if on[b]:
                    y = filled(spec, mp, amp[b], seeds[b], self.count[b])
                    self.count[b] += U32(1)
                else:
                    y = np.stack([(mp * spec[:, 0]).astype(F32), (mp * spec[:, 1]).astype(F32)], axis=-1)
                    y[0, 1] = y[K - 1, 1] = 0  # (bins 0 and 256 are real)
                rep[b, t, 0] = row_sum(energy_terms(spec))
                rep[b, t, 1] = row_sum(energy_terms(y))
                rep[b, t, 2] = row_sum(raw)
                out[b, t * 256:(t + 1) * 256] = oracle.synthesis(y, ONES, self.tail[b])
                self.hist[b] = fr
        return out, rep
