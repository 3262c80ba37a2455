"""
What the GPU cases of batch handles at 8, 12, 24, 32 and 48 kHz share (tests/test_gpu_sample_rate.py for 8, 32 and 48 kHz,
tests/test_gpu_rational_rate.py for 12 and 24 kHz; tools/sample_rate_figures.py reads the same inputs): handles, inputs, the recipe's expected
samples and the bar they are held to.  Not a test module.

The bar.  fp32: ==.  bf16: the largest distance is at most ceil(BF16_TOL * S) + 1 LSB, S = the out-stage's largest sum of |tap| over an
output phase (BF16_TOL LSB of the engine spread by the out-stage, one more for its rounding), and the share of samples further than 1 LSB
from the recipe is at most 4 x the share by which the jittered bf16 oracle (oracle.set_jitter: a second valid bf16 implementation) misses
the plain one through the same recipe on the same inputs -- the margin tools/frame_report_bars.py established.
"""
import functools
import math

import numpy as np

import gpu_kit
import sample_rate_recipe as srr
from conftest import model_file, synth_streams
from gpu_kit import BF16_TOL, frames
from oracle import oracle

NCLS = 6  # distinct streams; a batch repeats them (cls[b]) so that the CPU side stays small

# The call schedule and the handle's max_frames are part of a case, so every rate keeps the ones its cases were written with: 8, 32 and
# 48 kHz a 16-frame call among the mixed lengths, 12 and 24 kHz calls of 1, 2 and 5 frames.  max_frames is the longest call.
CALLS = {8000: (1, 3, 16, 2), 12000: (1, 2, 5, 5, 2, 1), 24000: (1, 2, 5, 5, 2, 1), 32000: (1, 3, 16, 2), 48000: (1, 3, 16, 2)}
TMAX = {rate: max(calls) for rate, calls in CALLS.items()}


def batch(model, B, T, precision, rate, **kw):
    return gpu_kit.batch(model, B, T, precision, sample_rate=rate, **kw)


def classes(B):
    return np.arange(B) % NCLS


def signal(rate, T, seed):
    """int16 [NCLS, T * frame_length]: the suite's synthetic streams, taken as samples at `rate`"""
    fl = srr.frame_length(rate)
    return np.ascontiguousarray(synth_streams(NCLS, T * fl // 256 + 1, seed=seed)[:, :T * fl])


def cut(x, rate, t0, t1):
    return frames(x, t0, t1, srr.frame_length(rate))


@functools.lru_cache(maxsize=None)
def expected(kind, precision, rate, jitter=0):
    """the recipe over the rate's calls on the NCLS class streams -> (input, [enhanced per call]); kind 'unity': the inner engine as a
    pure delay"""
    calls = CALLS[rate]
    x = signal(rate, sum(calls), seed=11)
    oracle.set_jitter(jitter)
    try:
        rec = srr.Recipe(None if kind == 'unity' else model_file('random', 1234), NCLS, precision, rate)
        out, t0 = [], 0
        for T in calls:
            out.append(rec.process(cut(x, rate, t0, t0 + T)))
            t0 += T
    finally:
        oracle.set_jitter(0)
    return x, out


def bf16_bound(rate):
    """LSB: BF16_TOL of the engine spread by the out-stage, one more for its rounding"""
    return math.ceil(BF16_TOL * srr.Recipe(None, 1, 'fp32', rate).s_out.abs_tap_sum()) + 1


def check(got, want, precision, rate, what, jitter_want=None):
    """prints the figures before it asserts"""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((d > 1).mean())
    print('%s %s %d Hz: max distance %d LSB, share > 1 LSB %.3e' % (what, precision, rate, int(d.max()), share), end='')
    if precision == 'fp32' or jitter_want is None:
        print()
        assert np.array_equal(got, want), what
        return
    bound = bf16_bound(rate)
    jshare = float((np.abs(jitter_want.astype(np.int32) - want.astype(np.int32)) > 1).mean())
    print(', bound %d LSB; jittered oracle misses %.3e -> allowed %.3e' % (bound, jshare, 4 * jshare))
    assert d.max() <= bound, (what, int(d.max()), bound)
    assert share <= 4 * jshare, (what, share, jshare)
