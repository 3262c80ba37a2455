"""
tests/segment_recipe.py pinned on the CPU: fed the oracle's own masks (`Oracle.process_with_mask`) it is tests/comfort_recipe.py's
ComfortRecipe -- `process` and `process_resets` -- sample for sample, e_out bit for bit, and counter for counter, in the fp32 and in the bf16
oracle mode.  16 streams x 7 frames a call, three calls (the last one with per-frame resets), the mixed settings of the GPU suite with every
fifth stream off.  Nothing here needs a GPU.
"""
import numpy as np
import pytest

from comfort_recipe import ComfortRecipe
from conftest import model_file, synth_streams
from frame_report_recipe import ReportRecipe
from oracle import oracle
from segment_recipe import SegmentRecipe, mixed, round_bf16

N, T = 16, 7
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def frames(x, t0, t1):
    return np.ascontiguousarray(x[:, t0 * 256:t1 * 256])


def resets():
    """[N, T]: frame 0, the last frame, two adjacent frames, an off stream (4)"""
    rs = np.zeros((N, T), np.uint8)
    rs[0, 0] = rs[8, T - 1] = rs[6, 2] = rs[6, 3] = rs[4, 1] = rs[15, 5] = 1
    return rs


def oracle_masks(o, x, reset=None):
    """the masks [T, N, 257] of an oracle of its own that is given the same frames and resets"""
    if reset is None:
        return o.process_with_mask(x)[1]
    out = []
    for t in range(x.shape[1] // 256):
        if reset[:, t].any():
            o.reset(reset[:, t])
        out.append(o.process_with_mask(frames(x, t, t + 1))[1])
    return np.concatenate(out)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('arm', ['profile', 'comfort'])
def test_fed_the_oracles_masks_it_is_the_comfort_recipe(precision, arm):
    model = model_file('random')
    lo, hi, g, amp, seeds, on = mixed(N)
    if arm == 'profile':
        on = np.zeros(N, bool)
    x = synth_streams(N, 3 * T, 71)
    o = oracle.Oracle(model, N, oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32)
    ref, rec = ComfortRecipe(model, N, precision), SegmentRecipe(model, N)
    rs = resets()
    for n in range(3):
        xn, r = frames(x, n * T, (n + 1) * T), rs if n == 2 else None
        m = oracle_masks(o, xn, r)
        want = ref.process(xn, g, lo, hi, amp, seeds, on) if r is None else ref.process_resets(xn, g, r, lo, hi, amp, seeds, on)
        got, rep = rec.process(xn, m, g, lo, hi, amp, seeds, on, reset=r)
        assert np.array_equal(got, want), (n, int((got != want).sum()))
        assert np.array_equal(bits(rep[:, :, 1]), bits(ref.e_out)), n
        assert np.array_equal(rec.count, ref.count), n
        assert not rep[:, :, 3].any() and (rep[:, :, 0] > 0).all()
    assert (rec.count[on] > 0).all() and not rec.count[~on].any()
    assert arm == 'profile' or rec.count[0] == T and rec.count[8] == 1 and rec.count[1] == 3 * T  # (reset at frame 0, at the last frame, never)


def test_the_rows_it_adds_are_the_frame_report_recipes():
    """e_in and mask_sum against tests/frame_report_recipe.py's ReportRecipe, which needs neither a profile nor a fill for them; with no
    profile and no fill e_out is that recipe's too"""
    model = model_file('random')
    _, _, g, _, _, _ = mixed(N)
    x = synth_streams(N, T, 72)
    want = ReportRecipe(model, N, 'fp32').process(x, g)
    _, m = oracle.Oracle(model, N).process_with_mask(x)
    _, rep = SegmentRecipe(model, N).process(x, m, g)
    assert np.array_equal(bits(rep), bits(want))


def test_round_bf16_rounds_to_nearest_even():
    a = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 0.0, 3.0e38], F32)  # 1 + 2^-8 is a tie (down to even), 1 + 3 * 2^-8 a tie (up)
    assert np.array_equal(round_bf16(a), np.array([1.0, 1.0, 1.015625, -1.0, 0.0, round_bf16(a)[5]], F32))
    assert not (round_bf16(a).view(np.uint32) & 0xffff).any()
