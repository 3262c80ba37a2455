"""
The per-stream settings' path on a real MI355X ("Per-stream settings"): every table's ring slots reused, and one set of
control rows under all three output stages.

Eight calls of three frames on a handle of 17 streams (one full 16-row tile and one row: the tables' padding rows 17 .. 31 matter) and of 1.
Before every call all five settings -- minimum gain, band profile, leveller, limiter, comfort noise -- change on some streams, so eight
revisions take every four-slot ring around twice; calls 3 and 6 hold two streams, calls 4 and 7 restart one stream at frame 0 and one at frame
2; the leveller, the limiter and comfort noise are on throughout on different subsets, the last stream has everything on.

No numpy rule here (the per-feature suites hold the kernels to theirs): the same sequence issued back to back and issued with a
synchronize() behind every setter and every call must agree bit for bit -- a slot rewritten while its copy is in flight, or a control row
that a later launch no longer finds, shows as a difference -- and so must the sequence with streams 0 and 16 swapped, rows swapped back: a
table row or control row indexed against the wrong stride or padding does not survive the move.  A held stream's rows of `enhanced` and of
the report are unspecified by contract and are left out of the comparisons.
"""
import functools

import numpy as np
import pytest

import gpu_kit
from band_profile_recipe import GAINS, profiles
from comfort_recipe import curves
from conftest import load_wav
from gpu_kit import DEV_LIB, same
from koala_amd import level
from level_recipe import OTHER, QUIET_DBFS, SETTING
from limiter_recipe import setting as limit_at

pytestmark = pytest.mark.gpu

T, CALLS = 3, 8
LOUD = 4  # (test_gpu_limiter.py's combined test: the recipe's -45 dBFS, four times as loud)
BOOST = level.settings(target_dbfs=-3.0, max_boost_db=30.0, attack_ms=0.0, slew_ms=0.0, theta=0.0, floor_dbfs=-200.0)
HOLD_CALLS, RESET_CALLS = (3, 6), (4, 7)


@functools.lru_cache(maxsize=None)
def _input(B):
    """int16 [B, CALLS * T * 256]: the noise fixture, every row its own stretch at QUIET_DBFS, then LOUD times that"""
    pcm = load_wav('noise.wav').astype(np.float64)
    n = CALLS * T * 256
    step = (len(pcm) - n) // max(B, 2)
    assert step > 0
    out = np.empty((B, n), np.int16)
    for b in range(B):
        x = pcm[b * step:b * step + n]
        want = 32768.0 * 10.0 ** (QUIET_DBFS / 20.0)
        out[b] = np.clip(np.rint(x * (want / max(np.sqrt(np.mean(x * x)), 1.0))) * LOUD, -32768, 32767).astype(np.int16)
    out.setflags(write=False)
    return out


def levels(B):
    return [b for b in range(B) if b % 3 == 0 or b == B - 1]


def limits(B):
    return [b for b in range(B) if b % 2 == 1 or b == B - 1]


def fills(B):
    return [b for b in range(B) if b % 4 < 2 or b == B - 1]


def ceiling(i, b):
    return float(48 + 8 * ((3 * i + b) % 7))  # (low: what the gate lets through of the noise must reach it)


def configure(kb, B, i, at, sync):
    """the changes in front of call i, on the streams {b: (b + i) % 3 == 0} and the last one; at[b]: the slot of stream b"""
    chosen = [b for b in range(B) if (b + i) % 3 == 0 or b == B - 1]
    slots = [at[b] for b in chosen]
    lo, hi = profiles(B, seed=i)
    amp = curves(B, seed=i)
    steps = [
        lambda: kb.set_min_gain([GAINS[(b + i) % len(GAINS)] for b in chosen], streams=slots),
        lambda: kb.set_band_profile(lo[chosen], hi[chosen], streams=slots),
        lambda: kb.set_level([(SETTING, OTHER, BOOST)[(b + i) % 3] if b in levels(B) else None for b in chosen], streams=slots),
        lambda: kb.set_limiter([limit_at(ceiling(i, b)) if b in limits(B) else None for b in chosen], streams=slots),
    ]
    on = [b for b in chosen if b in fills(B)]
    if on:
        steps.append(lambda: kb.set_comfort_noise(amp[on], seed=[7 * b + i for b in on], streams=[at[b] for b in on]))
    for step in steps:
        step()
        if sync:
            kb.synchronize()


def controls(B, i, at):
    """(reset, hold) of call i in the handle's slots"""
    two = sorted({1 % B, B - 1})
    if i in HOLD_CALLS:
        hold = np.zeros(B, np.uint8)
        hold[[at[b] for b in two]] = 1
        return None, hold
    if i in RESET_CALLS:
        reset = np.zeros((B, T), np.uint8)
        reset[at[two[0]], 0] = 1
        reset[at[two[-1]], 2] = 1
        return reset, None
    return None, None


def run(model, B, precision, sync, at=None):
    """the scenario on a fresh handle -> (out [B, CALLS T 256], report [B, CALLS T, 4], the three states), all in stream order"""
    import torch
    at = list(range(B)) if at is None else at
    x = _input(B)
    kb = gpu_kit.batch(model, B, T, precision, lib=DEV_LIB)
    # the stages are on from the first call: every stream of a stage gets a setting, then the calls' changes follow
    kb.set_level(BOOST, streams=[at[b] for b in levels(B)])
    kb.set_limiter([limit_at(ceiling(0, b)) for b in limits(B)], streams=[at[b] for b in limits(B)])
    kb.set_comfort_noise(curves(B, seed=99)[fills(B)], seed=[b + 1 for b in fills(B)], streams=[at[b] for b in fills(B)])
    slot_rows = np.argsort(at)  # slot s carries stream slot_rows[s]
    xin = [torch.from_numpy(np.ascontiguousarray(x[slot_rows, i * T * 256:(i + 1) * T * 256])).cuda() for i in range(CALLS)]
    out = [torch.zeros(B, T * 256, dtype=torch.int16, device='cuda') for _ in range(CALLS)]
    rep = [torch.zeros(B, T, 4, dtype=torch.float32, device='cuda') for _ in range(CALLS)]
    torch.cuda.synchronize()
    for i in range(CALLS):
        configure(kb, B, i, at, sync)
        reset, hold = controls(B, i, at)
        kb.process_device_call(T, xin[i].data_ptr(), out[i].data_ptr(), rep[i].data_ptr(), reset=reset, hold=hold)
        if sync:
            kb.synchronize()
    kb.synchronize()
    states = kb.level_state()[at], kb.limiter_state()[at], kb.comfort_state()[at]
    kb.delete()
    y = np.concatenate([o.cpu().numpy() for o in out], axis=1)[at]
    r = np.concatenate([q.cpu().numpy() for q in rep], axis=1)[at]
    return y, r, states


def specified(B):
    """[B, CALLS]: the stream's rows of the call are specified (it was not held)"""
    ok = np.ones((B, CALLS), bool)
    for i in HOLD_CALLS:
        ok[sorted({1 % B, B - 1}), i] = False
    return ok


def agree(a, b, B):
    ok = specified(B)
    ya, yb = a[0].reshape(B, CALLS, -1), b[0].reshape(B, CALLS, -1)
    ra, rb = a[1].reshape(B, CALLS, -1), b[1].reshape(B, CALLS, -1)
    return same(ya[ok], yb[ok]) and same(ra[ok], rb[ok]) and all(same(p, q) for p, q in zip(a[2], b[2]))


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('B', [17, 1])
def test_back_to_back_is_step_by_step(gate_model, precision, B):
    a = run(gate_model, B, precision, sync=False)
    b = run(gate_model, B, precision, sync=True)
    y, _, (lstate, _, counters) = a
    # the stages demonstrably act: a limited stream's samples reach its ceiling in some call, a levelling stream's gain has left 1, a filling
    # stream's frames were counted
    peaks = np.abs(y.astype(np.int64)).reshape(B, CALLS, -1).max(axis=2)
    last = {}
    hit = False
    for i in range(CALLS):
        for s in limits(B):
            if (s + i) % 3 == 0 or s == B - 1 or i == 0:
                last[s] = ceiling(i, s)
            assert peaks[s, i] <= last[s] or not specified(B)[s, i]
            hit = hit or (peaks[s, i] == last[s] and specified(B)[s, i])
    print('peaks of the limited streams', peaks[limits(B)].max(axis=1), 'gains', lstate[levels(B), 1], 'counters', counters[fills(B)])
    assert hit and (lstate[levels(B), 1] != 1).any() and (counters[fills(B)] > 0).all()
    assert agree(a, b, B)
    if B > 1:  # streams 0 and 16 change places: settings, input rows, `hold` rows and `reset` rows
        at = list(range(B))
        at[0], at[B - 1] = B - 1, 0
        assert agree(a, run(gate_model, B, precision, sync=False, at=at), B)
