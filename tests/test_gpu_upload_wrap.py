"""
Every table a call sends to the device (koala_amd/csrc/kns_engine.h, Engine::Upload), with more calls in flight than its ring has slots,
on a real MI355X.

Each case issues one sequence of nine calls -- more than two full turns of a four-slot ring -- on two fresh handles of the same model:
once back to back on device pointers, every call with its own input, output and report buffers and one synchronize() at the end, and once
with a synchronize() behind every call.  Routes and kernels are the same both ways, so every output sample, every report row, the frames
a packet call reports and the stream records exported at the end must agree bit for bit: a slot rewritten while the copy that reads it is
still in flight, or a copy on the wrong stream, shows as a difference.  No numpy rule here: the per-feature suites hold the kernels to theirs.

17 streams (two m-tiles, the second ragged), 3 frames per call on a handle of max_frames 4, fp32 and bf16.  A held stream's rows of
`enhanced` and of the report are unspecified by contract and are left out; a handle at 44 100 Hz has no stream records.
"""
import numpy as np
import pytest

import gpu_kit
from band_profile_recipe import GAINS, profiles
from gpu_kit import flen, same
from koala_amd import level
from koala_amd.packets import inner_samples
from level_recipe import OTHER, SETTING
from limiter_recipe import setting as limit_at

pytestmark = pytest.mark.gpu

B, T, TMAX, CALLS = 17, 3, 4, 9
N = 300  # max_samples of the packet handles
BOOST = level.settings(target_dbfs=-3.0, max_boost_db=30.0, attack_ms=0.0, slew_ms=0.0, theta=0.0, floor_dbfs=-200.0)
PRECISIONS = ['fp32', 'bf16']


def resets(i):
    """[B, T] of call i, another one every call.  Every third call only frame 0 is set: the mask goes through the reset table's ring to the
    frame-0 mask.  Else a stream restarts at frame 1 or 2 -- the reset table -- and another one at frame 0."""
    m = np.zeros((B, T), np.uint8)
    if i % 3 == 2:
        m[[(5 * i) % B, (5 * i + 9) % B], 0] = 1
    else:
        m[(7 * i + 1) % B, 1 + i % 2] = 1
        m[(3 * i + 16) % B, 0] = 1
    return m


def holds(i):
    h = np.zeros(B, np.uint8)
    h[[i % B, (i + 8) % B]] = 1
    return h


def frame_run(model, precision, sync, rate=16000, configure=None, reset=resets, hold=None, states=()):
    """nine calls on a fresh handle -> {name: array}, the unspecified rows zeroed"""
    import torch
    F = flen(rate)
    kb = gpu_kit.batch(model, B, TMAX, precision, sample_rate=rate)
    x = gpu_kit.streams(B, CALLS * T * F, seed=5)
    xin = [torch.from_numpy(np.ascontiguousarray(x[:, i * T * F:(i + 1) * T * F])).cuda() for i in range(CALLS)]
    out = [torch.zeros(B, T * F, dtype=torch.int16, device='cuda') for _ in range(CALLS)]
    rep = [torch.full((B, T, 4), -1.0, dtype=torch.float32, device='cuda') for _ in range(CALLS)]
    torch.cuda.synchronize()
    for i in range(CALLS):
        if configure:
            configure(kb, i)
        kb.process_device_call(T, xin[i].data_ptr(), out[i].data_ptr(), rep[i].data_ptr(), reset=reset(i) if reset else None,
                               hold=hold(i) if hold else None)
        if sync:
            kb.synchronize()
    kb.synchronize()
    got = {'records': kb.export_state()}
    for name in states:
        got[name] = getattr(kb, name)()
    kb.delete()
    y = np.stack([o.cpu().numpy() for o in out], axis=1)  # [B, CALLS, T F]
    r = np.stack([q.cpu().numpy() for q in rep], axis=1)
    for i in range(CALLS if hold else 0):
        y[hold(i) != 0, i] = 0
        r[hold(i) != 0, i] = 0
    got['out'], got['report'] = y, r
    return got


def agree(run):
    a, b = run(False), run(True)
    assert a.keys() == b.keys()
    for name in a:
        assert same(a[name], b[name]), name
    return a


# ---------------------------------------------------------------------------------------------------- (a) settings, reset table, frame-0 mask

def gains_and_profile(kb, i):
    kb.set_min_gain(GAINS[(np.arange(B) + i) % len(GAINS)])
    kb.set_band_profile(*profiles(B, seed=i))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_settings_and_reset_tables(random_model, precision):
    a = agree(lambda sync: frame_run(random_model, precision, sync, configure=gains_and_profile))
    assert (a['report'] != -1).all() and a['out'].any()


# ---------------------------------------------------------------------------------------------------- (b) leveller and limiter, control rows

def level_and_limit(kb, i):
    kb.set_level([(SETTING, OTHER, BOOST)[(b + i) % 3] for b in range(B)])
    kb.set_limiter([limit_at(400.0 + 300.0 * ((3 * i + b) % 7)) for b in range(B)])


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('control', ['resets', 'hold'])
def test_output_stage_tables_and_control_rows(random_model, precision, control):
    kw = dict(reset=None, hold=holds) if control == 'hold' else {}
    a = agree(lambda sync: frame_run(random_model, precision, sync, configure=level_and_limit, states=('level_state', 'limiter_state'), **kw))
    peaks = np.abs(a['out'].astype(np.int64)).max(axis=2)  # [B, CALLS]: every stream under the ceiling of its call
    ceilings = np.array([[400.0 + 300.0 * ((3 * i + b) % 7) for i in range(CALLS)] for b in range(B)])
    print('peaks', peaks.max(axis=1), 'gains', a['level_state'][:, 1], 'g', a['limiter_state'])
    assert (peaks <= ceilings).all()


# ---------------------------------------------------------------------------------------------------- (c) the rate stages' reset flags

@pytest.mark.parametrize('precision', PRECISIONS)
def test_rate_stage_reset_flags(random_model, precision):
    a = agree(lambda sync: frame_run(random_model, precision, sync, rate=48000))
    assert (a['report'] != -1).all() and a['out'].any()


# ---------------------------------------------------------------------------------------------------- (d), (e) packet and fractional tables

def packet_run(model, precision, sync, rate):
    import torch
    kb = gpu_kit.batch(model, B, 1, precision, sample_rate=rate, packet_samples=N)
    R = (N // kb.frame_length if kb.frame_length else int(inner_samples(N, rate)) // 256) + 1
    x = gpu_kit.streams(B, CALLS * N, seed=6)
    rng = np.random.default_rng(rate)
    counts = [(rng.integers(0, N + 1, B) * (rng.random(B) > 0.15)).astype(np.int32) for _ in range(CALLS)]
    restart = [(rng.random(B) < 0.2).astype(np.uint8) for _ in range(CALLS)]
    for i in range(CALLS):
        restart[i][(4 * i) % B] = 1  # (every call carries a restart)
    xin = [torch.from_numpy(np.ascontiguousarray(x[:, i * N:(i + 1) * N])).cuda() for i in range(CALLS)]
    out = [torch.full((B, N), 7, dtype=torch.int16, device='cuda') for _ in range(CALLS)]  # (nothing past counts[b] is written)
    rep = [torch.full((B, R, 4), -1.0, dtype=torch.float32, device='cuda') for _ in range(CALLS)]
    torch.cuda.synchronize()
    frames = []
    for i in range(CALLS):
        frames.append(kb.process_device_packets(N, counts[i], xin[i].data_ptr(), out[i].data_ptr(), restart[i], rep[i].data_ptr(), R))
        if sync:
            kb.synchronize()
    kb.synchronize()
    got = {'frames': np.stack(frames), 'out': np.stack([o.cpu().numpy() for o in out]), 'report': np.stack([q.cpu().numpy() for q in rep])}
    if kb.state_size:
        got['records'] = kb.export_state()
    kb.delete()
    return got


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('rate', [16000, 44100])
def test_packet_call_tables(random_model, precision, rate):
    a = agree(lambda sync: packet_run(random_model, precision, sync, rate))
    assert a['frames'].any() and (a['out'] != 7).any()


# ---------------------------------------------------------------------------------------------------- (f) the record table

@pytest.mark.parametrize('precision', PRECISIONS)
def test_record_tables(random_model, precision):
    kb = gpu_kit.batch(random_model, B, TMAX, precision)
    kb.process(gpu_kit.streams(B, T * 256, seed=7))
    full = kb.export_state()
    rng = np.random.default_rng(8)
    for i in range(CALLS):
        listed = rng.permutation(B)[:1 + (5 * i) % B]  # nine lists of 1 .. 17 streams, no two alike
        assert same(kb.export_state(listed), full[listed]), i
    kb.delete()
