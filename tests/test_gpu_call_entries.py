"""
Every entry of a frame call against the device-pointer call, with several of a call's tables in force at once: per-stream gains, a band
profile, a frame report and per-frame resets (koala_amd/csrc/kns_engine.cpp: run_call, process_host_async, process_host_pipelined and the
one-frame graph).  Each feature's own suite holds it to its recipe in some pointer modes; this one holds the entries to each other,
which differ only in how the call is cut and where its tables are put on the stream -- so samples and report are the device call's, bit
for bit, in both precisions (the routes give equal bits: test_gpu_parity.test_alternative_kernels_give_identical_pcm).

B = 20: two m-tiles, the second ragged.  KOALA_AMD_HOST_CHUNK=2 with KOALA_AMD_HOST_SCHED=2 cuts a six-frame host call into three
sub-chunks of two frames: the third one reuses the first one's staging slot.
"""
import functools

import numpy as np
import pytest

import gpu_kit
from band_profile_recipe import GAINS, profiles
from gpu_kit import DEV_LIB, frames, same, streams

pytestmark = pytest.mark.gpu

batch = functools.partial(gpu_kit.batch, lib=DEV_LIB)
call = gpu_kit.call
B, TMAX, T = 20, 8, 6
PRECISIONS = ['fp32', 'bf16']


def handle(model, precision):
    """gains (0, 0.25 and 1 among them) and a profile per stream, as tests/test_gpu_band_profile.py's mixed()"""
    kb = batch(model, B, TMAX, precision)
    kb.set_min_gain(np.resize(GAINS, B))
    kb.set_band_profile(*profiles(B, 0))
    return kb


def restarts():
    """one stream restarts at frame 0, one at frame 3 -- inside the second sub-chunk, in the ragged m-tile -- and one at frame 5"""
    reset = np.zeros((B, T), np.uint8)
    reset[[2, 17, 9], [0, 3, 5]] = 1
    return reset


def two_calls(kb, x, mode):
    """a six-frame call with resets, then one without, both with a report -> [samples, report, samples, report]"""
    got = call(kb, frames(x, 0, T), mode, report=True, reset=restarts()) + call(kb, frames(x, T, 2 * T), mode, report=True)
    kb.delete()
    return got


@functools.lru_cache(maxsize=None)
def device_calls(model, precision):
    """the reference, once per precision and left unchanged"""
    return two_calls(handle(model, precision), streams(B, 2 * T * 256, seed=71), 'device')


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('mode', ['host', 'pinned', 'async', 'offset'])
def test_six_frame_calls_are_the_device_call(random_model, monkeypatch, mode, precision):
    pytest.importorskip('torch')
    monkeypatch.setenv('KOALA_AMD_HOST_CHUNK', '2')
    monkeypatch.setenv('KOALA_AMD_HOST_SCHED', '2')
    want = device_calls(random_model, precision)
    got = two_calls(handle(random_model, precision), streams(B, 2 * T * 256, seed=71), mode)
    for i, what in enumerate(['samples, resets', 'report, resets', 'samples, next call', 'report, next call']):
        assert same(got[i], want[i]), (what, int((np.asarray(got[i]) != np.asarray(want[i])).sum()))
    assert want[1][:, :, 0].all() and not same(want[0], want[2])  # (a report was written, and the calls are not silence)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_frame_calls_are_the_device_call(random_model, monkeypatch, precision):
    """graph capture, then replay, under the profile; then the profile goes back to neutral and only the gains remain: a second graph
    set of the same handle, captured and replayed"""
    pytest.importorskip('torch')
    monkeypatch.setenv('KOALA_AMD_HOST_CHUNK', '2')
    x = streams(B, 4 * 256, seed=72)
    kb, twin = handle(random_model, precision), handle(random_model, precision)
    for t in range(4):
        if t == 2:
            kb.set_band_profile()
            twin.set_band_profile()
        (y, rep), (wy, wrep) = call(kb, frames(x, t, t + 1), 'host', report=True), call(twin, frames(x, t, t + 1), 'device', report=True)
        assert same(y, wy) and same(rep, wrep), (t, int((y != wy).sum()))
        assert wrep[:, :, 0].all()
    kb.delete()
    twin.delete()
