"""
Output leveller (include/pv_koala_batch.h, OUTPUT LEVELLER; DESIGN.md section 2, eleventh extension) without a GPU: the properties of the
rule (koala_amd/level.py), the constant between dBFS and the report's energies, the non-vacuity of the GPU suite's input on the oracle, and
the C ABI's argument checks and refusals under AddressSanitizer + UndefinedBehaviorSanitizer against the host-only engine double.
"""
import functools

import numpy as np
import pytest

import sanitized_build
from conftest import model_file
from frame_report_recipe import ReportRecipe
from koala_amd import level
from level_recipe import B, OTHER, SEQ, SETTING, over_calls, quiet_speech, vivid
from oracle import oracle

F32 = np.float32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def default_model_run(precision):
    """(E, report) of the oracle under the default model over the GPU suite's input"""
    model, x = model_file('adaptive'), quiet_speech()
    rep = ReportRecipe(model, B, precision).process(x)
    E = oracle.Oracle(model, B, oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32).process(x)
    return E, rep


def synthetic(rows=3, T=12, seed=1):
    """samples and report rows with speech-like and noise-like frames, no model involved"""
    rng = np.random.default_rng(seed)
    E = np.clip(np.rint(rng.standard_normal((rows, T * 256)) * 600), -32768, 32767).astype(np.int16)
    rep = np.zeros((rows, T, 4), F32)
    rep[..., 1] = (level.energy(-50.0) * 10.0 ** rng.uniform(-1.5, 1.0, (rows, T))).astype(F32)
    rep[..., 2] = rng.uniform(40.0, 257.0, (rows, T)).astype(F32)
    rep[..., 0] = rep[..., 1] * 2
    return E, rep


def test_off_is_identity_and_the_state_does_not_move():
    E, rep = synthetic()
    state = np.array([[5.0, 2.0], [0.0, 1.0], [7.0, 0.5]], F32)
    out, gains, new = level.apply(E, rep, None, state)
    assert same(out, E) and same(new, state) and (gains[:, 1:] == 1).all()
    out, gains, new = level.apply(E, rep, [SETTING, None, level.settings(on=False)], state)
    assert same(out[1:], E[1:]) and same(new[1:], state[1:]) and (out[0] != E[0]).any() and not same(new[0], state[0])


def test_want_is_clamped_at_both_ends():
    rep = np.zeros((2, 40, 4), F32)
    rep[..., 2] = 257.0
    rep[0, :, 1] = level.energy(-80.0)  # far below the target: the boost ends at max_boost
    rep[1, :, 1] = level.energy(0.0)    # far above: the cut ends at max_cut
    s = level.settings(floor_dbfs=-100.0, slew_ms=0.0)
    start, end, spoke, state = level.track(rep, s)
    assert spoke.all() and (end[0] == F32(s.max_boost)).all() and (end[1] == F32(s.max_cut)).all()
    slow = level.settings(floor_dbfs=-100.0)
    _, end, _, _ = level.track(rep, slow)
    assert (np.diff(end[0]) > 0).all() and end[0, -1] < slow.max_boost and (np.diff(end[1]) < 0).all() and end[1, -1] > slow.max_cut


def test_noise_frames_do_not_move_the_level():
    E, rep = synthetic()
    rep[:, 4:, 2] = 10.0  # the network gates everything from frame 4 on
    _, _, spoke, state = level.track(rep, SETTING)
    _, _, _, at4 = level.track(rep[:, :4], SETTING)
    assert not spoke[:, 4:].any() and same(state[:, 0], at4[:, 0])
    rep[..., 2] = 257.0
    rep[..., 1] = level.energy(-70.0)  # passed, and below the floor
    _, end, spoke, state = level.track(rep, SETTING)
    assert not spoke.any() and (end == 1).all() and same(state, level.fresh(3))


def test_any_cut_into_calls_gives_the_same_samples():
    E, rep = synthetic(T=9)
    whole, gains, state = over_calls(E, rep, [SETTING, OTHER, SETTING])
    for seq in ((3, 2, 1, 3), (1,) * 9, (4, 5), (8, 1)):
        out, g, st = over_calls(E, rep, [SETTING, OTHER, SETTING], seq)
        assert same(out, whole) and same(g, gains) and same(st, state)
    # continuity: the ramp of a frame begins with the gain the last one ended with
    start, end, _, _ = level.track(rep, SETTING)
    assert same(start[:, 1:], end[:, :-1]) and (start[:, 0] == 1).all()


def test_reset_and_hold():
    E, rep = synthetic(T=6)
    reset = np.zeros((3, 6), np.uint8)
    reset[1, 3] = 1
    out, gains, state = level.apply(E, rep, SETTING, None, reset)
    fresh, g2, st2 = level.apply(E[:, 3 * 256:], rep[:, 3:], SETTING)
    assert same(out[1, 3 * 256:], fresh[1]) and same(state[1], st2[1])  # stream 1 is fresh before its frame 3: the ramp starts from 1
    plain, _, pstate = level.apply(E, rep, SETTING)
    assert same(out[0], plain[0]) and same(out[2], plain[2]) and same(out[1, :3 * 256], plain[1, :3 * 256]) and same(state[[0, 2]], pstate[[0, 2]])
    before = np.array([[9.0, 3.0], [4.0, 2.0], [0.0, 1.0]], F32)
    held, gains, state = level.apply(E, rep, SETTING, before, hold=np.array([0, 1, 0]))
    assert same(state[1], before[1]) and same(held[1], E[1]) and not same(state[0], before[0])
    off_reset, _, st = level.apply(E, rep, [SETTING, None, SETTING], before, reset)
    assert same(st[1], before[1]) and same(off_reset[1], E[1])  # a stream that is off: untouched, reset flag or not


def test_saturation_is_the_only_limiter():
    E = np.full((1, 256), 30000, np.int16)
    E[0, ::2] = -30000
    rep = np.zeros((1, 1, 4), F32)
    rep[..., 1], rep[..., 2] = level.energy(-60.0), 257.0
    out, gains, _ = level.apply(E, rep, level.settings(floor_dbfs=-100.0, slew_ms=0.0))
    assert gains[0, 1] > 2 and out.max() == 32767 and out.min() == -32768


def test_to_pcm_rounds_half_away_from_zero():
    a = np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.49999997, 40000.0, -40000.0], F32)
    assert level.to_pcm(a).tolist() == [1, -1, 2, -2, 3, 0, 32767, -32768]


def test_settings_checks_its_ranges():
    s = level.settings(target_dbfs=-23, max_boost_db=18, max_cut_db=12)
    assert s.on == 1 and abs(level.rms_dbfs(s.target) + 23) < 1e-5 and abs(20 * np.log10(s.max_boost) - 18) < 1e-5 and abs(20 * np.log10(s.max_cut) + 12) < 1e-5
    assert 0 < s.a_down < s.a_up < 1 and 0 < s.slew < 1 and level.coefficient(0) == 1.0
    for bad in (dict(max_boost_db=-1), dict(max_cut_db=-1), dict(theta=1.5), dict(theta=float('nan')), dict(target_dbfs=float('-inf'))):
        with pytest.raises(ValueError):
            level.settings(**bad)


def test_the_dbfs_constant():
    """a -20 dBFS sine through the oracle with the unity-mask model reports an e_out whose implied RMS is within 0.1 dB of -20"""
    n = np.arange(12 * 256)
    amp = 32768.0 * 10.0 ** (-20.0 / 20.0) * np.sqrt(2.0)  # (the RMS of a sine is its amplitude / sqrt 2)
    x = np.rint(amp * np.sin(2.0 * np.pi * 1000.0 / 16000.0 * n)).astype(np.int16)[None]
    rep = ReportRecipe(model_file('unity'), 1, 'fp32').process(x)
    db = level.rms_dbfs(rep[0, 2:, 1])  # (from the third frame on both halves of the analysis block hold the sine)
    print('implied RMS of the -20 dBFS sine, dBFS:', db)
    assert np.abs(db + 20.0).max() < 0.1
    assert abs(level.rms_dbfs(level.energy(-20.0)) + 20.0) < 1e-9


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_the_gpu_suites_input_is_not_vacuous(precision):
    """with the oracle and the default model the rule classes at least a third of the frames as speech and ends with gain >= 2 somewhere"""
    E, rep = default_model_run(precision)
    for s in (SETTING, OTHER):
        out, gains, _ = over_calls(E, rep, s, SEQ)
        _, _, spoke, _ = level.track(rep, s)
        print(precision, 'speech frames %.2f, last gains' % spoke.mean(), gains[:, -1])
        assert vivid(rep, s, gains) and (out != E).any()


def test_abi_under_sanitizers(tmp_path):
    """tests/abi_level/driver.cpp (with koala_amd/csrc/pv_level.cpp) against koala_amd/csrc/pv_api*.cpp and the engine double: a stand-alone
    program, nothing is loaded into python"""
    run = sanitized_build.run(sanitized_build.build_abi_driver('abi_level', tmp_path), model_file('random', 1234), timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
