"""
What the output leveller's tests share (tests/test_level.py on the CPU, tests/test_gpu_level.py on the GPU): the input, the settings, the
call sequence and the rule applied over a sequence of calls.  The rule itself is koala_amd/level.py; not a test module.
"""
import numpy as np

from conftest import load_wav
from koala_amd import level

F32 = np.float32
B, TMAX, SEQ = 4, 3, (3, 2, 1, 3)
FRAMES = sum(SEQ)
QUIET_DBFS = -45.0
# the handle's settings in the tests: the defaults in physical units, and another target for the streams that are to differ
# (the default model is a spectral gate: its mean mask over all 257 bins stays near 0.3 on speech, and what it lets through of a -45 dBFS
# talker reads about -53 dBFS, so the speech gate's two thresholds sit below both)
SETTING = level.settings(theta=0.25, floor_dbfs=-56.0)
OTHER = level.settings(target_dbfs=-30.0, max_boost_db=12.0, slew_ms=50.0, theta=0.25, floor_dbfs=-56.0)


def quiet_speech(rows=B, frames=FRAMES, seed=7):
    """int16 [rows, frames * 256]: the speech fixture from where its first talker is under way, every row its own stretch, scaled to about
    QUIET_DBFS over the stretch, plus white noise 20 dB below that -- talkers that arrive far too quiet"""
    pcm = load_wav('test.wav').astype(np.float64)
    n = frames * 256
    loud = np.flatnonzero(np.abs(pcm) > 0.1 * np.abs(pcm).max())
    first = int(loud[0])
    rng = np.random.default_rng(seed)
    out = np.empty((rows, n), np.int16)
    for b in range(rows):
        at = first + b * 8000  # (half a second apart)
        assert at + n <= len(pcm)
        x = pcm[at:at + n]
        rms = np.sqrt(np.mean(x * x))
        want = 32768.0 * 10.0 ** (QUIET_DBFS / 20.0)
        y = x * (want / max(rms, 1.0)) + rng.standard_normal(n) * want * 0.1
        out[b] = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
    return out


def over_calls(E, report, setting, seq=None, state=None, resets=None, holds=None):
    """level.apply over consecutive calls of seq[i] frames (None: one call): E int16 [rows, T * 256] and report [rows, T, 4] of the whole
    stretch; setting: as level.apply's, or a list with one such per call; resets / holds: per call or None
    -> (out, gains of every frame [rows, T], the state behind the last call)"""
    T = E.shape[1] // 256
    seq = (T,) if seq is None else seq
    outs, gains, t0 = [], [], 0
    for i, n in enumerate(seq):
        s = setting[i] if isinstance(setting, dict) else setting
        o, g, state = level.apply(E[:, t0 * 256:(t0 + n) * 256], report[:, t0:t0 + n], s, state,
                                  None if resets is None else resets[i], None if holds is None else holds[i])
        outs.append(o)
        gains.append(g[:, 1:])
        t0 += n
    return np.concatenate(outs, axis=1), np.concatenate(gains, axis=1), state


def vivid(report, setting, gains):
    """the non-vacuity bar: the rule classes at least a third of the frames as speech and some stream ends at twice its level or more"""
    _, _, spoke, _ = level.track(report, setting)
    return spoke.mean() >= 1.0 / 3.0 and gains[:, -1].max() >= 2.0
