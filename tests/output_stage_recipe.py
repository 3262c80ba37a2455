"""
What the output stages' pattern tests share (tests/test_output_stage_patterns.py on the CPU, tests/test_gpu_output_stage_patterns.py on the
GPU): samples chosen one by one for limit_kernel, level_track_kernel and level_apply_kernel.  Under the unity-mask model a 16 kHz handle
returns its input one frame late, bit for bit, so the samples E the output kernels see are gpu_kit.delayed(x) for any x: every row below
is written for one path of a kernel.  The rules are koala_amd/limiter.py and koala_amd/level.py; not a test module.

Frames are the input's: the output stages see frame t of a row as their frame t + 1.
"""
import numpy as np

from koala_amd import level, limiter

F32 = np.float32
FRAME = 256
BASE = 100     # what a row holds where nothing else is said
PEAK = 30000
PEAK_AT = (0, 1, 2, 3, 4, 5, 7, 8, 16, 63, 64, 127, 128, 252, 255)
SEQ = (3, 2, 1, 2)  # the frames of the calls a stretch of T = 8 frames is cut into: a release crosses every kind of boundary
T = sum(SEQ)
TMAX = max(SEQ)


def rows(T=T):
    """-> (int16 [R, T * 256], names).  T >= 8."""
    assert T >= 8
    n = T * FRAME
    out, names = [], []

    def row(name, fill=BASE):
        out.append(np.full(n, fill, np.int64))
        names.append(name)
        return out[-1]

    # one peak at position p of frame 1 and a release that spans the frame: each shuffle distance of the envelope on its own, and the
    # lane boundaries of its levels 0 and 1 (p = 3, 4: the last sample of lane 0, the first of lane 1)
    for p in PEAK_AT:
        row('peak@%d' % p)[FRAME + p] = PEAK
    # a far, deep peak that must win over a near, shallow one
    x = row('far_deep')
    x[FRAME + 10], x[FRAME + 140] = 32767, 9000
    row('dc-', -32768)  # |v| = 32768 > c = 32767
    row('nyquist')[:] = np.where(np.arange(n) % 2 == 0, 32767, -32768)
    # tests/test_limiter.py::test_two_frames_by_hand with 3000 for 1000: G = (897 + n) / 1024 behind the peak, products on exact halves
    x = row('tie')
    x[FRAME - 1], x[FRAME:] = 16000, 3000
    # tests/test_limiter.py's noise: full range, with stretches of quiet in which the gain comes all the way back
    x = row('noise')
    x[:] = np.random.default_rng(11).integers(-32768, 32768, n)
    x[256:700] //= 64
    x[1500:1900] //= 300
    # the only sample over the ceiling of a frame in the wave's first lane, and in its last
    row('lane0')[2 * FRAME] = PEAK
    row('lane63')[2 * FRAME + 255] = PEAK
    # a deep peak, then whole frames below the ceiling but large: no sample over, g < 1, and a gain whose last bit shows in the samples
    x = row('tail')
    x[FRAME + 200], x[2 * FRAME:] = -32768, 13000
    # silence for two frames, then a 1 kHz sine at full scale: the leveller's lvl == 0 branch, then its cut
    x = row('ramp', 0)
    k = np.arange(n - 2 * FRAME)
    x[2 * FRAME:] = np.rint(32767.0 * np.sin(2.0 * np.pi * 1000.0 * k / 16000.0))
    row('flat')  # with c >= 100 nothing of this row is ever stored
    x = np.array(out)
    assert x.min() >= -32768 and x.max() <= 32767
    return x.astype(np.int16), names


DEFAULT_RELEASE = limiter.settings().release  # fl(1 / 800): the library's default, 50 ms
# (c, delta) of the limiter
SETTINGS = [(14000.0, 1.0 / 1024.0), (14000.0, DEFAULT_RELEASE), (1.0, DEFAULT_RELEASE), (32767.0, DEFAULT_RELEASE),
            (1000.5, float(F32(1.0 / 3.0))), (14000.0, 1.0), (14000.0, 2.0 ** -30)]


def setting(c, delta):
    s = limiter.Setting(1, float(c), float(delta))
    limiter.check(s)
    return s


def grid(T=T):
    """every row under every setting as one batch: stream s * R + r carries row r under SETTINGS[s]
    -> (x int16 [B, T * 256], one limiter.Setting per stream, names); B is no multiple of 4: the limiter's last workgroup and the
    setting tables' last tile of 16 are ragged"""
    x, names = rows(T)
    R = len(names)
    xs = [x] * len(SETTINGS)
    lim = [setting(*cd) for cd in SETTINGS for _ in range(R)]
    names = ['%s/%d' % (n, s) for s in range(len(SETTINGS)) for n in names]
    if len(lim) % 4 == 0:
        xs, lim, names = xs + [x[names.index('noise/0')][None]], lim + [setting(*SETTINGS[0])], names + ['noise/0+']
    x = np.ascontiguousarray(np.concatenate(xs))
    assert x.shape[0] == len(lim) == len(names) and len(lim) % 4 and len(lim) % 16
    return x, lim, names


def stream(names, row, s=0):
    """the stream of the grid that carries `row` under SETTINGS[s]"""
    return names.index('%s/%d' % (row, s))


LEVELS = {
    # tests/test_gpu_limiter.py's BOOST: 30 dB of boost, every frame with energy classed as speech, no smoothing
    'BOOST': level.settings(target_dbfs=-3.0, max_boost_db=30.0, attack_ms=0.0, slew_ms=0.0, theta=0.0, floor_dbfs=-200.0),
    # the cut clamp, which full-scale rows reach at once
    'CUT': level.settings(target_dbfs=-23.0, max_cut_db=12.0, attack_ms=0.0, slew_ms=0.0, theta=0.0, floor_dbfs=-200.0),
    # the default smoothing, and a speech gate that only a mean mask of exactly 1 passes
    'SLOW': level.settings(theta=1.0),
}


def thirds(B):
    """BOOST, CUT, SLOW over the streams in turn: the grid has 25 rows per limiter setting, so every row meets every one of the three"""
    return [LEVELS[('BOOST', 'CUT', 'SLOW')[b % 3]] for b in range(B)]


def products(E, start, end):
    """v = float(E) * fma(n / 256, g_t - g_{t-1}, g_{t-1}), float32 like E: the leveller's product before to_pcm"""
    rows_, T_ = start.shape
    w = (np.arange(FRAME, dtype=F32) / F32(FRAME)).astype(F32)
    ramp = level.fma32(np.broadcast_to(w, (rows_, T_, FRAME)), np.broadcast_to((end - start).astype(F32)[:, :, None], (rows_, T_, FRAME)),
                       np.broadcast_to(start[:, :, None], (rows_, T_, FRAME)))
    return (np.asarray(E).reshape(rows_, T_, FRAME).astype(F32) * ramp).astype(F32).reshape(np.asarray(E).shape)


def delayed(x, n=FRAME):
    """gpu_kit.delayed, for the CPU module (which must not import the GPU kit)"""
    return np.concatenate([np.zeros((x.shape[0], n), x.dtype), x[:, :-n]], axis=1)
