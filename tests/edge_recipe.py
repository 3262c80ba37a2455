"""
Edge inputs for the engine's own kernels (kns_stft.hip, kns_stft_synthesis.inc, kns_gemm.hip, kns_gru.hip, kns_gruq.hip), the fixed-mask
models that make the synthesis kernel's clamp reachable together with a mask that is not 1 everywhere, and which (model, input) pairs the
bf16 engine is held to the suite's bars on.  Shared by tests/test_edge_inputs.py (CPU) and tests/test_gpu_edge_inputs.py; not a test module.

Why a fixed mask.  On the random-weight models two valid bf16 implementations (the plain and the jittered bf16 oracle, oracle.set_jitter)
differ by 13-23 LSB on loud edge inputs: no bar that holds there could find a defect.  A zero network whose last head bias is +-30 per bin has a
mask of exactly 1.0 or about 1e-13 -- a brick-wall filter -- in every precision and under every jitter, so the engine can be compared with the
oracle by the suite's existing bars, and its output still leaves the int16 range (a high-pass on full-range noise, a low-pass on a square
wave: Gibbs overshoot).
"""
import os

import numpy as np

from conftest import load_wav, model_file
from koala_amd import params

# ---------------------------------------------------------------------------------------------------- inputs

NAMES = ['dc+', 'dc-', 'nyquist_hi', 'nyquist_lo', 'noise', 'impulse', 'step', 'dither', 'silence', 'silence_speech', 'speech_x8', 'square']
ROWS = len(NAMES)
SILENCE = NAMES.index('silence')
SPEECH_AT = 30 * 256  # where the excerpts of tests/golden/test.wav begin (the offset tests/test_gpu_parity.py reads it from, too)


def edge_streams(T, seed=1):
    """int16 [12, T * 256] and the rows' names"""
    assert T >= 3, T
    n = T * 256
    rng = np.random.default_rng(seed)
    x = np.zeros((ROWS, n), np.int16)
    x[0] = 32767
    x[1] = -32768
    x[2, 0::2], x[2, 1::2] = 32767, -32768  # the rails alternating at Nyquist, starting high
    x[3, 0::2], x[3, 1::2] = -32768, 32767  # ... starting low
    x[4] = rng.integers(-32768, 32768, n).astype(np.int16)  # uniform over the whole int16 range
    x[5, 3 * 256 - 1] = 32767  # one impulse, on the last sample of frame 2
    x[6, 2 * 256:] = 32767  # two frames of silence, then a full-scale step
    x[7] = rng.integers(-1, 2, n).astype(np.int16)  # +-1 LSB dither
    # x[8]: digital silence
    wav = load_wav('test.wav').astype(np.int64)
    half = (T // 2) * 256
    x[9, half:] = wav[SPEECH_AT:SPEECH_AT + n - half]  # silence for T / 2 frames, then speech
    x[10] = np.clip(8 * np.resize(wav[SPEECH_AT:], n), -32768, 32767)  # speech driven into the rails
    x[11] = np.where((np.arange(n) // 16) % 2 == 0, 32767, -32768)  # full-scale square wave, half period 16 samples (500 Hz)
    return x, list(NAMES)


# ---------------------------------------------------------------------------------------------------- models

# bins that pass (mask exactly 1.0); every other bin has mask sigmoid(-30), about 1e-13 (0 as the bf16 configuration's fp16 mask)
PASSBANDS = {
    'lowpass64': np.arange(257) < 64,
    'highpass8': np.arange(257) >= 8,
    'comb': np.arange(257) % 2 == 0,
}
FIXED = ['unity'] + sorted(PASSBANDS)                      # constant masks: nothing of the network reaches the samples
MODELS = ['random', 'random5', 'adaptive'] + FIXED         # every model of this suite


def fixed_mask_model(directory, name):
    """writes <directory>/<name>.kns: the zero network of params.make_constant_mask whose last head bias is +30 on the passband, -30 elsewhere"""
    t = params.make_constant_mask(0.0)
    t['s%d.b_head' % (params.STAGES - 1)][:] = np.where(PASSBANDS[name], 30.0, -30.0).astype(np.float32)
    path = os.path.join(str(directory), '%s.kns' % name)
    params.write_params(path, t)
    return path


def model_path(directory, name):
    """any model of MODELS; the fixed-mask ones are written to `directory` (a pytest temporary directory)"""
    if name in PASSBANDS:
        path = os.path.join(str(directory), '%s.kns' % name)
        return path if os.path.exists(path) else fixed_mask_model(directory, name)
    return model_file(name)


# ---------------------------------------------------------------------------------------------------- what a brick wall does, in float64

def unclamped(x, passband):
    """x int16 [n, T * 256], passband bool [257] -> float64 [n, T * 256]: analysis (sqrt-Hann 512 / 256 over [previous frame | frame]), the
    0 / 1 mask, overlap-add, one frame of delay -- in sample units, BEFORE rounding and clamping to int16.  From DESIGN.md section 2; shares no
    code with the oracle.  Only there so that the tests can say where the output must sit on a rail, and that such samples exist."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    n, T = x.shape[0], x.shape[1] // 256
    win = np.sin(np.pi * np.arange(512) / 512.0)
    padded = np.concatenate([np.zeros((n, 256)), x], axis=1)
    out, tail = np.zeros((n, T * 256)), np.zeros((n, 256))
    keep = np.asarray(passband, np.float64)
    for t in range(T):
        spec = np.fft.rfft(padded[:, t * 256:t * 256 + 512] * win, axis=1)
        blk = np.fft.irfft(spec * keep, 512, axis=1) * win
        out[:, t * 256:(t + 1) * 256] = tail + blk[:, :256]
        tail = blk[:, 256:]
    return out


def beyond(u):
    """-> (above, below): where the unrounded value rounds to something past a rail"""
    return u > 32767.5, u < -32768.5


# ---------------------------------------------------------------------------------------------------- what bf16 is held to

HORIZON = 64  # frames: the longest stream of tests/test_gpu_edge_inputs.py (the layer pipeline: two calls of 32 frames)

# (model, input) pairs on which the bf16 engine is held to the suite's bf16 bars (gpu_kit.check_pcm) against the bf16 oracle.  The condition for being
# listed (tests/test_edge_inputs.py, on the CPU): the jittered bf16 oracle, seeds 1 .. 8, stays within 1 LSB of the plain one over HORIZON
# frames -- i.e. two valid implementations agree there, so the bars mean on these pairs what they mean in the rest of the suite.  Every other
# pair is measured and printed by the GPU module, not asserted ("Edge inputs: what holds them").
BF16_ASSERTED = frozenset(
    [(m, i) for m in FIXED for i in NAMES]
    + [('adaptive', i) for i in NAMES if i != 'noise']
    + [(m, i) for m in ('random', 'random5') for i in ('impulse', 'dither', 'silence')])


def jitter_figures(path, x, seeds=range(1, 9)):
    """the distance between the plain and the jittered bf16 oracle on the rows of x, over the seeds: (max LSB [rows], share within 1 LSB [rows])"""
    from oracle import oracle
    oracle.set_jitter(0)
    plain = oracle.Oracle(path, x.shape[0], oracle.PREC_BF16).process(x).astype(np.int64)
    worst, within = np.zeros(x.shape[0], np.int64), np.ones(x.shape[0])
    try:
        for s in seeds:
            oracle.set_jitter(s)
            d = np.abs(oracle.Oracle(path, x.shape[0], oracle.PREC_BF16).process(x).astype(np.int64) - plain)
            worst, within = np.maximum(worst, d.max(axis=1)), np.minimum(within, (d <= 1).mean(axis=1))
    finally:
        oracle.set_jitter(0)
    return worst, within


def asserted_rows(model):
    """indices of the input rows asserted in bf16 for `model`"""
    return [r for r, i in enumerate(NAMES) if (model, i) in BF16_ASSERTED]
