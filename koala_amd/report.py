"""
Reading the frame report (include/pv_koala_batch.h, FRAME REPORT): rows of four float32 values -- e_in, e_out, mask_sum and the output
leveller's gain (0 for a stream that does not level) -- per stream and
frame, as returned by KoalaBatch.process_call(..., report=True), Koala.process_with_report() and enhance_corpus(..., report=True).  numpy
only; every function takes an array whose LAST axis is the row and returns an array without it.

e_in and e_out are sums of |X[k]|^2 over the 257 bins k = 0 .. 256 of the one-sided spectrum of a 512-sample block of samples / 32768
under the sqrt-Hann window w[n] = sin(pi n / 512).
"""

import numpy as np

BINS = 257
# Parseval for the real 512-point block y[n] = w[n] x[n]:  sum_n y[n]^2 = (1 / 512) (|Y0|^2 + |Y256|^2 + 2 sum_{k=1..255} |Yk|^2), so the
# one-sided sum E = sum_{k=0..256} |Yk|^2 is 256 sum_n y[n]^2 up to the (half-counted) DC and Nyquist bins.  For a stationary input of mean
# square P the window contributes sum_n w[n]^2 = 256 (sin^2 averages 1/2 over 512 points), hence E = 256 * 256 * P = 65536 P.
# A full-scale sine (P = 1/2) therefore reads -3.01 dBFS, a full-scale square wave 0 dBFS.
ENERGY_AT_FULL_SCALE = 65536.0


def mean_gain(report):
    """Mean over the 257 bins of the network's raw mask (before any attenuation limit), in [0, 1]: near 1 = the model passes the frame
    (speech, or nothing to remove), near 0 = the model gates it."""
    return np.asarray(report, np.float32)[..., 2] / np.float32(BINS)


def suppression_db(report):
    """10 log10(e_out / e_in): what the applied mask did to the frame's energy, <= 0 dB up to rounding.  NaN where e_in == 0 (a block of
    digital silence); -inf where only e_out is 0."""
    r = np.asarray(report, np.float64)
    e_in, e_out = r[..., 0], r[..., 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        db = 10.0 * np.log10(e_out / e_in)
    return np.where(e_in == 0, np.nan, db)


def input_dbfs(report):
    """Level of the frame's 512-sample analysis block in dB relative to a full-scale square wave: 10 log10(e_in / 65536) (see
    ENERGY_AT_FULL_SCALE: Parseval for the sqrt-Hann window).  -inf for digital silence."""
    with np.errstate(divide='ignore'):
        return 10.0 * np.log10(np.asarray(report, np.float64)[..., 0] / ENERGY_AT_FULL_SCALE)


def level_gain_db(report):
    """Column 3 of the row as dB: the output leveller's gain behind the frame (koala_amd.level; include/pv_koala_batch.h, OUTPUT LEVELLER).
    The column is 0 for a stream that does not level: 0 dB there."""
    g = np.asarray(report, np.float64)[..., 3]
    return 20.0 * np.log10(np.where(g > 0, g, 1.0))


__all__ = ['BINS', 'ENERGY_AT_FULL_SCALE', 'mean_gain', 'suppression_db', 'input_dbfs', 'level_gain_db']
