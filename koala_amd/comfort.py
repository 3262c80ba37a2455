"""
Comfort noise (include/pv_koala_batch.h, COMFORT NOISE; DESIGN.md section 2, twelfth extension): the rule in numpy, and a builder for the
amplitude curve on the handle's bin grid -- 257 bins, 31.25 Hz apart, bin 0 = DC, bin 256 = 8 kHz.

In every frame a stream with comfort noise on completes, with m' the mask after the attenuation limit and the band profile
(koala_amd.bands.apply), n the stream's frame counter and X the frame's spectrum:

    v  = seed ^ (n * 0x9E3779B9) ^ (k * 0x85EBCA6B)                          uint32, wrapping
    v ^= v >> 16;  v *= 0x7FEB352D;  v ^= v >> 15;  v *= 0x846CA68B;  v ^= v >> 16
    z_re = ((float) (v & 0xFFFF) - 32767.5) / 32768                          exact in float32
    z_im = ((float) (v >> 16)    - 32767.5) / 32768                          0 for k = 0 and k = 256
    w = 1 - m'[k];  a = w * A[k];  Y_re = (m'[k] * X_re) + (a * z_re)        every operation rounded to float32, none fused

`variates` and `apply` are what a handle does; numpy only, nothing here needs the library.
"""
import numpy as np

NUM_BINS = 257
BIN_HZ = 16000.0 / 512.0
F32 = np.float32
U32 = np.uint32
SHAPES = ('white', 'pink', 'hoth')

# The long-term spectrum of room noise after Hoth, as telephony test signals use it (spectrum density in dB against an arbitrary reference,
# at third-octave centre frequencies in Hz): about -5 dB per octave through the speech band, steeper towards 8 kHz.
_HOTH_HZ = (100, 125, 160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000)
_HOTH_DB = (32.4, 30.9, 29.1, 27.6, 26.0, 24.4, 22.7, 21.1, 19.5, 17.8, 16.2, 14.6, 12.9, 11.3, 9.6, 7.8, 5.4, 2.6, -1.3, -6.6)


def variates(seed, n):
    """(z_re, z_im), float32 [..., 257] each, uniform on 65536 levels in (-1, 1): `seed` and `n` are uint32 scalars or arrays of one shape
    [...] (the counter wraps modulo 2^32)."""
    seed, n = np.asarray(seed).astype(U32), np.asarray(n).astype(U32)
    k = np.arange(NUM_BINS, dtype=U32)
    with np.errstate(over='ignore'):
        v = (seed ^ (n * U32(0x9E3779B9)))[..., None] ^ (k * U32(0x85EBCA6B))
        v = v ^ (v >> U32(16))
        v = v * U32(0x7FEB352D)
        v = v ^ (v >> U32(15))
        v = v * U32(0x846CA68B)
        v = v ^ (v >> U32(16))
    z_re = (((v & U32(0xFFFF)).astype(F32) - F32(32767.5)) * F32(1.0 / 32768.0)).astype(F32)
    z_im = (((v >> U32(16)).astype(F32) - F32(32767.5)) * F32(1.0 / 32768.0)).astype(F32)
    z_im[..., 0] = 0
    z_im[..., NUM_BINS - 1] = 0
    return z_re, z_im


def apply(spectrum, m_prime, amplitude, seed, n):
    """Y float32 [..., 257, 2] of the spectrum X [..., 257, 2], the shaped mask m' [..., 257], the curve A [257] or [..., 257], and the
    stream's seed and counter value (scalars, or arrays of the leading shape)."""
    x, m, a = np.asarray(spectrum, F32), np.asarray(m_prime, F32), np.asarray(amplitude, F32)
    z_re, z_im = variates(seed, n)
    w = (F32(1.0) - m).astype(F32)
    aw = (w * a).astype(F32)
    y = np.empty(x.shape, F32)
    y[..., 0] = ((m * x[..., 0]).astype(F32) + (aw * z_re).astype(F32)).astype(F32)
    y[..., 1] = ((m * x[..., 1]).astype(F32) + (aw * z_im).astype(F32)).astype(F32)
    return y


def check(amplitude, rows=None):
    """The curve as a float32 array [257] (rows: [rows, 257]; one curve serves every row), refused the way the library refuses it: a value
    that is NaN, negative or infinite."""
    shape = (NUM_BINS,) if rows is None else (rows, NUM_BINS)
    a = np.ascontiguousarray(amplitude, dtype=F32)
    if rows is not None and a.shape == (NUM_BINS,):
        a = np.ascontiguousarray(np.broadcast_to(a, shape))
    if a.shape != shape:
        raise ValueError("`amplitude` must have shape %s, not %s" % (shape, a.shape))
    if not (np.isfinite(a) & (a >= 0)).all():
        raise ValueError("`amplitude` must be finite and >= 0 in every bin")
    return a + F32(0)


def shape_weights(shape='white'):
    """s[k], float64 [257]: the curve's form, A = c s.  'white': flat; 'pink': power ~ 1 / f (bin 0 as bin 1); 'hoth': room noise after Hoth,
    the table above interpolated over log f and held outside it."""
    if shape == 'white':
        return np.ones(NUM_BINS)
    k = np.maximum(np.arange(NUM_BINS, dtype=np.float64), 1.0)
    if shape == 'pink':
        return 1.0 / np.sqrt(k)
    if shape == 'hoth':
        db = np.interp(np.log(k * BIN_HZ), np.log(np.asarray(_HOTH_HZ, np.float64)), np.asarray(_HOTH_DB, np.float64))
        return 10.0 ** ((db - db.max()) / 20.0)
    raise ValueError("`shape` is one of %s" % (SHAPES,))


def curve(dbfs, shape='white'):
    """A float32 [257]: the curve under which a stream delivers noise of `dbfs` dB RMS against full scale (RMS 1 = 32768) where m' = 0.

    The constant, from DESIGN.md section 2's transform scaling.  Where m' = 0, Y[k] = A[k] (z_re + i z_im) with z_re, z_im independent,
    uniform on (-1, 1): variance 1/3 each (exactly (1 - 2^-32) / 3).  The frame's 512 samples are the inverse 512-point transform of the
    Hermitian spectrum, s[j] = (1/512) (Y[0] + (-1)^j Y[256] + 2 sum_{k=1..255} Re(Y[k] e^{2 pi i j k / 512})), so
        var s = (1/512^2) (A[0]^2 / 3 + A[256]^2 / 3 + sum_{k=1..255} 4 A[k]^2 / 3)      for every j.
    A sample of the output is w[j] s_t[j] + w[j + 256] s_{t-1}[j + 256], two independent frames under the sqrt-Hann window, whose squares sum
    to 1 across the overlap: the output is stationary with variance var s, in units of full scale.  With A = c s[k] and r = 10^(dbfs / 20):
        c = 512 r sqrt(3 / (s[0]^2 + s[256]^2 + 4 sum_{k=1..255} s[k]^2))."""
    if not np.isfinite(dbfs):
        raise ValueError("`dbfs` is a finite level in dB against full scale")
    s = shape_weights(shape)
    r = 10.0 ** (float(dbfs) / 20.0)
    c = 512.0 * r * np.sqrt(3.0 / (s[0] ** 2 + s[256] ** 2 + 4.0 * np.sum(s[1:256] ** 2)))
    return (c * s).astype(F32)


__all__ = ['NUM_BINS', 'BIN_HZ', 'SHAPES', 'variates', 'apply', 'check', 'shape_weights', 'curve']
