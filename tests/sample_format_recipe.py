"""
The sample formats of batch handles (fifth extension), restated from the table of the specification with Python integers,
one value at a time: tables over all 256 bytes and all 65 536 samples for the two G.711 laws, and the float conversion through Python's
exact rational arithmetic on doubles.  Written apart from koala_amd/formats.py, which the tests compare with it.
"""
import math

import numpy as np

S16, F32, ULAW, ALAW = 0, 1, 2, 3
NAMES = ('s16', 'f32', 'ulaw', 'alaw')
DTYPES = (np.int16, np.float32, np.uint8, np.uint8)


def ulaw_dec(b):
    u = ~b & 0xFF
    e, m = (u >> 4) & 7, u & 15
    mag = (((m << 3) + 0x84) << e) - 0x84
    return -mag if u & 0x80 else mag


def ulaw_enc(s):
    sign = 0x80 if s < 0 else 0
    mag = min(abs(s), 32635) + 0x84
    e = mag.bit_length() - 8
    m = (mag >> (e + 3)) & 15
    return ~(sign | e << 4 | m) & 0xFF


def alaw_dec(b):
    a = b ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    mag = (m << 4) + 8 if e == 0 else ((m << 4) + 0x108) << (e - 1)
    return mag if a & 0x80 else -mag


def alaw_enc(s):
    sign = 0x80 if s >= 0 else 0
    mag = s if s >= 0 else ~s
    e = 0 if mag < 256 else mag.bit_length() - 8
    m = (mag >> 4) & 15 if e == 0 else (mag >> (e + 3)) & 15
    return (sign | e << 4 | m) ^ 0x55


def f32_dec(x):
    """one float32 value (as a Python float) -> the sample"""
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return 32767 if x > 0 else -32768
    y = x * 32768.0  # exact: a float32 times a power of two, in double
    r = math.floor(abs(y) + 0.5)  # half away from zero (abs(y) + 0.5 is exact in double for every float32 below 2^52)
    r = r if y >= 0 else -r
    return max(-32768, min(32767, int(r)))


ALL_SAMPLES = np.arange(-32768, 32768, dtype=np.int32)
DEC = {ULAW: np.array([ulaw_dec(b) for b in range(256)], np.int16), ALAW: np.array([alaw_dec(b) for b in range(256)], np.int16)}
# ENC[law][s + 32768]
ENC = {ULAW: np.array([ulaw_enc(int(s)) for s in ALL_SAMPLES], np.uint8), ALAW: np.array([alaw_enc(int(s)) for s in ALL_SAMPLES], np.uint8)}


def decode(fmt, a):
    a = np.asarray(a)
    assert a.dtype == DTYPES[fmt], (fmt, a.dtype)
    if fmt == S16:
        return a.copy()
    if fmt == F32:
        return np.array([f32_dec(float(v)) for v in a.ravel()], np.int16).reshape(a.shape)
    return DEC[fmt][a]


def encode(fmt, s):
    s = np.asarray(s)
    assert s.dtype == np.int16
    if fmt == S16:
        return s.copy()
    if fmt == F32:
        return (s.astype(np.float64) / 32768.0).astype(np.float32)  # (exact: 16 bits and a power of two)
    return ENC[fmt][s.astype(np.int32) + 32768]


# float32 values at which the conversion can go wrong: zeros, full scale, the last level, ties, overflow, infinities, NaN, a denormal
F32_EDGES = np.array([0.0, -0.0, 1.0, -1.0, 1.0 - 2.0 ** -16, -(1.0 - 2.0 ** -16), 0.5 / 32768, -0.5 / 32768, 1.5 / 32768, -1.5 / 32768,
                      2.5 / 32768, -2.5 / 32768, 32766.5 / 32768, -32767.5 / 32768, 1e30, -1e30, np.inf, -np.inf, np.nan, 1e-40, -1e-40,
                      np.nextafter(np.float32(0.5 / 32768), np.float32(0))], np.float32)
# ((1 - 2^-16) 32768 = 32767.5 is a tie: away from zero and clipped it is 32767, its negative -32768)
F32_EDGES_WANT = np.array([0, 0, 32767, -32768, 32767, -32768, 1, -1, 2, -2, 3, -3, 32767, -32768, 32767, -32768, 32767, -32768, 0, 0, 0, 0],
                          np.int16)
