"""
The sample formats of batch handles in numpy (include/pv_koala_batch.h, pv_koala_sample_format_t; DESIGN.md section 2, fifth extension):
what a handle made with `create_batch(..., sample_format=...)` does to every sample on its way in (`decode`) and out (`encode`), for
callers that want to prepare input, interpret output or restate a handle's result as encode(S16 handle(decode(x))).

    's16'   int16    identity
    'f32'   float32  in: NaN -> 0, else x * 32768 rounded half away from zero, clipped to [-32768, 32767]; out: s / 32768 (exact)
    'ulaw'  uint8    ITU G.711 mu-law on a 16-bit scale: 255 levels in +-32124, the encoder truncates
    'alaw'  uint8    ITU G.711 A-law on a 16-bit scale: 256 levels in +-32256, the encoder truncates
"""

import numpy as np

FORMATS = ('s16', 'f32', 'ulaw', 'alaw')  # the index is the C ABI's value
DTYPES = {'s16': np.int16, 'f32': np.float32, 'ulaw': np.uint8, 'alaw': np.uint8}


def format_name(fmt) -> str:
    """'s16' / 'f32' / 'ulaw' / 'alaw' for a name or the C ABI's value 0 ... 3; ValueError otherwise."""
    if isinstance(fmt, str) and fmt in FORMATS:
        return fmt
    if isinstance(fmt, (int, np.integer)) and not isinstance(fmt, bool) and 0 <= int(fmt) < len(FORMATS):
        return FORMATS[int(fmt)]
    raise ValueError("sample format should be one of 's16', 'f32', 'ulaw', 'alaw'")


def dtype(fmt):
    """The numpy dtype of a format's elements."""
    return DTYPES[format_name(fmt)]


def _bit_length(v):
    """bit_length of non-negative int32 values below 2^16"""
    n = np.zeros(v.shape, np.int32)
    for k in range(16):
        n += (v >> k) > 0
    return n


def decode(fmt, a) -> np.ndarray:
    """Elements of the format -> the int16 samples the engine sees."""
    fmt = format_name(fmt)
    a = np.asarray(a)
    if a.dtype != DTYPES[fmt]:
        raise ValueError("decode('%s') expects %s, got %s" % (fmt, np.dtype(DTYPES[fmt]).name, a.dtype.name))
    if fmt == 's16':
        return a.copy()
    if fmt == 'f32':
        with np.errstate(over='ignore', invalid='ignore'):
            y = np.clip(a * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))  # (the product is exact or +-inf)
            y = np.where(np.isnan(y), np.float32(0.0), y)
            r = np.trunc(y)
            r = r + np.where(np.abs(y - r) >= np.float32(0.5), np.copysign(np.float32(1.0), y), np.float32(0.0))  # half away from zero
        return r.astype(np.int16)
    b = a.astype(np.int32)
    if fmt == 'ulaw':
        u = ~b & 0xFF
        e, m = (u >> 4) & 7, u & 15
        mag = (((m << 3) + 0x84) << e) - 0x84
        return np.where(u & 0x80, -mag, mag).astype(np.int16)
    x = b ^ 0x55
    e, m = (x >> 4) & 7, x & 15
    mag = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(x & 0x80, mag, -mag).astype(np.int16)


def encode(fmt, s) -> np.ndarray:
    """int16 samples -> elements of the format."""
    fmt = format_name(fmt)
    s = np.asarray(s)
    if s.dtype != np.int16:
        raise ValueError("encode() expects int16, got %s" % s.dtype.name)
    if fmt == 's16':
        return s.copy()
    if fmt == 'f32':
        return s.astype(np.float32) * np.float32(1.0 / 32768)
    v = s.astype(np.int32)
    if fmt == 'ulaw':
        sign = np.where(v < 0, 0x80, 0)
        mag = np.minimum(np.abs(v), 32635) + 0x84
        e = _bit_length(mag) - 8
        m = (mag >> (e + 3)) & 15
        return (~(sign | e << 4 | m) & 0xFF).astype(np.uint8)
    sign = np.where(v >= 0, 0x80, 0)
    mag = np.where(v >= 0, v, ~v)
    e = np.where(mag < 256, 0, _bit_length(mag) - 8)
    m = np.where(e == 0, (mag >> 4) & 15, (mag >> (e + 3)) & 15)
    return ((sign | e << 4 | m) ^ 0x55).astype(np.uint8)


__all__ = ['FORMATS', 'DTYPES', 'format_name', 'dtype', 'decode', 'encode']
