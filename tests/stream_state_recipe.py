"""
The stream record (include/pv_koala_batch.h: pv_koala_batch_export_state) in pure numpy: its layout, a packer and a
reader.  Shared by tests/test_stream_state.py and the GPU modules that read records; not a test module.
"""
import struct

import numpy as np

# ---- the record: header 32 | hist int16[256] | tail float[256] | h float[8][271] | fctx float[taps - 1][257]
MAGIC = b'KNSS'
VERSION = 1
HEADER = struct.Struct('<4sIIIQ8s')  # magic, version, front_taps, precision, model hash, reserved
OFF_HIST, OFF_TAIL, OFF_H, OFF_FCTX = 32, 32 + 512, 32 + 512 + 1024, 32 + 512 + 1024 + 8 * 271 * 4


def record_size(front_taps):
    """bytes of a record; whole 16-byte words (front_taps 1 and 5, the models that exist, need no padding)"""
    return (OFF_FCTX + (front_taps - 1) * 257 * 4 + 15) // 16 * 16


def pack_record(front_taps, precision, model_hash, hist, tail, h, fctx=None):
    out = np.zeros(record_size(front_taps), np.uint8)
    out[:32] = np.frombuffer(HEADER.pack(MAGIC, VERSION, front_taps, precision, model_hash, bytes(8)), np.uint8)
    out[OFF_HIST:OFF_TAIL] = np.ascontiguousarray(hist, '<i2').reshape(256).view(np.uint8)
    out[OFF_TAIL:OFF_H] = np.ascontiguousarray(tail, '<f4').reshape(256).view(np.uint8)
    out[OFF_H:OFF_FCTX] = np.ascontiguousarray(h, '<f4').reshape(8 * 271).view(np.uint8)
    if front_taps > 1:
        out[OFF_FCTX:OFF_FCTX + (front_taps - 1) * 1028] = np.ascontiguousarray(fctx, '<f4').reshape((front_taps - 1) * 257).view(np.uint8)
    return out


def unpack_record(blob):
    """-> dict(front_taps, precision, model_hash, hist [256] int16, tail [256] float32, h [8, 271] float32, fctx [taps - 1, 257] float32)"""
    raw = bytes(blob)
    magic, version, taps, precision, model_hash, reserved = HEADER.unpack(raw[:32])
    assert magic == MAGIC and version == VERSION and reserved == bytes(8), (magic, version, reserved)
    assert len(raw) == record_size(taps), (len(raw), taps)
    return dict(front_taps=taps, precision=precision, model_hash=model_hash,
                hist=np.frombuffer(raw, '<i2', 256, OFF_HIST), tail=np.frombuffer(raw, '<f4', 256, OFF_TAIL),
                h=np.frombuffer(raw, '<f4', 8 * 271, OFF_H).reshape(8, 271),
                fctx=np.frombuffer(raw, '<f4', (taps - 1) * 257, OFF_FCTX).reshape(taps - 1, 257))
