"""
Numpy restatement of packet handles (fourth extension), around ANY frame function.

A frame function is a stateful callable  frames int16 [k * F] -> enhanced int16 [k * F]  (k >= 1) standing for one stream of a frame handle:
the oracle (`oracle_stream`), or a pure delay by one frame (`DelayStream`, rate-agnostic: F is whatever the caller says).

`PacketStream` is one stream of a packet handle: fill = N mod F and ONE buffer of F - 1 int16 whose first `fill` entries are pending input and
whose last F - 1 - fill entries are pending output.  `push(samples)` returns as many output samples as it was given.
"""
import numpy as np


class DelayStream(object):
    """a frame handle's stream with a unity mask: the input delayed by one frame of F samples"""

    def __init__(self, F):
        self.F, self.prev = F, np.zeros(F, np.int16)

    def __call__(self, frames):
        assert frames.size and frames.size % self.F == 0
        out = np.concatenate([self.prev, frames])[:frames.size]
        self.prev = np.concatenate([self.prev, frames])[-self.F:].copy()
        return out.astype(np.int16)

    def state(self):
        return self.prev.copy()

    def set_state(self, s):
        self.prev = s.copy()


def oracle_stream(model, precision):
    """one oracle stream at 16 kHz as a frame function (precision: 'fp32' or 'bf16')"""
    from oracle import oracle
    o = oracle.Oracle(model, 1, oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32)
    return lambda frames: o.process(np.ascontiguousarray(frames[None]))[0]


def record_bytes(F):
    """the packet part of a version-3 record: uint32 fill, int16[F - 1], zero-padded to whole 16-byte words"""
    return (4 + 2 * (F - 1) + 15) // 16 * 16


class PacketStream(object):
    def __init__(self, frame_fn, F):
        self.fn, self.F = frame_fn, F
        self.reset()

    def reset(self):
        """NOT the frame function's reset: the caller makes a fresh one (`restart` = a fresh stream)"""
        self.fill, self.buf = 0, np.zeros(self.F - 1, np.int16)
        self.taken = self.given = self.frames = 0  # samples pushed, samples returned, frames completed since the reset

    def invariant(self):
        """pending input + pending output = F - 1 samples, counted from what went in and out, not from the buffer: the pending input is
        what was taken and is in no frame yet, the pending output the F - 1 zeros and the frames' samples that were not yet returned;
        the one buffer holds exactly these two, split at fill"""
        pending_in = self.taken - self.frames * self.F
        pending_out = self.F - 1 + self.frames * self.F - self.given
        return (0 <= pending_in < self.F and pending_out >= 0 and pending_in + pending_out == self.F - 1 and
                self.fill == pending_in == self.taken % self.F and self.buf.size - self.fill == pending_out and self.buf.dtype == np.int16)

    def frames_due(self, count):
        return (self.fill + count) // self.F

    def push(self, samples):
        """the next len(samples) output samples; len 0: nothing changes"""
        x = np.asarray(samples, np.int16)
        F, k = self.F, self.frames_due(x.size)
        pending_in, pending_out = self.buf[:self.fill], self.buf[self.fill:]
        cat = np.concatenate([pending_in, x])
        enhanced = self.fn(cat[:k * F]) if k else np.zeros(0, np.int16)
        assert enhanced.size == k * F
        out = np.concatenate([pending_out, enhanced])
        assert out.size >= x.size  # F - 1 - fill + k F >= count, always
        self.last_frames = k
        self.taken, self.given, self.frames = self.taken + x.size, self.given + x.size, self.frames + k
        self.fill = cat.size - k * F
        self.buf = np.concatenate([cat[k * F:], out[x.size:]]).astype(np.int16)
        assert self.buf.size == F - 1
        return out[:x.size].astype(np.int16)

    def record(self):
        """the packet part of the stream's version-3 record"""
        r = np.zeros(record_bytes(self.F), np.uint8)
        r[:4] = np.frombuffer(np.uint32(self.fill).tobytes(), np.uint8)
        r[4:4 + 2 * (self.F - 1)] = np.frombuffer(self.buf.astype('<i2').tobytes(), np.uint8)
        return r

    def set_record(self, r):
        r = np.asarray(r, np.uint8)
        assert r.size == record_bytes(self.F)
        self.fill = int(np.frombuffer(r[:4].tobytes(), '<u4')[0])
        assert self.fill < self.F
        self.buf = np.frombuffer(r[4:4 + 2 * (self.F - 1)].tobytes(), '<i2').astype(np.int16)
        self.taken = self.given = self.fill  # (the counts of a stream that got `fill` samples since its reset: all the invariant needs)
        self.frames = 0


def expected(frame_fn, F, x):
    """([0] * (F - 1) ++ frame_fn(x in frames))[:N]: what the packets' outputs must concatenate to, whatever the packet sizes"""
    x = np.asarray(x, np.int16)
    k = x.size // F
    e = frame_fn(x[:k * F]) if k else np.zeros(0, np.int16)
    return np.concatenate([np.zeros(F - 1, np.int16), e])[:x.size]
