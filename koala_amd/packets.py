"""
Packet handles in pure Python (fourth extension): what a call of `KoalaBatch.process_packets` will do, without a GPU.

`frames_due` and `plan` restate the engine's host-side plan (koala_amd/csrc/kns_engine.cpp, run_packets): which streams complete how many
frames in a call, and into which inner frame calls -- with which streams held -- the call is cut.  `PacketClock` collects packets as they
arrive from many callers into the `counts` / `pcm` rows of the next call.
"""

from typing import List, Optional, Tuple

import numpy as np


def frames_due(fill, counts, frame_length: int) -> Tuple[np.ndarray, np.ndarray]:
    """(k, new_fill): stream b, with fill[b] samples pending, is given counts[b] more: it completes k[b] = (fill + counts) // F frames and
    keeps new_fill[b] = (fill + counts) % F samples pending."""
    total = np.asarray(fill, np.int64) + np.asarray(counts, np.int64)
    return (total // frame_length).astype(np.int32), (total % frame_length).astype(np.int32)


def plan(k, max_frames: int) -> List[Tuple[int, int, Optional[np.ndarray]]]:
    """The inner frame calls of a packet call in which stream b completes k[b] frames: a list of (first_frame, num_frames, hold).
    The call's frames are cut at every distinct non-zero k[b] and so that no sub-call exceeds `max_frames`; `hold` is uint8
    [num_streams], non-zero for the streams that have completed all their frames before the sub-call's end -- or None when no stream
    is held (the plain frame call).  Equal k: one sub-call without hold.  All zero: no sub-call.  (On a handle no k[b] exceeds
    `max_frames`, so the engine cuts at the distinct k[b] alone; the cut at `max_frames` makes this function total over any k.)"""
    k = np.asarray(k, np.int64)
    cuts = [0]
    for v in np.unique(k):
        v = int(v)
        if v <= cuts[-1]:
            continue
        while v - cuts[-1] > max_frames:
            cuts.append(cuts[-1] + max_frames)
        cuts.append(v)
    out = []
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        hold = (k < c1).astype(np.uint8)
        out.append((c0, c1 - c0, hold if hold.any() else None))
    return out


# ---- packet handles at 44 100 and 22 050 Hz (sixth extension): 16 000 / rate = U / 441
FRACTIONAL_UP = {44100: 160, 22050: 320}


def inner_samples(n, sample_rate: int):
    """M(N): the samples of the inner 16 kHz stream that exist once a stream at `sample_rate` has received n samples in total,
    floor((U n - 1) / 441) + 1 with floor division (M(0) = 0).  An int for an int, else an int64 array."""
    U = FRACTIONAL_UP[sample_rate]
    if isinstance(n, (int, np.integer)):
        return (U * int(n) - 1) // 441 + 1
    return (U * np.asarray(n, np.int64) - 1) // 441 + 1


def inner_due(phase, counts, sample_rate: int) -> Tuple[np.ndarray, np.ndarray]:
    """(inner, new_phase): stream b, which has received N samples with N mod 441 = phase[b], is given counts[b] more: the call feeds its
    inner 16 kHz packet path inner[b] = M(N + counts) - M(N) samples (0 is possible) and leaves new_phase[b] = (phase + counts) mod 441.
    The engine plans from the same mirror (koala_amd/csrc/kns_engine.cpp, run_fractional); the inner path's frames then follow from
    `frames_due(fill, inner, 256)`."""
    phase, counts = np.asarray(phase, np.int64), np.asarray(counts, np.int64)
    inner = inner_samples(phase + counts, sample_rate) - inner_samples(phase, sample_rate)
    return inner.astype(np.int32), ((phase + counts) % 441).astype(np.int32)


class PacketClock(object):
    """Collects arriving packets into the rows of the next packet call.

        clock = PacketClock(num_streams, max_samples)
        clock.push(stream, samples)        # any number of times, any streams, any lengths: appended to the stream's row
        counts, pcm = clock.take()         # the next call's arguments; what did not fit into max_samples stays for the call after
        enhanced = handle.process_packets(pcm, counts)   # enhanced[b, :counts[b]] are stream b's next output samples
    """

    def __init__(self, num_streams: int, max_samples: int) -> None:
        if num_streams < 1 or max_samples < 1:
            raise ValueError("`num_streams` and `max_samples` must be positive")
        self.num_streams, self.max_samples = num_streams, max_samples
        self._queue = [np.zeros(0, np.int16) for _ in range(num_streams)]

    def push(self, stream: int, samples) -> None:
        s = np.asarray(samples)
        if s.ndim != 1 or s.dtype != np.int16:
            raise ValueError("a packet is a 1-d int16 array")
        self._queue[stream] = np.concatenate([self._queue[stream], s])

    def pending(self) -> np.ndarray:
        """samples waiting per stream, int32 [num_streams]"""
        return np.array([q.size for q in self._queue], np.int32)

    def take(self) -> Tuple[np.ndarray, np.ndarray]:
        counts = np.minimum(self.pending(), self.max_samples).astype(np.int32)
        pcm = np.zeros((self.num_streams, self.max_samples), np.int16)
        for b, n in enumerate(counts):
            pcm[b, :n] = self._queue[b][:n]
            self._queue[b] = self._queue[b][n:]
        return counts, pcm


__all__ = ['frames_due', 'plan', 'PacketClock', 'FRACTIONAL_UP', 'inner_samples', 'inner_due']
