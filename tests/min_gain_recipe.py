"""
What a limited stream must deliver (include/pv_koala_batch.h: pv_koala_batch_set_min_gain), from the oracle's stage functions, and the
table of shapes that walks the dispatch table under it.  Shared by tests/test_gpu_min_gain.py and tests/test_gpu_frame_report.py (which
reports on the same calls); not a test module.

`Oracle.process_with_mask` gives every frame's mask m, `Oracle.analysis` its spectrum, numpy float32 forms m' = g + (1 - g) m (one
subtraction, one product, one sum, each rounded to float32) and `oracle.synthesis` makes the samples.
"""
import numpy as np

from gpu_kit import ROUTE_CHUNKED, ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_SMALL, ROUTE_WAVE, frames, oracle_prec
from oracle import oracle

NCLS = 8
# per class: 0 (no limit), 1 (bypass) and values in between; a call's gains are this list rotated by the call's number
GAINS = np.array([0.0, 1.0, 0.25, 0.5, 0.1, 0.9, 0.031622775, 0.70710677], np.float32)

# (precision, streams, max frames, [(frames, mode)], routes that must have been taken)
SHAPES = [
    ('fp32', 21, 4, [(1, 'host'), (4, 'host'), (1, 'host'), (1, 'host'), (4, 'inplace')], (ROUTE_SMALL, ROUTE_WAVE)),
    ('bf16', 21, 4, [(1, 'host'), (1, 'host'), (4, 'host'), (1, 'device'), (4, 'inplace')], (ROUTE_SMALL, ROUTE_WAVE)),
    ('bf16', 1024, 48, [(48, 'device'), (1, 'device'), (32, 'device'), (1, 'host'), (8, 'inplace')],
     (ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_CHUNKED)),
    # host calls of 16 MiB: sub-chunks of 4 12 12 4 frames on three streams (each takes the route of a call of its length); asynchronous: whole
    ('bf16', 1024, 32, [(32, 'host'), (32, 'async'), (32, 'host')], (ROUTE_PIPELINED,)),
    ('bf16', 4100, 4, [(4, 'device'), (1, 'device'), (4, 'inplace')], (ROUTE_CHUNKED,)),  # resident8; 257 m-tiles, the last one ragged
    ('fp32', 4100, 2, [(2, 'device'), (1, 'device'), (2, 'inplace')], (ROUTE_CHUNKED,)),  # fp32 chunked (more than 256 m-tiles)
    ('fp32', 512, 4, [(4, 'device'), (1, 'host'), (4, 'host')], (ROUTE_WAVE, ROUTE_SMALL)),
]


class Recipe:
    """n streams of the spec with a minimum gain, from the oracle's stages (the module's docstring)"""

    def __init__(self, model, n, precision):
        self.o = oracle.Oracle(model, n, oracle_prec(precision))
        self.n = n
        self.hist = np.zeros((n, 256), np.int16)
        self.tail = np.zeros((n, 256), np.float32)

    def reset(self, rows):
        rows = np.asarray(rows, bool)
        if rows.any():
            self.o.reset(rows.astype(np.uint8))
            self.hist[rows] = 0
            self.tail[rows] = 0

    def process(self, x, gains):
        x = np.ascontiguousarray(x, np.int16)
        T = x.shape[1] // 256
        _, mask = self.o.process_with_mask(x)
        out = np.empty_like(x)
        for b in range(self.n):
            g = np.float32(gains[b])
            u = np.float32(1.0) - g
            for t in range(T):
                fr = x[b, t * 256:(t + 1) * 256]
                spec, _ = self.o.analysis(self.hist[b], fr)
                m = mask[t, b].astype(np.float32)
                mp = (g + (u * m).astype(np.float32)).astype(np.float32)
                out[b, t * 256:(t + 1) * 256] = oracle.synthesis(spec, mp, self.tail[b])
                self.hist[b] = fr
        return out

    def process_resets(self, x, gains, reset):
        """per-frame stream resets [n, T]: frame by frame, a reset right before its frame"""
        T = x.shape[1] // 256
        outs = []
        for t in range(T):
            self.reset(reset[:, t] != 0)
            outs.append(self.process(frames(x, t, t + 1), gains))
        return np.concatenate(outs, axis=1)
