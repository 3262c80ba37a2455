"""
The layout of multi-channel batch handles (include/pv_koala_batch.h, CHANNELS; DESIGN.md section 2, seventh extension) in numpy: a handle
with `channels=C` takes and delivers [G, n*C] arrays in which sample i of stream g*C + c is element [g, i*C + c].  Its result is exactly

    interleave(planar_handle(deinterleave(pcm, C)), C)

where the planar handle is the same configuration without channels.  Pure memory layout: any dtype, no arithmetic.
"""

import numpy as np

MAX_CHANNELS = 8
LINK_CHANNELS = (2, 4, 8)  # a linked group lies inside one 16-row mask tile


def _check(channels):
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError("`channels` should be an integer in [1, %d]" % MAX_CHANNELS)
    return int(channels)


def deinterleave(x, channels):
    """[G, n*C] (or [G, n, C], the same memory) -> [G*C, n]: row g*C + c holds elements [g, i*C + c], i = 0 .. n - 1"""
    C = _check(channels)
    x = np.asarray(x)
    if x.ndim == 3 and x.shape[2] == C:
        x = x.reshape(x.shape[0], -1)
    if x.ndim != 2 or x.shape[1] % C:
        raise ValueError("expected an array of shape [G, n*%d] or [G, n, %d]" % (C, C))
    G, n = x.shape[0], x.shape[1] // C
    return np.ascontiguousarray(x.reshape(G, n, C).transpose(0, 2, 1)).reshape(G * C, n)


def interleave(planar, channels):
    """[G*C, n] -> [G, n*C]: element [g, i*C + c] is sample i of row g*C + c"""
    C = _check(channels)
    p = np.asarray(planar)
    if p.ndim != 2 or p.shape[0] % C:
        raise ValueError("expected an array of shape [G*%d, n]" % C)
    G, n = p.shape[0] // C, p.shape[1]
    return np.ascontiguousarray(p.reshape(G, C, n).transpose(0, 2, 1)).reshape(G, n * C)


def link_masks(mask, channels):
    """The rule of linked channels (include/pv_koala_batch.h, LINKED CHANNELS; DESIGN.md section 2, eighth extension): mask [G*C, ...] ->
    the same shape, row g*C + c = the max over rows g*C .. g*C + C - 1, element by element.  A max of finite values: exact in any float
    dtype, whatever the order.  C must be 2, 4 or 8."""
    C = _check(channels)
    if C not in LINK_CHANNELS:
        raise ValueError("linked channels need `channels` 2, 4 or 8, not %d" % C)
    m = np.asarray(mask)
    if m.ndim < 1 or m.shape[0] % C:
        raise ValueError("expected an array of shape [G*%d, ...]" % C)
    grouped = m.reshape((m.shape[0] // C, C) + m.shape[1:])
    return np.ascontiguousarray(np.broadcast_to(grouped.max(axis=1, keepdims=True), grouped.shape)).reshape(m.shape)


__all__ = ['MAX_CHANNELS', 'LINK_CHANNELS', 'deinterleave', 'interleave', 'link_masks']
