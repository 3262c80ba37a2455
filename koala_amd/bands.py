"""
Band profile (include/pv_koala_batch.h, pv_koala_batch_set_band_profile; DESIGN.md section 2, tenth extension): the rule in numpy, and
builders for the curves on the handle's bin grid -- 257 bins, 31.25 Hz apart, bin 0 = DC, bin 256 = 8 kHz.

    m1[k] = g + (1 - g) m[k]                       the attenuation limit, two roundings
    m'[k] = min(ceiling[k], max(floor[k], m1[k]))  max first, then min; exact

`apply` is what a handle does to the network's mask in every frame; numpy only, nothing here needs the library.
"""
import numpy as np

NUM_BINS = 257
BIN_HZ = 16000.0 / 512.0
F32 = np.float32


def neutral():
    """(floor, ceiling) of a new handle: zeros and ones."""
    return np.zeros(NUM_BINS, F32), np.ones(NUM_BINS, F32)


def check(floor, ceiling, rows=None):
    """The pair as float32 arrays [..., 257] (None: the neutral curve), refused the way the library refuses it: a value that is NaN or
    outside [0, 1], a floor above its ceiling.  `rows`: the leading dimension both must have (None: a single curve [257])."""
    shape = (NUM_BINS,) if rows is None else (rows, NUM_BINS)
    lo = np.zeros(shape, F32) if floor is None else np.ascontiguousarray(floor, dtype=F32)
    hi = np.ones(shape, F32) if ceiling is None else np.ascontiguousarray(ceiling, dtype=F32)
    if rows is not None:  # (a single curve serves every listed stream)
        lo, hi = (np.ascontiguousarray(np.broadcast_to(a, shape)) if a.shape == (NUM_BINS,) else a for a in (lo, hi))
    for name, a in (('floor', lo), ('ceiling', hi)):
        if a.shape != shape:
            raise ValueError("`%s` must have shape %s, not %s" % (name, shape, a.shape))
        if not ((a >= 0) & (a <= 1)).all():  # (NaN fails both comparisons)
            raise ValueError("`%s` must lie in [0, 1]" % name)
    if (lo > hi).any():
        raise ValueError("`floor` must not be above `ceiling` in any bin")
    return lo + F32(0), hi + F32(0)


def apply(mask, g=0.0, floor=None, ceiling=None):
    """m' float32 [..., 257] of the mask m [..., 257], the minimum gain g (scalar or broadcastable to the mask's leading dimensions) and
    the curves [257] or [..., 257] (None: neutral).  Every operation rounded to float32, in the library's order."""
    m = np.asarray(mask, F32)
    g = np.asarray(g, F32)
    if g.ndim:
        g = g.reshape(g.shape + (1,))
    u = (F32(1.0) - g).astype(F32)
    m1 = (g + (u * m).astype(F32)).astype(F32)
    lo = F32(0) if floor is None else np.asarray(floor, F32)
    hi = F32(1) if ceiling is None else np.asarray(ceiling, F32)
    return np.minimum(hi, np.maximum(lo, m1)).astype(F32)


def _edge(hz, width_hz, rising=True):
    """A raised-cosine step on the bin grid: 0 below hz - width / 2, 1 above hz + width / 2 (rising); the mirror image (falling)."""
    f = np.arange(NUM_BINS, dtype=np.float64) * BIN_HZ
    if width_hz < 0:
        raise ValueError("an edge width is a number of Hz >= 0")
    if width_hz == 0:
        s = (f >= hz).astype(np.float64)
    else:
        x = np.clip((f - (hz - width_hz / 2.0)) / width_hz, 0.0, 1.0)
        s = 0.5 - 0.5 * np.cos(np.pi * x)
    return s if rising else 1.0 - s


def highpass(hz, width_hz=62.5):
    """A ceiling that lets nothing out below `hz`: 0 under the edge, 1 above, a raised-cosine edge `width_hz` wide centred on `hz`."""
    if not 0 <= hz <= 8000:
        raise ValueError("`hz` must lie in [0, 8000]")
    return np.clip(_edge(hz, width_hz), 0.0, 1.0).astype(F32)


def bandpass(lo_hz, hi_hz, width_hz=62.5):
    """A ceiling that is 1 inside [lo_hz, hi_hz] and 0 outside, with raised-cosine edges (300, 3400: the band in front of a G.711 trunk)."""
    if not 0 <= lo_hz < hi_hz <= 8000:
        raise ValueError("a band is 0 <= lo_hz < hi_hz <= 8000")
    return np.clip(_edge(lo_hz, width_hz) * _edge(hi_hz, width_hz, rising=False), 0.0, 1.0).astype(F32)


def depth_limit_db(points, width_hz=62.5):
    """A floor from a depth over frequency: `points` = [(hz, db), ...] with hz ascending, db >= 0 (inf: no limit) -- "at most db dB of
    suppression from hz on", up to the next point; below the first point its depth holds.  Neighbouring steps are joined by raised-cosine
    edges in the gain, `width_hz` wide.  [(0, 6), (300, 18)]: at most 6 dB below 300 Hz, at most 18 dB above."""
    pts = [(float(h), float(d)) for h, d in points]
    if not pts or any(b[0] <= a[0] for a, b in zip(pts, pts[1:])):
        raise ValueError("`points` is a non-empty list of (hz, db) with hz ascending")
    if any(not d >= 0 for _, d in pts):
        raise ValueError("a depth is a number of dB >= 0 (inf: unlimited)")
    gain = [0.0 if np.isinf(d) else 10.0 ** (-d / 20.0) for _, d in pts]
    curve = np.full(NUM_BINS, gain[0], np.float64)
    for (hz, _), g0, g1 in zip(pts[1:], gain, gain[1:]):
        curve = curve + (g1 - g0) * _edge(hz, width_hz)
    return np.clip(curve, 0.0, 1.0).astype(F32)


__all__ = ['NUM_BINS', 'BIN_HZ', 'neutral', 'check', 'apply', 'highpass', 'bandpass', 'depth_limit_db']
