"""Plain numpy restatement of the display map: OpenCV 3.4's
cv::normalize(src, dst, alpha, beta, NORM_MINMAX, CV_8U) for a CV_16S source
(normalize -> Mat::convertTo, its SSE2 / scalar form).

scale and shift are Python floats (IEEE double, every operation rounded on its
own); the two per-pixel operations run on float32 arrays, so the product and the
sum round separately; np.rint rounds half to even.  normalize_f64 and
normalize_fused are the two near misses a kernel can fall into: the same formula
evaluated wholly in double, and the product fused into the sum.
"""
import sys

import numpy as np

DBL_EPSILON = sys.float_info.epsilon


def scale_shift(smin, smax, alpha=0.0, beta=255.0):
    dmin, dmax = min(float(alpha), float(beta)), max(float(alpha), float(beta))
    rng = float(smax) - float(smin)
    recip = 1.0 / rng if rng > DBL_EPSILON else 0.0
    scale = (dmax - dmin) * recip
    prod = float(smin) * scale
    return scale, dmin - prod


def minmax(d, positive_only=False):
    v = d[d > 0] if positive_only else d.reshape(-1)
    if v.size == 0:
        return 32767, -32768
    return int(v.min()), int(v.max())


def normalize(d, alpha=0.0, beta=255.0):
    """(uint8 map, (smin, smax)) of one int16 map."""
    assert d.dtype == np.int16 and d.ndim == 2
    smin, smax = minmax(d)
    scale, shift = scale_shift(smin, smax, alpha, beta)
    sf, hf = np.float32(scale), np.float32(shift)
    p = d.astype(np.float32) * sf
    t = p + hf
    assert p.dtype == np.float32 and t.dtype == np.float32
    return np.clip(np.rint(t), 0, 255).astype(np.uint8), (smin, smax)


def normalize_f64(d, alpha=0.0, beta=255.0):
    scale, shift = scale_shift(*minmax(d), alpha, beta)
    t = d.astype(np.float64) * scale + shift
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def normalize_fused(d, alpha=0.0, beta=255.0):
    """fmaf(v, sf, hf): the float32 product is exact in double, the sum is rounded once."""
    scale, shift = scale_shift(*minmax(d), alpha, beta)
    sf, hf = np.float32(scale), np.float32(shift)
    t = (d.astype(np.float64) * np.float64(sf) + np.float64(hf)).astype(np.float32)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def ladder(lo, hi, shape=None):
    """Every value lo..hi, repeated to fill `shape` (rows, cols); one row without."""
    v = np.arange(lo, hi + 1, dtype=np.int64).astype(np.int16)
    if shape is None:
        return v.reshape(1, -1)
    assert shape[0] * shape[1] >= v.size
    return np.resize(v, shape)
