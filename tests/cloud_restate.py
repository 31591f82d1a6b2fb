"""Plain numpy restatement of the point cloud: the loop of Utility::dmap2pcl
(src/utility.cpp:248-259: every pixel with v > 0, row by row) with the grey
ply::write prints in WITH_COLOR mode (src/ply.cpp:90).

Coordinates come from the oracle's reproject (Utility::calcCoordinate per pixel);
compaction is a boolean mask in C order.  The grey is
int((z - (float)mn) / (float)(mx - mn) * 255.0) with mn / mx over the values > 0:
the difference and the quotient are np.float32 operations, the product is float64,
the conversion truncates; NaN and values outside int32 give INT32_MIN (what the
x86-64 conversion yields).  grey_f64 and grey_recip are the two near misses a
kernel can fall into: the same formula wholly in double, and the division
replaced by a multiplication with the reciprocal.
"""
import numpy as np

CLOUD_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("grey", "i4")])
INT32_MIN = -2 ** 31
INVALID = -16  # SGBM's marker (minDisparity - 1) * 16


def minmax(d):
    v = d[d > 0]
    if v.size == 0:
        return 32767, -32768
    return int(v.min()), int(v.max())


def _to_int32(t):
    """Truncation of a float64 array; INT32_MIN for NaN and what int32 cannot hold."""
    ok = np.isfinite(t) & (t > -2147483649.0) & (t < 2147483648.0)
    g = np.full(t.shape, INT32_MIN, np.int64)
    g[ok] = np.trunc(t[ok]).astype(np.int64)
    return g.astype(np.int32)


def grey(z, mn, mx):
    z = np.asarray(z, np.float32)
    with np.errstate(all="ignore"):
        num = z - np.float32(mn)
        q = num / np.float32(mx - mn)
        assert num.dtype == np.float32 and q.dtype == np.float32
        return _to_int32(q.astype(np.float64) * 255.0)


def grey_f64(z, mn, mx):
    z = np.asarray(z, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return _to_int32((z - float(mn)) / np.float64(mx - mn) * 255.0)


def grey_recip(z, mn, mx):
    z = np.asarray(z, np.float32)
    with np.errstate(all="ignore"):
        r = np.float32(1.0) / np.float32(mx - mn)
        q = (z - np.float32(mn)) * r
        assert q.dtype == np.float32
        return _to_int32(q.astype(np.float64) * 255.0)


def cloud(d, Q, reproject, grey_fn=grey):
    """(records, (mn, mx)) of one int16 map; reproject: oracle.reproject."""
    assert d.dtype == np.int16 and d.ndim == 2
    d = np.ascontiguousarray(d)
    pts = reproject(d, Q)
    xyz = pts[d > 0][:, :3]  # boolean mask: C order = raster order
    mn, mx = minmax(d)
    rec = np.zeros(len(xyz), CLOUD_DTYPE)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if len(xyz):
        rec["grey"] = grey_fn(xyz[:, 2], mn, mx)
    return rec, (mn, mx)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def ladder(lo, hi, shape):
    """Every value lo..hi once, in a map of `shape` whose other pixels alternate
    between the invalid marker and 0 -- spread over the map, not in a block."""
    n = shape[0] * shape[1]
    assert hi - lo + 1 <= n
    d = np.where(np.arange(n) % 2 == 0, INVALID, 0).astype(np.int16)
    at = (np.arange(hi - lo + 1, dtype=np.int64) * n) // (hi - lo + 1)
    d[at] = np.arange(lo, hi + 1, dtype=np.int64).astype(np.int16)
    return d.reshape(shape)


def random_map(seed, shape, valid=0.5, hi=4000):
    """About `valid` of the pixels positive (1..hi), the others -16 or 0."""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, hi + 1, size=shape).astype(np.int16)
    off = rng.random(shape) >= valid
    d[off] = np.where(rng.random(shape) < 0.5, INVALID, 0).astype(np.int16)[off]
    return d
