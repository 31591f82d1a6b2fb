"""Reference for StereoSGBM on 3-channel pairs (OpenCV 3.4 calcPixelCostBT, cn == 3).

TEST INFRASTRUCTURE ONLY.  Built on oracle/twin.py without editing it:

* ``pixel_cost``: the colour pixel cost is the sum over the channels of the twin's
  grey pixel cost (the ``>> 2`` of the raw plane is applied per plane, so the sum
  of the three grey costs is exact);
* ``compute_bgr``: that cost is substituted for ``twin.sgbm_pixel_cost`` while the
  twin's own cost volume (box sums, ``+ P2`` once, the never-refreshed column and
  rows), paths, WTA, LR check, median and speckle filter run.  The three *volumes*
  are not added: each would carry its own ``+ P2``;
* ``pixel_cost_planes``: a second, independent restatement of the pixel cost, a
  scalar loop written from the ``cn * 2``-plane form of calcPixelCostBT: planes
  0-2 are the channels' clipped x-Sobel rows, planes 3-5 the raw channels with
  ``>> 2``, and all twelve row ends equal ``tab[0]`` = ftzero.

The twin computes in int32: it is a reference only while no int16 cost wraps, so
``compute_bgr`` asserts ``C.max() <= 32767`` and refuses inputs beyond it.
"""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import twin

PARAM_NAMES = ("min_disparity", "num_disparities", "block_size", "p1", "p2", "disp12_max_diff",
               "pre_filter_cap", "uniqueness_ratio", "speckle_window_size", "speckle_range", "mode")


_grey_pixel_cost = twin.sgbm_pixel_cost  # the twin's own, whatever is substituted meanwhile


def params(**kw) -> dict:
    """A full parameter dict (oracle / twin names); everything not given is 0, D 16, block 3."""
    p = dict.fromkeys(PARAM_NAMES, 0)
    p.update(num_disparities=16, block_size=3)
    p.update(kw)
    return p


def _check(L, R):
    L = np.asarray(L)
    R = np.asarray(R)
    assert L.ndim == 3 and L.shape[2] == 3 and L.shape == R.shape
    assert L.dtype == np.uint8 and R.dtype == np.uint8
    return L, R


def pixel_cost(L, R, e: dict) -> np.ndarray:
    """Sum over the colour channels of the twin's BT pixel cost, (H, W1, D) int32."""
    L, R = _check(L, R)
    return sum(_grey_pixel_cost(L[:, :, c], R[:, :, c], e) for c in range(3))


def pixel_cost_planes(L, R, e: dict) -> np.ndarray:
    """The same cost as a scalar loop over calcPixelCostBT's six planes."""
    L, R = _check(L, R)
    H, W, cn = L.shape
    ftzero = e["ftzero"]
    tab0 = ftzero

    def planes(img, y):
        """[cn * 2][W] ints of row y: Sobel planes 0 .. cn-1, raw planes cn .. 2cn-1."""
        yn, ys = max(y - 1, 0), min(y + 1, H - 1)
        out = [[tab0] * W for _ in range(2 * cn)]
        for x in range(1, W - 1):
            for c in range(cn):
                g = ((int(img[y, x + 1, c]) - int(img[y, x - 1, c])) * 2
                     + int(img[yn, x + 1, c]) - int(img[yn, x - 1, c])
                     + int(img[ys, x + 1, c]) - int(img[ys, x - 1, c]))
                out[c][x] = min(max(g, -ftzero), ftzero) + ftzero
                out[c + cn][x] = int(img[y, x, c])
        return out

    def interval(row, x):
        v = row[x]
        a = (v + row[x - 1]) // 2 if x > 0 else v
        b = (v + row[x + 1]) // 2 if x < W - 1 else v
        return min(a, b, v), max(a, b, v)

    pix = np.zeros((H, e["W1"], e["D"]), np.int32)
    for y in range(H):
        pl, pr = planes(L, y), planes(R, y)
        for k in range(2 * cn):
            shift = 0 if k < cn else 2
            lrow, rrow = pl[k], pr[k]
            for xi in range(e["W1"]):
                x = xi + e["minX1"]
                u = lrow[x]
                u0, u1 = interval(lrow, x)
                for di in range(e["D"]):
                    xr = x - (di + e["minD"])
                    v = rrow[xr]
                    v0, v1 = interval(rrow, xr)
                    c0 = max(0, u - v1, v0 - u)
                    c1 = max(0, v - u1, u0 - v)
                    pix[y, xi, di] += min(c0, c1) >> shift
    return pix


@contextlib.contextmanager
def _colour_cost(L, R):
    saved = twin.sgbm_pixel_cost
    twin.sgbm_pixel_cost = lambda _l, _r, e: pixel_cost(L, R, e)
    try:
        yield
    finally:
        twin.sgbm_pixel_cost = saved


def cost_volume(L, R, p: dict, flags: int = 0) -> np.ndarray:
    """C(y, x, d) of the colour pair: the twin's volume on the summed pixel cost."""
    L, R = _check(L, R)
    with _colour_cost(L, R):
        return twin.sgbm_cost_volume(L[:, :, 0], R[:, :, 0], p, flags)


def compute_bgr(L, R, p: dict, flags: int = 0) -> np.ndarray:
    """The int16 map cv::StereoSGBM::compute gives for the CV_8UC3 pair (L, R)."""
    L, R = _check(L, R)
    e = twin.sgbm_effective(p, L.shape[1])
    if e["minX1"] < e["maxX1"]:
        C = cost_volume(L, R, p, flags)
        assert C.max() <= 32767, \
            f"cost {int(C.max())} wraps int16: outside the twin's range (use the grey-oracle identity)"
    with _colour_cost(L, R):
        return twin.sgbm_compute(L[:, :, 0], R[:, :, 0], p, flags)


def one_live_channel(Lg, Rg, channel: int, ftzero: int):
    """The colour pair whose channel `channel` is the grey pair and whose other two
    channels are the constant ftzero in both images: constant ftzero planes cost 0
    (their Sobel rows are ftzero everywhere, their raw rows too, forced ends
    included), so the pair has exactly the grey pair's pixel cost."""
    L = np.full(Lg.shape + (3,), ftzero, np.uint8)
    R = np.full(Rg.shape + (3,), ftzero, np.uint8)
    L[:, :, channel] = Lg
    R[:, :, channel] = Rg
    return L, R
