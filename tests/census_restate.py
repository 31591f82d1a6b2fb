"""Reference for StereoSGBM on a census matching cost (mvsv_sgbm_census).

TEST INFRASTRUCTURE ONLY.  Built on oracle/twin.py without editing it, the way
tests/sgbm_color_restate.py is:

* ``census``: the transform, vectorised.  For an odd cw x ch window the offsets run
  dy = -ch/2 .. ch/2 outside and dx = -cw/2 .. cw/2 inside, the centre is skipped, the
  others are numbered k = 0 .. cw*ch - 2 in that order, and bit k of T(y, x) is 1 iff
  I(clamp(y + dy), clamp(x + dx)) < I(y, x);
* ``pixel_cost``: popcount(T_L(y, x) ^ T_R(y, x - d)) over the twin's cost space;
* ``compute``: that cost is substituted for ``twin.sgbm_pixel_cost`` while the twin's
  own cost volume, paths, WTA, LR check, median and speckle filter run.  MODE_HH4 (3)
  goes through tests/hh4_restate.py, which calls ``twin.sgbm_pixel_cost`` too, so the
  two substitutions compose;
* ``pixel_cost_scalar``: a second, independent restatement of the pixel cost -- a
  scalar loop written from the contract that never forms a descriptor: it counts the
  window offsets at which the two comparisons disagree.

The twin computes in int32: it is a reference only while no int16 cost wraps, so
``compute`` asserts ``C.max() <= 32767`` (mvsv_sgbm_census_validate refuses parameters
that could exceed it).
"""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import twin
from tests import hh4_restate as hh4
from tests import sgbm_color_restate as cr

params = cr.params
MODE_HH4 = hh4.MODE_HH4


def window_ok(cw: int, ch: int) -> bool:
    return cw > 0 and ch > 0 and cw % 2 == 1 and ch % 2 == 1 and 3 <= cw * ch <= 65


def offsets(cw: int, ch: int):
    """[(dy, dx)] in bit order: dy outside, dx inside, the centre skipped."""
    return [(dy, dx) for dy in range(-(ch // 2), ch // 2 + 1) for dx in range(-(cw // 2), cw // 2 + 1)
            if (dy, dx) != (0, 0)]


def census(img, cw: int, ch: int) -> np.ndarray:
    """T(y, x) as uint64, (H, W)."""
    assert window_ok(cw, ch)
    I = np.asarray(img)
    assert I.ndim == 2 and I.dtype == np.uint8
    H, W = I.shape
    ys, xs = np.arange(H), np.arange(W)
    T = np.zeros((H, W), np.uint64)
    for k, (dy, dx) in enumerate(offsets(cw, ch)):
        nb = I[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)]
        T |= (nb < I).astype(np.uint64) << np.uint64(k)
    return T


def popcount64(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int32)


def pixel_cost(L, R, e: dict, window) -> np.ndarray:
    """popcount(T_L(y, x) ^ T_R(y, x - d)), (H, W1, D) int32, x in [minX1, maxX1), d in [minD, maxD)."""
    cw, ch = window
    TL, TR = census(L, cw, ch), census(R, cw, ch)
    xs = np.arange(e["minX1"], e["maxX1"])
    ds = np.arange(e["minD"], e["maxD"])
    xr = xs[:, None] - ds[None, :]
    assert xr.size == 0 or (xr.min() >= 0 and xr.max() < TL.shape[1])
    return popcount64(TL[:, xs][:, :, None] ^ TR[:, xr])


def pixel_cost_scalar(L, R, e: dict, window) -> np.ndarray:
    """The same cost, a scalar loop from the contract without descriptors."""
    cw, ch = window
    L = np.asarray(L)
    R = np.asarray(R)
    H, W = L.shape
    offs = offsets(cw, ch)

    def darker(img, y, x):
        c = int(img[y, x])
        return [int(img[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)]) < c for dy, dx in offs]

    pix = np.zeros((H, e["W1"], e["D"]), np.int32)
    for y in range(H):
        right = [darker(R, y, x) for x in range(W)]
        for xi in range(e["W1"]):
            x = xi + e["minX1"]
            a = darker(L, y, x)
            for di in range(e["D"]):
                b = right[x - (di + e["minD"])]
                pix[y, xi, di] = sum(p != q for p, q in zip(a, b))
    return pix


@contextlib.contextmanager
def _census_cost(L, R, window):
    saved = twin.sgbm_pixel_cost
    twin.sgbm_pixel_cost = lambda _l, _r, e: pixel_cost(L, R, e, window)
    try:
        yield
    finally:
        twin.sgbm_pixel_cost = saved


def cost_volume(L, R, p: dict, window, flags: int = 0) -> np.ndarray:
    """C(y, x, d) of the mode: the twin's volume (modes 0, 1) or the clean one (mode 3)."""
    with _census_cost(L, R, window):
        if p["mode"] == MODE_HH4:
            return hh4.clean_volume(L, R, dict(p, mode=0))
        return twin.sgbm_cost_volume(L, R, p, flags)


def compute(L, R, p: dict, window=(9, 7), flags: int = 0) -> np.ndarray:
    """The int16 map of mvsv_sgbm_census for the grey pair (L, R)."""
    L = np.asarray(L)
    R = np.asarray(R)
    assert L.ndim == 2 and L.shape == R.shape and L.dtype == np.uint8 and R.dtype == np.uint8
    assert window_ok(*window)
    e = twin.sgbm_effective(p, L.shape[1])
    if e["minX1"] < e["maxX1"]:
        C = cost_volume(L, R, p, window, flags)
        assert C.max() <= 32767, f"cost {int(C.max())} wraps int16: outside the contract"
    with _census_cost(L, R, window):
        if p["mode"] == MODE_HH4:
            return hh4.compute(L, R, p, flags)
        return twin.sgbm_compute(L, R, p, flags)


def compute_bt(L, R, p: dict, flags: int = 0) -> np.ndarray:
    """The Birchfield-Tomasi map of the same parameters (what the census map is told from)."""
    if p["mode"] == MODE_HH4:
        return hh4.compute(L, R, p, flags)
    return twin.sgbm_compute(L, R, p, flags)


# ---- inputs shared by the CPU and the GPU tests --------------------------------
def noise_shift_pair(seed: int, H: int = 32, W: int = 96, shift: int = 5):
    """Uniform noise in 0..127; the right image is the left one moved `shift` columns left."""
    L = np.random.default_rng(seed).integers(0, 128, (H, W)).astype(np.uint8)
    return L, np.roll(L, -shift, axis=1)


def radiometric(L, R):
    """L -> 2 L and R -> R + 100, both strictly increasing on 0..127: every census
    descriptor stays the same."""
    assert L.max() <= 127 and R.max() <= 127
    return (L.astype(np.int32) * 2).astype(np.uint8), (R.astype(np.int32) + 100).astype(np.uint8)


KNOWN_PARAMS = dict(num_disparities=16, block_size=5, p1=10, p2=120, uniqueness_ratio=5)
KNOWN_WINDOWS = ((9, 7), (5, 5))
KNOWN_MODES = (0, 1, 3)
KNOWN_SEEDS = (1, 2, 3)


def known_region(H, W, D=16):
    """Rows 6 .. H - 7, columns D + 5 + 6 .. W - 7 of the known-answer pairs."""
    return slice(6, H - 6), slice(D + 5 + 6, W - 6)


def grey_pair(seed, H, W, shift=4):
    """A lightly smoothed noise pair with a little per-pixel noise on the right view."""
    rng = np.random.default_rng(seed)
    Lg = rng.integers(0, 256, (H, W)).astype(np.uint8)
    Lg = ((Lg.astype(int) + np.roll(Lg, 1, axis=1)) // 2).astype(np.uint8)
    Rg = np.roll(Lg, -shift, axis=1)
    Rg = np.clip(Rg.astype(int) + rng.integers(-3, 4, Rg.shape), 0, 255).astype(np.uint8)
    return Lg, Rg


# ---- the committed fixture (tests/golden/census_fixtures.npz) --------------------
# (seed, H, W, shift, window, params): pairs no larger than 64 x 24
FIXTURE_CASES = (
    (11, 24, 64, 4, (9, 7), dict(num_disparities=16, block_size=5, p1=10, p2=120, uniqueness_ratio=10, mode=0)),
    (12, 17, 60, 3, (5, 5), dict(min_disparity=-3, num_disparities=16, block_size=3, p1=3, p2=12, mode=1)),
    (13, 20, 64, 6, (7, 9), dict(min_disparity=5, num_disparities=16, block_size=7, p1=72, p2=288,
                                 speckle_window_size=20, speckle_range=2, mode=3)),
    (14, 9, 63, 2, (3, 3), dict(num_disparities=32, block_size=1, uniqueness_ratio=10, mode=0)),
    (15, 24, 64, 5, (13, 5), dict(num_disparities=16, block_size=5, p1=10, p2=120, uniqueness_ratio=5, mode=1)),
    (16, 12, 64, 4, (1, 3), dict(num_disparities=16, block_size=3, p1=2, p2=5, disp12_max_diff=2, mode=3)),
    (17, 2, 40, 3, (3, 1), dict(num_disparities=16, block_size=3, p1=8, p2=32, mode=0)),
)


def fixture_arrays() -> dict:
    out = {"count": np.int32(len(FIXTURE_CASES))}
    for k, (seed, H, W, shift, window, kw) in enumerate(FIXTURE_CASES):
        L, R = grey_pair(seed, H, W, shift)
        p = params(**kw)
        out[f"L{k}"], out[f"R{k}"] = L, R
        out[f"params{k}"] = np.array([p[n] for n in cr.PARAM_NAMES], np.int32)
        out[f"window{k}"] = np.array(window, np.int32)
        out[f"map{k}"] = compute(L, R, p, window)
    return out


if __name__ == "__main__":  # python -m tests.census_restate: rewrites the fixture
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "census_fixtures.npz")
    np.savez_compressed(path, **fixture_arrays())
    print(path, os.path.getsize(path), "bytes")
