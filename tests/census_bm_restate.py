"""Reference for StereoBM on a census matching cost (mvsv_bm_census).

TEST INFRASTRUCTURE ONLY.  Written from the contract on top of tests/census_restate.py
and oracle/twin.py, without editing either:

* descriptors: ``census_restate.census``; Hamming distance: ``census_restate.popcount64``;
* ``window_cost``: the blockSize^2 sum of popcount(T_L(y, xl) ^ T_R(y, xr)) for every
  output row, virtual column and disparity index, with closed-form (integral image) sums
  over the clamped virtual columns j = x - lofs: left column lofs + clamp(j, -lofs,
  W - 1 - lofs), right column rofs + clamp(j, -rofs, W - nd - rofs) + k;
* ``window_cost_scalar``: a second, independent restatement of the same numbers -- a
  scalar loop that never forms a descriptor: per (y, x, k) it walks the block and the
  census window and counts the comparisons on which the two views disagree;
* ``compute``: argmin over k (ties -> smallest index), uniqueness test, parabola fit,
  FILTERED, ``twin._bm_validate`` on the minimum-cost map, the valid rectangle and
  ``twin.filter_speckles`` with BM's unscaled maxDiff.  ``twin.bm_compute`` cannot be
  substituted into (its SAD is inline), so the decision part is restated here.

pre_filter_type, pre_filter_size, pre_filter_cap and texture_threshold are not read.
"""
from __future__ import annotations

import numpy as np

from oracle import twin
from tests import census_restate as cs

PARAM_NAMES = ("pre_filter_type", "pre_filter_size", "pre_filter_cap", "block_size", "min_disparity",
               "num_disparities", "texture_threshold", "uniqueness_ratio", "speckle_window_size", "speckle_range",
               "disp12_max_diff")


def params(**kw) -> dict:
    """StereoBM::create(64, 21)'s values (mvsv_bm_params_default) with overrides."""
    p = dict(pre_filter_type=1, pre_filter_size=9, pre_filter_cap=31, block_size=21, min_disparity=0,
             num_disparities=64, texture_threshold=10, uniqueness_ratio=15, speckle_window_size=0, speckle_range=0,
             disp12_max_diff=-1)
    assert set(kw) <= set(p), set(kw) - set(p)
    p.update(kw)
    return p


def geometry(p: dict, W: int, H: int):
    """None where the call only fills the map, else the ranges of findStereoCorrespondenceBM."""
    nd, mind0 = p["num_disparities"], p["min_disparity"]
    lofs = max(nd - 1 + mind0, 0)
    rofs = -min(nd - 1 + mind0, 0)
    width1 = W - rofs - nd + 1
    if lofs >= W or rofs >= W or width1 < 1:
        return None
    w2 = p["block_size"] // 2
    xmin = max(0, mind0 + nd - 1) + w2
    xmax, ymin, ymax = W - w2, w2, H - w2
    ncol = min(width1, W - lofs)
    if xmax - xmin <= 0 or ymax - ymin <= 0 or ncol <= 0:
        return None
    return dict(nd=nd, mind0=mind0, lofs=lofs, rofs=rofs, width1=width1, w2=w2, xmin=xmin, xmax=xmax, ymin=ymin,
                ymax=ymax, ncol=ncol)


def column_pairs(g: dict, W: int):
    """(cl, cr): image columns of the virtual columns j = -w2 .. width1 + w2 - 1; the right
    column of disparity index k is cr + k."""
    j = np.arange(-g["w2"], g["width1"] + g["w2"])
    cl = g["lofs"] + np.clip(j, -g["lofs"], W - 1 - g["lofs"])
    cr = g["rofs"] + np.clip(j, -g["rofs"], W - g["nd"] - g["rofs"])
    return cl, cr


def window_cost(L, R, p: dict, window) -> np.ndarray:
    """(ymax - ymin, width1, nd) int64 window sums; requires geometry(...) is not None."""
    H, W = L.shape
    g = geometry(p, W, H)
    cw, ch = window
    TL, TR = cs.census(L, cw, ch), cs.census(R, cw, ch)
    cl, cr = column_pairs(g, W)
    rows = np.arange(g["ymin"] - g["w2"], g["ymax"] + g["w2"])
    Lc = TL[rows][:, cl]
    n = 2 * g["w2"] + 1
    out = np.zeros((g["ymax"] - g["ymin"], g["width1"], g["nd"]), np.int64)
    for k in range(g["nd"]):
        A = cs.popcount64(Lc ^ TR[rows][:, cr + k]).astype(np.int64)
        ii = np.cumsum(np.pad(A, ((1, 0), (1, 0))), axis=0).cumsum(axis=1)
        out[:, :, k] = ii[n:, n:] - ii[:-n, n:] - ii[n:, :-n] + ii[:-n, :-n]
    return out


def window_cost_scalar(L, R, p: dict, window) -> np.ndarray:
    """The same numbers by a scalar loop over block and census window, no descriptors."""
    L = np.asarray(L)
    R = np.asarray(R)
    H, W = L.shape
    g = geometry(p, W, H)
    offs = cs.offsets(*window)
    w2, nd, lofs, rofs = g["w2"], g["nd"], g["lofs"], g["rofs"]

    def darker(img, y, x):
        c = int(img[y, x])
        return tuple(int(img[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)]) < c for dy, dx in offs)

    dl = [[darker(L, y, x) for x in range(W)] for y in range(H)]
    dr = [[darker(R, y, x) for x in range(W)] for y in range(H)]
    out = np.zeros((g["ymax"] - g["ymin"], g["width1"], nd), np.int64)
    for yi, y in enumerate(range(g["ymin"], g["ymax"])):
        for x in range(g["width1"]):
            for k in range(nd):
                tot = 0
                for j in range(x - w2, x + w2 + 1):
                    xl = lofs + min(max(j, -lofs), W - 1 - lofs)
                    xr = rofs + min(max(j, -rofs), W - nd - rofs) + k
                    for yy in range(y - w2, y + w2 + 1):
                        a, b = dl[yy][xl], dr[yy][xr]
                        tot += sum(s != t for s, t in zip(a, b))
                out[yi, x, k] = tot
    return out


def compute(L, R, p: dict, window=(9, 7)) -> np.ndarray:
    """The int16 map of mvsv_bm_census for the grey pair (L, R)."""
    L = np.asarray(L)
    R = np.asarray(R)
    assert L.ndim == 2 and L.shape == R.shape and L.dtype == np.uint8 and R.dtype == np.uint8
    assert cs.window_ok(*window)
    H, W = L.shape
    nd, mind0 = p["num_disparities"], p["min_disparity"]
    FILTERED = (mind0 - 1) * 16
    out = np.full((H, W), FILTERED, np.int64)
    g = geometry(p, W, H)
    if g is None:
        return out.astype(np.int16)
    sad = window_cost(L, R, p, window)
    mind = np.argmin(sad, axis=-1)  # the first minimum
    minsad = sad.min(axis=-1)
    kk = np.arange(nd)
    filt = np.zeros(mind.shape, bool)
    if p["uniqueness_ratio"] > 0:
        thresh = minsad + (minsad * p["uniqueness_ratio"] // 100)
        far = (kk < mind[..., None] - 1) | (kk > mind[..., None] + 1)
        filt |= (far & (sad <= thresh[..., None])).any(axis=-1)
    pp = np.take_along_axis(sad, np.clip(mind + 1, 0, nd - 1)[..., None], -1)[..., 0]
    nn = np.take_along_axis(sad, np.clip(mind - 1, 0, nd - 1)[..., None], -1)[..., 0]
    inner = (mind > 0) & (mind < nd - 1)
    v1 = nd - mind - 1 + mind0
    num = np.where(inner, pp - nn, 0) * 256
    dd = np.where(inner, pp + nn - 2 * minsad + np.abs(pp - nn), 0)
    safe = np.where(dd != 0, dd, 1)
    q = np.where(dd != 0, np.sign(num) * (np.abs(num) // safe), 0)  # C division: towards zero
    disp = np.where(filt, FILTERED, (v1 * 256 + q + 15) >> 4)
    ncol, lofs, ymin, ymax = g["ncol"], g["lofs"], g["ymin"], g["ymax"]
    out[ymin:ymax, lofs:lofs + ncol] = disp[:, :ncol]
    if p["disp12_max_diff"] >= 0:
        cost = np.zeros((H, W), np.int64)
        cost[ymin:ymax, lofs:lofs + ncol] = minsad[:, :ncol]
        twin._bm_validate(out, cost, ymin, ymax, mind0, nd, p["disp12_max_diff"])
    out[ymin:ymax, :g["xmin"]] = FILTERED
    out[ymin:ymax, g["xmax"]:] = FILTERED
    out = out.astype(np.int16)
    if p["speckle_range"] >= 0 and p["speckle_window_size"] > 0:
        out = twin.filter_speckles(out, FILTERED, p["speckle_window_size"], p["speckle_range"])
    return out


# ---- inputs shared by the CPU and the GPU tests --------------------------------
KNOWN_SEEDS = (1, 2, 3)
KNOWN_WINDOWS = ((9, 7), (5, 5), (3, 3))
KNOWN_BLOCKS = (5, 9, 21)
KNOWN_D, KNOWN_SHIFT, KNOWN_W = 16, 5, 96


def known_pair(seed: int, block_size: int):
    return cs.noise_shift_pair(seed, 48 if block_size == 21 else 32, KNOWN_W, KNOWN_SHIFT)


def known_params(block_size: int) -> dict:
    return params(num_disparities=KNOWN_D, block_size=block_size, uniqueness_ratio=15)


def known_region(H, W, block_size, window):
    """Rows [w2 + ch/2, H - w2 - ch/2), columns [D - 1 + w2 + cw/2, W - w2 - cw/2 - shift): every
    descriptor of the block is computed away from the image border and from the wrap of
    np.roll."""
    w2, (cw, ch) = block_size // 2, window
    return (slice(w2 + ch // 2, H - w2 - ch // 2),
            slice(KNOWN_D - 1 + w2 + cw // 2, W - w2 - cw // 2 - KNOWN_SHIFT))


def low_contrast_pair(seed: int, H: int = 32, W: int = 96, shift: int = 5):
    """Noise in 0..15 and the same pair as a rig with unequal gain and offset would see it
    (L -> 4 L, R -> R + 100, both strictly increasing)."""
    L = np.random.default_rng(seed).integers(0, 16, (H, W)).astype(np.uint8)
    R = np.roll(L, -shift, axis=1)
    return (L, R), ((L.astype(np.int32) * 4).astype(np.uint8), (R.astype(np.int32) + 100).astype(np.uint8))


# ---- the committed fixture (tests/golden/census_bm_fixtures.npz) -----------------
# (seed, H, W, shift, window, params): pairs no larger than 64 x 24
FIXTURE_CASES = (
    (21, 24, 64, 4, (9, 7), dict(num_disparities=16, block_size=5, uniqueness_ratio=15)),
    (22, 17, 60, 3, (5, 5), dict(min_disparity=-5, num_disparities=16, block_size=7, uniqueness_ratio=0,
                                 disp12_max_diff=1)),
    (23, 24, 64, 6, (7, 9), dict(min_disparity=3, num_disparities=32, block_size=9, uniqueness_ratio=10,
                                 speckle_window_size=20, speckle_range=2, disp12_max_diff=0)),
    (24, 23, 63, 2, (3, 3), dict(num_disparities=16, block_size=21, uniqueness_ratio=5)),
    (25, 24, 64, 5, (13, 5), dict(num_disparities=48, block_size=5, uniqueness_ratio=15, disp12_max_diff=2)),
    (26, 12, 64, 4, (1, 3), dict(num_disparities=16, block_size=5, uniqueness_ratio=0, texture_threshold=500)),
    (27, 9, 40, 3, (3, 1), dict(min_disparity=-20, num_disparities=16, block_size=5, uniqueness_ratio=15)),
)


def fixture_arrays() -> dict:
    out = {"count": np.int32(len(FIXTURE_CASES))}
    for k, (seed, H, W, shift, window, kw) in enumerate(FIXTURE_CASES):
        L, R = cs.grey_pair(seed, H, W, shift)
        p = params(**kw)
        out[f"L{k}"], out[f"R{k}"] = L, R
        out[f"params{k}"] = np.array([p[n] for n in PARAM_NAMES], np.int32)
        out[f"window{k}"] = np.array(window, np.int32)
        out[f"map{k}"] = compute(L, R, p, window)
    return out


if __name__ == "__main__":  # python -m tests.census_bm_restate: rewrites the fixture
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "census_bm_fixtures.npz")
    np.savez_compressed(path, **fixture_arrays())
    print(path, os.path.getsize(path), "bytes")
