"""Reference for StereoSGBM MODE_HH4 (OpenCV computeDisparitySGBM_HH4, restated from recall).

TEST INFRASTRUCTURE ONLY.  Built on oracle/twin.py without editing it.  MODE_HH4 is
the twin's pipeline with two substitutions:

* ``clean_volume``: C(y, x, d) = P2 + the clamp-to-edge box sum of the pixel cost,
  with neither OpenCV 3.4 cost-row quirk (column 0 of rows >= 1 and the bottom SH2
  rows are computed like every other cell), in place of ``twin.sgbm_cost_volume``;
* ``DIRECTIONS``: the four axis directions L->R, down, up, R->L in place of
  ``twin.sgbm_directions``.

Meanwhile the twin runs with ``mode = 0``: the WTA is fused with the R->L pass as in
MODE_SGBM, so the tie rule is MODE_SGBM's (the 3.4 lane rule, or the smallest d
under flag 2).  Flag 1 (FIRSTCOL_FIX) has no effect: there is no quirk to fix.
Everything else -- pixel cost, recurrence, uniqueness, sub-pixel fit, LR check,
median, speckle filter -- is the twin's own.

``compute_bgr`` nests the substitution of tests/sgbm_color_restate.py (the pixel cost
summed over the channels) for 3-channel pairs.

The twin computes in int32: it is a reference only while no int16 cost wraps, so
``compute`` asserts ``C.max() <= 32767`` like its colour sibling.
"""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import twin
from tests import sgbm_color_restate as cr

MODE_HH4 = 3
# predecessor offsets (dx, dy) in twin.sgbm_path's convention
DIRECTIONS = ((1, 0), (0, 1), (0, -1), (-1, 0))

params = cr.params


def clean_volume(L, R, p: dict) -> np.ndarray:
    """C(y, x, d) = P2 + sum_{|i| <= SH2} sum_{|j| <= SW2} pix(clamp(y + i), clamp(x + j), d)."""
    H, W = L.shape
    e = twin.sgbm_effective(p, W)
    pix = twin.sgbm_pixel_cost(L, R, e)  # (whatever pixel cost is substituted meanwhile)
    W1, SW2, SH2 = e["W1"], e["SW2"], e["SH2"]
    xi, yi = np.arange(W1), np.arange(H)
    hs = np.zeros_like(pix)
    for k in range(-SW2, SW2 + 1):
        hs += pix[:, np.clip(xi + k, 0, W1 - 1), :]
    C = np.full_like(pix, e["P2"])
    for k in range(-SH2, SH2 + 1):
        C += hs[np.clip(yi + k, 0, H - 1)]
    return C


def _as_mode0(p: dict) -> dict:
    assert p["mode"] == MODE_HH4, "hh4_restate restates MODE_HH4 only"
    return dict(p, mode=0)


@contextlib.contextmanager
def _hh4():
    saved = twin.sgbm_cost_volume, twin.sgbm_directions
    twin.sgbm_cost_volume = lambda L, R, p, flags=0: clean_volume(L, R, p)
    twin.sgbm_directions = lambda mode: list(DIRECTIONS)
    try:
        yield
    finally:
        twin.sgbm_cost_volume, twin.sgbm_directions = saved


def _check_range(L, R, p0):
    e = twin.sgbm_effective(p0, L.shape[1])
    if e["minX1"] < e["maxX1"]:
        C = clean_volume(L, R, p0)
        assert C.max() <= 32767, f"cost {int(C.max())} wraps int16: outside the twin's range"


def aggregate(C: np.ndarray, P1: int, P2: int) -> np.ndarray:
    """S = min(sum of the four path costs, 32767) on the twin's vectorised path scan."""
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS:
        S += twin.sgbm_path(C, dx, dy, P1, P2)
    return np.minimum(S, twin.MAX_COST)


def core(L, R, p: dict, flags: int = 0) -> np.ndarray:
    """The map before the post filters (computeDisparitySGBM_HH4's output)."""
    p0 = _as_mode0(p)
    _check_range(L, R, p0)
    with _hh4():
        return twin.sgbm_core(L, R, p0, flags)


def compute(L, R, p: dict, flags: int = 0) -> np.ndarray:
    """The int16 map cv::StereoSGBM::compute gives in MODE_HH4 for the grey pair (L, R)."""
    p0 = _as_mode0(p)
    _check_range(L, R, p0)
    with _hh4():
        return twin.sgbm_compute(L, R, p0, flags)


def compute_bgr(L, R, p: dict, flags: int = 0) -> np.ndarray:
    """The same for a CV_8UC3 pair: the colour pixel cost under the HH4 substitutions."""
    p0 = _as_mode0(p)
    with cr._colour_cost(L, R):
        _check_range(L[:, :, 0], R[:, :, 0], p0)
        with _hh4():
            return twin.sgbm_compute(L[:, :, 0], R[:, :, 0], p0, flags)


# ---- inputs shared by the CPU and the GPU tests --------------------------------
def rand_pair(rng, H, W, shift, kind):
    """tests/test_gpu_parity.py's rand_pair (kind 0: a 3x3 mean of noise, 1: low
    texture, 2: noise), restated without scipy so that the CPU tests need only numpy."""
    if kind == 0:
        n = rng.integers(0, 256, (H, W)).astype(float)
        P = np.pad(n, 1, mode="symmetric")  # scipy.ndimage.uniform_filter's default 'reflect'
        L = (sum(P[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0).round().astype(np.uint8)
    elif kind == 1:
        L = (rng.integers(0, 4, (H, W)) * 60).astype(np.uint8)
        L[:, W // 3:W // 2] = 128
    else:
        L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R = np.roll(L, -shift, axis=1)
    R = np.clip(R.astype(int) + rng.integers(-2, 3, R.shape), 0, 255).astype(np.uint8)
    return L, R


RANDOM_SEEDS = tuple(range(16))


def random_case(seed: int):
    """(L, R, params, variant) of random case `seed`: the draw order is fixed (the
    speckle parameters and the variant come after the pair), test_hh4_restate.py
    checks that every case tells MODE_HH4 from MODE_SGBM and from MODE_HH."""
    rng = np.random.default_rng(4400 + seed)
    H, W = int(rng.integers(12, 70)), int(rng.integers(48, 120))
    D = int(rng.choice([16, 32, 48, 64]))
    minD = int(rng.integers(-6, 6))
    bs = int(rng.choice([0, 1, 3, 5, 7, 9, 11]))
    p1 = int(rng.choice([0, 2, 72, 300]))
    p2 = int(rng.choice([0, 5, 288, 2000, 4000]))
    disp12 = int(rng.integers(-1, 4))
    cap = int(rng.choice([0, 15, 31, 63]))
    uniq = int(rng.choice([-1, 0, 5, 15]))
    if W + min(minD, 0) - max(minD + D, 0) <= max(bs, 5) // 2:
        D = 16  # as tests/test_gpu_parity.py: keep the cost space wider than the block half-width
    L, R = rand_pair(rng, H, W, int(rng.integers(0, 16)), int(rng.integers(0, 3)))
    sw = int(rng.choice([0, 10, 50]))
    sr = int(rng.choice([1, 2, 4]))
    variant = int(rng.integers(0, 4))
    p = params(min_disparity=minD, num_disparities=D, block_size=bs, p1=p1, p2=p2, disp12_max_diff=disp12,
               pre_filter_cap=cap, uniqueness_ratio=uniq, speckle_window_size=sw, speckle_range=sr, mode=MODE_HH4)
    return L, R, p, variant


def shift_pair(W, H, s):
    """A noise-free constant-shift pair: R is L moved s columns to the left."""
    n = np.random.default_rng(W).integers(0, 256, (H + 2, W + s + 2))
    b = sum(n[i:i + H, j:j + W + s] for i in range(3) for j in range(3))
    b = ((2 * b + 9) // 18).astype(np.uint8)
    return np.ascontiguousarray(b[:, :W]), np.ascontiguousarray(b[:, s:s + W])


# (W, H, D, bs, P1, P2, s)
SHIFT_CASES = ((101, 37, 16, 5, 200, 800, 7), (120, 40, 32, 9, 0, 0, 11), (200, 40, 128, 13, 0, 0, 40),
               (150, 45, 64, 9, 648, 2592, 20), (300, 24, 256, 9, 648, 2592, 100))


def period7_pair():
    """Period-7 columns: every disparity congruent mod 7 costs the same, so the WTA
    tie rule decides (variant 0: the 3.4 lane rule, variant 2: the smallest d)."""
    T = np.random.default_rng(732).integers(0, 256, (20, 7))
    L = T[:, np.arange(90) % 7].astype(np.uint8)
    R = np.roll(L, -3, axis=1)
    return L, R, params(num_disparities=32, block_size=5, mode=MODE_HH4)
