"""StereoSGBM on colour pairs: the reference restatements against each other and
against the C oracle, and the argument rules of the host mirror (no GPU)."""
import ctypes

import numpy as np
import pytest

from oracle import twin
from tests import sgbm_color_restate as cr


def rand_bgr_pair(rng, H, W, shift):
    L = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    R = np.roll(L, -shift, axis=1)
    R = np.clip(R.astype(int) + rng.integers(-3, 4, R.shape), 0, 255).astype(np.uint8)
    return L, R


@pytest.mark.parametrize("H,W,minD,D,cap", [(5, 40, 0, 16, 0), (3, 37, -3, 16, 31), (4, 56, 5, 32, 63),
                                             (1, 30, 0, 16, 63)])
def test_pixel_cost_restatements_agree(H, W, minD, D, cap):
    rng = np.random.default_rng(H * 1000 + W)
    L, R = rand_bgr_pair(rng, H, W, 4)
    e = twin.sgbm_effective(cr.params(min_disparity=minD, num_disparities=D, pre_filter_cap=cap), W)
    a = cr.pixel_cost(L, R, e)
    b = cr.pixel_cost_planes(L, R, e)
    assert a.shape == (H, e["W1"], D)
    assert np.array_equal(a, b)
    assert a.max() <= 3 * (2 * e["ftzero"] + 63)


def test_pixel_cost_reaches_beyond_the_grey_bound():
    # black against white: every interior Sobel plane is flat (ftzero against ftzero), every
    # raw plane costs 255 >> 2 = 63 -- three of them, where a grey pair has one
    L = np.zeros((4, 40, 3), np.uint8)
    R = np.full((4, 40, 3), 255, np.uint8)
    e = twin.sgbm_effective(cr.params(pre_filter_cap=63), 40)
    a = cr.pixel_cost(L, R, e)
    assert a.max() == 3 * 63
    assert np.array_equal(a, cr.pixel_cost_planes(L, R, e))


@pytest.mark.parametrize("channel", [0, 1, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_one_live_channel_is_the_grey_pair(oracle, channel, mode):
    rng = np.random.default_rng(77 + channel)
    Lg = rng.integers(0, 256, (19, 61)).astype(np.uint8)
    Rg = np.roll(Lg, -3, axis=1)
    p = cr.params(num_disparities=16, block_size=5, p1=8, p2=40, pre_filter_cap=31, uniqueness_ratio=10,
                  speckle_window_size=20, speckle_range=2, mode=mode)
    ftzero = twin.sgbm_effective(p, 61)["ftzero"]
    L, R = cr.one_live_channel(Lg, Rg, channel, ftzero)
    got = cr.compute_bgr(L, R, p)
    assert np.array_equal(got, twin.sgbm_compute(Lg, Rg, p))
    assert np.array_equal(got, oracle.sgbm(Lg, Rg, p))


def test_three_live_channels_differ_from_any_grey_channel():
    rng = np.random.default_rng(5)
    L, R = rand_bgr_pair(rng, 17, 60, 4)
    p = cr.params(num_disparities=16, block_size=3, uniqueness_ratio=0)
    got = cr.compute_bgr(L, R, p)
    assert any(not np.array_equal(got, twin.sgbm_compute(L[:, :, c], R[:, :, c], p)) for c in range(3))


def test_restatement_refuses_wrapping_costs():
    # 8-pixel stripes against their inverse, blockSize 25: window sums beyond int16
    x = (np.arange(120) // 8) % 2
    Lg = np.tile((x * 255).astype(np.uint8), (30, 1))
    L = np.repeat(Lg[:, :, None], 3, axis=2)
    R = 255 - L
    p = cr.params(num_disparities=16, block_size=25, pre_filter_cap=63, p2=2592, p1=648)
    with pytest.raises(AssertionError, match="wraps int16"):
        cr.compute_bgr(L, R, p)


# ---- the host mirror's argument rules (raised before any device is touched) ----
def test_compute_bgr_rejects_shapes(mvsv):
    m = mvsv.StereoSGBM.create(0, 16, 3)
    grey = np.zeros((8, 40), np.uint8)
    bgr = np.zeros((8, 40, 3), np.uint8)
    with pytest.raises(mvsv.MvsvError):
        m.compute_bgr(grey, grey)
    with pytest.raises(mvsv.MvsvError):
        m.compute_bgr(bgr, np.zeros((8, 41, 3), np.uint8))
    with pytest.raises(mvsv.MvsvError):
        m.compute_bgr(np.zeros((8, 40, 4), np.uint8), np.zeros((8, 40, 4), np.uint8))
    with pytest.raises(mvsv.MvsvError):
        m.compute_bgr(bgr.astype(np.int16), bgr.astype(np.int16))
    with pytest.raises(mvsv.MvsvError):
        mvsv.Disparity.sgbm_bgr(mvsv.Stereopair(grey, grey), None, m)
    assert not hasattr(mvsv.StereoBM, "compute_bgr")


def test_workspace_bytes_counts_the_channel_planes(mvsv):
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    p = mvsv.StereoSGBM.create(0, 64, 9, 648, 2592)._params
    grey = lib.mvsv_sgbm_workspace_bytes(2, 320, 240, ctypes.byref(p))
    assert lib.mvsv_sgbm_workspace_bytes_cn(2, 320, 240, ctypes.byref(p), 1) == grey
    # the BT interval planes: 16 bytes per pixel and channel
    assert lib.mvsv_sgbm_workspace_bytes_cn(2, 320, 240, ctypes.byref(p), 3) == grey + 2 * 320 * 240 * 32
    assert lib.mvsv_sgbm_workspace_bytes_cn(2, 320, 240, ctypes.byref(p), 2) == 0
    # sgbm.yml's regime: a colour launch has neither residual nor bit-sliced planes
    q = mvsv.StereoSGBM.create(0, 128, 5)._params
    q.uniqueness_ratio = 0
    g = lib.mvsv_sgbm_workspace_bytes(8, 640, 480, ctypes.byref(q))
    c = lib.mvsv_sgbm_workspace_bytes_cn(8, 640, 480, ctypes.byref(q), 3)
    assert c < g + 8 * 640 * 480 * 32
