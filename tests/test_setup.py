"""Camera set-up primitives without a GPU: the numpy twin's own known answers for
the focus measure S4 (tests/setup_restate.py), mvsv_undistort_maps (host code of
the library) against the twin, and the argument checks of every new entry point
that needs no device."""
import ctypes
import glob
import os

import numpy as np
import pytest

from tests import setup_restate as twin
from tests.conftest import GOLDEN

CALIBS = sorted(glob.glob(os.path.join(GOLDEN, "calib", "*", "intrinsic.yml")))


# ---- S4: known answers -----------------------------------------------------------------
def test_constant_image_gives_zero():
    for shape in ((1, 1), (1, 7), (9, 1), (12, 17)):
        assert twin.sum4(np.full(shape, 137, np.uint8)) == 0


@pytest.mark.parametrize("v", [1, 100, 255])
def test_single_pixel(v):
    img = np.zeros((9, 11), np.uint8)
    img[4, 6] = v
    assert twin.sum4(img) == 32 * v          # sum |KX| = sum |KY| = 16
    img = np.zeros((9, 11), np.uint8)
    img[2, 2] = v                             # 2 from the border: the reflection does not see it
    assert twin.sum4(img) == 32 * v


@pytest.mark.parametrize("W,H", [(8, 5), (9, 6), (2, 2), (100, 70)])
def test_alternating_columns(W, H):
    img = np.zeros((H, W), np.uint8)
    img[:, 1::2] = 255
    assert twin.sum4(img) == 2040 * W * H     # reflect-101 continues the pattern at every border


def test_per_pixel_bound():
    rng = np.random.default_rng(5)
    img = rng.choice(np.array([0, 255], np.uint8), size=(40, 50))
    rx, ry = twin.responses(img)
    assert (np.abs(rx) + np.abs(ry)).max() <= 4080


ROIS_63 = [None, (17, 9, 50, 40), (0, 0, 20, 10), (43, 30, 63, 47), (0, 5, 63, 6), (10, 0, 11, 47), (62, 46, 63, 47)]
ROIS_100 = [None, (17, 9, 80, 61), (0, 9, 80, 61), (17, 0, 80, 61), (17, 9, 100, 61), (17, 9, 80, 70), (0, 0, 1, 1)]


@pytest.mark.parametrize("shape,seed,rois", [((47, 63), 63047, ROIS_63), ((70, 100), 100070, ROIS_100)])
def test_separable_float64_transcription_equals_sum4(shape, seed, rois):
    img = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    for roi in rois:
        s4 = twin.sum4(img, roi)
        assert twin.separable_float64(img, roi) == float(s4), roi
        assert s4 > 0


def test_interior_roi_takes_its_halo_from_the_parent():
    img = np.random.default_rng(100070).integers(0, 256, (70, 100), dtype=np.uint8)
    roi = (17, 9, 80, 61)
    crop = np.ascontiguousarray(img[9:61, 17:80])
    assert twin.sum4(img, roi) != twin.sum4(crop)


def test_mean_is_a_reciprocal_and_a_product():
    # 3 * (1.0 / 3) rounds to 1.0 where other N show the difference to a division
    found = False
    for n in range(3, 400, 2):
        s4 = 4 * 7 * n + 4
        if twin.value_of(s4, n) != (s4 / 4.0) / n:
            found = True
    assert found
    img = np.random.default_rng(3).integers(0, 256, (47, 63), dtype=np.uint8)
    assert twin.sharpness(img) == (twin.sum4(img) / 4.0) * (1.0 / (47 * 63))


# ---- mvsv_undistort_maps against the twin ----------------------------------------------
TIE_CAP = 1e-4  # at most 0.01 % of the entries may differ (a condition, not a measurement)


def synthetic_K(W, H):
    return np.array([[0.83 * W, 0, 0.4931 * W], [0, 0.81 * W, 0.5117 * H], [0, 0, 1]], np.float64)


def map_cases():
    cases = []
    K = synthetic_K(96, 64)
    for k1 in (0.3, -0.3):
        cases.append((f"96x64 k1={k1} nd4", K, [k1, 0.05, 1e-3, -2e-3], None, 96, 64))
    cases.append(("96x64 nd0", K, [], None, 96, 64))
    cases.append(("96x64 nd5", K, [-0.3, 0.11, 1e-3, -2e-3, 0.02], None, 96, 64))
    cases.append(("96x64 nd8", K, [0.3, 0.11, 1e-3, -2e-3, 0.02, 0.01, -0.02, 0.003], None, 96, 64))
    newK = K.copy()
    newK[0, 0] *= 0.9
    newK[1, 2] += 3.25
    cases.append(("96x64 new_K", K, [-0.3, 0.1, 0, 0], newK, 96, 64))
    K3 = synthetic_K(4100, 3)
    K3[1, 1] = K3[0, 0]
    cases.append(("4100x3 one-row stripes", K3, [-0.3, 0.1, 1e-4, 1e-4], None, 4100, 3))
    return cases


def calib_cases():
    from mvstereovision3_amd import calibration
    cases = []
    for path in CALIBS:
        name = os.path.basename(os.path.dirname(path))
        for side in ("Left", "Right"):
            K, _ = calibration.read_matrix(path, "cameraMatrix" + side)
            D, _ = calibration.read_matrix(path, "distCoeffs" + side)
            cases.append((f"{name} {side}", K, D.reshape(-1), None, 752, 480))
    return cases


def check_maps(mvsv, name, K, dist, new_K, W, H):
    near = twin.near_ties(K, dist, new_K, W, H)
    cap = TIE_CAP * near.size
    assert near.sum() <= cap, f"{name}: the twin itself has {near.sum()} near-tie entries"
    wxy, wfr = twin.undistort_maps(K, dist, new_K, W, H)
    xy, fr = mvsv.undistort_maps(K, dist, (W, H), new_K)
    assert xy.shape == (H, W, 2) and fr.shape == (H, W) and xy.dtype == np.int16 and fr.dtype == np.uint16
    # positions in 1/32 steps
    gx = xy[..., 0].astype(np.int64) * 32 + (fr & 31)
    gy = xy[..., 1].astype(np.int64) * 32 + (fr >> 5)
    wx = wxy[..., 0].astype(np.int64) * 32 + (wfr & 31)
    wy = wxy[..., 1].astype(np.int64) * 32 + (wfr >> 5)
    diff = (gx != wx) | (gy != wy)
    print(f"{name}: {int(diff.sum())} differing entries, {int(near.sum())} near ties of {near.size}")
    assert not (diff & ~near).any(), f"{name}: entries differ away from a rounding tie"
    assert max(np.abs(gx - wx).max(), np.abs(gy - wy).max()) <= 1
    assert diff.sum() <= cap
    return wxy, wfr


@pytest.mark.parametrize("case", map_cases(), ids=lambda c: c[0])
def test_undistort_maps_synthetic(mvsv, case):
    name, K, dist, new_K, W, H = case
    wxy, _ = check_maps(mvsv, *case)
    if W == 96 and len(dist) and new_K is None:
        sx, sy = wxy[..., 0], wxy[..., 1]
        outside = (sx < -1) | (sx >= W) | (sy < -1) | (sy >= H)
        # k1 > 0 pushes the corners' sources outside, k1 < 0 pulls them inside
        assert outside.any() == (dist[0] > 0), name


def test_undistort_maps_fixture_calibrations(mvsv):
    cases = calib_cases()
    assert len(cases) >= 2
    for case in cases:
        check_maps(mvsv, *case)


def test_undistort_maps_stripes_are_what_the_spec_says():
    assert min(max(1, 4096 // 96), 64) == 42 and 64 - 42 == 22
    assert min(max(1, 4096 // 752), 480) == 5
    assert min(max(1, 4096 // 4100), 3) == 1


def test_undistort_maps_no_distortion_is_the_identity(mvsv):
    K = synthetic_K(96, 64)
    xy, fr = mvsv.undistort_maps(K, None, (96, 64))
    yy, xx = np.mgrid[0:64, 0:96]
    gx = xy[..., 0].astype(np.int64) * 32 + (fr & 31)
    gy = xy[..., 1].astype(np.int64) * 32 + (fr >> 5)
    assert np.abs(gx - 32 * xx).max() <= 1 and np.abs(gy - 32 * yy).max() <= 1


# ---- argument checks that need no device -------------------------------------------------
def test_undistort_maps_validation(mvsv):
    from mvstereovision3_amd import _lib
    L = _lib.lib()
    K = synthetic_K(8, 4)
    d = np.array([0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    xy = np.zeros((4, 8, 2), np.int16)
    fr = np.zeros((4, 8), np.uint16)

    def call(K_=K.ctypes.data, d_=d.ctypes.data, nd=4, W=8, H=4, xy_=xy.ctypes.data, xs=8, fr_=fr.ctypes.data, fs=8):
        return L.mvsv_undistort_maps(K_, d_, nd, None, W, H, xy_, xs, fr_, fs)

    assert call() == 0
    assert call(nd=0, d_=None) == 0
    for bad in (dict(K_=None), dict(nd=3), dict(nd=6), dict(nd=4, d_=None), dict(W=0), dict(H=0), dict(xs=7),
                dict(fs=7), dict(xy_=None), dict(fr_=None)):
        assert call(**bad) == _lib.MVSV_E_INVALID_ARG, bad
    singular = np.zeros((3, 3))
    assert call(K_=singular.ctypes.data) == _lib.MVSV_E_INVALID_ARG
    with pytest.raises(mvsv.MvsvError):
        mvsv.undistort_maps(K, [0.1, 0.2, 0.3], (8, 4))
    with pytest.raises(mvsv.MvsvError):
        mvsv.undistort_maps(K, None, (0, 4))


def test_null_handles_are_invalid_arguments(mvsv):
    from mvstereovision3_amd import _lib
    L = _lib.lib()
    img = np.zeros((4, 8), np.uint8)
    s = ctypes.c_int64(0)
    v = ctypes.c_double(0)
    p = img.ctypes.data
    E = _lib.MVSV_E_INVALID_ARG
    assert L.mvsv_sharpness_device(None, 1, p, 8, 32, 8, 4, None, ctypes.addressof(s)) == E
    assert L.mvsv_sharpness(None, p, 8, 8, 4, None, ctypes.byref(v), ctypes.byref(s)) == E
    assert L.mvsv_remap_fixed_device(None, 1, p, 8, 32, 8, 4, p, 8, p, 8, p, 8, 32, 8, 4) == E
    K = synthetic_K(8, 4)
    assert L.mvsv_undistort_pair(None, p, 8, p, 8, 8, 4, K.ctypes.data, None, 0, K.ctypes.data, None, 0,
                                 p, 8, p, 8) == E
    assert L.mvsv_stream_enable_sharpness(None, None, None) == E
    assert L.mvsv_stream_disable_sharpness(None) == E
    assert L.mvsv_stream_front_sharpness(None, ctypes.byref(v), ctypes.addressof(s)) == E


def test_python_mirrors_reject_wrong_inputs(mvsv):
    with pytest.raises(mvsv.MvsvError):
        mvsv.sharpness(np.zeros((4, 8), np.int16))
    with pytest.raises(mvsv.MvsvError):
        mvsv.sharpness(np.zeros((8,), np.uint8))
    with pytest.raises(mvsv.MvsvError):
        mvsv.Utility.checkSharpness(np.zeros((2, 4, 8), np.uint8))
    with pytest.raises(mvsv.MvsvError):
        mvsv.undistort_pair(np.zeros((4, 8), np.uint8), np.zeros((4, 9), np.uint8), np.eye(3), None, np.eye(3), None)
    s = mvsv.Stereosystem(8, 4)
    assert hasattr(s, "getUndistortedImagepair") and s._undistort_maps is None
