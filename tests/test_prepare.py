"""Grey pair preparation without a GPU: the numpy restatement (prepare_restate)
against the oracle's one-channel resize, the host-side size and argument rules of
the C ABI, spot values of both grey variants, and the new kernel's scratch."""
import ctypes
import re

import numpy as np
import pytest

from tests import prepare_restate as ref

SIZES = [(2, 2), (5, 7), (7, 5), (64, 4), (129, 6), (70, 9)]  # (width, height)


def bgr_image(w, h, seed=0):
    return np.random.default_rng(1000 * w + h + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("w,h", SIZES)
def test_halving_is_the_oracles_resize_per_channel(oracle, w, h):
    """INTER_AREA's 2 x 2 path treats channels independently, so the one-channel
    oracle pins each plane of the 3-channel halving."""
    img = bgr_image(w, h)
    for c in range(3):
        plane = np.ascontiguousarray(img[..., c])
        want = oracle.resize_linear(plane, 0.5, 0.5)
        got = ref.halve_plane(plane)
        assert got.shape == want.shape == ref.prepare_size(w, h, True)[::-1]
        assert np.array_equal(got, want), f"channel {c}: {np.argwhere(got != want)[:5].tolist()}"
    # ties of the clipped blocks: a 2-pixel block summing to an odd value rounds to even
    edge = np.zeros((1, 2), np.uint8)
    edge[0] = (2, 3)
    assert ref.halve_plane(np.vstack([edge, edge, edge])).tolist() == [[3], [2]]  # (2+3+2+3+2)>>2, rint(2.5)
    assert oracle.resize_linear(np.vstack([edge, edge, edge]), 0.5, 0.5).tolist() == [[3], [2]]


@pytest.mark.parametrize("w,h,halve,want", [
    (5, 7, 1, (2, 4)), (7, 5, 1, (4, 2)), (2, 2, 1, (1, 1)), (64, 4, 1, (32, 2)), (129, 6, 1, (64, 3)),
    (70, 9, 1, (35, 4)), (1281, 5, 1, (640, 2)), (3, 3, 1, (2, 2)), (5, 7, 0, (5, 7)), (1, 1, 0, (1, 1))])
def test_prepare_size(mvsv, w, h, halve, want):
    from mvstereovision3_amd import _lib
    dw, dh = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.lib().mvsv_prepare_size(w, h, halve, ctypes.byref(dw), ctypes.byref(dh)) == 0
    assert (dw.value, dh.value) == want == ref.prepare_size(w, h, halve)
    assert mvsv.prepare_size(w, h, bool(halve)) == want
    if halve:
        rw, rh = ctypes.c_int(), ctypes.c_int()
        assert _lib.lib().mvsv_resize_size(w, h, 0.5, 0.5, ctypes.byref(rw), ctypes.byref(rh)) == 0
        assert (rw.value, rh.value) == want


@pytest.mark.parametrize("w,h,halve", [(1, 1, 1), (1, 8, 1), (8, 1, 1), (0, 4, 0), (4, -1, 0), (8, 8, 2), (8, 8, -1)])
def test_prepare_size_invalid(mvsv, w, h, halve):
    """A 1-pixel side halves to cvRound(0.5) = 0; other factors than 0.5 are out of scope."""
    from mvstereovision3_amd import _lib
    dw, dh = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.lib().mvsv_prepare_size(w, h, halve, ctypes.byref(dw), ctypes.byref(dh))
    assert rc == _lib.MVSV_E_INVALID_ARG
    assert _lib.lib().mvsv_prepare_size(8, 8, 1, None, ctypes.byref(dh)) == _lib.MVSV_E_INVALID_ARG


def test_gray_spot_values():
    px = lambda b, g, r: np.array([[[b, g, r]]], np.uint8)
    for v in (ref.Q14, ref.Q15):
        assert ref.gray(px(255, 255, 255), v)[0, 0] == 255
        assert ref.gray(px(0, 0, 0), v)[0, 0] == 0
    assert ref.gray(px(255, 0, 0), ref.Q14)[0, 0] == 29   # (255 * 1868 + 8192) >> 14
    assert ref.gray(px(0, 255, 0), ref.Q14)[0, 0] == 150
    assert ref.gray(px(0, 0, 255), ref.Q14)[0, 0] == 76
    # the weights of each variant sum to its one, so grey stays grey
    assert 1868 + 9617 + 4899 == 1 << 14 and 3735 + 19235 + 9798 == 1 << 15
    g = np.arange(256, dtype=np.uint8)
    grey = np.stack([g, g, g], -1)[None]
    assert np.array_equal(ref.gray(grey, ref.Q14)[0], g) and np.array_equal(ref.gray(grey, ref.Q15)[0], g)


def test_the_variants_differ_somewhere():
    """Found by search over a coarse lattice of colours: the switch does something."""
    v = np.arange(0, 256, 5, dtype=np.uint8)
    cube = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(1, -1, 3)
    a, b = ref.gray(cube, ref.Q14)[0], ref.gray(cube, ref.Q15)[0]
    diff = np.flatnonzero(a != b)
    assert diff.size > 0
    assert np.abs(a.astype(int) - b.astype(int)).max() == 1  # one rounding step apart at most
    bgr = cube[0, diff[0]]
    print(f"first differing colour (B, G, R) = {bgr.tolist()}: Q14 {a[diff[0]]}, Q15 {b[diff[0]]}")
    img = np.ascontiguousarray(cube[:, diff[:4]])
    assert not np.array_equal(ref.prepare(img, False, ref.Q14), ref.prepare(img, False, ref.Q15))


def test_rounding_before_the_conversion_matters():
    """Fusing must keep the 8-bit rounding of each halved channel: grey of the
    unrounded channel means would differ on this block."""
    blk = np.zeros((2, 2, 3), np.uint8)
    blk[..., 1] = [[1, 1], [0, 0]]   # G mean 0.5 -> (2 + 2) >> 2 = 1
    assert ref.prepare(blk)[0, 0] == ref.gray(np.array([[[0, 1, 0]]], np.uint8))[0, 0] == 1
    assert (2 * 9617 // 4 + 8192) >> 14 == 0  # what an unrounded fusion would give


def test_python_argument_checks(mvsv):
    with pytest.raises(mvsv.MvsvError):
        mvsv.prepare_gray(np.zeros((4, 4), np.uint8))
    with pytest.raises(mvsv.MvsvError):
        mvsv.prepare_gray(np.zeros((4, 4, 3), np.int16))
    with pytest.raises(mvsv.MvsvError):
        mvsv.prepare_size(1, 1)
    with pytest.raises(mvsv.MvsvError) as e:
        mvsv.DisparityStream(object(), 64, 48)
    assert "StereoSGBM or StereoBM" in str(e.value)


def test_prepare_kernel_has_no_scratch():
    from tests.test_kernel_scratch import LIB, LLVM, kernel_scratch
    import os
    if not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("library not built / no ROCm llvm tools")
    ks = {k: v for k, v in kernel_scratch().items() if re.search(r"bgr_gray_kernel", k)}
    assert len(ks) == 2, f"the halving and the plain instance expected: {sorted(ks)}"
    assert not any(ks.values()), f"bgr_gray_kernel instances with scratch: {ks}"
