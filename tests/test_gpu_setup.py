"""Camera set-up on the device: the focus measure (mvsv_sharpness_device,
Utility.checkSharpness, the streams' front_sharpness) and undistorted pairs
(mvsv_remap_fixed_device, mvsv_undistort_pair, Stereosystem.getUndistortedImagepair)
against the numpy twin tests/setup_restate.py.  Every comparison is bit-exact.

Shapes of the sum kernel: one pixel, sizes below a lane's 4 columns, odd sizes, a
width of more than eight 256-column strips (2072) and a height of 188 bands (1500),
so more than one block; strides that allow packed loads and strides that do not,
and every base alignment."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest

from tests import setup_restate as twin
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (3, 2), (63, 47), (100, 70), (127, 31), (2072, 5), (24, 1500)]  # (W, H)


@functools.lru_cache(maxsize=None)
def image(W, H, n=1):
    a = np.random.default_rng(W * 10007 + H).integers(0, 256, (n, H, W), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_sum4(W, H, roi=None):
    return twin.sum4(image(W, H)[0], roi)


def device_view(torch, frames, stride, offset, frame_pad=0, fill=0):
    """frames (n, H, W) as a device view with the given row stride, base offset
    (bytes from a 256-byte aligned allocation) and frame padding; the padding
    bytes hold `fill`."""
    n, H, W = frames.shape
    fs = H * stride + frame_pad
    buf = torch.full((offset + n * fs + 16,), fill, dtype=torch.uint8, device="cuda")
    v = buf.as_strided((n, H, W), (fs, stride, 1), offset)
    v.copy_(torch.from_numpy(np.array(frames)).cuda())
    return v


@pytest.mark.parametrize("W,H", SHAPES)
def test_sum4_shapes_strides_offsets(gpu, mvsv, W, H):
    want = want_sum4(W, H)
    npx = W * H
    for stride in (W, W + 9, (W + 15) & ~15):
        for offset in range(4):
            v = device_view(gpu, image(W, H), stride, offset, fill=255 - 37 * offset)[0]
            value, s4 = mvsv.sharpness(v, return_sums=True)
            assert s4 == want, f"{W}x{H} stride {stride} offset {offset}: {s4} != {want}"
            assert value == twin.value_of(want, npx)


ROIS = {
    "whole": (0, 0, 100, 70), "interior": (17, 9, 80, 61), "left": (0, 9, 80, 61), "top": (17, 0, 80, 61),
    "right": (17, 9, 100, 61), "bottom": (17, 9, 80, 70), "corner px": (99, 69, 100, 70), "first px": (0, 0, 1, 1),
    "interior px": (41, 33, 42, 34), "one row": (3, 40, 97, 41), "one column": (58, 2, 59, 69),
}


@pytest.mark.parametrize("name", list(ROIS))
def test_sum4_rois(gpu, mvsv, name):
    roi = ROIS[name]
    img = image(100, 70)[0]
    want = want_sum4(100, 70, roi)
    for stride, offset in ((100, 0), (109, 1), (112, 3)):
        v = device_view(gpu, image(100, 70), stride, offset, fill=91)[0]
        _, s4 = mvsv.sharpness(v, roi, return_sums=True)
        assert s4 == want, f"{name} stride {stride} offset {offset}: {s4} != {want}"
    if name == "interior":
        x0, y0, x1, y1 = roi
        crop = np.ascontiguousarray(img[y0:y1, x0:x1])
        want_crop = twin.sum4(crop)
        assert want_crop != want  # the halo comes from the parent, not from a reflection of the view
        _, s4 = mvsv.sharpness(gpu.from_numpy(crop).cuda(), return_sums=True)
        assert s4 == want_crop
    if name == "whole":
        assert want == want_sum4(100, 70)


def test_sum4_batch_ignores_padding(gpu, mvsv):
    frames = image(127, 31, 3)
    want = [twin.sum4(f) for f in frames]
    roi = (5, 3, 120, 30)
    want_roi = [twin.sum4(f, roi) for f in frames]
    got = []
    for fill in (0, 255):
        for stride, pad, offset in ((136, 24, 0), (131, 7, 2)):  # packed and narrow loads
            v = device_view(gpu, frames, stride, offset, frame_pad=pad, fill=fill)
            values, sums = mvsv.sharpness(v, return_sums=True)
            assert sums.tolist() == want and values.shape == (3,)
            assert values.tolist() == [twin.value_of(s, 127 * 31) for s in want]
            _, sums_roi = mvsv.sharpness(v, roi, return_sums=True)
            assert sums_roi.tolist() == want_roi
            got.append(sums.tobytes() + sums_roi.tobytes())
    assert len(set(got)) == 1
    assert len(set(want)) == 3


def test_sum4_needs_64_bits(gpu, mvsv):
    img = np.zeros((1100, 2048), np.uint8)
    img[:, 1::2] = 255
    _, s4 = mvsv.sharpness(gpu.from_numpy(img).cuda(), return_sums=True)
    assert s4 == 4_595_712_000 == 2040 * 2048 * 1100 and s4 > 2 ** 32


def test_python_mirrors_agree(gpu, mvsv):
    img = image(100, 70)[0]
    roi = ROIS["interior"]
    for r in (None, roi):
        want = twin.sharpness(img, r)
        assert mvsv.Utility.checkSharpness(img, r) == want
        assert mvsv.Utility.checkSharpness(gpu.from_numpy(img.copy()).cuda(), r) == want
        assert mvsv.sharpness(img, r) == want
    values, sums = mvsv.sharpness(image(127, 31, 3), return_sums=True)  # numpy batch
    assert sums.tolist() == [twin.sum4(f) for f in image(127, 31, 3)]
    view = image(100, 70)[0][:, 10:90]  # a numpy view with a row stride
    assert mvsv.sharpness(view) == twin.sharpness(np.ascontiguousarray(view))


def test_sharpness_device_validation(gpu, mvsv):
    from mvstereovision3_amd import _lib
    L = _lib.lib()
    ctx = _lib.context(0)
    t = gpu.zeros((70, 100), dtype=gpu.uint8, device="cuda")
    out = gpu.zeros((2,), dtype=gpu.int64, device="cuda")

    def call(n=1, img=t.data_ptr(), stride=100, W=100, H=70, roi=None, sums=out.data_ptr()):
        r = _lib.Rect(*roi) if roi is not None else None
        return L.mvsv_sharpness_device(ctx.handle, n, img, stride, 7000, W, H,
                                       ctypes.byref(r) if r is not None else None, sums)

    assert call() == 0
    for bad in (dict(n=0), dict(img=None), dict(sums=None), dict(stride=99), dict(W=0), dict(H=0),
                dict(roi=(5, 5, 5, 9)), dict(roi=(5, 5, 9, 5)), dict(roi=(-1, 0, 9, 9)), dict(roi=(0, 0, 101, 70)),
                dict(roi=(0, 0, 100, 71)), dict(W=65536, H=32768, stride=65536)):
        assert call(**bad) == _lib.MVSV_E_INVALID_ARG, bad
    _lib.synchronize(0)


# ---- undistorted pairs -------------------------------------------------------------------
def synthetic_K(W, H):
    return np.array([[0.83 * W, 0, 0.4931 * W], [0, 0.81 * W, 0.5117 * H], [0, 0, 1]], np.float64)


def as_i16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


@pytest.mark.parametrize("k1", [0.3, -0.3])
def test_remap_fixed_matches_the_twin(gpu, mvsv, k1):
    W, H = 96, 64
    src = image(W, H, 2)
    xy, frac = mvsv.undistort_maps(synthetic_K(W, H), [k1, 0.05, 1e-3, -2e-3], (W, H))
    want = np.stack([twin.remap_fixed(f, xy, frac) for f in src])
    if k1 > 0:  # sources outside the image: zeros must appear
        sx, sy = xy[..., 0], xy[..., 1]
        gone = (sx < -1) | (sx >= W) | (sy < -1) | (sy >= H)
        assert gone.any() and (want[:, gone] == 0).all()
    got = mvsv.remap_fixed(gpu.from_numpy(src.copy()).cuda(), as_i16(gpu, xy), as_i16(gpu, frac))
    assert np.array_equal(got.cpu().numpy(), want)
    one = mvsv.remap_fixed(gpu.from_numpy(src[1].copy()).cuda(), as_i16(gpu, xy), as_i16(gpu, frac))
    assert np.array_equal(one.cpu().numpy(), want[1])


def test_remap_fixed_odd_strides_and_batch(gpu, mvsv):
    from mvstereovision3_amd import _lib
    W, H = 96, 64
    src = image(W, H, 2)
    xy, frac = mvsv.undistort_maps(synthetic_K(W, H), [0.3, 0.05, 1e-3, -2e-3], (W, H))
    want = np.stack([twin.remap_fixed(f, xy, frac) for f in src])
    s = device_view(gpu, src, 105, 3, frame_pad=11, fill=200)
    dxy = gpu.zeros((H, 99, 2), dtype=gpu.int16, device="cuda")
    dxy[:, :W] = as_i16(gpu, xy)
    dfr = gpu.zeros((H, 101), dtype=gpu.int16, device="cuda")
    dfr[:, :W] = as_i16(gpu, frac)
    dst = gpu.full((1 + 2 * (H * 103 + 5),), 77, dtype=gpu.uint8, device="cuda")
    d = dst.as_strided((2, H, W), (H * 103 + 5, 103, 1), 1)
    ctx = _lib.context(0)
    _lib.check(_lib.lib().mvsv_set_stream(ctx.handle, ctypes.c_void_p(gpu.cuda.current_stream().cuda_stream)))
    _lib.check(_lib.lib().mvsv_remap_fixed_device(ctx.handle, 2, s.data_ptr(), 105, s.stride(0), W, H,
                                                  dxy.data_ptr(), 99, dfr.data_ptr(), 101, d.data_ptr(), 103,
                                                  d.stride(0), W, H), ctx.handle)
    assert np.array_equal(d.cpu().numpy(), want)
    pad = dst.clone()
    pad.as_strided((2, H, W), (H * 103 + 5, 103, 1), 1).fill_(77)
    assert bool((pad == 77).all())  # nothing outside the destination rows was written


def test_undistort_pair_in_place(gpu, mvsv):
    W, H = 96, 64
    KL, KR = synthetic_K(W, H), synthetic_K(W, H) + np.array([[1.5, 0, -2.25], [0, 0.5, 1.75], [0, 0, 0]])
    dl, dr = [0.3, 0.05, 1e-3, -2e-3], [-0.3, 0.1, 0, 0, 0.01]
    L, R = image(W, H, 2)
    oL, oR = mvsv.undistort_pair(L, R, KL, dl, KR, dr)
    assert np.array_equal(oL, twin.remap_fixed(L, *mvsv.undistort_maps(KL, dl, (W, H))))
    assert np.array_equal(oR, twin.remap_fixed(R, *mvsv.undistort_maps(KR, dr, (W, H))))
    iL, iR = L.copy(), R.copy()
    mvsv.undistort_pair(iL, iR, KL, dl, KR, dr, out=(iL, iR))  # maps cached by now
    assert np.array_equal(iL, oL) and np.array_equal(iR, oR)
    # another calibration replaces the cached maps; no coefficients: the identity away from the border
    nL, nR = mvsv.undistort_pair(L, R, KL, None, KR, [])
    assert np.array_equal(nL[1:-1, 1:-1], L[1:-1, 1:-1]) and np.array_equal(nR[1:-1, 1:-1], R[1:-1, 1:-1])
    aL, _ = mvsv.undistort_pair(L, R, KL, dl, KR, dr)
    assert np.array_equal(aL, oL)


def test_stereosystem_undistorted_pair(gpu, mvsv):
    path = sorted(glob.glob(os.path.join(GOLDEN, "calib", "*", "intrinsic.yml")))[0]
    W, H = 752, 480
    s = mvsv.Stereosystem(W, H)
    assert s.loadIntrinsic(path)
    L, R = image(W, H, 2)
    want = [twin.remap_fixed(img, *twin.undistort_maps(K, D.reshape(-1), None, W, H))
            for img, K, D in ((L, s.mIntrinsicLeft, s.mDistCoeffsLeft), (R, s.mIntrinsicRight, s.mDistCoeffsRight))]
    pair = mvsv.Stereopair(L.copy(), R.copy())
    assert s.getUndistortedImagepair(pair)
    assert np.array_equal(pair.mLeft, want[0]) and np.array_equal(pair.mRight, want[1])
    assert not np.array_equal(want[0], L)
    maps = s._undistort_maps
    assert maps is not None
    dev = mvsv.Stereopair(gpu.from_numpy(L.copy()).cuda(), gpu.from_numpy(R.copy()).cuda())
    assert s.getUndistortedImagepair(dev) and s._undistort_maps is maps  # built once per instance
    assert np.array_equal(dev.mLeft.cpu().numpy(), want[0]) and np.array_equal(dev.mRight.cpu().numpy(), want[1])
    s.resetRectification()
    assert s._undistort_maps is None
    assert s.getUndistortedImagepair(mvsv.Stereopair(L.copy(), R.copy())) and s._undistort_maps is not None
    assert s.loadIntrinsic(path) and s._undistort_maps is None
    # the C entry point gives the same pair
    oL, oR = mvsv.undistort_pair(L, R, s.mIntrinsicLeft, s.mDistCoeffsLeft, s.mIntrinsicRight, s.mDistCoeffsRight)
    assert np.array_equal(oL, want[0]) and np.array_equal(oR, want[1])


# ---- the frame stream ----------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 2])
def test_stream_brings_the_focus_values(gpu, mvsv, batch):
    from mvstereovision3_amd import _lib
    from tests.test_gpu_samplepoint import SD, SH, SW, plain_stream_results, stream_frames
    m = mvsv.StereoSGBM.create(0, SD, 9, 648, 2592)
    roi_u, _ = mvsv.create_dmap_rois((SH, SW), SD)
    roi_l, roi_r = (31, 17, 301, 199), (0, 100, SW, SH)
    frames = stream_frames()
    plain = plain_stream_results(batch)
    st = mvsv.DisparityStream(m, SW, SH, depth=3, grid_roi=roi_u, batch=batch)
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError) as e:  # never enabled
        st.front_sharpness()
    assert e.value.code == _lib.MVSV_E_INVALID_ARG and st.pending() == 1
    with pytest.raises(mvsv.MvsvError) as e:  # a frame is pending
        st.enable_sharpness(roi_l, roi_r)
    assert e.value.code == _lib.MVSV_E_INVALID_ARG
    d0, means0 = st.pop()
    assert np.array_equal(d0, plain[0][0]) and np.array_equal(means0, plain[0][1])
    for bad in ((0, 0, SW + 1, SH), (5, 5, 5, 9)):
        with pytest.raises(mvsv.MvsvError):
            st.enable_sharpness(bad, None)
    st.enable_sharpness(roi_l, roi_r)
    st.enable_display(roi_u)  # composes with the display map
    pushed = 0
    for i in range(5):
        while pushed < 5 and st.pending() < 3:
            st.push(*frames[pushed])
            pushed += 1
        values, sums = st.front_sharpness(return_sums=True)
        assert st.front_sharpness() == values  # the frame stays pending
        disp, mm = st.front_display()
        d, means = st.pop()
        assert d.tobytes() == plain[i][0].tobytes(), f"frame {i}: map differs from the plain stream's"
        assert means.tobytes() == plain[i][1].tobytes(), f"frame {i}: means differ from the plain stream's"
        L, R = frames[i]
        assert sums == (twin.sum4(L, roi_l), twin.sum4(R, roi_r)), f"frame {i}"
        off = (mvsv.sharpness(gpu.from_numpy(L.copy()).cuda(), roi_l), mvsv.sharpness(gpu.from_numpy(R.copy()).cuda(), roi_r))
        assert values == off == (twin.sharpness(L, roi_l), twin.sharpness(R, roi_r))
        x0, y0, x1, y1 = roi_u
        assert np.array_equal(disp, mvsv.normalize_minmax(np.ascontiguousarray(d[y0:y1, x0:x1])))
    assert sums[0] != sums[1]
    st.enable_sharpness()  # a second call replaces the first: whole images
    st.push(*frames[1])
    _, sums = st.front_sharpness(return_sums=True)
    assert sums == (twin.sum4(frames[1][0]), twin.sum4(frames[1][1]))
    st.pop()
    st.disable_sharpness()
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError):
        st.front_sharpness()
    d, means = st.pop()
    assert np.array_equal(d, plain[0][0]) and np.array_equal(means, plain[0][1])
    st.close()


@pytest.mark.parametrize("batch", [1, 2])
def test_raw_stream_measures_the_raw_pair(gpu, mvsv, batch):
    from tests.test_gpu_raw_stream import GRID, MAPS, ROI, matcher, raw_pair
    from tests.test_raw_stream_host import RAW_H, RAW_W
    roi_l, roi_r = (0, 0, RAW_W, RAW_H), (11, 7, RAW_W - 2, RAW_H - 1)  # in the raw frame, beyond the display ROI
    st = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI, depth=4, batch=batch, grid_roi=GRID)
    plain = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI, depth=4, batch=batch, grid_roi=GRID)
    with pytest.raises(mvsv.MvsvError):
        st.enable_sharpness((0, 0, RAW_W + 1, RAW_H), None)
    st.enable_sharpness(roi_l, roi_r)
    for seed in range(4):
        st.push_raw(*raw_pair(seed))
        plain.push_raw(*raw_pair(seed))
    for seed in range(4):
        values, sums = st.front_sharpness(return_sums=True)
        d, means = st.pop()
        pd, pm = plain.pop()
        assert d.tobytes() == pd.tobytes() and means.tobytes() == pm.tobytes()
        L, R = raw_pair(seed)
        assert sums == (twin.sum4(L, roi_l), twin.sum4(R, roi_r)), f"frame {seed}"
        assert values == (twin.sharpness(L, roi_l), twin.sharpness(R, roi_r))
        assert values[1] == mvsv.sharpness(gpu.from_numpy(R.copy()).cuda(), roi_r)
    st.close()
    plain.close()
