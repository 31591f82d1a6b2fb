"""The raw frame stream (mvsv_stream_create_raw, DisparityStream.raw): raw camera
pairs in, rectified -- remap, display-ROI crop, optional cv::resize -- on the
device ahead of SGBM and the 9x9 mean grid.  Every map, mean vector and rectified
pair is compared bit for bit with the oracle's remap_linear + crop (+ resize_linear)
+ sgbm + mean_disparity_grid; the new kernel is also compared with the existing
remap kernel (mvsv.rectify_pair).

Shapes: a 203 x 125 raw frame (no multiple of 4 or 64), ROI 181 x 108 (odd row
stride: dword and byte stores both occur) and the full frame (taps outside the
source).  The maps are quantised to 1/64 px, so about half of the x entries are
exact round-half-even ties, and the left and right maps differ."""
import ctypes
import functools

import numpy as np
import pytest

from tests.test_raw_stream_host import RAW_H, RAW_W, stream_maps

pytestmark = pytest.mark.gpu

ROI = (6, 5, 187, 113)       # 181 x 108
FULL = (0, 0, RAW_W, RAW_H)
GRID = (16, 0, 181, 108)     # x >= numDisparities / 2, as createDMapROIS places it
MAPS = stream_maps()


def matcher(mvsv, D=32):
    return mvsv.StereoSGBM.create(0, D, 5, 200, 800, 1, 31, 10, 50, 2, mvsv.MODE_SGBM)


@functools.lru_cache(maxsize=None)
def raw_pair(seed):
    """3x3 box blur (round half up) of u8 noise 64 columns wider than the frame;
    the right camera sees it 9 columns further on, with {-1, 0, +1} noise."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (RAW_H, RAW_W + 64)).astype(np.int64)
    P = np.pad(noise, 1, mode="edge")
    s = sum(P[dy:dy + RAW_H, dx:dx + RAW_W + 64] for dy in range(3) for dx in range(3))
    b = (2 * s + 9) // 18
    L = b[:, :RAW_W].astype(np.uint8)
    R = np.clip(b[:, 9:9 + RAW_W] + rng.integers(-1, 2, (RAW_H, RAW_W)), 0, 255).astype(np.uint8)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def _want(seed, roi, factor, D):
    """(rectified left, rectified right, map, params) from the oracle alone."""
    from oracle import pyoracle as oracle
    import mvstereovision3_amd as mvsv
    L, R = raw_pair(seed)
    x0, y0, x1, y1 = roi
    rl = np.ascontiguousarray(oracle.remap_linear(L, MAPS[0], MAPS[1])[y0:y1, x0:x1])
    rr = np.ascontiguousarray(oracle.remap_linear(R, MAPS[2], MAPS[3])[y0:y1, x0:x1])
    if factor is not None:
        rl, rr = oracle.resize_linear(rl, factor, factor), oracle.resize_linear(rr, factor, factor)
    p = {k: v for k, v in matcher(mvsv, D).params().items() if k != "variant"}
    d = oracle.sgbm(rl, rr, p)
    for a in (rl, rr, d):
        a.setflags(write=False)
    return rl, rr, d


def want(seed, roi=ROI, factor=None, D=32):
    return _want(seed, roi, factor, D)


def assert_map(got, w, what):
    assert got.shape == w.shape, f"{what}: shape {got.shape} != {w.shape}"
    bad = np.argwhere(got != w)
    assert bad.size == 0, f"{what}: {len(bad)} mismatches, first {bad[:5].tolist()}"
    assert (w > 0).mean() > 0.5, f"{what}: the oracle's map is mostly invalid"


def assert_image(got, w, what):
    assert got.shape == w.shape, f"{what}: shape {got.shape} != {w.shape}"
    bad = np.argwhere(got != w)
    assert bad.size == 0, f"{what}: {len(bad)} mismatches, first {bad[:5].tolist()}"


def test_ring_and_batches(gpu, mvsv, oracle):
    st = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI, depth=4, batch=3, grid_roi=GRID)
    assert (st.width, st.height) == (181, 108)
    got = []
    for seed in range(6):
        if st.pending() == 4:
            got.append(st.pop())
        st.push_raw(*raw_pair(seed))
    while st.pending():
        got.append(st.pop())
    st.close()
    assert len(got) == 6
    x0, y0, x1, y1 = GRID
    for seed, (d, means) in enumerate(got):
        w = want(seed)[2]
        assert_map(d, w, f"frame {seed}")
        wm = oracle.mean_disparity_grid(np.ascontiguousarray(w[y0:y1, x0:x1]))
        assert np.array_equal(means, wm), f"frame {seed}: means differ at {np.argwhere(means != wm)[:5].tolist()}"
        assert (wm != 0).all()


@pytest.mark.parametrize("roi", [ROI, FULL], ids=["roi", "full"])
def test_rectified_pair(gpu, mvsv, oracle, roi):
    m = matcher(mvsv)
    st = mvsv.DisparityStream.raw(m, MAPS, roi=roi, keep_rectified=True)
    L, R = raw_pair(7)
    st.push_raw(L, R)
    d, means, (rl, rr) = st.pop(rectified=True)
    st.close()
    assert means is None
    wl, wr, wd = want(7, roi)
    assert_image(rl, wl, "rectified left vs oracle")
    assert_image(rr, wr, "rectified right vs oracle")
    ol, orr = mvsv.rectify_pair(L, R, MAPS, roi)  # the existing remap kernel
    assert_image(rl, ol, "rectified left vs rectify_pair")
    assert_image(rr, orr, "rectified right vs rectify_pair")
    p = {k: v for k, v in m.params().items() if k != "variant"}
    assert_map(d, oracle.sgbm(rl, rr, p), "map vs oracle on the popped pair")
    assert_map(d, wd, "map vs oracle")
    assert not np.array_equal(wl, wr)


@pytest.mark.parametrize("factor", [0.5, 0.75])
def test_factor(gpu, mvsv, oracle, factor):
    from mvstereovision3_amd.rectify import resize_size
    st = mvsv.DisparityStream.raw(matcher(mvsv, 16), MAPS, roi=ROI, factor=factor, keep_rectified=True, depth=2,
                                  batch=2)
    assert (st.width, st.height) == resize_size(181, 108, factor)
    for seed in (8, 9):
        st.push_raw(*raw_pair(seed))
    for seed in (8, 9):
        d, _, (rl, rr) = st.pop(rectified=True)
        wl, wr, wd = want(seed, ROI, factor, 16)
        assert_image(rl, wl, f"frame {seed}: resized left")
        assert_image(rr, wr, f"frame {seed}: resized right")
        assert_map(d, wd, f"frame {seed}")
    st.close()


def test_inflight_order(gpu, mvsv):
    st = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI, depth=4, batch=2, inflight=2)
    got = []
    for seed in range(8):
        if st.pending() == 4:
            got.append(st.pop()[0])
        st.push_raw(*raw_pair(seed))
    while st.pending():
        got.append(st.pop()[0])
    st.close()
    assert len(got) == 8
    for seed, d in enumerate(got):
        assert_map(d, want(seed)[2], f"frame {seed}")
    assert not np.array_equal(want(0)[2], want(1)[2])  # an order mix-up would show


def _create_raw(mvsv, maps=MAPS, roi=ROI, factor=0.0, raw=(RAW_W, RAW_H), stride=RAW_W, null=None):
    """mvsv_stream_create_raw through ctypes: (rc, handle, ctx, keep-alive)."""
    from mvstereovision3_amd import _lib
    ctx = _lib.context(0)
    ms = [np.ascontiguousarray(a, np.float32) for a in maps]
    r = _lib.Rectification()
    r.raw_width, r.raw_height, r.map_stride = raw[0], raw[1], stride
    for i, a in enumerate(ms):
        r.maps[i] = None if i == null else a.ctypes.data
    r.roi = _lib.Rect(*roi)
    r.factor = factor
    p = matcher(mvsv)._params
    h = ctypes.c_void_p()
    rc = _lib.lib().mvsv_stream_create_raw(ctx.handle, ctypes.byref(r), ctypes.byref(p), 3, None, ctypes.byref(h))
    return rc, h, ctx


@pytest.mark.parametrize("case,kw", [
    ("roi past the right edge", dict(roi=(6, 5, RAW_W + 1, 113))),
    ("roi past the bottom", dict(roi=(6, 5, 187, RAW_H + 1))),
    ("roi negative", dict(roi=(-1, 5, 187, 113))),
    ("roi empty", dict(roi=(6, 5, 6, 113))),
    ("null map", dict(null=2)),
    ("map stride", dict(stride=RAW_W - 1)),
    ("factor negative", dict(factor=-0.5)),
    ("factor to nothing", dict(factor=1e-9)),
    ("factor nan", dict(factor=float("nan"))),
    ("raw too wide", dict(raw=(32768, RAW_H), stride=32768)),
])
def test_misuse_create(gpu, mvsv, case, kw):
    from mvstereovision3_amd import _lib
    rc, h, ctx = _create_raw(mvsv, **kw)
    assert rc == _lib.MVSV_E_INVALID_ARG, case
    assert not h.value
    assert _lib.lib().mvsv_last_error(ctx.handle), case
    # the context goes on working
    st = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI)
    st.push_raw(*raw_pair(0))
    assert_map(st.pop()[0], want(0)[2], f"after {case}")
    st.close()


def test_misuse_push_and_pop(gpu, mvsv):
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    L, R = raw_pair(1)
    # a raw stream of the full frame: a pair of the stream's own size is still no rectified pair
    st = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=FULL)
    assert lib.mvsv_stream_push(st._h, L.ctypes.data, RAW_W, R.ctypes.data, RAW_W) == _lib.MVSV_E_INVALID_ARG
    with pytest.raises(mvsv.MvsvError) as e:
        st.push(L, R)
    assert e.value.code == _lib.MVSV_E_INVALID_ARG and "push_raw" in str(e.value)
    assert st.pending() == 0
    st.push_raw(L, R)
    # rectified outputs need keep_rectified; the frame stays pending
    buf = np.empty((RAW_H, RAW_W), np.uint8)
    assert lib.mvsv_stream_pop_pair(st._h, None, 0, None, buf.ctypes.data, RAW_W, None, 0) == _lib.MVSV_E_INVALID_ARG
    with pytest.raises(mvsv.MvsvError):
        st.pop(rectified=True)
    assert st.pending() == 1
    assert_map(st.pop()[0], want(1, FULL)[2], "raw stream after the refused calls")
    st.close()
    # a stream of rectified pairs refuses raw pairs
    wl, wr, wd = want(1)
    st = mvsv.DisparityStream(matcher(mvsv), 181, 108)
    assert lib.mvsv_stream_push_raw(st._h, wl.ctypes.data, 181, wr.ctypes.data, 181) == _lib.MVSV_E_INVALID_ARG
    with pytest.raises(mvsv.MvsvError) as e:
        st.push_raw(wl, wr)
    assert e.value.code == _lib.MVSV_E_INVALID_ARG
    assert st.pending() == 0
    st.push(wl, wr)
    assert_map(st.pop()[0], wd, "rectified-pair stream after the refused calls")
    w, h = ctypes.c_int(), ctypes.c_int()
    assert lib.mvsv_stream_size(st._h, ctypes.byref(w), ctypes.byref(h)) == 0 and (w.value, h.value) == (181, 108)
    st.close()


def test_set_params_between_frames(gpu, mvsv):
    st = mvsv.DisparityStream.raw(matcher(mvsv, 32), MAPS, roi=ROI, depth=4, batch=4)
    st.push_raw(*raw_pair(2))
    st.push_raw(*raw_pair(3))
    st.set_params(matcher(mvsv, 16))  # frames 2, 3 are pending and keep D = 32
    st.push_raw(*raw_pair(4))
    for seed, D in ((2, 32), (3, 32), (4, 16)):
        assert_map(st.pop()[0], want(seed, D=D)[2], f"frame {seed} (D = {D})")
    st.close()
    assert not np.array_equal(want(4, D=16)[2], want(4, D=32)[2])
