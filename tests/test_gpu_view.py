"""Detection view on the device: view_kernel (behind mvsv_view_device / mvsv_view)
and the view in the frame stream, bit for bit against the numpy restatement in
tests/view_restate.py (tests/test_view.py shows that its near misses -- exclusive
rectangle corners, grids over the found obstacles, lines one pixel short --
differ from it on every all-layers input used here).

Shapes: 9 * dx == W (63), a remainder column that tile 8's inclusive edge reaches
(100), lattice steps 8 and 10 (127 x 31), one lattice point (17 x 16), no lattice
(15 x 9), a row longer than one pass of a wave (2072) and more rows than
blocks x waves (1500); input views on the packed and on the narrow path, output
views for every store width.
"""
import functools
import math

import numpy as np
import pytest

from tests import display_restate
from tests import view_restate as ref
from tests.test_gpu_display import assert_bytes, padded

pytestmark = pytest.mark.gpu

LAYER_SETS = [0, ref.SUBIMAGE_GRID, ref.OBSTACLE_GRID, ref.FOUND_TILES, ref.FOUND_POINTS, ref.ALL]


@functools.lru_cache(maxsize=None)
def case(W, H, seed=0):
    d, kw = ref.all_layers_case(W, H, seed)
    d.setflags(write=False)
    return d, kw


@functools.lru_cache(maxsize=None)
def want_view(W, H, layers, seed=0):
    d, kw = case(W, H, seed)
    img, mm = ref.view(d, **dict(kw, layers=layers))
    img.setflags(write=False)
    return img, mm


def dev_view(gpu, mvsv, t, kw, layers=None, **extra):
    return mvsv.detection_view(t, kw["layers"] if layers is None else layers, means=kw["means"],
                               mean_range=kw["mean_range"], values=kw["values"], sample_range=kw["sample_range"],
                               **extra)


@pytest.mark.parametrize("W,H", ref.SHAPES, ids=lambda v: str(v))
def test_every_layer_alone_and_all_together(gpu, mvsv, W, H):
    d, kw = case(W, H)
    t = gpu.from_numpy(d.copy()).cuda()
    for layers in LAYER_SETS:
        want, mm = want_view(W, H, layers)
        got, gmm = dev_view(gpu, mvsv, t, kw, layers, return_minmax=True)
        assert tuple(got.shape) == (H, W, 3) and got.is_cuda
        assert_bytes(got.cpu().numpy(), want, f"{W}x{H} layers {layers}")
        assert tuple(int(v) for v in gmm.cpu()) == mm
    # the all-layers view shows what it should: red, the grid's blue, and grey
    want = want_view(W, H, ref.ALL)[0]
    flat = want.reshape(-1, 3)
    assert (flat == ref.RED).all(axis=1).any() and (flat == ref.BLUE).all(axis=1).any()
    # numpy in, numpy out: the host entry point
    host, hmm = dev_view(gpu, mvsv, d, kw, return_minmax=True)
    assert isinstance(host, np.ndarray)
    assert_bytes(host, want, f"{W}x{H} host map")
    assert tuple(int(v) for v in hmm) == want_view(W, H, ref.ALL)[1]


def test_consistency_with_the_display_map_and_minmax(gpu, mvsv):
    W, H = 100, 70
    d, kw = case(W, H)
    t = gpu.from_numpy(d.copy()).cuda()
    for alpha, beta in ((0, 255), (32, 224), (224, 32)):
        v, vmm = mvsv.detection_view(t, 0, alpha=alpha, beta=beta, return_minmax=True)
        n = mvsv.normalize_minmax(t, alpha, beta)
        assert gpu.equal(v, n.unsqueeze(-1).expand(H, W, 3))
        assert gpu.equal(vmm, mvsv.minmax(t))
        assert_bytes(v.cpu().numpy(), ref.view(d, 0, alpha=alpha, beta=beta)[0], f"({alpha}, {beta})")
    # a constant map: every pixel saturate(dmin), the layers on top
    const = gpu.full((H, W), -16, dtype=gpu.int16, device="cuda")
    got = dev_view(gpu, mvsv, const, kw).cpu().numpy()
    assert_bytes(got, ref.view(np.full((H, W), -16, np.int16), **kw)[0], "constant map")


@pytest.mark.parametrize("W,H", [(127, 31), (100, 70), (2072, 48)], ids=lambda v: str(v))
def test_input_views_and_every_store_width(gpu, mvsv, W, H):
    """Input views as in the display tests (packed strides with every head length,
    narrow strides); output views at byte offsets 0, 1, 2, 4, 8 with strides 3 W,
    3 W + 5 and the next multiple of 16: 16-, 8-, 4-, 2- and 1-byte stores (2072: more
    than one pass of a wave on each).  The same bytes on every path, and nothing
    outside the view is written."""
    d, kw = case(W, H)
    want = want_view(W, H, ref.ALL)[0]
    if W == 127:
        inputs = [(128, 0), (128, 1), (136, 2), (136, 3), (128, 4), (144, 5), (128, 6), (128, 7),
                  (127, 0), (129, 1), (131, 4), (134, 0)]
    else:
        inputs = [(W, 0), ((W + 15) & ~7, 3), (W + 9 | 1, 1)]
    ostrides = [3 * W, 3 * W + 5, (3 * W + 15) & ~15]
    means = gpu.from_numpy(kw["means"]).cuda()
    values = gpu.from_numpy(kw["values"]).cuda()
    widths = set()
    for stride, offset in inputs:
        view = padded(gpu, d, stride, offset)
        for os_ in ostrides:
            for ooff in (0, 1, 2, 4, 8):
                obuf = gpu.full((H * os_ + 32,), 0xA5, dtype=gpu.uint8, device="cuda")
                out = gpu.as_strided(obuf, (H, W, 3), (os_, 3, 1), ooff)
                res = mvsv.detection_view(view, ref.ALL, means=means, mean_range=ref.MEAN_RANGE, values=values,
                                          sample_range=ref.SAMPLE_RANGE, out=out)
                assert res is out
                o = obuf.cpu().numpy()
                got = np.lib.stride_tricks.as_strided(o[ooff:], (H, W, 3), (os_, 3, 1))
                what = f"stride {stride} offset {offset} -> out stride {os_} offset {ooff}"
                assert_bytes(got, want, what)
                keep = np.ones(o.shape, bool)
                np.lib.stride_tricks.as_strided(keep[ooff:], (H, 3 * W), (os_, 1))[:] = False
                assert (o[keep] == 0xA5).all(), f"{what}: bytes outside the view written"
                if stride % 8 == 0:  # the packed path: groups start 3 * head bytes into a row
                    a = (out.data_ptr() + 3 * (((16 - (view.data_ptr() & 15)) & 15) // 2)) | os_
                    widths.add(16 if a % 16 == 0 else 8 if a % 8 == 0 else 4 if a % 4 == 0 else 2 if a % 2 == 0 else 1)
    assert 16 in widths and (W != 127 or widths == {1, 2, 4, 8, 16}), "the views above do not reach every store width"


def test_degenerate_frames(gpu, mvsv):
    W, H = 100, 70
    d, kw = case(W, H)
    t = gpu.from_numpy(d.copy()).cuda()
    grey = want_view(W, H, 0)[0]
    found = ref.FOUND_TILES | ref.FOUND_POINTS
    nothing = dict(kw, means=np.full(81, 700.0, np.float32), values=np.full_like(kw["values"], 1000.0))
    assert_bytes(dev_view(gpu, mvsv, t, nothing, found).cpu().numpy(), grey, "nothing found")
    assert_bytes(dev_view(gpu, mvsv, t, nothing).cpu().numpy(), ref.view(d, **nothing)[0], "nothing found, grids")
    everything = dict(kw, means=np.full(81, 300.0, np.float32), values=np.full_like(kw["values"], 400.0))
    want = ref.view(d, **everything)[0]
    assert (want[:64, :100] == ref.RED).all()  # 9 * dy = 63, 9 * dx = 99: the tiles cover rows 0..63, columns 0..99
    assert (want[64:] != ref.RED).any()
    assert_bytes(dev_view(gpu, mvsv, t, everything).cpu().numpy(), want, "everything found")
    only_points = dict(everything, layers=ref.FOUND_POINTS)
    assert_bytes(dev_view(gpu, mvsv, t, only_points).cpu().numpy(), ref.view(d, **only_points)[0], "every point found")
    for radius in range(4):
        got = dev_view(gpu, mvsv, t, only_points, point_radius=radius).cpu().numpy()
        assert_bytes(got, ref.view(d, radius=radius, **only_points)[0], f"radius {radius}")
    # ranges that are inf / NaN: the compares decide, nothing is found, nothing faults
    for rng in [(math.nan, 0.0), (0.0, math.nan), (math.nan, math.nan), (math.inf, math.inf),
                (-math.inf, -math.inf), (-math.inf, math.inf)]:
        k = dict(everything, mean_range=rng, sample_range=rng)
        assert_bytes(dev_view(gpu, mvsv, t, k, found).cpu().numpy(), grey, f"range {rng}")
    # and NaN / inf among the means and values themselves
    odd = dict(kw, means=kw["means"].copy(), values=kw["values"].copy())
    odd["means"][[0, 40, 80]] = [math.nan, math.inf, -math.inf]
    odd["values"][[0, 5, -1]] = [math.nan, math.inf, -math.inf]
    assert_bytes(dev_view(gpu, mvsv, t, odd).cpu().numpy(), ref.view(d, **odd)[0], "NaN / inf inputs")


def test_batch_of_three_with_padded_frames(gpu, mvsv):
    """Three frames with different min / max, means and values; input frame stride
    (H + 5) * (W + 9) and output frame stride (H + 3) * (3 W + 7): no multiples of 8."""
    W, H = 100, 70
    cases = [case(W, H, s) for s in range(3)]
    maps = [c[0] + np.int16(37 * s) for s, c in enumerate(cases)]
    maps[1] = np.where(maps[1] > 1500, np.int16(1500), maps[1])
    buf = gpu.full((3, H + 5, W + 9), 777, dtype=gpu.int16, device="cuda")
    view = buf[:, :H, :W]
    for f, m in enumerate(maps):
        view[f] = gpu.from_numpy(np.ascontiguousarray(m)).cuda()
    assert view.stride(0) % 8 != 0
    means = np.stack([c[1]["means"] for c in cases])
    values = np.stack([c[1]["values"] for c in cases])
    assert not np.array_equal(means[0], means[1]) and not np.array_equal(values[0], values[1])
    os_ = 3 * W + 7
    obuf = gpu.full((3, H + 3, os_), 0xA5, dtype=gpu.uint8, device="cuda")
    out = gpu.as_strided(obuf, (3, H, W, 3), ((H + 3) * os_, os_, 3, 1), os_ + 2)
    res, mm = mvsv.detection_view(view, ref.ALL, means=means, mean_range=ref.MEAN_RANGE, values=values,
                                  sample_range=ref.SAMPLE_RANGE, out=out, return_minmax=True)
    assert res is out
    o = obuf.cpu().numpy().reshape(-1)
    keep = np.ones(o.shape, bool)
    mms = set()
    for f in range(3):
        want, wmm = ref.view(np.ascontiguousarray(maps[f]), **dict(cases[f][1]))
        base = f * (H + 3) * os_ + os_ + 2
        got = np.lib.stride_tricks.as_strided(o[base:], (H, W, 3), (os_, 3, 1))
        assert_bytes(got, want, f"frame {f}")
        assert tuple(int(v) for v in mm[f].cpu()) == wmm
        mms.add(wmm)
        np.lib.stride_tricks.as_strided(keep[base:], (H, 3 * W), (os_, 1))[:] = False
        # one frame alone == the same frame in the batch
        alone = mvsv.detection_view(view[f], ref.ALL, means=means[f], mean_range=ref.MEAN_RANGE, values=values[f],
                                    sample_range=ref.SAMPLE_RANGE)
        assert_bytes(alone.cpu().numpy(), want, f"frame {f} alone")
    assert len(mms) == 3
    assert (o[keep] == 0xA5).all(), "bytes outside the output views were written"
    # host batch
    host = mvsv.detection_view(np.stack(maps), ref.ALL, means=means, mean_range=ref.MEAN_RANGE, values=values,
                               sample_range=ref.SAMPLE_RANGE)
    for f in range(3):
        assert_bytes(host[f], ref.view(np.ascontiguousarray(maps[f]), **dict(cases[f][1]))[0], f"host frame {f}")


def test_detectors_may_stand_for_arrays_and_ranges(gpu, mvsv, tmp_path):
    from tests.test_gpu_samplepoint import Q_REF
    W, H = 100, 70
    d, _ = case(W, H)
    t = gpu.from_numpy(d.copy()).cuda()
    md = mvsv.MeanDisparityDetection(pcl_dir=str(tmp_path))
    md.init((H, W), Q_REF, 0.5, 30.0)
    md.build(t)
    sd = mvsv.SamplepointDetection(pcl_dir=str(tmp_path))
    sd.init((H, W), Q_REF, 0.5, 30.0)
    sd.build(t)
    got = mvsv.detection_view(t, ref.ALL, means=md, values=sd).cpu().numpy()
    want = ref.view(d, ref.ALL, np.asarray(md.mMeanMap, np.float32), md.mRangeDisparity,
                    np.asarray(sd.mDistanceVec, np.float32), sd.mRangeDisparity)[0]
    assert_bytes(got, want, "detectors")


def test_validation_on_the_device(gpu, mvsv):
    import ctypes
    from mvstereovision3_amd import _lib
    from tests.test_view import spec_of
    lib, E = _lib.lib(), _lib.MVSV_E_INVALID_ARG
    ctx = _lib.context(0)
    W, H = 100, 70
    t = gpu.from_numpy(case(W, H)[0].copy()).cuda()
    o = gpu.full((H, W, 3), 0xA5, dtype=gpu.uint8, device="cuda")
    f = gpu.zeros(81, dtype=gpu.float32, device="cuda")
    p, q, fp = t.data_ptr(), o.data_ptr(), f.data_ptr()

    def call(spec, n=1, dmap=p, st=W, w=W, h=H, out=q, os_=3 * W):
        return lib.mvsv_view_device(ctx.handle, n, dmap, st, W * H, w, h, ctypes.byref(spec), out, os_, 3 * W * H, None)

    bad = [dict(spec=spec_of(_lib, 16)), dict(spec=spec_of(_lib, 4)), dict(spec=spec_of(_lib, 8)),
           dict(spec=spec_of(_lib, 8, values=fp, radius=4)), dict(spec=spec_of(_lib, 0, alpha=math.nan)),
           dict(spec=spec_of(_lib, 0, beta=math.inf)), dict(spec=spec_of(_lib, 0), os_=3 * W - 1),
           dict(spec=spec_of(_lib, 0), n=0), dict(spec=spec_of(_lib, 0), dmap=None), dict(spec=spec_of(_lib, 0), out=None),
           dict(spec=spec_of(_lib, 0), st=W - 1), dict(spec=spec_of(_lib, 0), w=8), dict(spec=spec_of(_lib, 0), h=8)]
    for k in bad:
        assert call(**k) == E, k
    assert b"9 x 9" in ctypes.cast(lib.mvsv_last_error(ctx.handle), ctypes.c_char_p).value
    assert (o.cpu().numpy() == 0xA5).all(), "a refused call launched"
    assert call(spec_of(_lib, 3)) == 0
    assert_bytes(o.cpu().numpy(), want_view(W, H, 3)[0], "device call without min / max")
    with pytest.raises(mvsv.MvsvError):
        mvsv.detection_view(t, ref.FOUND_TILES)  # no means
    with pytest.raises(mvsv.MvsvError):
        mvsv.detection_view(t, ref.FOUND_TILES, means=np.zeros(80, np.float32), mean_range=(1, 0))
    with pytest.raises(mvsv.MvsvError):
        mvsv.detection_view(t, ref.FOUND_POINTS, values=np.zeros(5, np.float32), sample_range=(1, 0))
    with pytest.raises(mvsv.MvsvError):
        mvsv.detection_view(t, 0, out=gpu.empty((H, W), dtype=gpu.uint8, device="cuda"))


# ---- the frame stream -------------------------------------------------------------------
TW, TH, TD = 100, 70, 16
ROI = (9, 3, 97, 67)  # 88 x 64 at an odd column: dx = 9, dy = 7, lattice 10 x 7


@functools.lru_cache(maxsize=None)
def stream_frames():
    import mvstereovision3_amd as mvsv
    return tuple(mvsv.synth_pair(0x5EED0000 + 900 + i, TW, TH, 0, TD) for i in range(5))


@pytest.mark.parametrize("batch", [1, 2])
def test_stream_brings_the_view_with_every_frame(gpu, mvsv, batch):
    from mvstereovision3_amd import _lib
    from tests.test_gpu_samplepoint import Q_REF
    E = _lib.MVSV_E_INVALID_ARG
    m = mvsv.StereoSGBM.create(0, TD, 9, 648, 2592)
    x0, y0, x1, y1 = ROI
    frames = stream_frames()
    st = mvsv.DisparityStream(m, TW, TH, depth=3, grid_roi=ROI, batch=batch)
    # a first frame without the view: its means give ranges that find about half of the tiles / points
    st.enable_samplepoints((Q_REF, 1e9, -1e9), roi=ROI)
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError) as e:  # the view is off: nothing to bring
        st.front_view()
    assert e.value.code == E and st.pending() == 1
    with pytest.raises(mvsv.MvsvError) as e:  # a frame is pending
        st.enable_view(ref.ALL, roi=ROI, mean_detector_or_range=(1.0, 0.0))
    assert e.value.code == E
    vals0, _, _ = st.front_samples()
    d0, means0 = st.pop()
    mean_range = (float(np.median(means0)) + 0.5, -1.0)
    sample_range = (float(np.median(vals0)) + 0.5, -1.0)
    print(f"ranges: tiles {mean_range}, points {sample_range}")
    st.disable_samplepoints()
    with pytest.raises(mvsv.MvsvError) as e:  # FOUND_POINTS without sample points
        st.enable_view(ref.FOUND_POINTS, roi=ROI)
    assert e.value.code == E
    with pytest.raises(mvsv.MvsvError) as e:  # FOUND_TILES over another ROI than the grid's
        st.enable_view(ref.FOUND_TILES, roi=(8, 3, 97, 67), mean_detector_or_range=mean_range)
    assert e.value.code == E
    st.enable_samplepoints((Q_REF, *sample_range), roi=ROI)
    st.enable_view(ref.ALL, roi=ROI, mean_detector_or_range=mean_range)
    st.enable_display(roi=ROI)
    with pytest.raises(mvsv.MvsvError) as e:  # the view draws the found points
        st.disable_samplepoints()
    assert e.value.code == E
    pushed = 0
    seen = set()
    for i in range(5):
        while pushed < 5 and st.pending() < 3:
            st.push(*frames[pushed])
            pushed += 1
        if st.pending() == 3:
            with pytest.raises(mvsv.MvsvError) as e:  # frames are pending
                st.disable_view()
            assert e.value.code == E
        img, mm = st.front_view()
        img2, mm2 = st.front_view()  # the frame stays pending
        assert np.array_equal(img, img2) and mm == mm2
        pinned, mm3 = st.front_view(copy="view")
        assert not pinned.flags.writeable and pinned.shape == img.shape and np.array_equal(pinned, img) and mm3 == mm
        del pinned
        disp, dmm = st.front_display()  # the display beside it
        vals, count, hits = st.front_samples()
        d, means = st.pop()
        work = np.ascontiguousarray(d[y0:y1, x0:x1])
        kw = dict(means=means, mean_range=mean_range, values=vals, sample_range=sample_range)
        off = mvsv.detection_view(gpu.from_numpy(d).cuda()[y0:y1, x0:x1], ref.ALL, **kw).cpu().numpy()
        assert_bytes(img, off, f"frame {i} vs the off-stream call")
        want, wmm = ref.view(work, ref.ALL, **kw)
        assert_bytes(img, want, f"frame {i} vs the restatement")
        assert mm == wmm == dmm
        assert_bytes(disp, display_restate.normalize(work)[0], f"frame {i}: display map")
        nt, npnt = int(ref.found(means, mean_range).sum()), int(ref.found(vals, sample_range).sum())
        print(f"frame {i}: {nt} tiles, {npnt} points found")
        assert npnt == count
        seen.add((nt > 0, npnt > 0))
    assert (True, True) in seen, "no frame had both found tiles and found points"
    st.enable_view(ref.SUBIMAGE_GRID | ref.OBSTACLE_GRID)  # a second call replaces the first: the whole map, grids only
    st.push(*frames[0])
    img, mm = st.front_view()
    d, _ = st.pop()
    assert np.array_equal(d, d0)
    assert_bytes(img, ref.view(d, 3)[0], "whole map, grids")
    st.disable_samplepoints()  # the view no longer uses them
    st.disable_view()
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError):
        st.front_view()
    st.pop()
    st.close()
