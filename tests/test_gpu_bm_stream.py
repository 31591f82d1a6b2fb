"""StereoBM in the frame stream (mvsv_stream_create_bm, mvsv_stream_set_bm_params,
mvsv_stream_create_raw_bm): every popped map equals the oracle's orc_bm_compute
and the one-shot mvsv_bm of its pair, through frame-batch runs of 3 and 2 across
the ring's wrap and on 1 and 2 compute lanes; every per-frame product (mean grid,
sample points, display map, detection view, point cloud) equals the one-shot
function applied to that frame's map; a stream switches between the matchers
without mixing them in a launch.

Parameter sets: (D 32, blockSize 9, defaults) takes bm_match2_kernel, (D 48,
blockSize 23, NORMALIZED_RESPONSE) the general kernel."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

Q_REF = np.array(json.load(open(os.path.join(GOLDEN, "q_matrix.json")))["Q"], np.float32)
SIZES = [(96, 64), (101, 67)]
PSETS = ["match2", "general"]
RANGE = (1e4, 16.0)  # (first, second): found where 16 < value < 1e4


def bm_matcher(mvsv, pset):
    if pset == "match2":
        return mvsv.StereoBM.create(32, 9)
    b = mvsv.StereoBM.create(48, 23)
    b.setUniquenessRatio(15)
    b.setPreFilterType(mvsv.PREFILTER_NORMALIZED_RESPONSE)
    return b


def sgbm_matcher(mvsv):
    return mvsv.StereoSGBM.create(0, 32, 5, 200, 800, 1, 31, 10, 50, 2, mvsv.MODE_SGBM)


@functools.lru_cache(maxsize=None)
def pair(size, seed):
    import mvstereovision3_amd as mvsv
    L, R = mvsv.synth_pair(0xB0000 + seed, size[0], size[1], 0, 32)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def want_bm(size, pset, seed):
    """The oracle's map, checked once against the one-shot mvsv_bm."""
    from oracle import pyoracle
    import mvstereovision3_amd as mvsv
    b = bm_matcher(mvsv, pset)
    L, R = pair(size, seed)
    w = pyoracle.bm(L, R, b.params())
    one = b.compute(L, R)
    assert np.array_equal(one, w), f"one-shot mvsv_bm differs from the oracle ({size}, {pset}, seed {seed})"
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def want_sgbm(size, seed):
    from oracle import pyoracle
    import mvstereovision3_amd as mvsv
    m = sgbm_matcher(mvsv)
    w = pyoracle.sgbm(*pair(size, seed), {k: v for k, v in m.params().items() if k != "variant"})
    assert np.array_equal(m.compute(*pair(size, seed)), w)
    w.setflags(write=False)
    return w


def assert_map(got, w, what):
    bad = np.argwhere(got != w)
    assert got.shape == w.shape and bad.size == 0, f"{what}: {len(bad)} mismatches, first {bad[:5].tolist()}"


@pytest.mark.parametrize("inflight", [1, 2])
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maps_and_products(gpu, mvsv, size, pset, inflight):
    from mvstereovision3_amd import _lib
    W, H = size
    whole = (0, 0, W, H)
    layers = mvsv.VIEW_SUBIMAGE_GRID | mvsv.VIEW_OBSTACLE_GRID | mvsv.VIEW_FOUND_TILES | mvsv.VIEW_FOUND_POINTS
    st = mvsv.DisparityStream(bm_matcher(mvsv, pset), W, H, depth=5, grid_roi=whole, batch=3, inflight=inflight)
    assert st.matcher() == _lib.MATCHER_BM == mvsv.MATCHER_BM
    st.enable_samplepoints((Q_REF, *RANGE), roi=whole)
    st.enable_display()
    st.enable_view(layers, roi=whole, mean_detector_or_range=RANGE)
    st.enable_cloud(Q_REF)
    got = []

    def pop():
        vals, count, hits = st.front_samples()
        disp, dmm = st.front_display()
        img, vmm = st.front_view()
        rec, ccount, cmm = st.front_cloud(return_minmax=True)
        d, means = st.pop()
        got.append((d, means, vals, count, hits, disp, dmm, img, vmm, rec, ccount, cmm))

    for seed in range(8):  # runs of 3 and 2 end at the ring's end; the next ones start at slot 0 again
        if st.pending() == 5:
            pop()
        st.push(*pair(size, seed))
    while st.pending():
        pop()
    st.close()
    assert len(got) == 8
    filtered = (bm_matcher(mvsv, pset).getMinDisparity() - 1) * 16
    for seed, (d, means, vals, count, hits, disp, dmm, img, vmm, rec, ccount, cmm) in enumerate(got):
        w = want_bm(size, pset, seed)
        assert_map(d, w, f"frame {seed}")
        assert (w == filtered).any(), "the map should hold FILTERED pixels"
        assert pset != "match2" or (w > 0).mean() > 0.25, "the map should hold valid pixels"
        t = gpu.from_numpy(np.array(w)).cuda()
        assert np.array_equal(means, mvsv.mean_disparity_grid(t).cpu().numpy()), f"frame {seed}: means"
        ov = mvsv.samplepoint_values(t, 2)
        assert np.array_equal(vals, ov.cpu().numpy()), f"frame {seed}: lattice values"
        oc, oh = mvsv.samplepoint_detect(ov, (H, W), Q_REF, RANGE)
        assert count == int(oc) == len(hits), f"frame {seed}: hit count"
        assert hits.tobytes() == oh.cpu().numpy()[:count].tobytes(), f"frame {seed}: hit records"
        od, omm = mvsv.normalize_minmax(t, return_minmax=True)
        assert np.array_equal(disp, od.cpu().numpy()) and dmm == tuple(int(v) for v in omm.cpu()), f"frame {seed}: display"
        oi, oimm = mvsv.detection_view(t, layers, means=means, mean_range=RANGE, values=vals, sample_range=RANGE,
                                       return_minmax=True)
        assert np.array_equal(img, oi.cpu().numpy()) and vmm == tuple(int(v) for v in oimm.cpu()), f"frame {seed}: view"
        orec, omm2 = mvsv.point_cloud(np.array(w), Q_REF, return_minmax=True)
        assert ccount == len(orec) == int((w > 0).sum()) and cmm == (int(omm2[0]), int(omm2[1])), f"frame {seed}: cloud"
        assert rec.tobytes() == orec.tobytes(), f"frame {seed}: cloud records"
    assert not np.array_equal(want_bm(size, pset, 0), want_bm(size, pset, 1))  # an order mix-up would show


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_switching_matchers(gpu, mvsv, size):
    """SGBM frame, set_params(StereoBM), BM frame, set_params(StereoSGBM), SGBM frame;
    pops only at the end.  batch = 3 would put all three into one launch: each
    switch launches what is pending first, so no launch mixes matchers."""
    W, H = size
    st = mvsv.DisparityStream(sgbm_matcher(mvsv), W, H, depth=4, batch=3)
    assert st.matcher() == mvsv.MATCHER_SGBM
    st.push(*pair(size, 0))
    st.set_params(bm_matcher(mvsv, "match2"))
    assert st.matcher() == mvsv.MATCHER_BM and st.pending() == 1
    st.push(*pair(size, 1))
    st.set_params(sgbm_matcher(mvsv))
    assert st.matcher() == mvsv.MATCHER_SGBM
    st.push(*pair(size, 2))
    st.set_params(bm_matcher(mvsv, "general"))  # BM with other parameters, and twice in a row
    st.set_params(bm_matcher(mvsv, "general"))
    st.push(*pair(size, 3))
    assert st.pending() == 4
    assert_map(st.pop()[0], want_sgbm(size, 0), "frame 0 (SGBM)")
    assert_map(st.pop()[0], want_bm(size, "match2", 1), "frame 1 (BM)")
    assert_map(st.pop()[0], want_sgbm(size, 2), "frame 2 (SGBM)")
    assert_map(st.pop()[0], want_bm(size, "general", 3), "frame 3 (BM, general kernel)")
    st.close()


def test_refused_parameters_leave_the_stream_as_it_was(gpu, mvsv):
    from mvstereovision3_amd import _lib
    size = SIZES[0]
    st = mvsv.DisparityStream(sgbm_matcher(mvsv), *size)
    bad = bm_matcher(mvsv, "match2")
    bad.setBlockSize(10)
    with pytest.raises(mvsv.MvsvError) as e:
        st.set_params(bad)
    assert e.value.code == _lib.MVSV_E_INVALID_ARG and st.matcher() == mvsv.MATCHER_SGBM
    wide = mvsv.StereoBM.create(32, 65)  # a block larger than the 64-row frame
    with pytest.raises(mvsv.MvsvError):
        st.set_params(wide)
    with pytest.raises(mvsv.MvsvError):
        st.set_params(object())
    st.push(*pair(size, 0))
    assert_map(st.pop()[0], want_sgbm(size, 0), "after the refused calls")
    st.close()
    with pytest.raises(mvsv.MvsvError):
        mvsv.DisparityStream(bad, *size)
    with pytest.raises(mvsv.MvsvError):
        mvsv.DisparityStream(object(), *size)
    lib, ctx = _lib.lib(), _lib.context(0)
    h = ctypes.c_void_p()
    assert lib.mvsv_stream_create_bm(ctx.handle, size[0], size[1], None, 3, None, ctypes.byref(h)) == _lib.MVSV_E_INVALID_ARG
    assert not h.value and lib.mvsv_stream_matcher(None) == -1


def test_raw_bm_stream(gpu, mvsv, oracle):
    """Raw camera pairs into a StereoBM stream: mvsv_rectify_pair, then mvsv_bm."""
    from tests.test_gpu_raw_stream import GRID, MAPS, ROI, raw_pair
    b = bm_matcher(mvsv, "match2")
    st = mvsv.DisparityStream.raw(b, MAPS, roi=ROI, depth=4, batch=3, grid_roi=GRID)
    assert st.matcher() == mvsv.MATCHER_BM and (st.width, st.height) == (181, 108)
    for seed in range(4):
        st.push_raw(*raw_pair(seed))
    x0, y0, x1, y1 = GRID
    maps = []
    for seed in range(4):
        d, means = st.pop()
        rl, rr = mvsv.rectify_pair(*raw_pair(seed), MAPS, ROI)
        w = b.compute(rl, rr)
        assert_map(d, w, f"frame {seed} vs rectify_pair + mvsv_bm")
        assert_map(d, oracle.bm(rl, rr, b.params()), f"frame {seed} vs the oracle")
        assert np.array_equal(means, oracle.mean_disparity_grid(np.ascontiguousarray(w[y0:y1, x0:x1])))
        assert (w > 0).any()
        maps.append(d)
    st.set_params(sgbm_matcher(mvsv))  # a raw stream switches too
    st.push_raw(*raw_pair(0))
    rl, rr = mvsv.rectify_pair(*raw_pair(0), MAPS, ROI)
    assert_map(st.pop()[0], sgbm_matcher(mvsv).compute(rl, rr), "SGBM frame on the raw BM stream")
    st.close()
    assert not np.array_equal(maps[0], maps[1])
