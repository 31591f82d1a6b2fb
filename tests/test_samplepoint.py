"""SamplepointDetection mirror: layout and host decisions (no GPU).

Reference: src/SamplePointDetection.cpp:29-75 (init), :134-178 (detectObstacles),
inc/Samplepoint.h:17-40.  The lattice values are supplied directly here (their
kernel is checked in test_gpu_samplepoint.py); these tests pin the layout, the
range, the host decision and the PLY counter against tests/samplepoint_restate.py.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import samplepoint_restate as ref
from tests.conftest import GOLDEN
from tests.test_kernel_scratch import LIB, LLVM, kernel_scratch

Q_REF = np.array(json.load(open(os.path.join(GOLDEN, "q_matrix.json")))["Q"], np.float32)


@pytest.mark.parametrize("W,H,want", [
    (1280, 960, (8, 8, 159, 119)),
    (752, 480, (8, 8, 93, 59)),
    (688, 480, (8, 8, 85, 59)),
    (100, 70, (8, 8, 11, 7)),
    (63, 47, (9, 9, 6, 4)),
    (127, 31, (8, 10, 14, 2)),
])
def test_layout(mvsv, W, H, want):
    assert mvsv.samplepoint_layout(W, H) == want
    assert ref.layout(W, H) == want
    assert len(ref.centres(W, H)) == want[2] * want[3]


def test_layout_without_points(mvsv):
    from mvstereovision3_amd import _lib
    sx, sy, nx, ny = mvsv.samplepoint_layout(15, 100)
    assert nx * ny == 0 and ref.centres(15, 100) == []
    assert mvsv.samplepoint_layout(100, 15)[2] * mvsv.samplepoint_layout(100, 15)[3] == 0
    v = [ctypes.c_int() for _ in range(4)]
    assert _lib.lib().mvsv_samplepoint_layout(0, 100, *[ctypes.byref(x) for x in v]) == _lib.MVSV_E_INVALID_ARG
    d = mvsv.SamplepointDetection()
    d.init((100, 15), Q_REF, 0.1, 1.5)
    assert d.getSamplepointVec() == [] and d.getFoundObstacles() == []


@pytest.mark.parametrize("W,H", [(100, 70), (63, 47), (127, 31)])
def test_centres_are_column_major(mvsv, W, H):
    d = mvsv.SamplepointDetection()
    d.init((H, W), Q_REF, 0.1, 1.5)
    got = [s.center for s in d.getSamplepointVec()]
    assert got == ref.centres(W, H)
    sx, sy, nx, ny = mvsv.samplepoint_layout(W, H)
    assert got[0] == (sx, sy) and got[1] == (sx, 2 * sy) and got[ny] == (2 * sx, sy)
    s = d.getSamplepointVec()[0]
    assert s.radius == 2 and s.roi == (sx - 2, sy - 2, 5, 5)


def test_init_range_layout_and_getters(mvsv):
    d = mvsv.SamplepointDetection()
    d.init((480, 752 - 64), Q_REF, 0.1, 1.5)
    q = Q_REF.reshape(4, 4)
    for z, got in ((100.0, d.mRangeDisparity[0]), (1500.0, d.mRangeDisparity[1])):
        disp = np.float32((np.float32(q[2, 3]) - np.float32(z) * np.float32(q[3, 3])) /
                          (np.float32(z) * np.float32(q[3, 2])))
        assert np.float32(got).view(np.uint32) == np.float32(disp * np.float32(16)).view(np.uint32)
    assert d.getRangeDisparity() == d.mRangeDisparity
    # the whole layout, for the visualisation, until the first detectObstacles
    assert [s.center for s in d.getFoundObstacles()] == ref.centres(688, 480)
    assert np.array_equal(d.getCenterPoint(), np.array([0, 0, 1, 0], np.float32))
    # setRange is stored (and truncated by the getter) but detection never reads it
    before = d.mRangeDisparity
    d.setRange(0.9, 2.7)
    assert d.getRange() == (0, 2) and d.mRangeDisparity == before
    d.setRange(3.999, 120.5)
    assert d.getRange() == (3, 120)


def test_samplepoint_value_rule(mvsv, oracle):
    """Samplepoint.calculateSamplepointValue: the mean grid's rule on the patch for
    radius > 0 (cross-checked on single patches), the raw centre for radius 0."""
    rng = np.random.default_rng(5)
    dmap = ref.make_map(rng, 70, 100)
    want = ref.values(dmap, 2)
    for i, (cx, cy) in enumerate(ref.centres(100, 70)):
        s = mvsv.Samplepoint((cx, cy), 2)
        s.calculateSamplepointValue(dmap)
        assert np.float32(s.value) == want[i]
        # a map that is one patch in each of its 9x9 tiles... the grid rule on the patch alone
        patch = np.ascontiguousarray(np.tile(dmap[cy - 2:cy + 3, cx - 2:cx + 3], (9, 9)))
        assert oracle.mean_disparity_grid(patch)[0] == want[i]
        s0 = mvsv.Samplepoint((cx, cy), 0)
        s0.calculateSamplepointValue(dmap)
        assert s0.value == float(dmap[cy, cx])
    assert (want == 0).any() and (ref.values(dmap, 0) < 0).any()


def _detector(mvsv, tmp_path, H=480, W=688):
    d = mvsv.SamplepointDetection(pcl_dir=str(tmp_path))
    d.init((H, W), Q_REF, 0.1, 1.5)
    return d


def test_detect_obstacles_bounds_points_and_ply(mvsv, tmp_path):
    from mvstereovision3_amd.utility import Utility, dMapValues
    d = _detector(mvsv, tmp_path)
    first, second = (np.float32(v) for v in d.mRangeDisparity)
    assert second < first
    n = len(d.getSamplepointVec())
    rng = np.random.default_rng(11)
    vals = rng.uniform(float(second) - 40, float(first) + 40, n).astype(np.float32)
    big, small = np.float32(1e9), np.float32(-1e9)
    edge = [first, second, np.nextafter(first, big), np.nextafter(first, small),
            np.nextafter(second, big), np.nextafter(second, small)]
    vals[:6] = edge
    vals[-6:] = edge
    dmap = np.full((480, 688), 200, np.int16)
    d.build(dmap, 0, 0, values=vals)
    assert [s.value for s in d.getSamplepointVec()] == [float(v) for v in vals]
    d.detectObstacles()
    want = ref.hits(vals, first, second)
    assert 3 in want and 4 in want and not {0, 1, 2, 5} & set(want)
    assert n - 3 in want and n - 2 in want and not {n - 6, n - 5, n - 4, n - 1} & set(want)
    assert len(want) > 100
    cs = ref.centres(688, 480)
    assert [s.center for s in d.getFoundObstacles()] == [cs[i] for i in want]
    assert [s.value for s in d.getFoundObstacles()] == [float(vals[i]) for i in want]
    pts = d.getFoundPoints()
    assert len(pts) == len(want)
    for got, i in zip(pts, want):
        w = Utility.calcCoordinate(dMapValues(vals[i], cs[i][0], cs[i][1]), d.mQ_32F)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), w.view(np.uint32))
    assert (tmp_path / "pcl_0000.ply").exists() and d.getObstacleCounter() == 1
    text = (tmp_path / "pcl_0000.ply").read_text()
    assert text.startswith("ply\nformat ascii 1.0\ncomment author: Hagen Hiller")
    assert f"element vertex {len(want)}\n" in text
    d.detectObstacles()
    assert (tmp_path / "pcl_0001.ply").exists() and d.getObstacleCounter() == 2


def test_detect_obstacles_without_hit_writes_nothing(mvsv, tmp_path):
    d = _detector(mvsv, tmp_path, 70, 100)
    first, second = d.mRangeDisparity
    n = len(d.getSamplepointVec())
    vals = np.full(n, first, np.float32)
    vals[::2] = second
    d.build(np.full((70, 100), 200, np.int16), 0, 0, values=vals)
    d.detectObstacles()
    assert d.getFoundObstacles() == [] and d.getFoundPoints() == []
    assert d.getObstacleCounter() == 0 and list(tmp_path.iterdir()) == []


def test_detect_obstacles_from_hit_records(mvsv, tmp_path):
    """detectObstacles(hits=...) takes a stream frame's records for the decision: the
    same obstacles, points and PLY bytes as the host path when the records are what
    the host would have found."""
    from mvstereovision3_amd.utility import Utility, dMapValues
    a = _detector(mvsv, tmp_path / "a", 70, 100)
    b = _detector(mvsv, tmp_path / "b", 70, 100)
    os.makedirs(a.pcl_dir)
    os.makedirs(b.pcl_dir)
    first, second = (np.float32(v) for v in a.mRangeDisparity)
    n = len(a.getSamplepointVec())
    vals = np.linspace(float(second) - 5, float(first) + 5, n).astype(np.float32)
    dmap = np.full((70, 100), 200, np.int16)
    a.build(dmap, 0, 0, values=vals)
    b.build(dmap, 0, 0, values=vals)
    a.detectObstacles()
    want = ref.hits(vals, first, second)
    rec = np.zeros(len(want), mvsv.SAMPLE_HIT_DTYPE)
    cs = ref.centres(100, 70)
    for k, i in enumerate(want):
        p = Utility.calcCoordinate(dMapValues(vals[i], cs[i][0], cs[i][1]), a.mQ_32F)
        rec[k] = (i, p[0], p[1], p[2])
    b.detectObstacles(hits=(len(want), rec))
    assert len(want) > 10
    assert [s.center for s in b.getFoundObstacles()] == [s.center for s in a.getFoundObstacles()]
    assert np.array_equal(np.stack(a.getFoundPoints()).view(np.uint32), np.stack(b.getFoundPoints()).view(np.uint32))
    assert open(os.path.join(a.pcl_dir, "pcl_0000.ply"), "rb").read() == \
        open(os.path.join(b.pcl_dir, "pcl_0000.ply"), "rb").read()


def test_build_rejects_wrong_sizes(mvsv):
    d = mvsv.SamplepointDetection()
    d.init((70, 100), Q_REF, 0.1, 1.5)
    rec = np.zeros(1, mvsv.SAMPLE_HIT_DTYPE)
    with pytest.raises(mvsv.MvsvError):  # hit records need build()'s values first
        d.detectObstacles(hits=(1, rec))
    assert len(d.getFoundObstacles()) == 77  # untouched: still the layout
    with pytest.raises(mvsv.MvsvError):
        d.build(np.zeros((70, 100), np.int16), 0, 0, values=np.zeros(5, np.float32))
    with pytest.raises(mvsv.MvsvError):
        d.build(np.zeros((80, 100), np.int16), 0, 0)


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"),
                    reason="library not built / no ROCm llvm tools")
def test_samplepoint_kernels_have_no_scratch():
    ks = kernel_scratch()
    for pat in (r"sample_grid_kernel", r"sample_detect_kernel", r"reproject_kernel"):
        picked = {k: v for k, v in ks.items() if re.search(pat, k)}
        assert picked, f"no kernel matches {pat}"
        assert not any(picked.values()), f"kernels with scratch: {picked}"
