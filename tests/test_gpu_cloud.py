"""Point clouds on the device (mvsv_point_cloud_device and what is built on it)
against the numpy restatement in tests/cloud_restate.py, bit for bit: the records
of the pixels with v > 0 in raster order, their count and (min, max), nothing
written behind min(count, capacity) or into another frame's slot (the output is
pre-filled with a sentinel), the same bytes on the packed and the narrow row path
and on every run; the host entry points, Utility.dmap2pcl from a device tensor,
and both kinds of frame stream.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import pyoracle
from tests import cloud_restate as ref
from tests.test_cloud import LADDER_SHAPE, LADDERS, Q_REF

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def want_cloud(key):
    """(records, (mn, mx)) of a map made by MAPS[key]() -- computed once."""
    return ref.cloud(host_map(key), Q_REF, pyoracle.reproject)


def _with_extremes(d):
    """-16, 0, 1 and 32767 somewhere in a map that has room for them."""
    f = d.reshape(-1)
    if f.size >= 8:
        at = (np.arange(4) * f.size) // 4 + 1
        f[at] = [-16, 0, 1, 32767]
    return d


MAPS = {
    "1x1 valid": lambda: np.array([[345]], np.int16),
    "1x1 invalid": lambda: np.array([[-16]], np.int16),
    "257x1": lambda: _with_extremes(ref.random_map(11, (1, 257))),
    "64x4": lambda: _with_extremes(ref.random_map(12, (4, 64))),
    "100x70": lambda: _with_extremes(ref.random_map(13, (70, 100))),
    # a row is a tile of the scan: 4099 per frame, more than the scan block's
    # width (256 rows per step), so its loop runs 17 times and carries the base over
    "3x4099": lambda: _with_extremes(ref.random_map(14, (4099, 3))),
    "640x480": lambda: _with_extremes(ref.random_map(15, (480, 640), valid=0.5)),
    "100x70 none": lambda: np.where(np.arange(7000) % 3 == 0, -16, 0).astype(np.int16).reshape(70, 100),
    "100x70 all": lambda: ref.random_map(16, (70, 100), valid=1.0),
    "100x70 const": lambda: np.full((70, 100), 500, np.int16),
    "67x5": lambda: _with_extremes(ref.random_map(17, (5, 67))),
}


@functools.lru_cache(maxsize=None)
def host_map(key):
    d = MAPS[key]()
    d.flags.writeable = False
    return d


def run(gpu, mvsv, view, cap=None):
    """point_cloud of a device view into a sentinel-filled output: (int32 words
    (N, cap, 4) on the host, counts, minmax pairs)."""
    n = view.shape[0] if view.dim() == 3 else 1
    H, W = view.shape[-2:]
    cap = H * W if cap is None else cap
    buf = gpu.full((n, cap, 4) if view.dim() == 3 else (cap, 4), SENTINEL, dtype=gpu.int32, device="cuda")
    out, counts, mm = mvsv.point_cloud(view, Q_REF, return_minmax=True, out=buf.view(gpu.float32))
    assert out.data_ptr() == buf.data_ptr()
    words = buf.cpu().numpy().reshape(n, cap, 4)
    return words, [int(c) for c in counts.cpu().reshape(-1)], [tuple(int(v) for v in p) for p in mm.cpu().reshape(-1, 2)]


def assert_frame(words, count, mm, want, wmm, what):
    """One frame's slot: the first min(count, cap) records are the restatement's, the rest is untouched."""
    cap = len(words)
    assert count == len(want), f"{what}: count {count}, restatement {len(want)}"
    assert mm == wmm, f"{what}: min / max {mm}, restatement {wmm}"
    k = min(count, cap)
    got = words[:k].view(ref.CLOUD_DTYPE).reshape(-1)
    if not ref.same_bytes(got, want[:k]):
        bad = np.flatnonzero((words[:k] != want[:k].view(np.int32).reshape(-1, 4)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {k} records differ, first at {bad[:3].tolist()}: "
                             f"{got[bad[:3]].tolist()} != {want[bad[:3]].tolist()}")
    assert (words[k:] == SENTINEL).all(), f"{what}: words behind record {k} were written"


def upload(gpu, d):
    return gpu.from_numpy(np.array(d)).cuda()


def padded(gpu, frames, stride, frame_pad=0, offset=0):
    """Host maps of one shape on the device as a batch view with the given row
    stride, `frame_pad` elements between frames, `offset` elements into the
    buffer; everything around the maps is 777 (positive: a stray read would count)."""
    n = len(frames)
    H, W = frames[0].shape
    fs = H * stride + frame_pad
    buf = gpu.full((n * fs + offset + 16,), 777, dtype=gpu.int16, device="cuda")
    view = gpu.as_strided(buf, (n, H, W), (fs, stride, 1), offset)
    view.copy_(gpu.from_numpy(np.stack(frames)).cuda())
    return view


SHAPE_KEYS = ["1x1 valid", "1x1 invalid", "257x1", "64x4", "100x70", "3x4099", "640x480"]


@pytest.mark.parametrize("key", SHAPE_KEYS)
def test_shapes(gpu, mvsv, key):
    d = host_map(key)
    want, wmm = want_cloud(key)
    if key == "640x480":
        assert 0.45 < len(want) / d.size < 0.55
    if d.size >= 8:
        assert {-16, 0, 1, 32767} <= set(np.unique(d).tolist()) and wmm == (1, 32767)
    words, counts, mm = run(gpu, mvsv, upload(gpu, d))
    assert_frame(words[0], counts[0], mm[0], want, wmm, key)
    again, counts2, mm2 = run(gpu, mvsv, upload(gpu, d))
    assert again.tobytes() == words.tobytes() and counts2 == counts and mm2 == mm, f"{key}: two runs differ"


def test_batch_of_none_all_and_random(gpu, mvsv):
    keys = ["100x70 none", "100x70 all", "100x70"]
    view = upload(gpu, np.stack([host_map(k) for k in keys]))
    words, counts, mm = run(gpu, mvsv, view)
    for f, k in enumerate(keys):
        assert_frame(words[f], counts[f], mm[f], *want_cloud(k), k)
    assert counts[0] == 0 and mm[0] == (32767, -32768) and (words[0] == SENTINEL).all()
    assert counts[1] == 7000


def test_constant_frame_greys_are_int32_min(gpu, mvsv):
    keys = ["100x70", "100x70 const"]
    words, counts, mm = run(gpu, mvsv, upload(gpu, np.stack([host_map(k) for k in keys])))
    for f, k in enumerate(keys):
        assert_frame(words[f], counts[f], mm[f], *want_cloud(k), k)
    assert mm[1] == (500, 500) and counts[1] == 7000 and (words[1][:, 3] == ref.INT32_MIN).all()


def test_ladders_pin_the_grey(gpu, mvsv):
    """The ladders on which a grey wholly in double, or a reciprocal multiply, would show."""
    frames = [ref.ladder(lo, hi, LADDER_SHAPE) for lo, hi in LADDERS]
    words, counts, mm = run(gpu, mvsv, upload(gpu, np.stack(frames)))
    for f, d in enumerate(frames):
        want, wmm = ref.cloud(d, Q_REF, pyoracle.reproject)
        assert_frame(words[f], counts[f], mm[f], want, wmm, f"ladder {LADDERS[f]}")


@pytest.mark.parametrize("pad_w", [9, 12], ids=["narrow", "packed"])
def test_batch_with_padded_frames_and_rows(gpu, mvsv, pad_w):
    keys = ["100x70 all", "100x70", "100x70 none"]
    frames = [host_map(k) for k in keys]
    view = padded(gpu, frames, 100 + pad_w, frame_pad=8 if pad_w == 12 else 5)
    words, counts, mm = run(gpu, mvsv, view)
    for f, k in enumerate(keys):
        assert_frame(words[f], counts[f], mm[f], *want_cloud(k), f"{k}, rows padded by {pad_w}")


def test_odd_view_of_a_wider_map(gpu, mvsv):
    """A 67 x 5 view at an odd column of a wider map: 2-byte loads only, and
    x / y count from the view's corner."""
    d = host_map("67x5")
    wide = gpu.full((9, 131), 777, dtype=gpu.int16, device="cuda")
    view = wide[2:7, 21:88]
    view.copy_(upload(gpu, d))
    assert view.data_ptr() % 4 == 2 and view.stride(0) == 131
    words, counts, mm = run(gpu, mvsv, view)
    assert_frame(words[0], counts[0], mm[0], *want_cloud("67x5"), "odd view")
    want = want_cloud("67x5")[0]
    pts = pyoracle.reproject(d, Q_REF)
    r, c = np.argwhere(d > 0)[0]
    assert (want["x"][0], want["y"][0]) == (pts[r, c, 0], pts[r, c, 1])


def test_capacity_truncates_and_counts_stay_whole(gpu, mvsv):
    keys = ["100x70", "100x70 all", "100x70 none"]
    view = upload(gpu, np.stack([host_map(k) for k in keys]))
    count = len(want_cloud("100x70")[0])
    for cap in (count, count - 1, 1):
        words, counts, mm = run(gpu, mvsv, view, cap=cap)
        assert counts == [count, 7000, 0]
        for f, k in enumerate(keys):
            assert_frame(words[f], counts[f], mm[f], *want_cloud(k), f"{k}, capacity {cap}")
    rec, c = mvsv.point_cloud(view[0], Q_REF, max_points=5)
    assert rec.shape == (5, 4) and int(c) == count
    assert rec.view(gpu.int32)[:, 3].cpu().numpy().tolist() == want_cloud("100x70")[0]["grey"][:5].tolist()


def test_packed_and_narrow_paths_give_the_same_bytes(gpu, mvsv):
    d = host_map("100x70")
    want, wmm = want_cloud("100x70")
    results = set()
    # stride % 8 == 0: packed, with a head of 0..7 elements by the offset; others: narrow
    for stride, offset in [(104, 0), (104, 1), (104, 3), (104, 7), (112, 4), (100, 0), (101, 0), (103, 5), (108, 2)]:
        view = padded(gpu, [d], stride, offset=offset)[0]
        words, counts, mm = run(gpu, mvsv, view)
        assert_frame(words[0], counts[0], mm[0], want, wmm, f"stride {stride} offset {offset}")
        results.add(words.tobytes())
    assert len(results) == 1


def test_host_entry_point_and_validation(gpu, mvsv):
    from mvstereovision3_amd import _lib
    lib, E = _lib.lib(), _lib.MVSV_E_INVALID_ARG
    ctx = _lib.context(0)
    d = host_map("100x70")
    want, wmm = want_cloud("100x70")
    rec, mm = mvsv.point_cloud(d, Q_REF, return_minmax=True)
    assert rec.dtype == mvsv.CLOUD_DTYPE and ref.same_bytes(rec, want) and tuple(int(v) for v in mm) == wmm
    assert ref.same_bytes(mvsv.point_cloud(d, Q_REF, max_points=9), want[:9])
    wide = np.full((70, 111), 777, np.int16)  # a strided host map
    wide[:, 4:104] = d
    assert ref.same_bytes(mvsv.point_cloud(wide[:, 4:104], Q_REF), want)
    assert len(mvsv.point_cloud(host_map("100x70 none"), Q_REF)) == 0
    # the C call: a short buffer gets the prefix, the count stays whole, nothing behind is written
    buf = np.full((12, 4), SENTINEL, np.int32)
    n = ctypes.c_int(-1)
    q = np.ascontiguousarray(Q_REF)
    assert lib.mvsv_point_cloud(ctx.handle, d.ctypes.data, 100, 100, 70, q.ctypes.data, buf.ctypes.data, 10,
                                ctypes.byref(n), None) == 0
    assert n.value == len(want) and ref.same_bytes(buf[:10].view(ref.CLOUD_DTYPE).reshape(-1), want[:10])
    assert (buf[10:] == SENTINEL).all()
    p, r = d.ctypes.data, buf.ctypes.data
    for a in [(None, 100, 100, 70, q.ctypes.data, r, 10), (p, 100, 100, 70, None, r, 10),
              (p, 100, 100, 70, q.ctypes.data, None, 10), (p, 100, 0, 70, q.ctypes.data, r, 10),
              (p, 100, 100, 0, q.ctypes.data, r, 10), (p, 99, 100, 70, q.ctypes.data, r, 10),
              (p, 100, 100, 70, q.ctypes.data, r, 0)]:
        assert lib.mvsv_point_cloud(ctx.handle, *a, ctypes.byref(n), None) == E, a
    assert lib.mvsv_point_cloud(ctx.handle, p, 100, 100, 70, q.ctypes.data, r, 10, None, None) == E
    t = upload(gpu, d)
    o = gpu.empty((7000, 4), dtype=gpu.float32, device="cuda")
    c = gpu.empty((1,), dtype=gpu.int32, device="cuda")
    tp, op, cp = t.data_ptr(), o.data_ptr(), c.data_ptr()
    for a in [(0, tp, 100, 7000, 100, 70, q.ctypes.data, op, 7000, cp), (1, None, 100, 7000, 100, 70, q.ctypes.data, op, 7000, cp),
              (1, tp, 100, 7000, 100, 70, None, op, 7000, cp), (1, tp, 100, 7000, 100, 70, q.ctypes.data, None, 7000, cp),
              (1, tp, 100, 7000, 100, 70, q.ctypes.data, op, 7000, None), (1, tp, 99, 7000, 100, 70, q.ctypes.data, op, 7000, cp),
              (1, tp, 100, 7000, 0, 70, q.ctypes.data, op, 7000, cp), (1, tp, 100, 7000, 100, -1, q.ctypes.data, op, 7000, cp),
              (1, tp, 100, 7000, 100, 70, q.ctypes.data, op, 0, cp), (1, tp, 100, 7000, 100, 70, q.ctypes.data, op + 4, 7000, cp)]:
        assert lib.mvsv_point_cloud_device(ctx.handle, *a, None) == E, a
    assert b"point cloud" in ctypes.cast(lib.mvsv_last_error(ctx.handle), ctypes.c_char_p).value
    for bad in (gpu.zeros((4, 4), dtype=gpu.float32, device="cuda"), np.zeros((4, 4), np.float32)):
        with pytest.raises(mvsv.MvsvError):
            mvsv.point_cloud(bad, Q_REF)
    with pytest.raises(mvsv.MvsvError):
        mvsv.point_cloud(t, Q_REF, max_points=0)


def test_dmap2pcl_from_a_device_tensor_and_from_numpy(gpu, mvsv, tmp_path):
    d = host_map("100x70")
    want, _ = want_cloud("100x70")
    predicted = str(tmp_path / "predicted.ply")
    xyz = np.stack([want["x"], want["y"], want["z"]], axis=1)
    assert mvsv.ply("Hagen Hiller", "disparity pointcloud", d).write(predicted, xyz, mvsv.ply.WITH_COLOR)
    text = open(predicted).read()
    greys = [int(ln.split()[3]) for ln in text.split("end_header\n")[1].splitlines()]
    assert greys == want["grey"].tolist()  # what the file holds is what the records hold
    for name, arg in [("numpy", d), ("device", upload(gpu, d)),
                      ("device view", padded(gpu, [d], 131, offset=3)[0])]:
        path = str(tmp_path / f"{name}.ply")
        mvsv.Utility.dmap2pcl(path, arg, Q_REF)
        assert open(path).read() == text, name
    for arg in (host_map("100x70 none"), upload(gpu, host_map("100x70 none"))):
        with pytest.raises(mvsv.MvsvError) as e:
            mvsv.Utility.dmap2pcl(str(tmp_path / "none.ply"), arg, Q_REF)
        assert e.value.code == -1 and "no positive disparity" in str(e.value)


# ---- the frame stream -------------------------------------------------------------------
from tests.test_gpu_samplepoint import SD, SH, SW, plain_stream_results, stream_frames  # noqa: E402


def off_stream(gpu, mvsv, work, cap=None):
    """point_cloud of a popped map's roi: (records as a structured array, count, (mn, mx))."""
    out, count, mm = mvsv.point_cloud(upload(gpu, np.ascontiguousarray(work)), Q_REF, max_points=cap,
                                      return_minmax=True)
    k = min(int(count), out.shape[0])
    return (out[:k].cpu().numpy().view(ref.CLOUD_DTYPE).reshape(-1), int(count), tuple(int(v) for v in mm.cpu()))


@pytest.mark.parametrize("batch", [1, 2])
def test_stream_brings_the_cloud_with_every_frame(gpu, mvsv, batch):
    from mvstereovision3_amd import _lib
    m = mvsv.StereoSGBM.create(0, SD, 9, 648, 2592)
    roi_u, _ = mvsv.create_dmap_rois((SH, SW), SD)
    x0, y0, x1, y1 = roi_u
    st = mvsv.DisparityStream(m, SW, SH, depth=3, grid_roi=roi_u, batch=batch)
    frames = stream_frames()
    plain = plain_stream_results(batch)
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError) as e:  # the cloud is off: nothing to bring
        st.front_cloud()
    assert e.value.code == _lib.MVSV_E_INVALID_ARG and st.pending() == 1
    with pytest.raises(mvsv.MvsvError) as e:  # a frame is pending
        st.enable_cloud(Q_REF, roi=roi_u)
    assert e.value.code == _lib.MVSV_E_INVALID_ARG
    d0, means0 = st.pop()
    assert np.array_equal(d0, plain[0][0]) and np.array_equal(means0, plain[0][1])

    def run_frames(roi, cap, others, cloud_first):
        rx0, ry0, rx1, ry1 = roi if roi is not None else (0, 0, SW, SH)
        pushed = 0
        for i in range(5):
            while pushed < 5 and st.pending() < 3:
                st.push(*frames[pushed])
                pushed += 1
            if others and not cloud_first:
                disp, dmm = st.front_display()
                vals, nhits, hits = st.front_samples()
            rec, count, mm = st.front_cloud(return_minmax=True)
            rec2, count2 = st.front_cloud()  # the frame stays pending
            assert ref.same_bytes(rec, rec2) and count == count2
            dev, count3 = st.front_cloud(copy=False)
            assert dev.is_cuda and dev.dtype == gpu.float32 and count3 == count
            assert ref.same_bytes(dev.cpu().numpy().view(ref.CLOUD_DTYPE).reshape(-1), rec)
            del dev
            if others and cloud_first:
                disp, dmm = st.front_display()
                vals, nhits, hits = st.front_samples()
            d, means = st.pop()
            assert np.array_equal(d, plain[i][0]), f"frame {i}: map differs from the plain stream's"
            assert np.array_equal(means, plain[i][1]), f"frame {i}: means differ from the plain stream's"
            work = np.ascontiguousarray(d[ry0:ry1, rx0:rx1])
            orec, ocount, omm = off_stream(gpu, mvsv, work, cap)
            want, wmm = ref.cloud(work, Q_REF, pyoracle.reproject)
            k = len(want) if cap is None else min(cap, len(want))
            assert count == ocount == len(want) > 1000 and mm == omm == wmm
            assert len(rec) == k and ref.same_bytes(rec, orec), f"frame {i} vs the off-stream call"
            assert ref.same_bytes(rec, want[:k]), f"frame {i} vs the restatement"
            if others:
                wd, wdmm = mvsv.normalize_minmax(upload(gpu, work), return_minmax=True)
                assert np.array_equal(disp, wd.cpu().numpy()) and nhits == len(hits)

    st.enable_cloud(Q_REF, roi=roi_u)
    run_frames(roi_u, None, False, True)
    st.enable_display(roi=roi_u)  # all three at the same time, asked for in either order
    st.enable_samplepoints((Q_REF, 1e4, 16.0), roi=roi_u)
    run_frames(roi_u, None, True, True)
    run_frames(roi_u, None, True, False)
    st.disable_samplepoints()
    st.disable_display()
    st.enable_cloud(Q_REF)  # a second call replaces the first: the whole map
    run_frames(None, None, False, True)
    st.enable_cloud(Q_REF, roi=roi_u, max_points=777)  # fewer than the frames hold
    run_frames(roi_u, 777, False, True)
    st.disable_cloud()
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError):
        st.front_cloud()
    d, means = st.pop()
    assert np.array_equal(d, plain[0][0]) and np.array_equal(means, plain[0][1])
    st.close()


def test_raw_stream_brings_the_cloud(gpu, mvsv):
    from tests.test_gpu_raw_stream import GRID, MAPS as RAW_MAPS, ROI, matcher, raw_pair
    st = mvsv.DisparityStream.raw(matcher(mvsv), RAW_MAPS, roi=ROI, depth=4, batch=3, grid_roi=GRID)
    st.enable_cloud(Q_REF, roi=GRID)
    plain = mvsv.DisparityStream.raw(matcher(mvsv), RAW_MAPS, roi=ROI, depth=4, batch=3, grid_roi=GRID)
    for seed in range(4):
        st.push_raw(*raw_pair(seed))
        plain.push_raw(*raw_pair(seed))
    x0, y0, x1, y1 = GRID
    for seed in range(4):
        rec, count, mm = st.front_cloud(return_minmax=True)
        d, means = st.pop()
        pd, pm = plain.pop()
        assert np.array_equal(d, pd) and np.array_equal(means, pm)
        want, wmm = ref.cloud(np.ascontiguousarray(d[y0:y1, x0:x1]), Q_REF, pyoracle.reproject)
        assert count == len(want) > 0 and mm == wmm
        assert ref.same_bytes(rec, want), f"frame {seed}"
    st.close()
    plain.close()
