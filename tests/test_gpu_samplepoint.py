"""SamplepointDetection on the device: the lattice values (sample_grid_kernel), the
ordered hit compaction (sample_detect_kernel) and both in the frame stream, bit for
bit against the plain-loop restatement in tests/samplepoint_restate.py and against
mvsv_calc_coordinates.

Shapes: every step from 8 to 10, remainder rows and columns, a 2-byte-aligned view
with stride > width, a lattice row longer than a wave and a 256-thread block
(nx = 258) whose 1290 points need two 1024-thread chunks of the detection kernel.
"""
import functools
import json
import os

import numpy as np
import pytest

from tests import samplepoint_restate as ref
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

Q_REF = np.array(json.load(open(os.path.join(GOLDEN, "q_matrix.json")))["Q"], np.float32)
WIDE = (2072, 48)  # nx = 258, ny = 5: 1290 points


@functools.lru_cache(maxsize=None)
def host_map(W, H, seed=0):
    d = ref.make_map(np.random.default_rng(1000 + seed + W * 7 + H), H, W)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def want_values(W, H, radius, seed=0):
    v = ref.values(host_map(W, H, seed), radius)
    v.setflags(write=False)
    return v


def assert_values(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} differ, first {[(int(i), float(got[i]), float(want[i])) for i in bad[:5]]}"


@pytest.mark.parametrize("W,H", [(63, 47), (100, 70), (127, 31), WIDE], ids=lambda v: str(v))
@pytest.mark.parametrize("radius", [2, 0, 3])
def test_values_match_restatement(gpu, mvsv, W, H, radius):
    d = host_map(W, H)
    got = mvsv.samplepoint_values(gpu.from_numpy(d.copy()).cuda(), radius).cpu().numpy()
    want = want_values(W, H, radius)
    assert_values(got, want, f"{W}x{H} r{radius}")
    if radius == 0:
        assert (want < 0).any()      # negatives pass through
    else:
        assert (want == 0).any() and (want > 0).any()
        # total / count truncates somewhere
        assert any(v != np.float32(t) for v, t in zip(want, _exact_means(d, radius)) if t)


def _exact_means(d, radius):
    H, W = d.shape
    out = []
    for cx, cy in ref.centres(W, H):
        p = d[cy - radius:cy + radius + 1, cx - radius:cx + radius + 1].astype(np.int64)
        out.append(float(p[p > 1].mean()) if (p > 1).any() else 0.0)
    return out


def test_values_of_an_unaligned_view(gpu, mvsv):
    """A 688 x 480 view at x0 = 63 of a 752-wide map: stride > width, 2-byte-aligned base."""
    full = host_map(752, 480)
    t = gpu.from_numpy(full.copy()).cuda()
    view = t[:, 63:63 + 688]
    assert view.data_ptr() % 4 == 2 and view.stride(0) == 752
    got = mvsv.samplepoint_values(view, 2).cpu().numpy()
    want = ref.values(np.ascontiguousarray(full[:, 63:63 + 688]), 2)
    assert_values(got, want, "view")
    assert got.size == 85 * 59


def test_values_of_a_batch_with_padded_frames(gpu, mvsv):
    W, H = 100, 70
    maps = [host_map(W, H, s) for s in range(3)]
    buf = gpu.full((3, H + 5, W + 9), 777, dtype=gpu.int16, device="cuda")
    view = buf[:, :H, :W]
    for f, m in enumerate(maps):
        view[f] = gpu.from_numpy(m.copy()).cuda()
    assert view.stride(0) > H * view.stride(1)
    got = mvsv.samplepoint_values(view, 2).cpu().numpy()
    assert got.shape == (3, 77)
    for f in range(3):
        assert_values(got[f], want_values(W, H, 2, f), f"frame {f}")
    assert not np.array_equal(got[0], got[1])


def test_values_edge_sizes(gpu, mvsv):
    from mvstereovision3_amd import _lib
    none = mvsv.samplepoint_values(gpu.zeros((100, 15), dtype=gpu.int16, device="cuda"), 2)
    assert none.numel() == 0
    d = gpu.from_numpy(host_map(100, 70).copy()).cuda()
    with pytest.raises(mvsv.MvsvError) as e:
        mvsv.samplepoint_values(d, 8)  # steps are 8
    assert e.value.code == _lib.MVSV_E_INVALID_ARG
    assert_values(mvsv.samplepoint_values(d, 7).cpu().numpy(), want_values(100, 70, 7), "r7")
    # the host-map sibling, through the detector's build()
    det = mvsv.SamplepointDetection()
    det.init((70, 100), Q_REF, 0.1, 1.5)
    det.build(host_map(100, 70))
    assert_values(np.array(det.mDistanceVec, np.float32), want_values(100, 70, 2), "host map")
    det.build(d)
    assert_values(np.array(det.mDistanceVec, np.float32), want_values(100, 70, 2), "device map")


# ---- detection -------------------------------------------------------------------
def check_detect(gpu, mvsv, vals, shape, first, second, max_hits=None):
    """Device detection of `vals` against the restatement + mvsv_calc_coordinates."""
    from mvstereovision3_amd import _lib
    H, W = shape
    count, rec = mvsv.samplepoint_detect(gpu.from_numpy(vals.copy()).cuda(), shape, Q_REF, (first, second), max_hits)
    count = int(count.cpu())
    rec = rec.cpu().numpy().view(mvsv.SAMPLE_HIT_DTYPE).reshape(-1)
    want = ref.hits(vals, first, second)
    assert count == len(want)
    cap = vals.size if max_hits is None else max_hits
    kept = want[:cap]
    assert rec["index"][:len(kept)].tolist() == kept
    cs = ref.centres(W, H)
    xyd = np.array([(cs[i][0], cs[i][1], vals[i]) for i in kept], np.float32).reshape(len(kept), 3)
    pts = np.empty((len(kept), 4), np.float32)
    _lib.lib().mvsv_calc_coordinates(len(kept), xyd.ctypes.data, Q_REF.ctypes.data, pts.ctypes.data)
    for k, name in enumerate("xyz"):
        assert np.array_equal(rec[name][:len(kept)].view(np.uint32), pts[:, k].copy().view(np.uint32)), name
    assert not rec[len(kept):].view(np.uint8).any()  # nothing written past the hits
    return count


def test_detect_on_kernel_values(gpu, mvsv):
    W, H = WIDE
    vals = want_values(W, H, 2)
    assert vals.size == 1290
    n = check_detect(gpu, mvsv, vals, (H, W), 400.0, 2.5)
    assert 100 < n < 1290
    assert check_detect(gpu, mvsv, vals, (H, W), 400.0, 2.5, max_hits=37) == n  # count stays total
    assert check_detect(gpu, mvsv, vals, (H, W), 400.0, 2.5, max_hits=0) == n
    assert check_detect(gpu, mvsv, vals, (H, W), -1e30, -2e30) == 0
    assert check_detect(gpu, mvsv, vals, (H, W), 3e38, -3e38) == 1290
    assert check_detect(gpu, mvsv, vals, (H, W), 3e38, -3e38, max_hits=1025) == 1290


def test_detect_hand_made_values(gpu, mvsv):
    W, H = WIDE
    shape = (H, W)
    first, second = np.float32(300.0), np.float32(100.0)
    inside = np.float32(200.0)
    big, small = np.float32(1e9), np.float32(-1e9)
    # hits only in the last chunk
    v = np.zeros(1290, np.float32)
    v[[1024, 1025, 1087, 1088, 1289]] = inside
    assert check_detect(gpu, mvsv, v, shape, first, second) == 5
    # alternating hits across every wave and chunk boundary
    v = np.where(np.arange(1290) % 2 == 0, inside, np.float32(0)).astype(np.float32)
    assert check_detect(gpu, mvsv, v, shape, first, second) == 645
    v = np.where(np.arange(1290) % 2 == 1, inside, np.float32(500)).astype(np.float32)
    assert check_detect(gpu, mvsv, v, shape, first, second) == 645
    assert check_detect(gpu, mvsv, v, shape, first, second, max_hits=513) == 645
    # hits on both sides of each wave / chunk boundary only
    v = np.zeros(1290, np.float32)
    edges = [i for b in range(64, 1290, 64) for i in (b - 1, b)]
    v[edges] = inside + np.arange(len(edges), dtype=np.float32)
    assert check_detect(gpu, mvsv, v, shape, first, second) == len(edges)
    # the bounds themselves are no hits; their neighbours decide by float compare
    v = np.full(1290, first, np.float32)
    v[1::2] = second
    assert check_detect(gpu, mvsv, v, shape, first, second) == 0
    v[[0, 63, 64, 1023, 1024, 1289]] = [np.nextafter(first, small), np.nextafter(first, big),
                                        np.nextafter(second, big), np.nextafter(second, small),
                                        np.nextafter(first, small), np.nextafter(second, big)]
    assert check_detect(gpu, mvsv, v, shape, first, second) == 4
    # a batch: per-frame counts and records
    batch = np.stack([np.where(np.arange(1290) % 3 == k, inside, np.float32(0)) for k in range(3)]).astype(np.float32)
    counts, rec = mvsv.samplepoint_detect(gpu.from_numpy(batch).cuda(), shape, Q_REF, (first, second), 500)
    assert counts.cpu().tolist() == [430, 430, 430]
    rec = rec.cpu().numpy().view(mvsv.SAMPLE_HIT_DTYPE).reshape(3, 500)
    for k in range(3):
        assert rec[k]["index"][:430].tolist() == list(range(k, 1290, 3))


# ---- the frame stream -----------------------------------------------------------------
SW, SH, SD = 376, 240, 64


@functools.lru_cache(maxsize=None)
def stream_frames():
    import mvstereovision3_amd as mvsv
    return tuple(mvsv.synth_pair(0x5EED0000 + 700 + i, SW, SH, 0, SD) for i in range(5))


@functools.lru_cache(maxsize=None)
def plain_stream_results(batch):
    """(map, means) of every frame from a stream without the lattice."""
    import mvstereovision3_amd as mvsv
    m = mvsv.StereoSGBM.create(0, SD, 9, 648, 2592)
    roi_u, _ = mvsv.create_dmap_rois((SH, SW), SD)
    st = mvsv.DisparityStream(m, SW, SH, depth=5, grid_roi=roi_u, batch=batch)
    for L, R in stream_frames():
        st.push(L, R)
    out = [st.pop() for _ in range(5)]
    st.close()
    return out


def detector(mvsv, pcl_dir, shape):
    d = mvsv.SamplepointDetection(pcl_dir=str(pcl_dir))
    d.init(shape, Q_REF, 1.45, 2.9)  # disparity * 16 in about (199, 397)
    return d


def off_stream(gpu, mvsv, work, det, max_hits=None):
    """values, count and records of the off-stream device functions on a host map."""
    vals = mvsv.samplepoint_values(gpu.from_numpy(np.ascontiguousarray(work)).cuda(), det.RADIUS)
    count, rec = mvsv.samplepoint_detect(vals, work.shape, Q_REF, det.mRangeDisparity, max_hits)
    rec = rec.cpu().numpy().view(mvsv.SAMPLE_HIT_DTYPE).reshape(-1)
    return vals.cpu().numpy(), int(count.cpu()), rec[:min(int(count.cpu()), rec.size)]


@pytest.mark.parametrize("batch", [1, 2])
def test_stream_brings_the_lattice_with_every_frame(gpu, mvsv, tmp_path, batch):
    from mvstereovision3_amd import _lib
    m = mvsv.StereoSGBM.create(0, SD, 9, 648, 2592)
    roi_u, _ = mvsv.create_dmap_rois((SH, SW), SD)
    x0, y0, x1, y1 = roi_u
    for k in "ab":
        (tmp_path / k).mkdir()
    a = detector(mvsv, tmp_path / "a", (y1 - y0, x1 - x0))
    b = detector(mvsv, tmp_path / "b", (y1 - y0, x1 - x0))
    st = mvsv.DisparityStream(m, SW, SH, depth=3, grid_roi=roi_u, batch=batch)
    frames = stream_frames()
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError) as e:  # the lattice is off: nothing to bring
        st.front_samples()
    assert e.value.code == _lib.MVSV_E_INVALID_ARG and st.pending() == 1
    with pytest.raises(mvsv.MvsvError) as e:  # a frame is pending
        st.enable_samplepoints(a, roi=roi_u)
    assert e.value.code == _lib.MVSV_E_INVALID_ARG
    d0, means0 = st.pop()
    plain = plain_stream_results(batch)
    assert np.array_equal(d0, plain[0][0]) and np.array_equal(means0, plain[0][1])
    st.enable_samplepoints(a, roi=roi_u)
    pushed = 0
    any_hits = False
    for i in range(5):
        while pushed < 5 and st.pending() < 3:
            st.push(*frames[pushed])
            pushed += 1
        vals, count, hits = st.front_samples()
        vals2, count2, hits2 = st.front_samples()  # the frame stays pending
        assert np.array_equal(vals, vals2) and count == count2 and np.array_equal(hits, hits2)
        d, means = st.pop()
        assert np.array_equal(d, plain[i][0]), f"frame {i}: map differs from the plain stream's"
        assert np.array_equal(means, plain[i][1]), f"frame {i}: means differ from the plain stream's"
        work = d[y0:y1, x0:x1]
        wv, wc, wh = off_stream(gpu, mvsv, work, a)
        assert_values(vals, wv, f"frame {i} values")
        assert count == wc and np.array_equal(hits, wh), f"frame {i} hits"
        if i == 0:
            assert_values(vals, ref.values(np.ascontiguousarray(work), 2), "frame 0 vs restatement")
            assert hits["index"].tolist() == ref.hits(vals, *a.mRangeDisparity)
            assert 0 < count < vals.size
        # both layers: the stream's records and the host decision on the popped map
        a.build(work, values=vals)
        a.detectObstacles(hits=(count, hits))
        b.build(np.ascontiguousarray(work))
        b.detectObstacles()
        assert [s.center for s in a.getFoundObstacles()] == [s.center for s in b.getFoundObstacles()]
        assert len(a.getFoundPoints()) == count
        if count:
            any_hits = True
            assert np.array_equal(np.stack(a.getFoundPoints()).view(np.uint32),
                                  np.stack(b.getFoundPoints()).view(np.uint32))
        assert a.getObstacleCounter() == b.getObstacleCounter()
    assert any_hits and a.getObstacleCounter() > 0
    for k in range(a.getObstacleCounter()):
        name = f"pcl_000{k}.ply"
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    # max_hits caps the records, not the count; disable takes the lattice off again
    st.enable_samplepoints(a, roi=roi_u, max_hits=7)
    st.push(*frames[0])
    vals, count, hits = st.front_samples()
    wv, wc, wh = off_stream(gpu, mvsv, plain[0][0][y0:y1, x0:x1], a)
    assert count == wc > 7 and np.array_equal(hits, wh[:7])
    st.pop()
    st.disable_samplepoints()
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError):
        st.front_samples()
    d, means = st.pop()
    assert np.array_equal(d, plain[0][0]) and np.array_equal(means, plain[0][1])
    st.close()


def test_raw_stream_brings_the_lattice(gpu, mvsv):
    from tests.test_gpu_raw_stream import GRID, MAPS, ROI, matcher, raw_pair
    st = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI, depth=4, batch=3, grid_roi=GRID)
    args = (Q_REF, 1e4, 16.0)  # every valid disparity
    st.enable_samplepoints(args, roi=GRID, max_hits=100)
    plain = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI, depth=4, batch=3, grid_roi=GRID)
    for seed in range(4):
        st.push_raw(*raw_pair(seed))
        plain.push_raw(*raw_pair(seed))
    x0, y0, x1, y1 = GRID
    for seed in range(4):
        vals, count, hits = st.front_samples()
        d, means = st.pop()
        pd, pm = plain.pop()
        assert np.array_equal(d, pd) and np.array_equal(means, pm)
        work = np.ascontiguousarray(d[y0:y1, x0:x1])
        assert_values(vals, ref.values(work, 2), f"frame {seed} values")
        want = ref.hits(vals, args[1], args[2])
        assert count == len(want) > 100 and hits["index"].tolist() == want[:100]
        wv = mvsv.samplepoint_values(gpu.from_numpy(work).cuda(), 2)
        _, rec = mvsv.samplepoint_detect(wv, work.shape, Q_REF, args[1:], 100)
        assert np.array_equal(hits, rec.cpu().numpy().view(mvsv.SAMPLE_HIT_DTYPE).reshape(-1))
    st.close()
    plain.close()
