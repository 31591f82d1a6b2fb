"""Every optional stage of the frame stream at once, byte for byte against the
library's own stand-alone entry points on each frame's popped map or pushed pair
(Disparity.sgbm, mean_disparity_grid, samplepoint_values / samplepoint_detect,
normalize_minmax, detection_view, point_cloud, sharpness).  The stand-alone entry
points are held against their numpy restatements by the tests of each stage; this
file holds the stream's plumbing -- which slot, which ROI, which ring offset --
against them, with no tolerance.

Shapes: 112 x 72, depth 3, batch 2.  Seven frames pushed two in, one out: runs of
two, a run of one that ends at the ring's end, and a last partial group that a
front_* call launches.  The display ROI is 31 x 21 at an odd origin (651 bytes: the
pinned slot's padding); the grid, the sample points and the view share a 96 x 64 ROI.
"""
import functools

import numpy as np
import pytest

from tests.test_gpu_samplepoint import Q_REF

pytestmark = pytest.mark.gpu

W, H, D = 112, 72, 16
DEPTH, BATCH, FRAMES = 3, 2, 7
GRID = (9, 3, 105, 67)    # grid_roi, sample points and view
DISP = (7, 5, 38, 26)     # 31 x 21
CLOUD = (5, 4, 66, 41)    # 61 x 37
CLOUD_CAP = 700           # fewer than the ROI's 2257 pixels
SHARP = ((3, 2, 100, 61), (1, 1, 111, 70))
RADIUS, MAX_HITS = 2, 5
RANGE = (1e4, 16.0)       # (first, second): found where 16 < value < 1e4
VIEW_ALL = 15


def matcher(mvsv):
    return mvsv.StereoSGBM.create(0, D, 5, 200, 800)


@functools.lru_cache(maxsize=None)
def frames():
    import mvstereovision3_amd as mvsv
    out = tuple(mvsv.synth_pair(0x5EED0000 + 1700 + i, W, H, 0, D) for i in range(FRAMES))
    for L, R in out:
        L.setflags(write=False)
        R.setflags(write=False)
    return out


def crop(t, roi):
    x0, y0, x1, y1 = roi
    return t[y0:y1, x0:x1]


@functools.lru_cache(maxsize=None)
def expected(i):
    """What the stand-alone entry points make of frame i, computed once."""
    import torch

    import mvstereovision3_amd as mvsv
    L, R = frames()[i]
    d = np.asarray(mvsv.Disparity.sgbm(mvsv.Stereopair(L.copy(), R.copy()), None, matcher(mvsv)))
    t = torch.from_numpy(d.copy()).cuda()
    e = {"map": d}
    work = crop(t, GRID)
    e["means"] = mvsv.mean_disparity_grid(work).cpu().numpy().reshape(81)
    vals = mvsv.samplepoint_values(work, RADIUS)
    e["values"] = vals.cpu().numpy()
    count, rec = mvsv.samplepoint_detect(vals, tuple(work.shape), Q_REF, RANGE, MAX_HITS)
    e["count"] = int(count)
    e["hits"] = rec.cpu().numpy().view(mvsv.SAMPLE_HIT_DTYPE).reshape(-1)[:min(int(count), MAX_HITS)]
    for name, roi in (("display", DISP), ("display_whole", (0, 0, W, H))):
        img, mm = mvsv.normalize_minmax(crop(t, roi), return_minmax=True)
        e[name] = (img.cpu().numpy(), tuple(int(v) for v in mm.cpu()))
    img, mm = mvsv.detection_view(work, VIEW_ALL, means=e["means"], mean_range=RANGE, values=e["values"],
                                  sample_range=RANGE, return_minmax=True)
    e["view"] = (img.cpu().numpy(), tuple(int(v) for v in mm.cpu()))
    rec, count, mm = mvsv.point_cloud(crop(t, CLOUD), Q_REF, max_points=CLOUD_CAP, return_minmax=True)
    k = min(int(count), CLOUD_CAP)
    e["cloud"] = (rec[:k].cpu().numpy().view(mvsv.CLOUD_DTYPE).reshape(-1), int(count), tuple(int(v) for v in mm.cpu()))
    sides = [mvsv.sharpness(torch.from_numpy(img.copy()).cuda(), roi, return_sums=True) for img, roi in zip((L, R), SHARP)]
    e["sharp"] = ((sides[0][0], sides[1][0]), (sides[0][1], sides[1][1]))
    return e


def open_stream(mvsv):
    st = mvsv.DisparityStream(matcher(mvsv), W, H, depth=DEPTH, grid_roi=GRID, batch=BATCH)
    st.enable_samplepoints((Q_REF, RANGE[0], RANGE[1], RADIUS), roi=GRID, max_hits=MAX_HITS)
    st.enable_display(roi=DISP)
    st.enable_view(VIEW_ALL, roi=GRID, mean_detector_or_range=RANGE)
    st.enable_cloud(Q_REF, roi=CLOUD, max_points=CLOUD_CAP)
    st.enable_sharpness(*SHARP)
    return st


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes(), what


def check_front_and_pop(st, i, display="display", view=True):
    """The oldest pending frame is frame i: every stage's output, then the map."""
    e = expected(i)
    if view:  # first: for the last frame this call launches the partial group
        img, mm = st.front_view()
        same(img, e["view"][0], f"frame {i}: view")
        assert mm == e["view"][1], f"frame {i}: view min / max"
        pinned, mm = st.front_view(copy="view")
        same(pinned, e["view"][0], f"frame {i}: pinned view")
        del pinned
        dev, mm = st.front_view(copy="device")
        same(dev.cpu().numpy(), e["view"][0], f"frame {i}: device view")
        assert mm == e["view"][1]
        del dev
    img, mm = st.front_display()
    same(img, e[display][0], f"frame {i}: display")
    assert mm == e[display][1], f"frame {i}: display min / max"
    pinned, _ = st.front_display(copy="view")
    same(pinned, e[display][0], f"frame {i}: pinned display")
    del pinned
    dev, mm = st.front_display(copy="device")
    same(dev.cpu().numpy(), e[display][0], f"frame {i}: device display")
    assert mm == e[display][1]
    del dev
    values, count, hits = st.front_samples()
    same(values, e["values"], f"frame {i}: lattice values")
    assert count == e["count"], f"frame {i}: hit count"
    same(hits, e["hits"], f"frame {i}: hits")
    rec, count, mm = st.front_cloud(return_minmax=True)
    assert (count, mm) == e["cloud"][1:], f"frame {i}: cloud header"
    same(rec, e["cloud"][0], f"frame {i}: cloud records")
    assert st.front_sharpness(return_sums=True) == e["sharp"], f"frame {i}: sharpness"
    dmap, _ = st.front_map()
    same(dmap.cpu().numpy(), e["map"], f"frame {i}: device map")
    del dmap
    d, means = st.pop()
    same(d, e["map"], f"frame {i}: map")
    same(means, e["means"], f"frame {i}: mean grid")


def two_in_one_out(st, push, n, **kw):
    """Push up to two frames, pop one, until n frames went through."""
    pushed = 0
    for i in range(n):
        for _ in range(2):
            if pushed < n and st.pending() < DEPTH:
                push(pushed)
                pushed += 1
        check_front_and_pop(st, i, **kw)
    assert pushed == n and st.pending() == 0


def test_the_frames_are_worth_comparing(gpu, mvsv):
    sx, sy, nx, ny = mvsv.samplepoint_layout(GRID[2] - GRID[0], GRID[3] - GRID[1])
    assert nx >= 2 and ny >= 2 and RADIUS < min(sx, sy)
    assert ((DISP[2] - DISP[0]) * (DISP[3] - DISP[1])) % 2 == 1 and DISP[0] % 2 == 1
    maps = [expected(i)["map"] for i in range(FRAMES)]
    assert all(not np.array_equal(maps[0], m) for m in maps[1:])
    for i in range(FRAMES):
        e = expected(i)
        assert (e["map"] > 0).mean() > 0.25, f"frame {i}: hardly any valid disparity"
        assert e["count"] > MAX_HITS and e["cloud"][1] > CLOUD_CAP  # both caps cut
        assert e["display"][1][0] < e["display"][1][1] and len(np.unique(e["display"][0])) > 4
        assert e["sharp"][1][0] > 0 and e["sharp"][1][0] != e["sharp"][1][1]


def test_all_stages_with_every_frame_then_display_alone_over_the_whole_map(gpu, mvsv):
    from mvstereovision3_amd import _lib
    st = open_stream(mvsv)
    two_in_one_out(st, lambda i: st.push(*frames()[i]), FRAMES)
    # the ring is empty: display and view off, the display back on over the whole map
    st.disable_display()
    st.disable_view()
    for front, text in ((st.front_display, "the display is not enabled on this stream"),
                        (st.front_view, "the view is not enabled on this stream")):
        for copy in (True, "view", "device"):
            with pytest.raises(mvsv.MvsvError) as e:
                front(copy=copy)
            assert e.value.code == _lib.MVSV_E_INVALID_ARG and text in str(e.value), (text, copy)
    st.enable_display()
    two_in_one_out(st, lambda i: st.push(*frames()[i]), 2, display="display_whole", view=False)
    st.disable_samplepoints()
    with pytest.raises(mvsv.MvsvError) as e:
        st.front_samples()
    assert e.value.code == _lib.MVSV_E_INVALID_ARG and "sample points are not enabled on this stream" in str(e.value)
    st.close()


def test_the_same_frames_as_colour_pairs(gpu, mvsv):
    """Grey replicated to three channels, not halved: the conversion gives the grey
    back, so every stage brings what it brought for the grey push."""
    assert mvsv.prepare_size(W, H, halve=False) == (W, H)
    st = open_stream(mvsv)
    st.enable_bgr((H, W), halve=False)

    def push(i):
        st.push_bgr(*(np.repeat(g[:, :, None], 3, axis=2) for g in frames()[i]))

    two_in_one_out(st, push, FRAMES)
    st.close()


def test_the_same_frames_from_device_tensors(gpu, mvsv):
    st = open_stream(mvsv)
    two_in_one_out(st, lambda i: st.push(*(gpu.from_numpy(g.copy()).cuda() for g in frames()[i])), FRAMES)
    st.close()
