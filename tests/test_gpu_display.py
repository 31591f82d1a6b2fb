"""Display maps on the device: minmax_kernel / minmax_final_kernel /
normalize_u8_kernel and the display map in the frame stream, bit for bit against
the numpy restatement of OpenCV 3.4's cv::normalize(NORM_MINMAX, CV_8U) in
tests/display_restate.py.

Shapes: odd widths whose head / tail elements go through the narrow accesses, a
row longer than one pass of a wave's packed loads (2072), more rows than
blocks x waves (1500), 2-byte-aligned views, strides that take the packed path
(multiples of 8 elements) and strides that take the narrow one, and every store
width of the 8-bit output (8, 4, 2, 1 bytes by the alignment of the view).
"""
import functools

import numpy as np
import pytest

from tests import display_restate as ref

pytestmark = pytest.mark.gpu

SHAPES = [(63, 47), (100, 70), (127, 31), (2072, 48), (24, 1500)]
LADDERS = [(-16, 74), (-16, 164), (-16, 222)]


@functools.lru_cache(maxsize=None)
def host_map(W, H, seed=0):
    """Values 100..1999 with zeros and SGBM's invalid marker -16 sprinkled in."""
    rng = np.random.default_rng(4000 + seed + W * 7 + H)
    d = rng.integers(100, 2000, (H, W)).astype(np.int16)
    d[rng.random((H, W)) < 0.1] = -16
    d[rng.random((H, W)) < 0.05] = 0
    d.setflags(write=False)
    return d


def assert_bytes(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first {[(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:5]]}"


def dev_minmax(gpu, mvsv, view, positive_only=False):
    r = mvsv.minmax(view, positive_only).cpu().numpy()
    return [tuple(int(v) for v in p) for p in r.reshape(-1, 2)]


def padded(gpu, d, stride, offset=0):
    """d on the device as a view with the given row stride, `offset` elements into
    its buffer; everything around it is 777."""
    H, W = d.shape
    buf = gpu.full((H * stride + offset + 16,), 777, dtype=gpu.int16, device="cuda")
    view = buf[offset:offset + H * stride].view(H, stride)[:, :W]
    view.copy_(gpu.from_numpy(d.copy()).cuda())
    return view


# ---- min / max ------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_minmax_finds_extremes_wherever_they_are(gpu, mvsv, W, H):
    base = host_map(W, H)
    spots = {"first pixel": (0, 0), "last pixel": (H - 1, W - 1), "last column of a middle row": (H // 2, W - 1),
             "tail column of the last row": (H - 1, W - 1 - (W % 8) // 2),
             "head column of a middle row": (H // 3, 0)}
    for stride, offset in ((W, 0), ((W + 15) & ~7, 3), (W + 9 | 1, 1)):
        for what, (y, x) in spots.items():
            for lo_first in (True, False):
                d = base.copy()
                y2, x2 = (H - 1 - y, W - 1 - x)
                (ya, xa), (yb, xb) = ((y, x), (y2, x2)) if lo_first else ((y2, x2), (y, x))
                d[ya, xa] = -300
                d[yb, xb] = 30000
                got = dev_minmax(gpu, mvsv, padded(gpu, d, stride, offset))
                assert got == [(-300, 30000)], f"{W}x{H} stride {stride} offset {offset}: {what}"
    # a single extreme pixel in the unvectorisable tail / head of a view
    d = base.copy()
    d[H - 1, W - 1] = 2500
    d[0, 0] = -17
    assert dev_minmax(gpu, mvsv, padded(gpu, d, (W + 15) & ~7, 5)) == [(-17, 2500)]
    assert dev_minmax(gpu, mvsv, gpu.from_numpy(base.copy()).cuda()) == [ref.minmax(base)]


def test_minmax_positive_only_and_full_range(gpu, mvsv):
    W, H = 100, 70
    d = host_map(W, H).copy()
    assert (d == 0).any() and (d < 0).any()
    d[H - 1, W - 1] = 1  # the smallest positive value, in the tail
    t = gpu.from_numpy(d).cuda()
    assert dev_minmax(gpu, mvsv, t, True) == [ref.minmax(d, True)] == [(1, int(d.max()))]
    assert dev_minmax(gpu, mvsv, t, False) == [(-16, int(d.max()))]
    assert mvsv.Utility.calcMinMaxDisparity(t) == mvsv.Utility.calcMinMaxDisparity(d) == (1, int(d.max()))
    # a batch whose middle frame has no positive value
    none = np.where(d > 0, 0, d)
    batch = np.stack([d, none, host_map(W, H, 1)])
    got = dev_minmax(gpu, mvsv, gpu.from_numpy(batch).cuda(), True)
    assert got == [ref.minmax(f, True) for f in batch] and got[1] == (32767, -32768)
    with pytest.raises(mvsv.MvsvError):
        mvsv.Utility.calcMinMaxDisparity(gpu.from_numpy(none).cuda())
    # the whole int16 range
    full = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16).reshape(256, 256)
    assert dev_minmax(gpu, mvsv, gpu.from_numpy(full).cuda()) == [(-32768, 32767)]
    assert dev_minmax(gpu, mvsv, gpu.from_numpy(full).cuda(), True) == [(1, 32767)]
    for v in (-32768, 32767, 0):
        const = gpu.full((31, 127), v, dtype=gpu.int16, device="cuda")
        assert dev_minmax(gpu, mvsv, const) == [(v, v)]


# ---- normalize --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder_batch():
    """Six 100 x 70 frames, each with a range of its own."""
    shape = (70, 100)
    frames = [ref.ladder(lo, hi, shape) for lo, hi in LADDERS]
    frames.append(ref.ladder(0, 510, shape))
    frames.append(ref.ladder(0, 1, shape))
    full = np.resize(np.arange(-32768, 32768, 9, dtype=np.int64).astype(np.int16), shape).copy()
    full[-1, -1] = 32767
    frames.append(full)
    b = np.stack(frames)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def ladder_want(alpha=0.0, beta=255.0):
    return [ref.normalize(f, alpha, beta) for f in ladder_batch()]


def test_normalize_batch_of_ladders(gpu, mvsv):
    b = ladder_batch()
    out, mm = mvsv.normalize_minmax(gpu.from_numpy(b.copy()).cuda(), return_minmax=True)
    out, mm = out.cpu().numpy(), mm.cpu().numpy()
    want = ladder_want()
    assert [tuple(int(v) for v in p) for p in mm] == [w[1] for w in want]
    assert [w[1] for w in want] == LADDERS + [(0, 510), (0, 1), (-32768, 32767)]
    for f, (w, _) in enumerate(want):
        assert_bytes(out[f], w, f"frame {f}")
    # the ladders tell the pinned arithmetic from double evaluation and from an fma
    for f in range(3):
        assert (out[f] != ref.normalize_f64(b[f])).any() and (out[f] != ref.normalize_fused(b[f])).any()
    assert out[3].reshape(-1)[:8].tolist() == [0, 0, 1, 2, 2, 2, 3, 4]  # half to even
    assert set(np.unique(out[4]).tolist()) == {0, 255}
    # one frame alone == the same frame in the batch; numpy in, numpy out
    for f in (0, 5):
        assert_bytes(mvsv.normalize_minmax(gpu.from_numpy(b[f].copy()).cuda()).cpu().numpy(), want[f][0], f"single {f}")
    host, hmm = mvsv.normalize_minmax(b[2], return_minmax=True)
    assert_bytes(host, want[2][0], "host map")
    assert tuple(int(v) for v in hmm) == want[2][1]
    assert_bytes(mvsv.normalize_minmax(b), np.stack([w[0] for w in want]), "host batch")


def test_normalize_constant_frame_in_a_batch_and_alpha_beta(gpu, mvsv):
    b = ladder_batch()
    const = np.full((70, 100), -16, np.int16)
    batch = np.stack([b[0], const, b[2]])
    t = gpu.from_numpy(batch).cuda()
    out = mvsv.normalize_minmax(t).cpu().numpy()
    assert (out[1] == 0).all()
    assert_bytes(out[0], ladder_want()[0][0], "frame 0")
    assert_bytes(out[2], ladder_want()[2][0], "frame 2")
    out = mvsv.normalize_minmax(t, 32, 224).cpu().numpy()
    for f in range(3):
        assert_bytes(out[f], ref.normalize(batch[f], 32, 224)[0], f"(32, 224) frame {f}")
    assert (out[1] == 32).all() and out[0].min() == 32 and out[0].max() == 224
    assert_bytes(mvsv.normalize_minmax(t, 224, 32).cpu().numpy(), out, "(224, 32) == (32, 224)")
    assert_bytes(mvsv.normalize_minmax(t, 255, 0).cpu().numpy(), mvsv.normalize_minmax(t).cpu().numpy(), "(255, 0)")
    assert (mvsv.normalize_minmax(t[1], 300, 400).cpu().numpy() == 255).all()  # saturate(dmin)


@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_normalize_shapes(gpu, mvsv, W, H):
    d = host_map(W, H)
    want, mm = ref.normalize(d)
    got, gmm = mvsv.normalize_minmax(gpu.from_numpy(d.copy()).cuda(), return_minmax=True)
    assert_bytes(got.cpu().numpy(), want, f"{W}x{H}")
    assert tuple(int(v) for v in gmm.cpu()) == mm
    assert_bytes(mvsv.normalize_minmax(d), want, f"{W}x{H} host map")


# ---- views ------------------------------------------------------------------------------
def test_unaligned_view_of_a_wider_map(gpu, mvsv):
    """A 688 x 480 view at x0 = 63 of a 752-wide map: stride > width, 2-byte-aligned base."""
    full = host_map(752, 480).copy()
    full[:, :63] = -30000  # what lies outside the view must not count
    full[:, 63 + 688:] = 30000
    t = gpu.from_numpy(full).cuda()
    view = t[:, 63:63 + 688]
    assert view.data_ptr() % 4 == 2 and view.stride(0) == 752
    work = np.ascontiguousarray(full[:, 63:63 + 688])
    want, mm = ref.normalize(work)
    got, gmm = mvsv.normalize_minmax(view, return_minmax=True)
    assert_bytes(got.cpu().numpy(), want, "view")
    assert tuple(int(v) for v in gmm.cpu()) == mm == dev_minmax(gpu, mvsv, view)[0]
    assert mm[0] == -16 and mm[1] < 2000


@pytest.mark.parametrize("pad_w", [9, 12], ids=["narrow", "packed"])
def test_batch_with_padded_frames_and_rows(gpu, mvsv, pad_w):
    """Row stride W + 9 = 109 takes the narrow path, W + 12 = 112 the packed one; the
    padding (777 in, a sentinel out) is neither read into the result nor written."""
    W, H = 100, 70
    maps = [host_map(W, H, s) for s in range(3)]
    buf = gpu.full((3, H + 5, W + pad_w), 777, dtype=gpu.int16, device="cuda")
    view = buf[:, :H, 3:3 + W] if pad_w == 12 else buf[:, :H, :W]
    for f, m in enumerate(maps):
        view[f] = gpu.from_numpy(m.copy()).cuda()
    obuf = gpu.full((3, H + 3, W + 13), 0xA5, dtype=gpu.uint8, device="cuda")
    out = obuf[:, 1:1 + H, 5:5 + W]
    assert out.stride(1) % 2 == 1  # odd output stride: byte stores
    res, mm = mvsv.normalize_minmax(view, out=out, return_minmax=True)
    assert res is out
    o = obuf.cpu().numpy()
    for f in range(3):
        want, wmm = ref.normalize(maps[f])
        assert_bytes(o[f, 1:1 + H, 5:5 + W], want, f"frame {f}")
        assert tuple(int(v) for v in mm[f].cpu()) == wmm
    keep = np.ones(o.shape, bool)
    keep[:, 1:1 + H, 5:5 + W] = False
    assert (o[keep] == 0xA5).all(), "bytes outside the output view were written"


def test_packed_and_narrow_paths_give_the_same_bytes(gpu, mvsv):
    """One map through row strides that take the packed path (multiples of 8 elements,
    every head length 0..7) and through strides that do not, into outputs aligned for
    8-, 4-, 2- and 1-byte stores."""
    W, H = 127, 31
    d = host_map(W, H)
    want, mm = ref.normalize(d)
    results = []
    for stride, offset in [(128, 0), (128, 1), (136, 2), (136, 3), (128, 4), (144, 5), (128, 6), (128, 7),
                           (127, 0), (129, 1), (131, 4), (134, 0)]:
        view = padded(gpu, d, stride, offset)
        assert dev_minmax(gpu, mvsv, view) == [mm], f"stride {stride} offset {offset}"
        for ostride, ooff in [(128, 0), (136, 4), (130, 2), (129, 1), (128, 7)]:
            obuf = gpu.full((H * ostride + 32,), 0x5A, dtype=gpu.uint8, device="cuda")
            out = obuf[ooff:ooff + H * ostride].view(H, ostride)[:, :W]
            mvsv.normalize_minmax(view, out=out)
            o = obuf.cpu().numpy()
            got = o[ooff:ooff + H * ostride].reshape(H, ostride)[:, :W]
            assert_bytes(got, want, f"stride {stride} offset {offset} -> out stride {ostride} offset {ooff}")
            keep = np.ones(o.shape, bool)
            keep[ooff:ooff + H * ostride].reshape(H, ostride)[:, :W] = False
            assert (o[keep] == 0x5A).all(), f"out stride {ostride} offset {ooff}: bytes outside the view written"
            results.append(got.tobytes())
    assert len(set(results)) == 1


# ---- validation ---------------------------------------------------------------------------
def test_host_entry_point_and_validation(gpu, mvsv):
    import ctypes
    from mvstereovision3_amd import _lib
    lib, E = _lib.lib(), _lib.MVSV_E_INVALID_ARG
    ctx = _lib.context(0)
    d = host_map(100, 70)
    out = np.full((70, 120), 0xA5, np.uint8)
    mm = np.zeros(2, np.int16)
    # a strided host map into a strided host image
    wide = np.full((70, 111), 777, np.int16)
    wide[:, 4:104] = d
    src = wide[:, 4:104]
    assert lib.mvsv_normalize_minmax(ctx.handle, src.ctypes.data, 111, 100, 70, 0.0, 255.0, out.ctypes.data, 120,
                                     mm.ctypes.data) == 0
    want, wmm = ref.normalize(d)
    assert_bytes(out[:, :100], want, "host")
    assert (out[:, 100:] == 0xA5).all() and tuple(int(v) for v in mm) == wmm
    assert lib.mvsv_normalize_minmax(ctx.handle, src.ctypes.data, 111, 100, 70, 0.0, 255.0, out.ctypes.data, 120,
                                     None) == 0
    bad_host = [
        (None, 111, 100, 70, 0.0, 255.0, out.ctypes.data, 120),
        (src.ctypes.data, 111, 100, 70, 0.0, 255.0, None, 120),
        (src.ctypes.data, 111, 0, 70, 0.0, 255.0, out.ctypes.data, 120),
        (src.ctypes.data, 111, 100, 0, 0.0, 255.0, out.ctypes.data, 120),
        (src.ctypes.data, 99, 100, 70, 0.0, 255.0, out.ctypes.data, 120),
        (src.ctypes.data, 111, 100, 70, 0.0, 255.0, out.ctypes.data, 99),
        (src.ctypes.data, 111, 100, 70, float("nan"), 255.0, out.ctypes.data, 120),
        (src.ctypes.data, 111, 100, 70, 0.0, float("inf"), out.ctypes.data, 120),
    ]
    for a in bad_host:
        assert lib.mvsv_normalize_minmax(ctx.handle, *a, None) == E, a
    t = gpu.from_numpy(d.copy()).cuda()
    o = gpu.empty((70, 100), dtype=gpu.uint8, device="cuda")
    m = gpu.empty((2,), dtype=gpu.int16, device="cuda")
    p, q, r = t.data_ptr(), o.data_ptr(), m.data_ptr()
    bad_dev = [
        (0, p, 100, 7000, 100, 70, 0.0, 255.0, q, 100, 7000, r),
        (1, None, 100, 7000, 100, 70, 0.0, 255.0, q, 100, 7000, r),
        (1, p, 100, 7000, 100, 70, 0.0, 255.0, None, 100, 7000, r),
        (1, p, 99, 7000, 100, 70, 0.0, 255.0, q, 100, 7000, r),
        (1, p, 100, 7000, 100, 70, 0.0, 255.0, q, 99, 7000, r),
        (1, p, 100, 7000, 0, 70, 0.0, 255.0, q, 100, 7000, r),
        (1, p, 100, 7000, 100, -1, 0.0, 255.0, q, 100, 7000, r),
        (1, p, 100, 7000, 100, 70, float("-inf"), 255.0, q, 100, 7000, r),
        (1, p, 100, 7000, 100, 70, 0.0, float("nan"), q, 100, 7000, r),
    ]
    for a in bad_dev:
        assert lib.mvsv_normalize_minmax_device(ctx.handle, *a) == E, a
    assert lib.mvsv_normalize_minmax_device(ctx.handle, 1, p, 100, 7000, 100, 70, 0.0, 255.0, q, 100, 7000, None) == 0
    assert_bytes(o.cpu().numpy(), want, "device call without min / max")
    for a in [(0, p, 100, 7000, 100, 70, 0, r), (1, None, 100, 7000, 100, 70, 0, r), (1, p, 100, 7000, 100, 70, 0, None),
              (1, p, 99, 7000, 100, 70, 0, r), (1, p, 100, 7000, 0, 70, 0, r), (1, p, 100, 7000, 100, 0, 1, r)]:
        assert lib.mvsv_minmax_device(ctx.handle, *a) == E, a
    assert b"min / max" in ctypes.cast(lib.mvsv_last_error(ctx.handle), ctypes.c_char_p).value
    with pytest.raises(mvsv.MvsvError):
        mvsv.normalize_minmax(gpu.zeros((4, 4), dtype=gpu.float32, device="cuda"))
    with pytest.raises(mvsv.MvsvError):
        mvsv.normalize_minmax(np.zeros((4, 4), np.float32))


# ---- the frame stream -------------------------------------------------------------------
from tests.test_gpu_samplepoint import SD, SH, SW, Q_REF, plain_stream_results, stream_frames  # noqa: E402


def off_stream(gpu, mvsv, work):
    out, mm = mvsv.normalize_minmax(gpu.from_numpy(np.ascontiguousarray(work)).cuda(), return_minmax=True)
    return out.cpu().numpy(), tuple(int(v) for v in mm.cpu())


@pytest.mark.parametrize("batch", [1, 2])
def test_stream_brings_the_display_map_with_every_frame(gpu, mvsv, batch):
    from mvstereovision3_amd import _lib
    m = mvsv.StereoSGBM.create(0, SD, 9, 648, 2592)
    roi_u, _ = mvsv.create_dmap_rois((SH, SW), SD)
    x0, y0, x1, y1 = roi_u
    st = mvsv.DisparityStream(m, SW, SH, depth=3, grid_roi=roi_u, batch=batch)
    frames = stream_frames()
    plain = plain_stream_results(batch)
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError) as e:  # the display is off: nothing to bring
        st.front_display()
    assert e.value.code == _lib.MVSV_E_INVALID_ARG and st.pending() == 1
    with pytest.raises(mvsv.MvsvError) as e:  # a frame is pending
        st.enable_display(roi=roi_u)
    assert e.value.code == _lib.MVSV_E_INVALID_ARG
    d0, means0 = st.pop()
    assert np.array_equal(d0, plain[0][0]) and np.array_equal(means0, plain[0][1])

    def run(roi, lattice):
        rx0, ry0, rx1, ry1 = roi if roi is not None else (0, 0, SW, SH)
        pushed = 0
        for i in range(5):
            while pushed < 5 and st.pending() < 3:
                st.push(*frames[pushed])
                pushed += 1
            disp, mm = st.front_display()
            disp2, mm2 = st.front_display()  # the frame stays pending
            assert np.array_equal(disp, disp2) and mm == mm2
            view, mm3 = st.front_display(copy="view")
            assert not view.flags.writeable and np.array_equal(view, disp) and mm3 == mm
            del view
            if lattice:
                vals, count, hits = st.front_samples()
            d, means = st.pop()
            assert np.array_equal(d, plain[i][0]), f"frame {i}: map differs from the plain stream's"
            assert np.array_equal(means, plain[i][1]), f"frame {i}: means differ from the plain stream's"
            work = d[ry0:ry1, rx0:rx1]
            wd, wmm = off_stream(gpu, mvsv, work)
            assert_bytes(disp, wd, f"frame {i} vs the off-stream call")
            want, rmm = ref.normalize(np.ascontiguousarray(work))
            assert_bytes(disp, want, f"frame {i} vs the restatement")
            assert mm == wmm == rmm and mm[0] == -16 and mm[1] > 0
            if lattice:
                sv = mvsv.samplepoint_values(gpu.from_numpy(np.ascontiguousarray(d[y0:y1, x0:x1])).cuda(), 2)
                assert np.array_equal(vals, sv.cpu().numpy()) and count == len(hits) > 0

    st.enable_display(roi=roi_u)
    run(roi_u, False)
    st.enable_samplepoints((Q_REF, 1e4, 16.0), roi=roi_u)  # both at the same time
    run(roi_u, True)
    st.disable_samplepoints()
    st.enable_display()  # a second call replaces the first: the whole map
    run(None, False)
    st.enable_display(roi=roi_u, alpha=32, beta=224)
    st.push(*frames[0])
    disp, mm = st.front_display()
    assert_bytes(disp, ref.normalize(np.ascontiguousarray(plain[0][0][y0:y1, x0:x1]), 32, 224)[0], "(32, 224)")
    st.pop()
    st.disable_display()
    st.push(*frames[0])
    with pytest.raises(mvsv.MvsvError):
        st.front_display()
    d, means = st.pop()
    assert np.array_equal(d, plain[0][0]) and np.array_equal(means, plain[0][1])
    st.close()


def test_raw_stream_brings_the_display_map(gpu, mvsv):
    from tests.test_gpu_raw_stream import GRID, MAPS, ROI, matcher, raw_pair
    st = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI, depth=4, batch=3, grid_roi=GRID)
    st.enable_display(roi=GRID)
    plain = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI, depth=4, batch=3, grid_roi=GRID)
    for seed in range(4):
        st.push_raw(*raw_pair(seed))
        plain.push_raw(*raw_pair(seed))
    x0, y0, x1, y1 = GRID
    for seed in range(4):
        disp, mm = st.front_display()
        d, means = st.pop()
        pd, pm = plain.pop()
        assert np.array_equal(d, pd) and np.array_equal(means, pm)
        want, wmm = ref.normalize(np.ascontiguousarray(d[y0:y1, x0:x1]))
        assert_bytes(disp, want, f"frame {seed}")
        assert mm == wmm
    st.close()
    plain.close()
