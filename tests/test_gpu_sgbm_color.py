"""StereoSGBM on colour (BGR) pairs on the device, bit for bit.

References: tests/sgbm_color_restate.py (the twin's pipeline on the summed pixel
cost; valid while no int16 cost wraps) and, through the one-live-channel identity,
the C oracle on the grey pair -- the only reference where costs do wrap.

The general cost kernel's tile is TX = 4 * max(512 / D, 1) columns by 16 rows, so
the shapes are small: cost-space widths around one and two tiles, heights of one
row, two rows, one tile + 1 and two tiles + 1.
"""
import ctypes

import numpy as np
import pytest

from oracle import twin
from tests import sgbm_color_restate as cr

pytestmark = pytest.mark.gpu

INVALID_ARG = -1


def report(a, b):
    bad = np.argwhere(a != b)
    if bad.size == 0:
        return ""
    pts = [(int(y), int(x), int(a[y, x]), int(b[y, x])) for y, x in bad[:10]]
    return f"{len(bad)} mismatches of {a.size}; first (y, x, gpu, reference): {pts}"


def matcher(mvsv, p):
    m = mvsv.StereoSGBM.create(p["min_disparity"], p["num_disparities"], p["block_size"], p["p1"], p["p2"],
                               p["disp12_max_diff"], p["pre_filter_cap"], p["uniqueness_ratio"],
                               p["speckle_window_size"], p["speckle_range"], p["mode"])
    return m


def image_width(W1, minD, D):
    """The image width whose cost space is W1 columns wide."""
    return W1 - min(minD, 0) + max(minD + D, 0)


def bgr_pair(seed, H, W, shift=3):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    # smooth a little along x so that matches exist, per channel
    L = ((L.astype(int) + np.roll(L, 1, axis=1) + np.roll(L, 2, axis=1)) // 3).astype(np.uint8)
    R = np.roll(L, -shift, axis=1)
    R = np.clip(R.astype(int) + rng.integers(-4, 5, R.shape), 0, 255).astype(np.uint8)
    return L, R


MIN_D = (-3, 0, 5)
BLOCK = (3, 5, 7)
CAP = (0, 31, 63)
UNIQ = (0, 10)
SPECKLE = ((0, 0), (20, 2))
PEN = ((0, 0), (3, 12), (8, 30), (72, 288))  # nibble, byte and u16 path planes


def case_params(i, D, mode):
    sw, sr = SPECKLE[(i // 2) % 2]
    p1, p2 = PEN[i % 4]
    return cr.params(min_disparity=MIN_D[i % 3], num_disparities=D, block_size=BLOCK[(i // 3) % 3], p1=p1, p2=p2,
                     pre_filter_cap=CAP[(i + i // 3) % 3], uniqueness_ratio=UNIQ[i % 2], speckle_window_size=sw,
                     speckle_range=sr, mode=mode)


def tile_cases():
    out = []
    for D in (16, 128):
        TX = 4 * max(512 // D, 1)
        i = 0
        for W1 in (TX - 1, TX, TX + 1, 2 * TX + 3):
            for H in (1, 2, 17, 33):
                out.append(pytest.param(D, W1, H, i, id=f"D{D}-W1_{W1}-H{H}"))
                i += 1
    # one case each: the other 16-lane path widths, the widest D, and a D no 16-lane kernel takes
    out.append(pytest.param(32, 72, 24, 5, id="D32"))
    out.append(pytest.param(64, 72, 24, 6, id="D64"))
    out.append(pytest.param(256, 72, 24, 7, id="D256"))
    out.append(pytest.param(48, 45, 19, 8, id="D48"))
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D,W1,H,i", tile_cases())
def test_color_map_equals_restatement(gpu, mvsv, D, W1, H, i, mode):
    p = case_params(i, D, mode)
    W = image_width(W1, p["min_disparity"], D)
    assert twin.sgbm_effective(p, W)["W1"] == W1
    L, R = bgr_pair(7000 + 31 * i + D, H, W)
    want = cr.compute_bgr(L, R, p)
    got = matcher(mvsv, p).compute_bgr(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()).cpu().numpy()
    assert got.dtype == np.int16 and got.shape == (H, W)
    assert np.array_equal(got, want), report(got, want)


# ---- one live channel: the grey pair's map, whatever the channel ---------------
def grey_pair(seed, H, W, shift=4):
    rng = np.random.default_rng(seed)
    Lg = rng.integers(0, 256, (H, W)).astype(np.uint8)
    Lg = ((Lg.astype(int) + np.roll(Lg, 1, axis=1)) // 2).astype(np.uint8)
    Rg = np.roll(Lg, -shift, axis=1)
    Rg = np.clip(Rg.astype(int) + rng.integers(-3, 4, Rg.shape), 0, 255).astype(np.uint8)
    return Lg, Rg


@pytest.fixture(scope="module")
def identity_refs(oracle):
    """(params, grey pair, oracle map) per (regime, mode), computed once."""
    refs = {}
    for mode in (0, 1):
        # no int16 can wrap, colour bound included: 2 * 40 + 25 * 3 * (2 * 31 + 63) <= 32767
        refs["nowrap", mode] = cr.params(num_disparities=32, block_size=5, p1=10, p2=40, pre_filter_cap=31,
                                         uniqueness_ratio=10, speckle_window_size=20, speckle_range=2, mode=mode)
        # the colour bound 2 * 2592 + 169 * 3 * 189 is beyond int16: the general recurrence
        refs["wrap", mode] = cr.params(num_disparities=32, block_size=13, p1=648, p2=2592, pre_filter_cap=63,
                                       uniqueness_ratio=5, mode=mode)
    out = {}
    for key, p in refs.items():
        Lg, Rg = grey_pair(99 + key[1], 37, 90)
        out[key] = (p, Lg, Rg, oracle.sgbm(Lg, Rg, p))
    return out


@pytest.mark.parametrize("channel", [0, 1, 2])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("regime", ["nowrap", "wrap"])
def test_one_live_channel_equals_grey_oracle(gpu, mvsv, identity_refs, regime, mode, channel):
    p, Lg, Rg, want = identity_refs[regime, mode]
    bs = p["block_size"]
    ftzero = twin.sgbm_effective(p, Lg.shape[1])["ftzero"]
    bound = 2 * p["p2"] + bs * bs * 3 * (2 * ftzero + 63)
    assert (bound <= 32767) == (regime == "nowrap")
    L, R = cr.one_live_channel(Lg, Rg, channel, ftzero)
    got = matcher(mvsv, p).compute_bgr(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()).cpu().numpy()
    assert np.array_equal(got, want), report(got, want)


# ---- layouts and entry points --------------------------------------------------
@pytest.fixture(scope="module")
def layout_ref():
    p = cr.params(min_disparity=-2, num_disparities=16, block_size=5, p1=8, p2=32, pre_filter_cap=31,
                  uniqueness_ratio=10, speckle_window_size=20, speckle_range=2)
    pairs = [bgr_pair(500 + k, 21, 150) for k in range(3)]
    maps = [cr.compute_bgr(L, R, p) for L, R in pairs]
    return p, pairs, maps


def strided_frames(torch, frames, row_stride, frame_stride, offset, fill):
    """The frames (N, H, W, 3) inside one flat byte buffer filled with `fill`: rows
    row_stride bytes apart, frames frame_stride apart, first byte at `offset`."""
    n, H, W, _ = frames.shape
    flat = torch.full((offset + n * frame_stride + 64,), fill, dtype=torch.uint8, device="cuda")
    view = flat.as_strided((n, H, W, 3), (frame_stride, row_stride, 3, 1), offset)
    view.copy_(torch.from_numpy(frames).cuda())
    return flat, view


def test_padded_rows_with_odd_base(gpu, mvsv, layout_ref):
    p, pairs, maps = layout_ref
    L, R = pairs[0]
    H, W, _ = L.shape
    rs = 3 * W + 5
    fl, lv = strided_frames(gpu, L[None], rs, H * rs, 1, 0xA5)
    fr, rv = strided_frames(gpu, R[None], rs, H * rs, 1, 0x5A)
    before = (fl.clone(), fr.clone())
    # output rows padded too, sentinel around and between them
    obuf = gpu.full((7 + H * (W + 3) + 9,), -12345, dtype=gpu.int16, device="cuda")
    ov = obuf.as_strided((H, W), (W + 3, 1), 7)
    got = matcher(mvsv, p).compute_bgr(lv[0], rv[0], ov)
    assert got.data_ptr() == ov.data_ptr()
    assert np.array_equal(got.cpu().numpy(), maps[0]), report(got.cpu().numpy(), maps[0])
    assert gpu.equal(fl, before[0]) and gpu.equal(fr, before[1])
    guard = gpu.ones_like(obuf, dtype=gpu.bool)
    guard.as_strided((H, W), (W + 3, 1), 7).fill_(False)
    assert bool((obuf[guard] == -12345).all())


def test_batch_with_padded_frame_stride(gpu, mvsv, layout_ref):
    p, pairs, maps = layout_ref
    Ls = np.stack([a for a, _ in pairs])
    Rs = np.stack([b for _, b in pairs])
    n, H, W, _ = Ls.shape
    rs = 3 * W + 5
    _, lv = strided_frames(gpu, Ls, rs, H * rs + 11, 1, 0xA5)
    _, rv = strided_frames(gpu, Rs, rs + 1, H * (rs + 1) + 2, 3, 0x5A)
    got = matcher(mvsv, p).compute_bgr(lv, rv).cpu().numpy()
    assert got.shape == (n, H, W)
    for k in range(n):
        assert np.array_equal(got[k], maps[k]), f"frame {k}: " + report(got[k], maps[k])


def test_host_entry_and_roi_views(gpu, mvsv, layout_ref):
    p, pairs, maps = layout_ref
    L, R = pairs[1]
    H, W, _ = L.shape
    m = matcher(mvsv, p)
    got = m.compute_bgr(L, R)
    assert isinstance(got, np.ndarray) and np.array_equal(got, maps[1]), report(got, maps[1])
    # ROI views of larger images: step > 3 * cols, as a cropped cv::Mat has
    bigL = np.full((H + 4, W + 9, 3), 77, np.uint8)
    bigR = np.full((H + 4, W + 9, 3), 33, np.uint8)
    bigL[2:2 + H, 5:5 + W] = L
    bigR[1:1 + H, 4:4 + W] = R
    pair = mvsv.Stereopair(bigL[2:2 + H, 5:5 + W], bigR[1:1 + H, 4:4 + W])
    got = mvsv.Disparity.sgbm_bgr(pair, None, m)
    assert np.array_equal(got, maps[1]), report(got, maps[1])
    # a batch of host frames
    got = m.compute_bgr(np.stack([pairs[0][0], pairs[2][0]]), np.stack([pairs[0][1], pairs[2][1]]))
    assert np.array_equal(got[0], maps[0]) and np.array_equal(got[1], maps[2])


def test_side_stream(gpu, mvsv, layout_ref):
    p, pairs, maps = layout_ref
    L, R = pairs[2]
    Lt, Rt = gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()
    gpu.cuda.synchronize()
    s = gpu.cuda.Stream()
    with gpu.cuda.stream(s):
        got = matcher(mvsv, p).compute_bgr(Lt, Rt)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), maps[2]), report(got.cpu().numpy(), maps[2])
    # the grey entry on the same context afterwards is untouched by the colour launch
    g = matcher(mvsv, p).compute(Lt[:, :, 0].contiguous(), Rt[:, :, 0].contiguous()).cpu().numpy()
    assert np.array_equal(g, twin.sgbm_compute(L[:, :, 0], R[:, :, 0], p))


def test_plan_of_a_colour_launch(gpu, mvsv):
    import os

    from mvstereovision3_amd import _lib
    from tests.conftest import CONFIGS
    m = mvsv.StereoSGBM.create(0, 0, 0, 0, 0)
    assert mvsv.Disparity.loadSGBMParameters(os.path.join(CONFIGS, "sgbm.yml"), m, mvsv.sgbmParameters())
    m.setMode(mvsv.MODE_HH)
    ctx = _lib.context(0)
    for n in (1, 8):
        grey = _lib.sgbm_plan(ctx, n, 640, 480, m._params)
        colour = _lib.sgbm_plan(ctx, n, 640, 480, m._params, channels=3)
        assert grey & _lib.PLAN_BITSLICE
        assert not colour & (_lib.PLAN_BITSLICE | _lib.PLAN_RESIDUAL)
        assert colour & (_lib.PLAN_SIDE | _lib.PLAN_STRIPS)
    # and such a launch computes the restatement's map (sgbm.yml's parameters, small frame)
    p = {k: v for k, v in m.params().items() if k != "variant"}
    L, R = bgr_pair(321, 20, 128 + 40)
    want = cr.compute_bgr(L, R, p)
    got = m.compute_bgr(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()).cpu().numpy()
    assert np.array_equal(got, want), report(got, want)


def test_error_paths(gpu, mvsv):
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    ctx = _lib.context(0)
    H, W = 8, 40
    p = mvsv.StereoSGBM.create(0, 16, 3)._params
    Lt = gpu.zeros((H, W, 3), dtype=gpu.uint8, device="cuda")
    out = gpu.zeros((H, W), dtype=gpu.int16, device="cuda")
    a, o = Lt.data_ptr(), out.data_ptr()
    dev = lib.mvsv_sgbm_bgr_device
    assert dev(ctx.handle, 1, a, 3 * W, 3 * W * H, a, 3 * W, 3 * W * H, W, H, ctypes.byref(p), o, W, W * H) == 0
    # a row stride below 3 * W, on either side; an output stride below W
    assert dev(ctx.handle, 1, a, 3 * W - 1, 3 * W * H, a, 3 * W, 3 * W * H, W, H, ctypes.byref(p), o, W, W * H) == INVALID_ARG
    assert dev(ctx.handle, 1, a, 3 * W, 3 * W * H, a, W, 3 * W * H, W, H, ctypes.byref(p), o, W, W * H) == INVALID_ARG
    assert dev(ctx.handle, 1, a, 3 * W, 3 * W * H, a, 3 * W, 3 * W * H, W, H, ctypes.byref(p), o, W - 1, W * H) == INVALID_ARG
    # null pointers, no frames, null context
    assert dev(ctx.handle, 1, None, 3 * W, 3 * W * H, a, 3 * W, 3 * W * H, W, H, ctypes.byref(p), o, W, W * H) == INVALID_ARG
    assert dev(ctx.handle, 1, a, 3 * W, 3 * W * H, a, 3 * W, 3 * W * H, W, H, ctypes.byref(p), None, W, W * H) == INVALID_ARG
    assert dev(ctx.handle, 1, a, 3 * W, 3 * W * H, a, 3 * W, 3 * W * H, W, H, None, o, W, W * H) == INVALID_ARG
    assert dev(ctx.handle, 0, a, 3 * W, 3 * W * H, a, 3 * W, 3 * W * H, W, H, ctypes.byref(p), o, W, W * H) == INVALID_ARG
    assert dev(None, 1, a, 3 * W, 3 * W * H, a, 3 * W, 3 * W * H, W, H, ctypes.byref(p), o, W, W * H) == INVALID_ARG
    gpu.cuda.synchronize()
    # the host entry: the same rules
    Lh = np.zeros((H, W, 3), np.uint8)
    oh = np.zeros((H, W), np.int16)
    host = lib.mvsv_sgbm_bgr
    assert host(ctx.handle, Lh.ctypes.data, 3 * W, Lh.ctypes.data, 3 * W, W, H, ctypes.byref(p), oh.ctypes.data, W) == 0
    assert host(ctx.handle, Lh.ctypes.data, 3 * W - 1, Lh.ctypes.data, 3 * W, W, H, ctypes.byref(p), oh.ctypes.data, W) == INVALID_ARG
    assert host(ctx.handle, None, 3 * W, Lh.ctypes.data, 3 * W, W, H, ctypes.byref(p), oh.ctypes.data, W) == INVALID_ARG
    assert host(ctx.handle, Lh.ctypes.data, 3 * W, Lh.ctypes.data, 3 * W, W, H, ctypes.byref(p), None, W) == INVALID_ARG
    # mvsv_sgbm_validate's rules hold: numDisparities not a multiple of 16
    bad = mvsv.StereoSGBM.create(0, 24, 3)
    with pytest.raises(mvsv.MvsvError):
        bad.compute_bgr(Lt, Lt)
    # the wrapper: mismatched shapes, mixed host / device, grey input
    m = mvsv.StereoSGBM.create(0, 16, 3)
    with pytest.raises(mvsv.MvsvError):
        m.compute_bgr(Lt, gpu.zeros((H, W + 1, 3), dtype=gpu.uint8, device="cuda"))
    with pytest.raises(mvsv.MvsvError):
        m.compute_bgr(Lt, Lh)
    with pytest.raises(mvsv.MvsvError):
        m.compute_bgr(Lt[:, :, 0], Lt[:, :, 0])
    # and the context still works
    z = m.compute_bgr(Lt, Lt)
    assert z.shape == (H, W)


# ---- the frame stream: BGR frames matched in colour ------------------------------
STREAM_SRC = (192, 80)  # (width, height) of the colour frames; the stream's frames are 96 x 40


@pytest.fixture(scope="module")
def stream_frames(mvsv):
    """Per seed: the colour pair, its restated halved BGR pair and prepared grey pair."""
    from tests import prepare_restate as prep
    w, h = STREAM_SRC
    out = []
    for seed in range(4):
        rng = np.random.default_rng(40 + seed)
        pair = []
        for g in mvsv.synth_pair(0xC0100 + seed, w, h, 0, 32):
            # colour that matters: every channel its own gain and noise
            c = g[..., None].astype(np.int64) * np.array([3, 4, 2]) // 4 + rng.integers(-20, 21, (h, w, 3))
            pair.append(np.clip(c, 0, 255).astype(np.uint8))
        half = tuple(np.stack([prep.halve_plane(c[..., k]) for k in range(3)], axis=-1) for c in pair)
        grey = tuple(prep.prepare(c) for c in pair)
        out.append((tuple(pair), half, grey))
    return out


def stream_matcher(mvsv):
    return mvsv.StereoSGBM.create(0, 32, 5, 8, 32, 1, 31, 10, 20, 2, mvsv.MODE_SGBM)


def test_stream_matches_bgr_frames_in_colour(gpu, mvsv, oracle, stream_frames):
    m = stream_matcher(mvsv)
    p = {k: v for k, v in m.params().items() if k != "variant"}
    assert mvsv.prepare_size(*STREAM_SRC) == (96, 40)
    colour_want = [cr.compute_bgr(half[0], half[1], p) for _, half, _ in stream_frames]
    grey_want = [oracle.sgbm(grey[0], grey[1], p) for _, _, grey in stream_frames]
    for a, b in zip(colour_want, grey_want):
        assert not np.array_equal(a, b)  # the inputs tell the two matchers apart
    # the one-shot colour entry on the restated halved pair
    one = m.compute_bgr(gpu.from_numpy(stream_frames[0][1][0]).cuda(), gpu.from_numpy(stream_frames[0][1][1]).cuda())
    assert np.array_equal(one.cpu().numpy(), colour_want[0])

    st = mvsv.DisparityStream(m, 96, 40, depth=4, batch=2, grid_roi=(0, 0, 96, 40))
    st.enable_bgr((STREAM_SRC[1], STREAM_SRC[0]))
    st.enable_sharpness()

    def run(order):
        got = []

        def pop():
            sharp = st.front_sharpness(return_sums=True)
            d, means = st.pop()
            got.append((d, means, sharp))
        for k, how in enumerate(order):
            if st.pending() == 4:
                pop()
            pair, _, grey = stream_frames[k % 4]
            if how == "c":
                st.push_bgr(*pair)
            else:
                st.push(*grey)
        while st.pending():
            pop()
        return got

    # every BGR frame matched in grey first: the products to compare with
    order = ["c", "g", "c", "c", "g", "g", "c", "c"]
    plain = run(order)
    for k, (d, _, _) in enumerate(plain):
        assert np.array_equal(d, grey_want[k % 4]), f"grey-matched frame {k}"
    st.bgr_match(True)
    # colour and grey frames alternate under batch 2: a launch of two frames of one
    # kind, and pairs of different kinds that must not share one
    got = run(order)
    for k, (d, means, sharp) in enumerate(got):
        want = colour_want[k % 4] if order[k] == "c" else grey_want[k % 4]
        assert np.array_equal(d, want), f"frame {k} ({order[k]}): " + report(d, want)
        # the products of the map follow the map; those of the grey pair are unchanged
        assert np.array_equal(means, twin.mean_disparity_grid(want)), f"frame {k}: mean grid"
        assert sharp == plain[k][2], f"frame {k}: sharpness"
    # device pushes take the same path
    Lt, Rt = (gpu.from_numpy(c).cuda() for c in stream_frames[1][0])
    st.push_bgr(Lt, Rt)
    st.push(*stream_frames[1][2])
    assert np.array_equal(st.pop()[0], colour_want[1])
    assert np.array_equal(st.pop()[0], grey_want[1])
    # a switch to StereoBM is refused while colour matching is on, and nothing changes
    with pytest.raises(mvsv.MvsvError):
        st.set_params(mvsv.StereoBM.create(32, 9))
    assert st.matcher() == mvsv.MATCHER_SGBM
    st.push_bgr(*stream_frames[2][0])
    from mvstereovision3_amd import _lib
    assert _lib.lib().mvsv_stream_set_bgr_match(st._h, 0) == INVALID_ARG  # a frame is pending
    assert np.array_equal(st.pop()[0], colour_want[2])
    st.bgr_match(False)
    st.push_bgr(*stream_frames[2][0])
    assert np.array_equal(st.pop()[0], grey_want[2])
    st.set_params(mvsv.StereoBM.create(32, 9))  # allowed again
    with pytest.raises(mvsv.MvsvError):
        st.bgr_match(True)  # not with the BM matcher
    st.close()


def test_stream_colour_match_without_halving(gpu, mvsv, stream_frames):
    m = stream_matcher(mvsv)
    p = {k: v for k, v in m.params().items() if k != "variant"}
    L, R = stream_frames[3][1]  # a 96 x 40 colour pair, pushed as it is
    st = mvsv.DisparityStream(m, 96, 40, depth=2)
    with pytest.raises(mvsv.MvsvError):
        st.bgr_match(True)  # enable_bgr first
    st.enable_bgr((40, 96), halve=False)
    st.bgr_match(True)
    st.push_bgr(L, R)
    want = cr.compute_bgr(L, R, p)
    got = st.pop()[0]
    assert np.array_equal(got, want), report(got, want)
    st.close()
