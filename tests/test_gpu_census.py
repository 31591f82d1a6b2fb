"""StereoSGBM on the census cost on the device, bit for bit against tests/census_restate.py.

The transform kernel alone (every window shape, images smaller than the window, strided
inputs and outputs with guard bytes), the maps over the LDS-ring cost kernel's tile shapes
(TX = 4 * max(512 / D, 1) columns by 16 rows, as tests/test_gpu_sgbm_color.py), the entry
points, the plan and the error paths.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import twin
from tests import census_restate as cs
from tests.conftest import GOLDEN
from tests.test_gpu_sgbm_color import image_width, matcher, report

pytestmark = pytest.mark.gpu

INVALID_ARG = -1


# ---- the transform alone -----------------------------------------------------------
WINDOWS = ((9, 7), (7, 9), (5, 5), (3, 3), (1, 3), (3, 1), (13, 5))
HEIGHTS = (1, 2, 3, 8, 33)
WIDTHS = (2, 5, 63, 64, 65, 257)
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_transform_equals_restatement(gpu, mvsv, window):
    """Three frames per shape: rows W + 5 bytes apart from an odd base address, frames a
    padded stride apart; output rows W + 3 words apart, frames padded, guards untouched."""
    from mvstereovision3_amd import _lib
    lib, ctx = _lib.lib(), _lib.context(0)
    cw, ch = window
    n = 3
    for H in HEIGHTS:
        for W in WIDTHS:
            rng = np.random.default_rng(1000 * H + W + cw)
            # few grey levels: ties (equal is not darker) everywhere
            frames = rng.integers(0, 256 if (H + W) % 2 else 6, (n, H, W)).astype(np.uint8)
            rs, off = W + 5, 3
            fs = H * rs + 11
            flat = gpu.full((off + n * fs + 64,), 0xA5, dtype=gpu.uint8, device="cuda")
            view = flat.as_strided((n, H, W), (fs, rs, 1), off)
            view.copy_(gpu.from_numpy(frames).cuda())
            assert view.data_ptr() % 2 == 1
            ors, ooff = W + 3, 2
            ofs = H * ors + 7
            obuf = gpu.full((ooff + n * ofs + 9,), SENTINEL, dtype=gpu.int64, device="cuda")
            oview = obuf.as_strided((n, H, W), (ofs, ors, 1), ooff)
            ctx_d = _lib.device_context(flat)
            rc = lib.mvsv_census_device(ctx_d.handle, n, view.data_ptr(), rs, fs, W, H, cw, ch, oview.data_ptr(), ors, ofs)
            assert rc == 0, lib.mvsv_last_error(ctx_d.handle)
            got = oview.cpu().numpy().view(np.uint64)
            for k in range(n):
                want = cs.census(frames[k], cw, ch)
                assert np.array_equal(got[k], want), f"H {H} W {W} frame {k}: " + report(got[k], want)
            guard = gpu.ones_like(obuf, dtype=gpu.bool)
            guard.as_strided((n, H, W), (ofs, ors, 1), ooff).fill_(False)
            assert bool((obuf[guard] == SENTINEL).all()), f"H {H} W {W}: guard words written"
    assert ctx is not None


def test_transform_wrappers_numpy_and_torch(gpu, mvsv):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (19, 70)).astype(np.uint8)
    want = cs.census(img, 9, 7)
    got = mvsv.census_transform(img)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint64 and np.array_equal(got, want)
    # a ROI view of a larger host image
    big = np.full((25, 80), 9, np.uint8)
    big[3:22, 4:74] = img
    assert np.array_equal(mvsv.census_transform(big[3:22, 4:74], (9, 7)), want)
    t = mvsv.census_transform(gpu.from_numpy(img).cuda(), window=(5, 5))
    assert t.is_cuda and np.array_equal(t.cpu().numpy().view(np.uint64), cs.census(img, 5, 5))
    tb = mvsv.census_transform(gpu.from_numpy(np.stack([img, img[::-1].copy()])).cuda(), window=(13, 5))
    assert np.array_equal(tb[1].cpu().numpy().view(np.uint64), cs.census(img[::-1], 13, 5))
    with pytest.raises(mvsv.MvsvError, match="census window"):
        mvsv.census_transform(img, (4, 4))
    with pytest.raises(mvsv.MvsvError, match="census window"):
        mvsv.census_transform(gpu.from_numpy(img).cuda(), (9, 9))


# ---- maps ---------------------------------------------------------------------------
MIN_D = (-3, 0, 5)
BLOCK = (1, 3, 5, 7)
PEN = ((0, 0), (3, 12), (10, 120), (72, 288))  # nibble, byte and u16 path planes
UNIQ = (0, 10)
SPECKLE = ((0, 0), (20, 2))
WINDOW = ((9, 7), (5, 5), (7, 9), (3, 3))


def case_params(i, D, mode):
    sw, sr = SPECKLE[(i // 2) % 2]
    p1, p2 = PEN[(i + i // 4) % 4]
    p = cs.params(min_disparity=MIN_D[i % 3], num_disparities=D, block_size=BLOCK[(i // 3) % 4], p1=p1, p2=p2,
                  pre_filter_cap=(0, 31, 63)[i % 3], uniqueness_ratio=UNIQ[i % 2], speckle_window_size=sw,
                  speckle_range=sr, mode=mode)
    return p, WINDOW[(i + i // 2) % 4]


def tile_cases():
    out = []
    for D in (16, 128):
        TX = 4 * max(512 // D, 1)
        i = 0
        for W1 in (TX - 1, TX, TX + 1, 2 * TX + 3):
            for H in (1, 2, 17, 33):
                out.append(pytest.param(D, W1, H, i, id=f"D{D}-W1_{W1}-H{H}"))
                i += 1
    out.append(pytest.param(32, 72, 24, 5, id="D32"))
    out.append(pytest.param(64, 72, 24, 6, id="D64"))
    out.append(pytest.param(256, 72, 24, 7, id="D256"))
    out.append(pytest.param(48, 45, 19, 8, id="D48"))
    return out


def test_the_cycled_parameters_cover_every_value():
    seen = {k: set() for k in ("minD", "bs", "pen", "uniq", "speckle", "window")}
    for c in tile_cases():
        D, _, _, i = c.values
        p, w = case_params(i, D, 0)
        seen["minD"].add(p["min_disparity"])
        seen["bs"].add(p["block_size"])
        seen["pen"].add((p["p1"], p["p2"]))
        seen["uniq"].add(p["uniqueness_ratio"])
        seen["speckle"].add((p["speckle_window_size"], p["speckle_range"]))
        seen["window"].add(w)
    assert seen == {"minD": set(MIN_D), "bs": set(BLOCK), "pen": set(PEN), "uniq": set(UNIQ),
                    "speckle": set(SPECKLE), "window": set(WINDOW)}


def pair_for(D, W1, H, i, p):
    W = image_width(W1, p["min_disparity"], D)
    assert twin.sgbm_effective(p, W)["W1"] == W1
    return cs.grey_pair(8000 + 31 * i + D, H, W, shift=3)


@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("D,W1,H,i", tile_cases())
def test_census_map_equals_restatement(gpu, mvsv, D, W1, H, i, mode):
    p, window = case_params(i, D, mode)
    L, R = pair_for(D, W1, H, i, p)
    want = cs.compute(L, R, p, window)
    got = matcher(mvsv, p).compute_census(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda(), window=window)
    got = got.cpu().numpy()
    assert got.dtype == np.int16 and got.shape == L.shape
    assert np.array_equal(got, want), report(got, want)


@pytest.fixture
def schedule(mvsv):
    """set(value): MVSV_OPT_PATH_SCHEDULE for the test, back to 0 afterwards."""
    yield lambda v: mvsv.set_option(mvsv.OPT_PATH_SCHEDULE, v)
    mvsv.set_option(mvsv.OPT_PATH_SCHEDULE, 0)


@functools.lru_cache(maxsize=None)
def d64_ref(mode):
    p = cs.params(num_disparities=64, block_size=5, p1=3, p2=12, uniqueness_ratio=10, speckle_window_size=20,
                  speckle_range=2, mode=mode)
    L, R = cs.grey_pair(640 + mode, 21, 64 + 75, shift=9)
    return p, L, R, cs.compute(L, R, p, (9, 7))


@pytest.mark.parametrize("sched", [0, 1, 2])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_d64_under_every_path_schedule(gpu, mvsv, schedule, mode, sched):
    p, L, R, want = d64_ref(mode)
    schedule(sched)
    got = matcher(mvsv, p).compute_census(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()).cpu().numpy()
    assert np.array_equal(got, want), report(got, want)


def test_fixture_maps(gpu, mvsv):
    z = np.load(os.path.join(GOLDEN, "census_fixtures.npz"))
    for k in range(int(z["count"])):
        p = dict(zip(cs.cr.PARAM_NAMES, (int(v) for v in z[f"params{k}"])))
        window = tuple(int(v) for v in z[f"window{k}"])
        got = matcher(mvsv, p).compute_census(z[f"L{k}"], z[f"R{k}"], window=window)
        assert np.array_equal(got, z[f"map{k}"]), f"fixture {k}: " + report(got, z[f"map{k}"])


# ---- properties and entry points ------------------------------------------------------
@pytest.mark.parametrize("mode", cs.KNOWN_MODES)
@pytest.mark.parametrize("window", cs.KNOWN_WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_invariance_and_known_answer_on_the_device(gpu, mvsv, window, mode):
    p = cs.params(mode=mode, **cs.KNOWN_PARAMS)
    m = matcher(mvsv, p)
    for seed in cs.KNOWN_SEEDS:
        L, R = cs.noise_shift_pair(seed)
        L2, R2 = cs.radiometric(L, R)
        # the census statement holds on the restatement itself first
        want = cs.compute(L, R, p, window)
        rows, cols = cs.known_region(*L.shape)
        assert (want[rows, cols] == 16 * 5).all() and np.array_equal(want, cs.compute(L2, R2, p, window))
        a = m.compute_census(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda(), window=window).cpu().numpy()
        b = m.compute_census(gpu.from_numpy(L2).cuda(), gpu.from_numpy(R2).cuda(), window=window).cpu().numpy()
        assert np.array_equal(a, b), f"seed {seed}: the map changes under v -> 2v / v -> v + 100: " + report(a, b)
        assert (a[rows, cols] == 16 * 5).all(), f"seed {seed}"
        assert np.array_equal(a, want), report(a, want)
        # pre_filter_cap has no effect on a census call
        m2 = matcher(mvsv, dict(p, pre_filter_cap=63))
        assert np.array_equal(m2.compute_census(L, R, window=window), want)


@pytest.fixture(scope="module")
def layout_ref():
    p = cs.params(min_disparity=-2, num_disparities=16, block_size=5, p1=8, p2=32, uniqueness_ratio=10,
                  speckle_window_size=20, speckle_range=2)
    pairs = [cs.grey_pair(500 + k, 21, 150) for k in range(3)]
    maps = [cs.compute(L, R, p, (9, 7)) for L, R in pairs]
    return p, pairs, maps


def strided_frames(torch, frames, row_stride, frame_stride, offset, fill):
    n, H, W = frames.shape
    flat = torch.full((offset + n * frame_stride + 64,), fill, dtype=torch.uint8, device="cuda")
    view = flat.as_strided((n, H, W), (frame_stride, row_stride, 1), offset)
    view.copy_(torch.from_numpy(frames).cuda())
    return flat, view


def test_host_entry_on_roi_views(gpu, mvsv, layout_ref):
    p, pairs, maps = layout_ref
    L, R = pairs[1]
    H, W = L.shape
    m = matcher(mvsv, p)
    got = m.compute_census(L, R)
    assert isinstance(got, np.ndarray) and np.array_equal(got, maps[1]), report(got, maps[1])
    bigL = np.full((H + 4, W + 9), 77, np.uint8)
    bigR = np.full((H + 4, W + 9), 33, np.uint8)
    bigL[2:2 + H, 5:5 + W] = L
    bigR[1:1 + H, 4:4 + W] = R
    pair = mvsv.Stereopair(bigL[2:2 + H, 5:5 + W], bigR[1:1 + H, 4:4 + W])
    out = np.full((H + 2, W + 6), -999, np.int16)
    got = mvsv.Disparity.binary_sgbm(pair, out[1:1 + H, 3:3 + W], m)
    assert np.array_equal(got, maps[1]), report(got, maps[1])
    assert np.shares_memory(got, out) and (out[0] == -999).all() and (out[:, :3] == -999).all()
    # the default window is (9, 7); another one gives another map
    assert not np.array_equal(mvsv.Disparity.binary_sgbm(pair, None, m, (3, 3)), maps[1])


def test_device_batch_with_padded_frame_stride(gpu, mvsv, layout_ref):
    p, pairs, maps = layout_ref
    Ls = np.stack([a for a, _ in pairs])
    Rs = np.stack([b for _, b in pairs])
    n, H, W = Ls.shape
    fl, lv = strided_frames(gpu, Ls, W + 5, H * (W + 5) + 11, 1, 0xA5)
    fr, rv = strided_frames(gpu, Rs, W + 6, H * (W + 6) + 2, 3, 0x5A)
    before = (fl.clone(), fr.clone())
    got = matcher(mvsv, p).compute_census(lv, rv).cpu().numpy()
    assert got.shape == (n, H, W)
    for k in range(n):
        assert np.array_equal(got[k], maps[k]), f"frame {k}: " + report(got[k], maps[k])
    assert gpu.equal(fl, before[0]) and gpu.equal(fr, before[1])


def test_side_stream_and_bt_afterwards(gpu, mvsv, layout_ref):
    p, pairs, maps = layout_ref
    L, R = pairs[2]
    Lt, Rt = gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()
    gpu.cuda.synchronize()
    s = gpu.cuda.Stream()
    with gpu.cuda.stream(s):
        got = matcher(mvsv, p).compute_census(Lt, Rt)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), maps[2]), report(got.cpu().numpy(), maps[2])
    # the BT entry on the same context afterwards is untouched by the census launch
    g = matcher(mvsv, p).compute(Lt, Rt).cpu().numpy()
    assert np.array_equal(g, twin.sgbm_compute(L, R, p))
    assert not np.array_equal(g, maps[2])


def test_plan_of_a_census_launch(gpu, mvsv):
    from mvstereovision3_amd import _lib
    from tests.conftest import CONFIGS
    m = mvsv.StereoSGBM.create(0, 0, 0, 0, 0)
    assert mvsv.Disparity.loadSGBMParameters(os.path.join(CONFIGS, "sgbm.yml"), m, mvsv.sgbmParameters())
    ctx = _lib.context(0)
    lib = _lib.lib()
    for mode in (mvsv.MODE_SGBM, mvsv.MODE_HH):
        m.setMode(mode)
        for n in (1, 8):
            bt = _lib.sgbm_plan(ctx, n, 1280, 960, m._params)
            census = _lib.sgbm_plan(ctx, n, 1280, 960, m._params, census=(9, 7))
            assert bt & (_lib.PLAN_BITSLICE | _lib.PLAN_RESIDUAL), (mode, n)
            assert not census & (_lib.PLAN_BITSLICE | _lib.PLAN_RESIDUAL), (mode, n)
            assert census & (_lib.PLAN_SIDE | _lib.PLAN_STRIPS)
            # the workspace query follows: no residual / bit planes, so not the BT figure
            wb = lib.mvsv_sgbm_workspace_bytes_census(n, 1280, 960, ctypes.byref(m._params), 9, 7)
            assert wb > 0 and wb != lib.mvsv_sgbm_workspace_bytes(n, 1280, 960, ctypes.byref(m._params))
    assert lib.mvsv_sgbm_workspace_bytes_census(1, 1280, 960, ctypes.byref(m._params), 9, 9) == 0


def test_error_paths_name_the_rule(gpu, mvsv):
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    ctx = _lib.context(0)
    H, W = 8, 40
    p = mvsv.StereoSGBM.create(0, 16, 3)._params
    Lt = gpu.zeros((H, W), dtype=gpu.uint8, device="cuda")
    out = gpu.zeros((H, W), dtype=gpu.int16, device="cuda")
    a, o = Lt.data_ptr(), out.data_ptr()
    dev = lib.mvsv_sgbm_census_device

    def call(*, n=1, l=a, ls=W, r=a, rs=W, par=p, dst=o, os_=W, cw=9, ch=7, h=ctx.handle):
        return dev(h, n, l, ls, W * H, r, rs, W * H, W, H, ctypes.byref(par) if par is not None else None, dst, os_,
                   W * H, cw, ch)

    def message():
        return lib.mvsv_last_error(ctx.handle).decode()

    assert call() == 0
    for cw, ch in ((8, 7), (9, 9), (1, 1), (0, 0), (-1, 3)):
        assert call(cw=cw, ch=ch) == INVALID_ARG and "census window" in message(), (cw, ch)
    big = mvsv.StereoSGBM.create(0, 16, 21, 10, 5426)._params
    assert call(par=big) == INVALID_ARG and "32767" in message() and "census cost" in message()
    assert call(par=mvsv.StereoSGBM.create(0, 16, 3, mode=2)._params) == INVALID_ARG and "MODE_SGBM_3WAY" in message()
    assert call(par=mvsv.StereoSGBM.create(0, 24, 3)._params) == INVALID_ARG and "numDisparities" in message()
    assert call(ls=W - 1) == INVALID_ARG and "stride" in message()
    assert call(os_=W - 1) == INVALID_ARG and "stride" in message()
    assert call(l=None) == INVALID_ARG and call(dst=None) == INVALID_ARG and call(n=0) == INVALID_ARG
    assert call(par=None) == INVALID_ARG and call(h=None) == INVALID_ARG
    gpu.cuda.synchronize()
    # the plan query and the host entry: the same rules
    plan = ctypes.c_int(0)
    assert lib.mvsv_sgbm_plan_census(ctx.handle, 1, W, H, ctypes.byref(p), 9, 9, ctypes.byref(plan)) == INVALID_ARG
    assert "census window" in message()
    Lh = np.zeros((H, W), np.uint8)
    oh = np.zeros((H, W), np.int16)
    host = lib.mvsv_sgbm_census
    assert host(ctx.handle, Lh.ctypes.data, W, Lh.ctypes.data, W, W, H, ctypes.byref(p), oh.ctypes.data, W, 9, 7) == 0
    assert host(ctx.handle, Lh.ctypes.data, W, Lh.ctypes.data, W, W, H, ctypes.byref(p), oh.ctypes.data, W, 6, 7) == INVALID_ARG
    assert "census window" in message()
    assert host(ctx.handle, Lh.ctypes.data, W - 1, Lh.ctypes.data, W, W, H, ctypes.byref(p), oh.ctypes.data, W, 9, 7) == INVALID_ARG
    assert lib.mvsv_census(ctx.handle, Lh.ctypes.data, W - 1, W, H, 9, 7, oh.ctypes.data, W) == INVALID_ARG
    assert lib.mvsv_census_device(ctx.handle, 1, a, W, W * H, W, H, 9, 7, o, W - 1, W * H) == INVALID_ARG
    # the wrapper: mixed host / device, mismatched shapes
    m = mvsv.StereoSGBM.create(0, 16, 3)
    with pytest.raises(mvsv.MvsvError):
        m.compute_census(Lt, Lh)
    with pytest.raises(mvsv.MvsvError):
        m.compute_census(Lt, gpu.zeros((H, W + 1), dtype=gpu.uint8, device="cuda"))
    with pytest.raises(mvsv.MvsvError, match="census window"):
        m.compute_census(Lt, Lt, window=(2, 2))
    # and the context still works
    assert m.compute_census(Lt, Lt).shape == (H, W)
