"""StereoBM on the census cost on the device, bit for bit against tests/census_bm_restate.py.

The shapes are where the kernels can go wrong, not the workload's: the fast kernel
(bm_census_match2_kernel: blockSize 5 .. 21, D <= 128) takes BC = 64 output columns per
block for D <= 64 and 32 above (two waves per column group), in column groups of 16, by
TY output rows (pinned through MVSV_OPT_BM_TILE_ROWS); the general form
(bm_census_match_kernel) takes 16 x 16 tiles.

One case of the issue cannot exist: ymax - ymin = 1 needs H = blockSize, which
mvsv_bm_validate's inherited rule (blockSize < min(W, H)) refuses; the smallest map has
two output rows.  test_one_output_row_is_refused_by_the_inherited_rule pins that.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import twin
from tests import census_bm_restate as cb
from tests import census_restate as cs
from tests.conftest import CONFIGS, GOLDEN
from tests.test_gpu_sgbm_color import report

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
TY = 8  # the pinned tile height of the row cases

MIN_D = (-5, 0, 3)
UNIQ = (0, 15)
D12 = (-1, 0, 1)
SPECKLE = ((0, 0), (20, 2))
WINDOWS = ((5, 5), (3, 3), (1, 3), (3, 1), (9, 7), (7, 9), (13, 5))  # four one-word, three two-word


def cycled(i, D, bs):
    sw, sr = SPECKLE[(i // 2) % 2]
    p = cb.params(min_disparity=MIN_D[i % 3], num_disparities=D, block_size=bs, uniqueness_ratio=UNIQ[i % 2],
                  disp12_max_diff=D12[(i + i // 3) % 3], speckle_window_size=sw, speckle_range=sr,
                  texture_threshold=(0, 10, 4000)[i % 3], pre_filter_cap=(1, 31, 63)[(i + 1) % 3])
    return p, WINDOWS[i % 7]


def matcher(mvsv, p):
    m = mvsv.StereoBM.create(p["num_disparities"], p["block_size"])
    for k, v in p.items():
        setattr(m._params, k, v)
    return m


def width_for(ncol, p, H):
    """The image width whose computed column count (min(width1, W - lofs)) is ncol."""
    for W in range(p["block_size"] + 1, 4096):
        g = cb.geometry(p, W, H)
        if g is not None and g["ncol"] == ncol:
            return W
    raise AssertionError(f"no width gives {ncol} columns")


@pytest.fixture
def tile_rows(mvsv):
    """set(ty): MVSV_OPT_BM_TILE_ROWS for the test, back to 0 (chosen per launch) afterwards."""
    from mvstereovision3_amd import _lib
    yield lambda ty: _lib.set_option(_lib.OPT_BM_TILE_ROWS, ty)
    _lib.set_option(_lib.OPT_BM_TILE_ROWS, 0)


def run(gpu, mvsv, L, R, p, window):
    got = matcher(mvsv, p).compute_census(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda(), window=window)
    got = got.cpu().numpy()
    assert got.dtype == np.int16 and got.shape == L.shape
    return got


# ---- the fast kernel ---------------------------------------------------------------
def column_cases():
    out, i = [], 0
    for D, BC in ((16, 64), (128, 32)):
        for ncol in (15, 16, 17, BC - 1, BC, BC + 1, 2 * BC + 3):
            out.append(pytest.param(D, ncol, i, id=f"D{D}-ncol{ncol}"))
            i += 1
    return out


@pytest.mark.parametrize("D,ncol,i", column_cases())
def test_fast_kernel_output_columns(gpu, mvsv, D, ncol, i):
    bs = (5, 9, 7)[i % 3]
    p, window = cycled(i, D, bs)
    H = bs + 6
    W = width_for(ncol, p, H)
    L, R = cs.grey_pair(7000 + 31 * i + D, H, W, shift=3)
    want = cb.compute(L, R, p, window)
    got = run(gpu, mvsv, L, R, p, window)
    assert np.array_equal(got, want), f"{p} {window}: " + report(got, want)


@pytest.mark.parametrize("rows", (2, TY - 1, TY, TY + 1, 2 * TY + 3))
@pytest.mark.parametrize("D", (16, 128))
def test_fast_kernel_output_rows(gpu, mvsv, tile_rows, D, rows):
    i = rows + D
    bs = 9
    p, window = cycled(i, D, bs)
    H = rows + bs - 1
    L, R = cs.grey_pair(7500 + i, H, D + 50, shift=4)
    want = cb.compute(L, R, p, window)
    assert cb.geometry(p, D + 50, H)["ymax"] - cb.geometry(p, D + 50, H)["ymin"] == rows
    tile_rows(TY)
    got = run(gpu, mvsv, L, R, p, window)
    assert np.array_equal(got, want), f"{p} {window}: " + report(got, want)


def test_one_output_row_is_refused_by_the_inherited_rule(gpu, mvsv):
    m = mvsv.StereoBM.create(16, 9)
    img = np.zeros((9, 80), np.uint8)
    with pytest.raises(mvsv.MvsvError, match="SADWindowSize"):
        m.compute_census(img, img)


PARAM_CASES = [pytest.param(D, bs, 3 * a + b, id=f"D{D}-bs{bs}")
               for a, D in enumerate((16, 32, 64, 80, 128)) for b, bs in enumerate((5, 9, 21))]


@pytest.mark.parametrize("D,bs,i", PARAM_CASES)
def test_fast_kernel_disparities_blocks_and_windows(gpu, mvsv, D, bs, i):
    """D 80 has padded lanes, D 128 two waves per group; the windows cycle over one- and
    two-word descriptors; the tile height is the launch's own choice."""
    p, window = cycled(i, D, bs)
    H, W = bs + 13, D + 75
    L, R = cs.grey_pair(7700 + i, H, W, shift=5)
    want = cb.compute(L, R, p, window)
    got = run(gpu, mvsv, L, R, p, window)
    assert np.array_equal(got, want), f"{p} {window}: " + report(got, want)


def test_the_cycled_parameters_cover_every_value():
    seen = {k: set() for k in ("minD", "uniq", "d12", "speckle", "window")}
    cases = [(c.values[0], c.values[1], c.values[2]) for c in PARAM_CASES]
    cases += [(c.values[0], (5, 9, 7)[c.values[2] % 3], c.values[2]) for c in column_cases()]
    for D, bs, i in cases:
        p, w = cycled(i, D, bs)
        seen["minD"].add(p["min_disparity"])
        seen["uniq"].add(p["uniqueness_ratio"])
        seen["d12"].add(p["disp12_max_diff"])
        seen["speckle"].add((p["speckle_window_size"], p["speckle_range"]))
        seen["window"].add(w)
    assert seen == {"minD": set(MIN_D), "uniq": set(UNIQ), "d12": set(D12), "speckle": set(SPECKLE),
                    "window": set(WINDOWS)}
    # (window, words) pairs reach both block shapes of the fast kernel
    assert {(D > 64, w[0] * w[1] - 1 > 32) for D, bs, i in cases for w in [cycled(i, D, bs)[1]]} == \
        {(False, False), (False, True), (True, False), (True, True)}


# ---- the general form ---------------------------------------------------------------
@pytest.mark.parametrize("D,bs,i", [(16, 23, 4), (144, 9, 5), (512, 9, 6)], ids=["bs23-D16", "D144-bs9", "D512-scratch"])
def test_general_form(gpu, mvsv, D, bs, i):
    """blockSize > 21, D > 128, and D 512 whose window sums (512 x 256 x 2 bytes) leave LDS
    for the global scratch slab."""
    p, window = cycled(i, D, bs)
    H, W = bs + 19, D + 55
    L, R = cs.grey_pair(7900 + i, H, W, shift=6)
    want = cb.compute(L, R, p, window)
    got = run(gpu, mvsv, L, R, p, window)
    assert np.array_equal(got, want), f"{p} {window}: " + report(got, want)


def test_general_form_where_the_fast_kernel_applies(gpu, mvsv, monkeypatch):
    """MVSV_KERNELS=bm-tile (read by mvsv_create) switches the lanes kernels off: a fresh
    context runs the general form on a fast-range shape; both equal the restatement."""
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    for i, (D, bs) in enumerate(((64, 9), (128, 21), (16, 5))):
        p, window = cycled(i + 1, D, bs)
        H, W = bs + 18, D + 70
        L, R = cs.grey_pair(8100 + i, H, W, shift=4)
        want = cb.compute(L, R, p, window)
        fast = matcher(mvsv, p).compute_census(L, R, window=window)
        assert np.array_equal(fast, want), f"fast {p} {window}: " + report(fast, want)
        monkeypatch.setenv("MVSV_KERNELS", "bm-tile")
        h = ctypes.c_void_p()
        assert lib.mvsv_create(ctypes.byref(h), 0) == 0
        monkeypatch.delenv("MVSV_KERNELS")
        try:
            out = np.full((H, W), -999, np.int16)
            rc = lib.mvsv_bm_census(h, L.ctypes.data, W, R.ctypes.data, W, W, H, ctypes.byref(matcher(mvsv, p)._params),
                                    out.ctypes.data, W, window[0], window[1])
            assert rc == 0, lib.mvsv_last_error(h)
        finally:
            lib.mvsv_destroy(h)
        assert np.array_equal(out, want), f"general {p} {window}: " + report(out, want)


def test_a_shape_no_kernel_form_holds_is_refused(gpu, mvsv):
    """blockSize 101: the two descriptor tiles of a 16 x 16 block are (116 x 116 + 116 x 132)
    x 8 bytes > 160 KiB of LDS."""
    m = mvsv.StereoBM.create(16, 101)
    img = np.zeros((110, 140), np.uint8)
    with pytest.raises(mvsv.MvsvError, match="do not fit in LDS"):
        m.compute_census(img, img)
    assert m.census_validate(140, 110)  # the parameter rules alone accept it
    # and the context still works
    assert mvsv.StereoBM.create(16, 5).compute_census(img, img).shape == img.shape


# ---- degenerate shapes ----------------------------------------------------------------
@pytest.mark.parametrize("window", [(65, 1), (1, 65), (21, 3)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_window_larger_than_the_image(gpu, mvsv, window):
    p = cb.params(num_disparities=16, block_size=5, uniqueness_ratio=0, disp12_max_diff=1)
    L, R = cs.grey_pair(8300 + window[0], 8, 40, shift=2)
    want = cb.compute(L, R, p, window)
    got = run(gpu, mvsv, L, R, p, window)
    assert np.array_equal(got, want), report(got, want)


@pytest.mark.parametrize("minD", (0, -40))
def test_no_column_to_compute_gives_all_filtered(gpu, mvsv, minD):
    p = cb.params(min_disparity=minD, num_disparities=16, block_size=5)
    L, R = cs.grey_pair(8400, 12, 12, shift=1)
    assert cb.geometry(p, 12, 12) is None
    got = run(gpu, mvsv, L, R, p, (9, 7))
    assert (got == (minD - 1) * 16).all() and np.array_equal(got, cb.compute(L, R, p, (9, 7)))


# ---- entry points -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout_ref():
    p = cb.params(min_disparity=-2, num_disparities=32, block_size=7, uniqueness_ratio=10, disp12_max_diff=1,
                  speckle_window_size=20, speckle_range=2)
    pairs = [cs.grey_pair(600 + k, 23, 130, shift=3 + k) for k in range(3)]
    maps = [cb.compute(L, R, p, (9, 7)) for L, R in pairs]
    return p, pairs, maps


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
    got = mvsv.Disparity.binary_bm(pair, out[1:1 + H, 3:3 + W], m)
    assert np.array_equal(got, maps[1]), report(got, maps[1])
    assert np.shares_memory(got, out) and (out[0] == -999).all() and (out[:, :3] == -999).all()
    assert (out[-1] == -999).all() and (out[:, 3 + W:] == -999).all()
    # the default window is (9, 7); another one gives another map, and compute() the SAD map
    assert not np.array_equal(mvsv.Disparity.binary_bm(pair, None, m, (3, 3)), maps[1])
    assert np.array_equal(mvsv.Disparity.bm(pair, None, m), twin.bm_compute(L, R, p))


def strided(torch, frames, row_stride, frame_stride, offset, fill, dtype):
    n, H, W = frames.shape
    flat = torch.full((offset + n * frame_stride + 64,), fill, dtype=dtype, device="cuda")
    view = flat.as_strided((n, H, W), (frame_stride, row_stride, 1), offset)
    view.copy_(torch.from_numpy(frames).cuda())
    return flat, view


def test_device_batch_with_padded_strides_and_guard_words(gpu, mvsv, layout_ref):
    p, pairs, maps = layout_ref
    Ls = np.stack([a for a, _ in pairs])
    Rs = np.stack([b for _, b in pairs])
    n, H, W = Ls.shape
    fl, lv = strided(gpu, Ls, W + 5, H * (W + 5) + 11, 1, 0xA5, gpu.uint8)
    fr, rv = strided(gpu, Rs, W + 6, H * (W + 6) + 2, 3, 0x5A, gpu.uint8)
    before = (fl.clone(), fr.clone())
    GUARD = -12345
    fo, ov = strided(gpu, np.full((n, H, W), GUARD, np.int16), W + 3, H * (W + 3) + 7, 2, GUARD, gpu.int16)
    got = matcher(mvsv, p).compute_census(lv, rv, ov)
    assert got.data_ptr() == ov.data_ptr()
    got = got.cpu().numpy()
    for k in range(n):
        assert np.array_equal(got[k], maps[k]), f"frame {k}: " + report(got[k], maps[k])
    assert gpu.equal(fl, before[0]) and gpu.equal(fr, before[1])
    guard = gpu.ones_like(fo, dtype=gpu.bool)
    guard.as_strided((n, H, W), (H * (W + 3) + 7, W + 3, 1), 2).fill_(False)
    assert bool((fo[guard] == GUARD).all()), "guard words after a row or a frame were written"


def test_side_stream_and_sad_afterwards(gpu, mvsv, layout_ref):
    p, pairs, maps = layout_ref
    L, R = pairs[2]
    Lt, Rt = gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()
    gpu.cuda.synchronize()
    s = gpu.cuda.Stream()
    with gpu.cuda.stream(s):
        got = matcher(mvsv, p).compute_census(Lt, Rt)  # device_context: mvsv_set_stream(current stream)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), maps[2]), report(got.cpu().numpy(), maps[2])
    # the SAD entry on the same context afterwards is untouched by the census launch
    g = matcher(mvsv, p).compute(Lt, Rt).cpu().numpy()
    assert np.array_equal(g, twin.bm_compute(L, R, p))
    assert not np.array_equal(g, maps[2])


def test_fixture_maps(gpu, mvsv):
    z = np.load(os.path.join(GOLDEN, "census_bm_fixtures.npz"))
    for k in range(int(z["count"])):
        p = dict(zip(cb.PARAM_NAMES, (int(v) for v in z[f"params{k}"])))
        window = tuple(int(v) for v in z[f"window{k}"])
        got = matcher(mvsv, p).compute_census(z[f"L{k}"], z[f"R{k}"], window=window)
        assert np.array_equal(got, z[f"map{k}"]), f"fixture {k}: " + report(got, z[f"map{k}"])


@functools.lru_cache(maxsize=None)
def known_ref(seed, bs, window):
    L, R = cb.known_pair(seed, bs)
    return L, R, cb.compute(L, R, cb.known_params(bs), window)


@pytest.mark.parametrize("bs", cb.KNOWN_BLOCKS)
@pytest.mark.parametrize("window", cb.KNOWN_WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_known_answer_and_invariance_on_the_device(gpu, mvsv, window, bs):
    m = matcher(mvsv, cb.known_params(bs))
    for seed in cb.KNOWN_SEEDS:
        L, R, want = known_ref(seed, bs, window)
        L2, R2 = cs.radiometric(L, R)
        a = m.compute_census(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda(), window=window).cpu().numpy()
        b = m.compute_census(gpu.from_numpy(L2).cuda(), gpu.from_numpy(R2).cuda(), window=window).cpu().numpy()
        assert np.array_equal(a, b), f"seed {seed}: the map changes under v -> 2v / v -> v + 100: " + report(a, b)
        rows, cols = cb.known_region(*L.shape, bs, window)
        assert (((a[rows, cols].astype(np.int32) + 8) >> 4) == cb.KNOWN_SHIFT).all(), f"seed {seed}"
        assert np.array_equal(a, want), report(a, want)


def test_low_contrast_gain_on_the_device(gpu, mvsv):
    """The invariance pair: census keeps its map under L -> 4 L, R -> R + 100, the SAD
    matcher of the same build does not; texture and prefilter fields change nothing."""
    (L, R), (L2, R2) = cb.low_contrast_pair(1)
    p = cb.params(num_disparities=16, block_size=5, uniqueness_ratio=15, texture_threshold=0)
    m = matcher(mvsv, p)
    a, b = m.compute_census(L, R), m.compute_census(L2, R2)
    assert np.array_equal(a, b) and np.array_equal(a, cb.compute(L, R, p, (9, 7)))
    assert not np.array_equal(m.compute(L, R), m.compute(L2, R2))
    for kw in (dict(texture_threshold=100000), dict(pre_filter_cap=63), dict(pre_filter_type=0, pre_filter_size=51)):
        assert np.array_equal(matcher(mvsv, dict(p, **kw)).compute_census(L, R), a), kw


def test_bm_yml_through_binary_bm(gpu, mvsv):
    b = mvsv.StereoBM.create(0, 0)
    assert mvsv.Disparity.loadBMParameters(os.path.join(CONFIGS, "bm.yml"), b)
    p = b.params()
    assert p["num_disparities"] == 80 and p["block_size"] == 21
    L, R = cs.grey_pair(8600, 120, 160, shift=7)
    got = mvsv.Disparity.binary_bm(mvsv.Stereopair(L, R), None, b)
    want = cb.compute(L, R, {k: p[k] for k in cb.PARAM_NAMES}, (9, 7))
    assert np.array_equal(got, want), report(got, want)
    assert (want != (p["min_disparity"] - 1) * 16).any()


def test_error_paths_name_the_rule(gpu, mvsv):
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    ctx = _lib.context(0)
    H, W = 12, 40
    p = mvsv.StereoBM.create(16, 5)._params
    Lt = gpu.zeros((H, W), dtype=gpu.uint8, device="cuda")
    out = gpu.zeros((H, W), dtype=gpu.int16, device="cuda")
    a, o = Lt.data_ptr(), out.data_ptr()
    dev = lib.mvsv_bm_census_device

    def call(*, n=1, l=a, ls=W, r=a, rs=W, par=p, dst=o, os_=W, cw=9, ch=7, h=ctx.handle):
        return dev(h, n, l, ls, W * H, r, rs, W * H, W, H, ctypes.byref(par) if par is not None else None, dst, os_,
                   W * H, cw, ch)

    def message():
        return lib.mvsv_last_error(ctx.handle).decode()

    def bm(**kw):
        m = mvsv.StereoBM.create(16, 5)
        for k, v in kw.items():
            setattr(m._params, k, v)
        return m._params

    assert call() == 0
    for cw, ch in ((8, 7), (9, 9), (1, 1), (0, 0), (-1, 3)):
        assert call(cw=cw, ch=ch) == INVALID_ARG and "census window" in message(), (cw, ch)
    assert call(par=bm(num_disparities=24)) == INVALID_ARG and "numDisparities" in message()
    assert call(par=bm(block_size=4)) == INVALID_ARG and "SADWindowSize" in message()
    assert call(par=bm(block_size=13)) == INVALID_ARG and "SADWindowSize" in message()  # not smaller than H
    assert call(par=bm(pre_filter_cap=64)) == INVALID_ARG and "preFilterCap" in message()
    assert call(par=bm(pre_filter_size=4)) == INVALID_ARG and "preFilterSize" in message()
    assert call(par=bm(pre_filter_type=7)) == INVALID_ARG and "preFilterType" in message()
    assert call(par=bm(texture_threshold=-1)) == INVALID_ARG and "texture threshold" in message()
    assert call(par=bm(uniqueness_ratio=-1)) == INVALID_ARG and "uniqueness ratio" in message()
    assert call(ls=W - 1) == INVALID_ARG and "stride" in message()
    assert call(os_=W - 1) == INVALID_ARG and "stride" in message()
    assert call(l=None) == INVALID_ARG and call(dst=None) == INVALID_ARG and call(n=0) == INVALID_ARG
    assert call(par=None) == INVALID_ARG and call(h=None) == INVALID_ARG
    gpu.cuda.synchronize()
    Lh = np.zeros((H, W), np.uint8)
    oh = np.zeros((H, W), np.int16)
    host = lib.mvsv_bm_census
    assert host(ctx.handle, Lh.ctypes.data, W, Lh.ctypes.data, W, W, H, ctypes.byref(p), oh.ctypes.data, W, 9, 7) == 0
    assert host(ctx.handle, Lh.ctypes.data, W, Lh.ctypes.data, W, W, H, ctypes.byref(p), oh.ctypes.data, W, 6, 7) == INVALID_ARG
    assert "census window" in message()
    assert host(ctx.handle, Lh.ctypes.data, W - 1, Lh.ctypes.data, W, W, H, ctypes.byref(p), oh.ctypes.data, W, 9, 7) == INVALID_ARG
    # the wrapper: mixed host / device, mismatched shapes, colour
    m = mvsv.StereoBM.create(16, 5)
    with pytest.raises(mvsv.MvsvError):
        m.compute_census(Lt, Lh)
    with pytest.raises(mvsv.MvsvError):
        m.compute_census(Lt, gpu.zeros((H, W + 1), dtype=gpu.uint8, device="cuda"))
    with pytest.raises(mvsv.MvsvError):
        m.compute_census(gpu.zeros((H, W, 3), dtype=gpu.uint8, device="cuda"), gpu.zeros((H, W, 3), dtype=gpu.uint8, device="cuda"))
    with pytest.raises(mvsv.MvsvError, match="census window"):
        m.compute_census(Lt, Lt, window=(2, 2))
    # and the context still works
    assert m.compute_census(Lt, Lt).shape == (H, W)
