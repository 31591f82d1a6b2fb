"""Colour frames into a stream of rectified pairs (mvsv_stream_enable_bgr,
mvsv_stream_push_bgr): a BGR pair is uploaded once, halved and converted to grey
on the device ahead of the matcher.  BGR and grey frames alternate inside one
frame-batch launch, under SGBM and under StereoBM; every map equals the matcher on
the restatement's (and on prepare_gray's) grey pair.  Sources: 192 x 128 (whole
2 x 2 blocks, packed loads) and 203 x 135 (clipped last column and row, staged
rows padded to 4 bytes)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import prepare_restate as ref

pytestmark = pytest.mark.gpu

SOURCES = [(192, 128), (203, 135)]  # (width, height) of the colour frames


@functools.lru_cache(maxsize=None)
def bgr_pair(src, seed):
    """A synthetic stereo pair with a little colour: each channel is the grey image
    plus its own {-3 .. 3} noise."""
    import mvstereovision3_amd as mvsv
    w, h = src
    rng = np.random.default_rng(seed)
    out = []
    for g in mvsv.synth_pair(0xC0100 + seed, w, h, 0, 64):
        c = np.clip(g[..., None].astype(np.int64) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
        c.setflags(write=False)
        out.append(c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gray_pair(src, seed, halve=True, variant=ref.Q14):
    out = tuple(ref.prepare(c, halve, variant) for c in bgr_pair(src, seed))
    for g in out:
        g.setflags(write=False)
    return out


def matchers(mvsv):
    sg = mvsv.StereoSGBM.create(0, 32, 5, 200, 800, 1, 31, 10, 50, 2, mvsv.MODE_SGBM)
    return {"sgbm": sg, "bm": mvsv.StereoBM.create(32, 9)}


def oracle_map(oracle, mvsv, kind, L, R):
    m = matchers(mvsv)[kind]
    if kind == "bm":
        return oracle.bm(L, R, m.params())
    return oracle.sgbm(L, R, {k: v for k, v in m.params().items() if k != "variant"})


def assert_map(got, w, what):
    bad = np.argwhere(got != w)
    assert got.shape == w.shape and bad.size == 0, f"{what}: {len(bad)} mismatches, first {bad[:5].tolist()}"


@pytest.mark.parametrize("kind", ["sgbm", "bm"])
@pytest.mark.parametrize("src", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bgr_and_grey_frames_alternate(gpu, mvsv, oracle, src, kind):
    W, H = mvsv.prepare_size(*src)
    assert (W, H) == ref.prepare_size(src[0], src[1], True)
    m = matchers(mvsv)[kind]
    st = mvsv.DisparityStream(m, W, H, depth=4, batch=3)
    st.enable_bgr((src[1], src[0]))
    st.enable_sharpness()
    # B B g | B (ring end) ; g B ...: colour and grey slots inside one launch
    order = ["bgr", "bgr", "grey", "bgr", "grey", "bgr"]
    got = []

    def pop():
        sharp = st.front_sharpness(return_sums=True)
        got.append((st.pop()[0], sharp))

    for seed, how in enumerate(order):
        if st.pending() == 4:
            pop()
        if how == "bgr":
            st.push_bgr(*bgr_pair(src, seed))
        else:
            st.push(*gray_pair(src, seed))
    while st.pending():
        pop()
    for seed, (d, (values, sums)) in enumerate(got):
        L, R = gray_pair(src, seed)
        assert_map(d, oracle_map(oracle, mvsv, kind, L, R), f"frame {seed} ({order[seed]}) vs the oracle on the restated pair")
        # the sharpness product of a colour frame is that of its prepared grey pair
        ws = [mvsv.sharpness(g, return_sums=True) for g in (L, R)]
        assert sums == (ws[0][1], ws[1][1]) and values == (ws[0][0], ws[1][0]), f"frame {seed}: sharpness"
    # the one-shot path: prepare_gray, then the matcher
    pl, pr = (mvsv.prepare_gray(c) for c in bgr_pair(src, 0))
    assert np.array_equal(pl, gray_pair(src, 0)[0]) and np.array_equal(pr, gray_pair(src, 0)[1])
    assert_map(got[0][0], m.compute(pl, pr), "frame 0 vs prepare_gray + the one-shot matcher")
    assert not np.array_equal(got[0][0], got[1][0])
    # the other variant, the conversion alone, and switching both back
    st.enable_bgr((src[1], src[0]), halve=True, variant=mvsv.GRAY_Q15)
    st.push_bgr(*bgr_pair(src, 1))
    assert_map(st.pop()[0], oracle_map(oracle, mvsv, kind, *gray_pair(src, 1, True, ref.Q15)), "Q15")
    st.disable_bgr()
    with pytest.raises(mvsv.MvsvError):
        st.push_bgr(*bgr_pair(src, 1))
    st.push(*gray_pair(src, 1))
    assert_map(st.pop()[0], got[1][0], "grey frame after disable_bgr")
    st.close()


def test_conversion_alone_and_views(gpu, mvsv, oracle):
    """halve = False: the colour frame has the stream's size; pushed as a ROI view of
    a larger image (rows further apart than 3 * width, entered 3 bytes in)."""
    src = (101, 67)
    st = mvsv.DisparityStream(matchers(mvsv)["bm"], *src, depth=2)
    st.enable_bgr((src[1], src[0]), halve=False)
    cl, cr = bgr_pair(src, 3)
    parent = np.full((2, src[1] + 2, src[0] + 6, 3), 7, np.uint8)
    parent[0, 1:-1, 1:-5], parent[1, 1:-1, 1:-5] = cl, cr
    st.push_bgr(parent[0, 1:-1, 1:-5], parent[1, 1:-1, 1:-5])
    L, R = gray_pair(src, 3, False)
    assert_map(st.pop()[0], oracle_map(oracle, mvsv, "bm", L, R), "conversion alone, ROI views")
    st.close()


def test_misuse(gpu, mvsv):
    from mvstereovision3_amd import _lib
    from tests.test_gpu_raw_stream import MAPS, ROI, matcher
    lib, E = _lib.lib(), _lib.MVSV_E_INVALID_ARG
    src = SOURCES[0]
    cl, cr = bgr_pair(src, 0)
    L, R = gray_pair(src, 0)
    m = matchers(mvsv)["sgbm"]
    st = mvsv.DisparityStream(m, 96, 64)
    push = lambda s, ls=3 * src[0]: lib.mvsv_stream_push_bgr(s._h, cl.ctypes.data, ls, cr.ctypes.data, 3 * src[0])
    assert push(st) == E and st.pending() == 0                       # without enable_bgr
    with pytest.raises(mvsv.MvsvError):
        st.push_bgr(cl, cr)
    assert lib.mvsv_stream_enable_bgr(st._h, 190, 128, 1, 0) == E    # halves to 95 x 64, not the stream's size
    assert lib.mvsv_stream_enable_bgr(st._h, 96, 64, 1, 0) == E
    assert lib.mvsv_stream_enable_bgr(st._h, 192, 128, 0, 0) == E    # the conversion alone keeps 192 x 128
    assert lib.mvsv_stream_enable_bgr(st._h, 192, 128, 2, 0) == E    # another factor
    assert lib.mvsv_stream_enable_bgr(st._h, 192, 128, 1, 7) == E    # unknown variant
    assert push(st) == E
    st.push(L, R)
    assert lib.mvsv_stream_enable_bgr(st._h, 192, 128, 1, 0) == E    # a frame is pending
    want = st.pop()[0]
    st.enable_bgr((128, 192))
    assert push(st, 3 * src[0] - 1) == E and st.pending() == 0       # stride < 3 * width
    assert lib.mvsv_stream_push_bgr(st._h, None, 576, cr.ctypes.data, 576) == E
    with pytest.raises(mvsv.MvsvError):
        st.push_bgr(cl[:, :-1], cr[:, :-1])                          # not enable_bgr's shape
    st.push_bgr(cl, cr)
    assert lib.mvsv_stream_disable_bgr(st._h) == E                   # a frame is pending
    for _ in range(2):
        st.push_bgr(cl, cr)
    assert push(st) == E and st.pending() == 3                       # full
    for _ in range(3):
        assert_map(st.pop()[0], want, "after the refused calls")
    st.close()
    # raw streams take no colour
    raw = mvsv.DisparityStream.raw(matcher(mvsv), MAPS, roi=ROI)
    assert lib.mvsv_stream_enable_bgr(raw._h, 2 * raw.width, 2 * raw.height, 1, 0) == E
    assert lib.mvsv_stream_push_bgr(raw._h, cl.ctypes.data, 576, cr.ctypes.data, 576) == E
    with pytest.raises(mvsv.MvsvError):
        raw.enable_bgr((2 * raw.height, 2 * raw.width))
    raw.close()
