"""Detection view, CPU side: the numpy restatement (tests/view_restate.py) pins
the drawing rules the kernel is compared with bit for bit in
tests/test_gpu_view.py; its near misses differ from it on every input the GPU
tests use, so those tests can tell them apart; the library declares and binds
the new entry points, refuses every invalid argument without a device, and its
host painter (View.drawSubimageGrid / drawObstacleGrid) agrees with the
restatement."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import view_restate as ref
from tests.test_kernel_scratch import LIB, LLVM, kernel_scratch

NEW_SYMBOLS = ["mvsv_view_device", "mvsv_view", "mvsv_view_draw", "mvsv_stream_enable_view",
               "mvsv_stream_disable_view", "mvsv_stream_front_view", "mvsv_stream_front_view_view"]


def test_circle_tables():
    """Circle()'s filled spans, as worked by hand in DESIGN 4k."""
    assert [ref.half_widths(r) for r in range(4)] == [[0], [1, 0], [2, 1, 0], [3, 2, 2, 0]]


@pytest.mark.parametrize("W,H", ref.SHAPES, ids=lambda v: str(v))
def test_near_misses_differ_on_every_gpu_input(W, H):
    for seed in (0, 1):
        d, kw = ref.all_layers_case(W, H, seed)
        want, mm = ref.view(d, **kw)
        assert want.shape == (H, W, 3) and mm == (int(d.min()), int(d.max()))
        for miss in ref.MISSES:
            n = int((ref.view(d, miss=miss, **kw)[0] != want).any(axis=2).sum())
            print(f"{W}x{H} seed {seed}: {miss} differs in {n} pixels")
            assert n >= 1, miss
        # both found layers are (0, 0, 255): their order cannot show
        for miss in ref.INVISIBLE_MISSES:
            assert np.array_equal(ref.view(d, miss=miss, **kw)[0], want)


def test_fixed_pixels():
    """100 x 70: dx = 11, dy = 7; lattice steps 8, nx = 11, ny = 7."""
    W, H = 100, 70
    d, kw = ref.all_layers_case(W, H)
    img, _ = ref.view(d, **kw)
    assert ref.layout(W, H) == (8, 8, 11, 7)
    grey = ref.view(d, 0)[0]
    assert (grey[..., 0] == grey[..., 1]).all() and (grey[..., 1] == grey[..., 2]).all()
    assert tuple(img[0, 0]) == ref.RED                   # tile 0 is found
    assert tuple(img[7, 11]) == ref.RED                  # its inclusive br corner
    assert tuple(img[3, 12]) == tuple(grey[3, 12])       # tile 1 is not found
    assert tuple(img[3, 22]) == ref.RED                  # column 2 * dx: the left edge of found tile 2
    assert tuple(img[66, 22]) == ref.BLUE                # the same column below the last tile row (9 * dy = 63)
    assert tuple(img[63, 99]) == ref.RED and tuple(img[64, 99]) == tuple(grey[64, 99])  # tile 80's br = (99, 63)
    assert tuple(img[69, 33]) == ref.RED                 # obstacle grid column 33 in the last row
    only = ref.view(d, ref.FOUND_POINTS, values=kw["values"], sample_range=ref.SAMPLE_RANGE)[0]
    assert tuple(only[8, 8]) == ref.RED and tuple(only[8, 11]) == ref.RED and tuple(only[8, 12]) == tuple(grey[8, 12])
    assert tuple(only[11, 8]) == ref.RED and tuple(only[11, 9]) == tuple(grey[11, 9])  # half-width 0 at offset 3
    assert tuple(only[10, 10]) == ref.RED and tuple(only[10, 11]) == tuple(grey[10, 11])
    # ranges that are inf / NaN find nothing
    for rng in [(math.nan, 0.0), (0.0, math.nan), (math.inf, math.inf), (-math.inf, -math.inf), (-math.inf, math.inf)]:
        got = ref.view(d, ref.FOUND_TILES | ref.FOUND_POINTS, kw["means"], rng, kw["values"], rng)[0]
        assert np.array_equal(got, grey), rng


def spec_of(_lib, layers=0, alpha=0.0, beta=255.0, means=None, values=None, radius=3):
    s = _lib.ViewSpec()
    s.layers, s.alpha, s.beta, s.point_radius = layers, alpha, beta, radius
    s.means = means
    s.values = values
    return s


def test_library_declares_and_binds_the_view(mvsv):
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    assert callable(mvsv.detection_view)
    assert (mvsv.VIEW_SUBIMAGE_GRID, mvsv.VIEW_OBSTACLE_GRID, mvsv.VIEW_FOUND_TILES, mvsv.VIEW_FOUND_POINTS) == (1, 2, 4, 8)
    for m in ("enable_view", "disable_view", "front_view"):
        assert callable(getattr(mvsv.DisparityStream, m))
    for m in ("drawObstacleGrid", "drawSubimageGrid"):
        assert callable(getattr(mvsv.View, m))
    E = _lib.MVSV_E_INVALID_ARG
    s = spec_of(_lib)
    assert lib.mvsv_view(None, None, 0, 0, 0, ctypes.byref(s), None, 0, None) == E
    assert lib.mvsv_view_device(None, 1, None, 0, 0, 0, 0, ctypes.byref(s), None, 0, 0, None) == E
    assert lib.mvsv_stream_enable_view(None, None, ctypes.byref(s)) == E
    assert lib.mvsv_stream_disable_view(None) == E
    assert lib.mvsv_stream_front_view(None, None, 0, None) == E
    assert lib.mvsv_stream_front_view_view(None, None, None) == E
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mvsv.h")).read()
    table = text[:text.index("#ifndef")]
    for name in ("mvsv_view", "mvsv_stream_enable_view"):
        assert name in table, f"{name} missing from the header's table of reference counterparts"


def test_invalid_arguments_are_refused_without_a_device(mvsv):
    """The one-shot calls share one argument check; mvsv_view_draw runs it (and
    nothing else) without a context."""
    from mvstereovision3_amd import _lib
    lib, E = _lib.lib(), _lib.MVSV_E_INVALID_ARG
    W, H = 30, 20
    img = np.zeros((H, W, 3), np.uint8)
    f = np.zeros(81, np.float32)
    p, fp = img.ctypes.data, f.ctypes.data

    def draw(spec, w=W, h=H, stride=3 * W, ptr=p):
        return lib.mvsv_view_draw(ptr, stride, w, h, ctypes.byref(spec) if spec is not None else None)

    assert draw(spec_of(_lib, 15, means=fp, values=fp)) == 0
    assert draw(spec_of(_lib, 3)) == 0
    assert draw(None) == E
    assert draw(spec_of(_lib, 16)) == E and draw(spec_of(_lib, -1)) == E      # unknown layer bits
    assert draw(spec_of(_lib, 4)) == E and draw(spec_of(_lib, 4, values=fp)) == E   # FOUND_TILES without means
    assert draw(spec_of(_lib, 8)) == E and draw(spec_of(_lib, 8, means=fp)) == E    # FOUND_POINTS without values
    for bad in (math.nan, math.inf, -math.inf):
        assert draw(spec_of(_lib, 1, alpha=bad)) == E and draw(spec_of(_lib, 1, beta=bad)) == E
    assert draw(spec_of(_lib, 1), stride=3 * W - 1) == E                        # out_stride < 3 * width
    roomy = np.zeros(H * (3 * W + 1), np.uint8)
    assert draw(spec_of(_lib, 1), stride=3 * W + 1, ptr=roomy.ctypes.data) == 0
    for r in (-1, 4):
        assert draw(spec_of(_lib, 8, values=fp, radius=r)) == E and draw(spec_of(_lib, 0, radius=r)) == E
    for r in range(4):
        assert draw(spec_of(_lib, 8, values=fp, radius=r)) == 0
    assert draw(spec_of(_lib, 1), w=8) == E and draw(spec_of(_lib, 1), h=8) == E   # the view needs 9 x 9
    assert draw(spec_of(_lib, 1), ptr=None) == E
    # Python: what cannot be an image or a map
    with pytest.raises(mvsv.MvsvError):
        mvsv.View.drawSubimageGrid(np.zeros((8, 30, 3), np.uint8))
    with pytest.raises(mvsv.MvsvError):
        mvsv.View.drawSubimageGrid(np.zeros((20, 30), np.uint8))
    with pytest.raises(mvsv.MvsvError):
        mvsv.detection_view(np.zeros((20, 30), np.float32), 0)


@pytest.mark.parametrize("W,H", ref.SHAPES[:5] + [(9, 9), (640, 480)], ids=lambda v: str(v))
def test_view_class_draws_the_grids_on_a_host_image(mvsv, W, H):
    rng = np.random.default_rng(W * 31 + H)
    base = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    for fn, layer in ((mvsv.View.drawSubimageGrid, ref.SUBIMAGE_GRID), (mvsv.View.drawObstacleGrid, ref.OBSTACLE_GRID)):
        got = base.copy()
        fn(got)
        want = ref.paint(base.copy(), layer)
        assert np.array_equal(got, want), fn.__name__
        assert (got != base).any()
    # both, in demo.cpp's order, into a view of a wider image: nothing outside is touched
    wide = np.full((H + 2, W + 5, 3), 0xA5, np.uint8)
    img = wide[1:1 + H, 2:2 + W]
    img[:] = base
    mvsv.View.drawSubimageGrid(img, 0)
    mvsv.View.drawObstacleGrid(img, 0)
    assert np.array_equal(img, ref.paint(base.copy(), ref.SUBIMAGE_GRID | ref.OBSTACLE_GRID))
    keep = np.ones(wide.shape, bool)
    keep[1:1 + H, 2:2 + W] = False
    assert (wide[keep] == 0xA5).all()


def test_host_painter_draws_the_found_layers_like_the_restatement(mvsv):
    from mvstereovision3_amd import _lib
    for W, H in ref.SHAPES[:5]:
        d, kw = ref.all_layers_case(W, H)
        base = np.repeat(ref.view(d, 0)[0][:, :, :1], 3, axis=2).copy()
        got = base.copy()
        vals = kw["values"] if kw["values"].size else np.zeros(1, np.float32)
        s = spec_of(_lib, 15, means=kw["means"].ctypes.data, values=vals.ctypes.data)
        s.tile_first, s.tile_second = ref.MEAN_RANGE
        s.point_first, s.point_second = ref.SAMPLE_RANGE
        assert _lib.lib().mvsv_view_draw(got.ctypes.data, 3 * W, W, H, ctypes.byref(s)) == 0
        assert np.array_equal(got, ref.view(d, **kw)[0]), (W, H)


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"),
                    reason="library not built / no ROCm llvm tools")
def test_view_kernel_has_no_scratch():
    picked = {k: v for k, v in kernel_scratch().items() if re.search(r"view_kernel", k)}
    assert picked, "no view kernel in the library"
    assert not any(picked.values()), f"kernels with scratch: {picked}"
