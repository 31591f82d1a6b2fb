"""Display maps, CPU side: the numpy restatement of OpenCV 3.4's
cv::normalize(NORM_MINMAX, CV_8U) (tests/display_restate.py) pins the arithmetic
the kernels are compared with bit for bit in tests/test_gpu_display.py, the
library declares and exports the new entry points, and the new kernels carry no
scratch."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import display_restate as ref
from tests.test_kernel_scratch import LIB, LLVM, kernel_scratch

# value ranges with SGBM's invalid marker (minDisparity - 1) * 16 = -16 as the minimum
LADDERS = [(-16, 74), (-16, 164), (-16, 222)]

NEW_SYMBOLS = ["mvsv_minmax_device", "mvsv_normalize_minmax_device", "mvsv_normalize_minmax",
               "mvsv_stream_enable_display", "mvsv_stream_disable_display", "mvsv_stream_front_display",
               "mvsv_stream_front_display_view"]


def test_library_exports_the_display_entry_points():
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    import mvstereovision3_amd as mvsv
    assert callable(mvsv.normalize_minmax) and callable(mvsv.minmax)
    for m in ("enable_display", "disable_display", "front_display"):
        assert callable(getattr(mvsv.DisparityStream, m))
    # no device needed: a null handle is refused before anything else
    assert lib.mvsv_normalize_minmax(None, None, 0, 0, 0, 0.0, 255.0, None, 0, None) == _lib.MVSV_E_INVALID_ARG
    assert lib.mvsv_stream_enable_display(None, None, 0.0, 255.0) == _lib.MVSV_E_INVALID_ARG
    assert lib.mvsv_stream_front_display(None, None, 0, None) == _lib.MVSV_E_INVALID_ARG


@pytest.mark.parametrize("lo,hi", LADDERS)
def test_ladders_tell_the_pinned_arithmetic_from_its_near_misses(mvsv, lo, hi):
    """A kernel that evaluates the pixel in double, or fuses the product into the
    sum, differs from the restatement on every one of these ladders."""
    assert callable(mvsv.normalize_minmax)
    d = ref.ladder(lo, hi)
    want, mm = ref.normalize(d)
    assert mm == (lo, hi) and want[0, 0] == 0 and want[0, -1] == 255
    n64 = int((want != ref.normalize_f64(d)).sum())
    nfma = int((want != ref.normalize_fused(d)).sum())
    print(f"ladder ({lo}, {hi}): {n64} pixels differ from float64, {nfma} from a fused multiply-add")
    assert n64 >= 1 and nfma >= 1
    # the same ladder laid out as the GPU test's 100 x 70 frame keeps every value
    tiled = ref.ladder(lo, hi, (70, 100))
    assert ref.minmax(tiled) == (lo, hi)
    assert (ref.normalize(tiled)[0] != ref.normalize_f64(tiled)).any()
    assert (ref.normalize(tiled)[0] != ref.normalize_fused(tiled)).any()


def test_half_to_even(mvsv):
    assert callable(mvsv.normalize_minmax)
    scale, shift = ref.scale_shift(0, 510)
    assert scale == 0.5 and shift == 0.0
    out, _ = ref.normalize(ref.ladder(0, 510))
    assert out[0, :8].tolist() == [0, 0, 1, 2, 2, 2, 3, 4]  # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    assert out[0, 509] == 254 and out[0, 510] == 255


def test_fixed_cases(mvsv):
    assert callable(mvsv.normalize_minmax)
    d = np.array([[0, 1, 1, 0]], np.int16)
    assert ref.normalize(d)[0].tolist() == [[0, 255, 255, 0]]
    const = np.full((3, 5), -16, np.int16)
    assert ref.scale_shift(-16, -16) == (0.0, 0.0)
    assert (ref.normalize(const)[0] == 0).all()
    assert (ref.normalize(const, 32, 224)[0] == 32).all()
    assert (ref.normalize(const, 300, 400)[0] == 255).all()  # saturate(dmin)
    lad = ref.ladder(-16, 222)
    a, _ = ref.normalize(lad, 0, 255)
    b, _ = ref.normalize(lad, 255, 0)
    assert np.array_equal(a, b)  # dmin / dmax are ordered, the map is not inverted
    c, _ = ref.normalize(lad, 32, 224)
    assert c[0, 0] == 32 and c[0, -1] == 224 and (np.diff(c[0].astype(int)) >= 0).all()
    assert ref.minmax(np.array([[0, -5, 7, 3]], np.int16), positive_only=True) == (3, 7)
    assert ref.minmax(np.array([[0, -5]], np.int16), positive_only=True) == (32767, -32768)


def test_header_lists_the_reference_counterparts():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mvsv.h")).read()
    table = text[:text.index("#ifndef")] if "#ifndef" in text else text
    for name in ("mvsv_normalize_minmax", "mvsv_minmax_device", "mvsv_stream_enable_display"):
        assert name in table, f"{name} missing from the header's table of reference counterparts"


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"),
                    reason="library not built / no ROCm llvm tools")
def test_display_kernels_have_no_scratch():
    ks = kernel_scratch()
    for pat in (r"minmax_kernelILb0", r"minmax_kernelILb1", r"minmax_final_kernel", r"normalize_u8_kernel"):
        picked = {k: v for k, v in ks.items() if re.search(pat, k)}
        assert picked, f"no kernel matches {pat}"
        assert not any(picked.values()), f"kernels with scratch: {picked}"
