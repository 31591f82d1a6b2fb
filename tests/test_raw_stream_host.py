"""Host side of the raw frame stream (no GPU): mvsv_convert_maps against a numpy
restatement of cv::convertMaps(CV_16SC2, CV_16UC1) -- the arithmetic of the first
lines of the remap kernel -- and the declarations of the new entry points in
include/mvsv.h and _lib.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

RAW_W, RAW_H = 203, 125
NEW_FUNCTIONS = ("mvsv_convert_maps", "mvsv_stream_create_raw", "mvsv_stream_size", "mvsv_stream_push_raw",
                 "mvsv_stream_pop_pair")


def stream_maps():
    """The maps of tests/test_gpu_raw_stream.py: quantised to 1/64 px, so that about
    half of the x entries are exact ties of the rounding to 1/32 px."""
    y, x = np.mgrid[0:RAW_H, 0:RAW_W].astype(np.float64)

    def q(m):
        return (np.round(m * 64) / 64).astype(np.float32)
    lx = q(x + 1.25 + 0.01 * (y - 60))
    ly = q(y + 2 * np.sin(x / 23) - 1)
    rx = q(x + 4.75 + 0.01 * (y - 60))
    return lx, ly, rx, ly.copy()


def restated(mx, my):
    """X = cvRound(mx * 32) in float arithmetic, half to even (np.rint)."""
    X = np.rint(np.asarray(mx, np.float32) * np.float32(32)).astype(np.int64)
    Y = np.rint(np.asarray(my, np.float32) * np.float32(32)).astype(np.int64)
    xy = np.stack([np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    frac = ((Y & 31) * 32 + (X & 31)).astype(np.uint16)
    return xy, frac


def check_maps(mvsv, mx, my):
    xy, frac = mvsv.convert_maps(mx, my)
    wxy, wfrac = restated(mx, my)
    assert xy.dtype == np.int16 and frac.dtype == np.uint16
    bad = np.argwhere(xy != wxy)
    assert bad.size == 0, f"xy: {len(bad)} mismatches, first {bad[:5].tolist()}"
    bad = np.argwhere(frac != wfrac)
    assert bad.size == 0, f"frac: {len(bad)} mismatches, first {bad[:5].tolist()}"
    return xy, frac


def test_convert_maps_stream_maps(mvsv):
    lx, ly, rx, ry = stream_maps()
    v = lx.astype(np.float64) * 32
    assert (np.abs(v - np.floor(v) - 0.5) < 1e-9).mean() > 0.4  # the ties are there
    xy, _ = check_maps(mvsv, lx, ly)
    assert xy[..., 1].min() < 0  # rows above the frame
    check_maps(mvsv, rx, ry)


def test_convert_maps_negative_ties_saturation(mvsv):
    k = np.arange(-200, 200, dtype=np.float64)
    rows = [
        k / 32 + 1 / 64,          # exact ties, both sides of even and odd, negative and positive
        k / 32 - 1 / 64,
        k / 32,                   # exact 1/32 steps: >> 5 and & 31 of negatives
        k / 32 + 1 / 128,
        k * 0.37 - 40.2,          # general fractions
        np.where(k < 0, -1, 1) * (1000 + 8 * np.abs(k)) + 0.515625,  # up to +-2600
        np.where(k < 0, -1, 1) * (32000 + 10 * np.abs(k)) + 0.25,    # across the short's range
        np.where(k < 0, -1, 1) * (60000.0 + 1000 * np.abs(k)),       # far beyond it
    ]
    mx = np.array(rows, np.float32)
    my = np.ascontiguousarray(mx[::-1])
    xy, frac = check_maps(mvsv, mx, my)
    assert xy.min() == -32768 and xy.max() == 32767
    # what the expectations above rely on, spelled out
    one = np.array([[0.515625, 1.515625, -0.515625, -1.515625, -0.5, -1.0 / 32]], np.float32)  # .5 ties of *32
    xy1, frac1 = mvsv.convert_maps(one, np.zeros_like(one))
    # X = 16 (16.5 -> even), 48 (48.5 -> even), -16, -48, -16, -1
    assert xy1[0, :, 0].tolist() == [0, 1, -1, -2, -1, -1]
    assert frac1[0].tolist() == [16, 16, 16, 16, 16, 31]


def test_convert_maps_strides(mvsv):
    from mvstereovision3_amd import _lib
    lx, ly, _, _ = stream_maps()
    # the Python mirror on views with a row stride (a ROI of the maps)
    check_maps(mvsv, lx[5:113, 6:187], ly[5:113, 6:187])
    # the C entry point with padded output rows: the padding stays untouched
    h, w = 7, 13
    mx = np.ascontiguousarray(lx[:h, :w + 4])
    my = np.ascontiguousarray(ly[:h, :w + 4])
    xy = np.full((h, w + 3, 2), 77, np.int16)
    frac = np.full((h, w + 5), 99, np.uint16)
    rc = _lib.lib().mvsv_convert_maps(mx.ctypes.data, my.ctypes.data, w + 4, w, h, xy.ctypes.data, w + 3,
                                      frac.ctypes.data, w + 5)
    assert rc == 0
    wxy, wfrac = restated(mx[:, :w], my[:, :w])
    assert np.array_equal(xy[:, :w], wxy) and np.array_equal(frac[:, :w], wfrac)
    assert (xy[:, w:] == 77).all() and (frac[:, w:] == 99).all()


@pytest.mark.parametrize("bad", ["null", "stride", "size"])
def test_convert_maps_rejects(mvsv, bad):
    from mvstereovision3_amd import _lib
    m = np.zeros((4, 8), np.float32)
    xy = np.zeros((4, 8, 2), np.int16)
    fr = np.zeros((4, 8), np.uint16)
    args = [m.ctypes.data, m.ctypes.data, 8, 8, 4, xy.ctypes.data, 8, fr.ctypes.data, 8]
    if bad == "null":
        args[1] = None
    elif bad == "stride":
        args[2] = 7
    else:
        args[3] = 0
    assert _lib.lib().mvsv_convert_maps(*args) == _lib.MVSV_E_INVALID_ARG


def test_convert_maps_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/cpp/convert_maps_check.cpp) with the HIP-free
    translation unit, built with AddressSanitizer + UBSan: exact-size buffers."""
    exe = tmp_path / "convert_maps_check"
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "convert_maps_check.cpp"),
                    os.path.join(ROOT, "mvstereovision3_amd", "csrc", "mvsv_io.cpp"), "-o", str(exe), "-lm"],
                   check=True)
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout


def test_header_and_binding_declare_the_raw_stream(mvsv):
    from mvstereovision3_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvsv.h")).read()
    declared = set(re.findall(r"MVSV_API\s+[\w\s\*]+?\b(mvsv_\w+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW_FUNCTIONS:
        assert name in declared, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    body = re.search(r"typedef struct \{([^}]*)\}\s*mvsv_rectification;", hdr)
    assert body, "mvsv_rectification is not declared"
    for field in ("raw_width", "raw_height", "maps[4]", "map_stride", "roi", "factor", "keep_rectified"):
        assert field in body.group(1), field
    r = _lib.Rectification()
    assert [f[0] for f in r._fields_] == ["raw_width", "raw_height", "maps", "map_stride", "roi", "factor",
                                          "keep_rectified"]
    assert hasattr(mvsv.DisparityStream, "raw") and hasattr(mvsv.DisparityStream, "push_raw")
