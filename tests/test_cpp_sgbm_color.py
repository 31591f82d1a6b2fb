"""The C++ mirror of Disparity::sgbm on a CV_8UC3 Stereopair (include/mvsv_disparity.hpp)
compiled with g++ against the C ABI: disparityTest's loop (trgt/disparityTest.cpp:201-232)
without its two cvtColor lines."""
import os
import subprocess

import numpy as np
import pytest

from tests import sgbm_color_restate as cr
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def color_bin(tmp_path_factory):
    from mvstereovision3_amd import _lib
    _lib.lib()
    out = str(tmp_path_factory.mktemp("cppcolor") / "sgbm_color_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-implicit-fallthrough",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "sgbm_color_check.cpp"),
                    "-L", libdir, "-lmvsv", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_sgbm_color_cpu(color_bin):
    r = subprocess.run([color_bin, "cpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_sgbm_color_gpu(color_bin, gpu, tmp_path):
    dump = str(tmp_path / "pair_and_map.bin")
    r = subprocess.run([color_bin, "gpu", dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
    raw = open(dump, "rb").read()
    H, W = np.frombuffer(raw, np.int32, 2)
    L = np.frombuffer(raw, np.uint8, H * W * 3, 8).reshape(H, W, 3)
    R = np.frombuffer(raw, np.uint8, H * W * 3, 8 + H * W * 3).reshape(H, W, 3)
    got = np.frombuffer(raw, np.int16, H * W, 8 + 2 * H * W * 3).reshape(H, W)
    # the matcher the program creates: create(0, 32, 5, 200, 800, 0, 31, 10, 20, 2)
    p = cr.params(num_disparities=32, block_size=5, p1=200, p2=800, pre_filter_cap=31, uniqueness_ratio=10,
                  speckle_window_size=20, speckle_range=2)
    want = cr.compute_bgr(L, R, p)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} differ"
