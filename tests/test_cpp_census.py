"""The C++ mirror of Disparity::binary_sgbm (include/mvsv_disparity.hpp) compiled with g++
against the C ABI, in the way of tests/test_cpp_sgbm_color.py: the call the reference left
commented out (src/disparity.cpp:12-15), on a Stereopair of ROI views."""
import os
import subprocess

import numpy as np
import pytest

from tests import census_restate as cs
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def census_bin(tmp_path_factory):
    from mvstereovision3_amd import _lib
    _lib.lib()
    out = str(tmp_path_factory.mktemp("cppcensus") / "census_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-implicit-fallthrough",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "census_check.cpp"),
                    "-L", libdir, "-lmvsv", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_census_cpu(census_bin):
    r = subprocess.run([census_bin, "cpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_census_gpu(census_bin, gpu, tmp_path):
    dump = str(tmp_path / "pair_and_map.bin")
    r = subprocess.run([census_bin, "gpu", dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
    raw = open(dump, "rb").read()
    H, W = np.frombuffer(raw, np.int32, 2)
    L = np.frombuffer(raw, np.uint8, H * W, 8).reshape(H, W)
    R = np.frombuffer(raw, np.uint8, H * W, 8 + H * W).reshape(H, W)
    got = np.frombuffer(raw, np.int16, H * W, 8 + 2 * H * W).reshape(H, W)
    # the matcher the program creates: create(0, 32, 5, 10, 120, 0, 0, 10, 20, 2), window (9, 7)
    p = cs.params(num_disparities=32, block_size=5, p1=10, p2=120, uniqueness_ratio=10,
                  speckle_window_size=20, speckle_range=2)
    want = cs.compute(L, R, p, (9, 7))
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} differ"
