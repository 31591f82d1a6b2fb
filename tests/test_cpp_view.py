"""The C++ mirror of the detection view (include/mvsv_detection.hpp: mvsv::View,
mvsv::Utility::detectionView, the streams' enableView / frontView) compiled with g++
against the C ABI, in the reference's call pattern (trgt/demo.cpp:280-298)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def view_bin(tmp_path_factory):
    from mvstereovision3_amd import _lib
    _lib.lib()
    out = str(tmp_path_factory.mktemp("cppview") / "view_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-implicit-fallthrough",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "view_check.cpp"),
                    "-L", libdir, "-lmvsv", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_view_cpu(view_bin, tmp_path):
    r = subprocess.run([view_bin, "cpu", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_view_gpu(view_bin, gpu, tmp_path):
    r = subprocess.run([view_bin, "gpu", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
