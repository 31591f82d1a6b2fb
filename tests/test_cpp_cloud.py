"""The C++ mirror of the point cloud (include/mvsv_detection.hpp:
mvsv::Utility::pointCloud, the streams' enableCloud / frontCloud) compiled with g++
against the C ABI, in the reference's call pattern (trgt/demo.cpp:394 and the other
detector loops' dmap2pcl call)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def cloud_bin(tmp_path_factory):
    from mvstereovision3_amd import _lib
    _lib.lib()
    out = str(tmp_path_factory.mktemp("cppcloud") / "cloud_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-implicit-fallthrough",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "cloud_check.cpp"),
                    "-L", libdir, "-lmvsv", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_cloud_cpu(cloud_bin):
    r = subprocess.run([cloud_bin, "cpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_cloud_gpu(cloud_bin, gpu):
    r = subprocess.run([cloud_bin, "gpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
