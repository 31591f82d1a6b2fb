"""The C++ mirror of the lattice detector (include/mvsv_detection.hpp:
mvsv::Samplepoint, mvsv::SamplepointDetection, the streams' enableSamplepoints /
frontSamples) compiled with g++ against the C ABI, in the reference's call pattern
(src/SamplePointDetection.cpp, trgt/demo.cpp:206-209,271-276)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def samplepoint_bin(tmp_path_factory):
    from mvstereovision3_amd import _lib
    _lib.lib()
    out = str(tmp_path_factory.mktemp("cppsp") / "samplepoint_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-implicit-fallthrough",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "samplepoint_check.cpp"),
                    "-L", libdir, "-lmvsv", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_samplepoint_cpu(samplepoint_bin, tmp_path):
    r = subprocess.run([samplepoint_bin, "cpu", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok" in r.stdout
    assert sorted(p.name for p in tmp_path.iterdir()) == ["pcl_0000.ply", "pcl_0001.ply"]


@pytest.mark.gpu
def test_cpp_samplepoint_gpu(samplepoint_bin, tmp_path, gpu):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    r = subprocess.run([samplepoint_bin, "gpu", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
