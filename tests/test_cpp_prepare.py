"""The C++ mirrors of the disparityTest loop (include/mvsv_detection.hpp:
mvsv::Utility::prepareGray, DisparityStream with a StereoBM matcher, enableBgr /
pushBgr; include/mvsv_stereosystem.hpp: RawDisparityStream's StereoBM constructor)
compiled with g++ against the C ABI, in the reference's call pattern
(trgt/disparityTest.cpp:201-211,267-268)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def prepare_bin(tmp_path_factory):
    from mvstereovision3_amd import _lib
    _lib.lib()
    out = str(tmp_path_factory.mktemp("cppprep") / "prepare_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-implicit-fallthrough",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "prepare_check.cpp"),
                    "-L", libdir, "-lmvsv", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_prepare_cpu(prepare_bin):
    r = subprocess.run([prepare_bin, "cpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_prepare_gpu(prepare_bin, gpu):
    r = subprocess.run([prepare_bin, "gpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
