"""The C++ mirror of the stream's device ends (include/mvsv_detection.hpp:
DisparityStream::pushDevice / popDevice / frontMapDevice / hostOutputs / fence)
compiled with g++ against the C ABI: seven 101 x 67 frames from device memory through
a ring of three, compared in the program with host pushes and here with the oracle."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def device_stream_bin(tmp_path_factory):
    from mvstereovision3_amd import _lib
    _lib.lib()
    out = str(tmp_path_factory.mktemp("cppds") / "device_stream_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "device_stream_check.cpp"),
                    "-L", libdir, "-lmvsv", "-ldl", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_device_stream_cpu(device_stream_bin):
    r = subprocess.run([device_stream_bin, "cpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok" in r.stdout


def _load(path, dtype=np.uint8):
    with open(path, "rb") as f:
        h, w = map(int, f.readline().split())
        return np.frombuffer(f.read(), dtype).reshape(h, w)


@pytest.mark.gpu
def test_cpp_device_stream_gpu(device_stream_bin, tmp_path, gpu, oracle, mvsv):
    r = subprocess.run([device_stream_bin, "gpu", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
    left, right = _load(tmp_path / "left.bin"), _load(tmp_path / "right.bin")
    disp = _load(tmp_path / "disp.bin", np.int16)
    m = mvsv.StereoSGBM.create(0, 32, 5, 200, 800, 1, 31, 10, 50, 2)
    p = {k: v for k, v in m.params().items() if k != "variant"}
    H = 67
    assert left.shape == (7 * H, 101) and disp.shape == left.shape
    for i in range(7):
        rows = slice(i * H, (i + 1) * H)
        want = oracle.sgbm(np.ascontiguousarray(left[rows]), np.ascontiguousarray(right[rows]), p)
        bad = np.argwhere(disp[rows] != want)
        assert bad.size == 0, f"frame {i}: {len(bad)} mismatches, first {bad[:5].tolist()}"
        assert (want > 0).mean() > 0.25
