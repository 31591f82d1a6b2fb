"""The C++ mirror of the two set-up loops (include/mvsv_detection.hpp:
mvsv::Utility::checkSharpness, the streams' enableSharpness / frontSharpness;
include/mvsv_stereosystem.hpp: Stereosystem::getUndistortedImagepair) compiled with
g++ against the C ABI, in the reference's call patterns (trgt/liveView.cpp:94-117,
trgt/liveUndistortion.cpp:58).  The expected numbers come from the numpy twin and
are passed to the program."""
import glob
import os
import subprocess

import numpy as np
import pytest

from tests import setup_restate as twin
from tests.conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def setup_bin(tmp_path_factory):
    from mvstereovision3_amd import _lib
    _lib.lib()
    out = str(tmp_path_factory.mktemp("cppsetup") / "setup_demo")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-implicit-fallthrough",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "setup_demo.cpp"),
                    "-L", libdir, "-lmvsv", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_setup_cpu(setup_bin):
    r = subprocess.run([setup_bin, "cpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_setup_gpu(setup_bin, gpu, tmp_path):
    from mvstereovision3_amd import calibration
    W, H = 752, 480
    pair = np.random.default_rng(752480).integers(0, 256, (2, H, W), dtype=np.uint8)
    x, y, rw, rh = 301, 187, 150, 111  # the clicked view area
    roi = (x, y, x + rw, y + rh)
    s4 = [twin.sum4(img, roi) for img in pair]
    values = [twin.value_of(s, rw * rh) for s in s4]
    intrinsic = sorted(glob.glob(os.path.join(GOLDEN, "calib", "*", "intrinsic.yml")))[0]
    want = []
    for img, side in zip(pair, ("Left", "Right")):
        K, _ = calibration.read_matrix(intrinsic, "cameraMatrix" + side)
        D, _ = calibration.read_matrix(intrinsic, "distCoeffs" + side)
        want.append(twin.remap_fixed(img, *twin.undistort_maps(K, D.reshape(-1), None, W, H)))
    (tmp_path / "pair.bin").write_bytes(pair.tobytes())
    (tmp_path / "want.bin").write_bytes(np.stack(want).tobytes())
    r = subprocess.run([setup_bin, "gpu", str(tmp_path / "pair.bin"), str(W), str(H), str(x), str(y), str(rw), str(rh),
                        str(s4[0]), str(s4[1]), values[0].hex(), values[1].hex(), str(twin.sum4(pair[0])),
                        intrinsic, str(tmp_path / "want.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
