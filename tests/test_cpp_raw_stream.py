"""The C++ RawDisparityStream (include/mvsv_stereosystem.hpp) compiled with g++
against the C ABI: the camera loop of trgt/liveDisparity.cpp:82-101 from a
Stereosystem (baseline_small, 376 x 240 with binning) as push_raw / pop, three
frames through a ring of two, checked against the oracle's remap + crop + sgbm."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

CAL = os.path.join(ROOT, "tests", "golden", "calib")


@pytest.fixture(scope="module")
def raw_stream_bin(tmp_path_factory):
    from mvstereovision3_amd import _lib
    _lib.lib()
    out = str(tmp_path_factory.mktemp("cpprs") / "raw_stream_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "raw_stream_check.cpp"),
                    "-L", libdir, "-lmvsv", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_raw_stream_cpu(raw_stream_bin, tmp_path):
    r = subprocess.run([raw_stream_bin, "cpu", CAL, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok" in r.stdout


def _load(path, dtype=np.uint8):
    with open(path, "rb") as f:
        h, w = map(int, f.readline().split())
        return np.frombuffer(f.read(), dtype).reshape(h, w)


@pytest.mark.gpu
def test_cpp_raw_stream_gpu(raw_stream_bin, tmp_path, gpu, oracle, mvsv):
    from mvstereovision3_amd import calibration as calib
    r = subprocess.run([raw_stream_bin, "gpu", CAL, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
    # the same rectification state through the Python mirror (same host maps)
    s = calib.Stereosystem(376, 240, binning=True)
    assert s.loadIntrinsic(os.path.join(CAL, "baseline_small", "intrinsic.yml"))
    assert s.loadExtrinisic(os.path.join(CAL, "baseline_small", "extrinsic.yml"))
    assert s.initRectification()
    x0, y0, x1, y1 = s.mDisplayROI
    m = mvsv.StereoSGBM.create(0, 64, 5, 200, 800, 1, 31, 10, 50, 2)
    p = {k: v for k, v in m.params().items() if k != "variant"}
    for i in range(3):
        rect = []
        for side, k in (("l", 0), ("r", 1)):
            raw = _load(tmp_path / f"raw_{side}_{i}.bin")
            w = np.ascontiguousarray(oracle.remap_linear(raw, s.mMap1[k], s.mMap2[k])[y0:y1, x0:x1])
            got = _load(tmp_path / f"rect_{side}_{i}.bin")
            bad = np.argwhere(got != w)
            assert got.shape == w.shape and bad.size == 0, \
                f"frame {i} {side}: {len(bad)} mismatches, first {bad[:5].tolist()}"
            rect.append(w)
        want = oracle.sgbm(rect[0], rect[1], p)
        got = _load(tmp_path / f"disp_{i}.bin", np.int16)
        bad = np.argwhere(got != want)
        assert got.shape == want.shape and bad.size == 0, \
            f"frame {i}: {len(bad)} mismatches, first {bad[:5].tolist()}"
        assert (want > 0).mean() > 0.5
        if i == 0:
            half = [oracle.resize_linear(a, 0.5, 0.5) for a in rect]
            wh = oracle.sgbm(half[0], half[1], p)
            assert (wh > 0).mean() > 0.5
            gh = _load(tmp_path / "half_0.bin", np.int16)
            bad = np.argwhere(gh != wh)
            assert gh.shape == wh.shape and bad.size == 0, \
                f"factor 0.5: {len(bad)} mismatches, first {bad[:5].tolist()}"
