"""The staging layouts of the host-pointer calls (no GPU): the HIP-free part of
mvsv_stage.hpp in a stand-alone program under ASan + UBSan.  tests/cpp/stage_layout_check.cpp
reserves what each of the host entry points reserves, through the layout structs
they use, over widths 1 .. 1281 and heights 1 .. 23: slices disjoint, inside the total
and 256-byte aligned, pitches as before the arena, and no more memory than the three
staging buffers took."""
import os
import subprocess

from tests.conftest import ROOT

# every entry point of include/mvsv.h that takes one frame from host memory
HOST_CALLS = ["mvsv_sgbm", "mvsv_sgbm_bgr", "mvsv_bm", "mvsv_tm", "mvsv_mean_disparity_grid", "mvsv_samplepoint_values",
              "mvsv_normalize_minmax", "mvsv_view", "mvsv_point_cloud", "mvsv_dmap2pcl", "mvsv_resize",
              "mvsv_prepare_gray", "mvsv_rectify_pair", "mvsv_sharpness", "mvsv_undistort_pair"]


def test_stage_layouts_under_asan_ubsan(tmp_path):
    exe = tmp_path / "stage_layout_check"
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "mvstereovision3_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "stage_layout_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "layouts:" in r.stdout and ", 0 failures" in r.stdout
    names = [line.split()[1:] for line in r.stdout.splitlines() if line.startswith("calls:")]
    assert names and sorted(names[0]) == sorted(HOST_CALLS), names
