"""The SGBM launch plan of MODE_HH4 (mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp), host-pure.

tests/cpp/hh4_plan_check.cpp (plain g++, no library, no GPU) checks that no MODE_HH4
launch runs a strip chain or a bit-sliced kernel or sizes a spin-wait buffer (status,
strip boundary granules) -- at sgbm.yml's and liveDisparity's values, at D 16 and D 48,
and over a grid of shapes, parameters and options -- that its planes are three side by
side and one per direction, and that MODE_SGBM and MODE_HH plan at the same shapes
exactly as the header did before the mode existed (tests/cpp/hh4_plan_before.inc)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hh4_plan_check(tmp_path):
    exe = tmp_path / "hpc"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "hh4_plan_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " plans, 0 violations" in r.stdout
