"""The launch plan of a census call (tests/cpp/census_plan_check.cpp: plain g++, no library,
no GPU) over the shape grid of tests/cpp/sgbm_plan_check.cpp: never the register-ring cost
kernel, a residual plane or bit planes; everything else as the existing rules decide; and
total_bytes() equal to the allocations."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_plan_invariants(tmp_path):
    exe = tmp_path / "cpc"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpp", "census_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " violations" in r.stdout and ", 0 violations" in r.stdout
