"""The SGBM launch plan (mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp): one pure
function decides schedule, kernel family, planes and every buffer size of an
sgbm_device call; the launchers, mvsv_sgbm_plan and mvsv_sgbm_workspace_bytes read it.

tests/cpp/sgbm_plan_check.cpp (plain g++, no library, no GPU) pins the plans of the
shapes this repository's comments and tests name and checks invariants of every plan
over a grid of shapes, parameters, options and CU counts.  The GPU test replays plan
words recorded from the library before the plan existed (tests/golden/sgbm_plan_bits.json)
against the built library."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sgbm_plan_bits.json")


def test_sgbm_plan_pins_and_invariants(tmp_path):
    exe = tmp_path / "spc"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "sgbm_plan_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " plans, 0 violations" in r.stdout


@pytest.mark.gpu
def test_sgbm_plan_bits_match_the_recorded_ones(gpu, mvsv):
    """mvsv_sgbm_plan[_cn] of the built library == the words the library gave when every
    launcher still decided for itself, entry by entry (options through mvsv_set_option)."""
    from mvstereovision3_amd import _lib
    with open(GOLDEN) as f:
        rec = json.load(f)
    ctx = _lib.Context(0)
    opts = (("path_sched", _lib.OPT_PATH_SCHEDULE), ("strip_waves", _lib.OPT_STRIP_WAVES),
            ("cost_res", _lib.OPT_COST_RESIDUAL), ("bitslice", _lib.OPT_BITSLICE))
    try:
        assert rec["cus"] == gpu.cuda.get_device_properties(0).multi_processor_count, "recorded on another CU count"
        assert len(rec["rows"]) >= 200
        bad = []
        for row in rec["rows"]:
            ent = dict(zip(rec["columns"], row))
            for name, opt in opts:
                _lib.check(_lib.lib().mvsv_set_option(ctx.handle, opt, ent[name]), ctx.handle)
            p = _lib.SgbmParams(**{f: ent[f] for f in _lib.SGBM_FIELDS})
            got = _lib.sgbm_plan(ctx, ent["n"], ent["width"], ent["height"], p, ent["channels"])
            if got != ent["bits"]:
                bad.append((ent, got))
        assert not bad, f"{len(bad)} of {len(rec['rows'])} differ, first: {bad[0]}"
    finally:
        ctx.close()
