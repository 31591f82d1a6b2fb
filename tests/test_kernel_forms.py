"""Every case of tests/kernel_form_cases.py reaches the kernel form it states (no GPU).

tests/cpp/kernel_forms_check.cpp (plain g++) runs sgbm_make_plan of the real header on each
case's KernelOptions, parameters and launch shape at 256 CUs; the plan fields it prints are
compared with the case's ``form``.  This is the evidence that H, W, n and the switches select
the tile height, the band permutation, lines_aux, the family and the schedule: the library
itself reports only the MVSV_PLAN_* word."""
import os
import subprocess

import pytest

from tests import kernel_form_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{case name: printed plan fields} of every SGBM / colour case at kc.CUS CUs."""
    exe = tmp_path_factory.mktemp("kfc") / "kfc"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "kernel_forms_check.cpp"),
                    "-o", str(exe)], check=True)
    cases = [c for c in kc.all_cases() if c.kind != "bm"]
    r = subprocess.run([str(exe)], input="".join(kc.check_line(c) + "\n" for c in cases), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = r.stdout.split("\n")[:-1]
    assert len(rows) == len(cases)
    return {c.name: dict(zip(kc.PLAN_FIELDS, map(int, row.split()))) for c, row in zip(cases, rows)}


def test_every_case_reaches_its_form(plans):
    bad = []
    for c in kc.all_cases():
        if c.kind == "bm":
            continue
        got = plans[c.name]
        stated = {k: int(v) for k, v in c.form.items() if k in kc.PLAN_FIELDS}
        print(f"{c.name:34s} {' '.join(f'{k}={got[k]}' for k in kc.PLAN_FIELDS)} xcd={int(kc.xcd_permutes(c.opts, got))}")
        diff = {k: (v, got[k]) for k, v in stated.items() if got[k] != v}
        if diff:
            bad.append((c.name, diff))
    assert not bad, f"{len(bad)} cases miss their form, (stated, plan): {bad[:8]}"


def test_env_and_options_name_the_same_choice():
    """env is what mvsv_create parses into opts: MVSV_KERNELS words clear their field, the
    integer switches set theirs, everything else keeps the KernelOptions default."""
    for c in kc.all_cases():
        want = dict(kc.OPTION_DEFAULTS)
        for w in filter(None, c.env.get("MVSV_KERNELS", "").split(",")):
            want[kc.KERNEL_WORDS[w]] = 0
        for k, v in c.env.items():
            assert k in kc.ENV_ALL
            if k != "MVSV_KERNELS":
                want[kc.ENV_INTS[k]] = int(v)
        assert c.opts == want, c.name


def test_groups_hold_the_edges():
    """What the groups exist for, stated over the table (and so checked against the plan above)."""
    by = {g: [c for c in kc.all_cases() if c.group == g] for g in ("ty", "xcd", "gen", "lines")}
    # 1. every height with an image shorter than a tile, a one-row last tile and three tiles
    for TY in kc.TILE_HEIGHTS:
        hs = {c.H for c in by["ty"] if c.form["cost_ty"] == TY}
        assert hs == {TY - 1, TY + 1, 2 * TY + 3}
    assert {(c.form["cost2"], c.form["family"] == kc.BITSLICE, c.kind) for c in by["ty"]} == \
        {(1, False, "sgbm"), (1, True, "sgbm"), (0, False, "bgr")}
    # 2. permutation on at 8 and 24 bands with 2 and 3 tile columns, single- and multi-frame; off by switch; off by count
    on = [c for c in by["xcd"] if kc.xcd_permutes(c.opts, c.form)]
    assert {c.form["gyn"] for c in on} == {8, 24} and {c.form["gx"] for c in on} == {2, 3} and {c.n for c in on} == {1, 2, 8}
    off = [c for c in by["xcd"] if not kc.xcd_permutes(c.opts, c.form)]
    assert {c.form["gyn"] for c in off} == {8, 24, 9} and len(on) == 9 and len(off) == 15
    assert all(c.form["cost2"] and c.form["cost_ty"] == 16 and c.form["gx"] % 8 for c in by["xcd"])
    # 3. every MVSV_KERNELS word; the full path forms; schedule 0 on the 16-lane family
    assert {w for c in by["gen"] for w in c.env["MVSV_KERNELS"].split(",")} == set(kc.KERNEL_WORDS)
    assert {c.params["num_disparities"] for c in by["gen"] if c.form.get("family") == kc.GENERIC} >= {128, 256}
    assert {c.params["num_disparities"] for c in by["gen"]
            if c.form.get("family") == kc.PACKED16 and c.form["sched"] == 0} == {32, 64, 128, 256}
    # 4. every placement on every plane format, n = 3
    assert {(c.form["lines_aux"], c.form["acc"], c.form["residual"], c.form["nw"]) for c in by["lines"]} == \
        {(a, *f) for a in (0, 1, 2) for f in ((kc.NIB, 1, 1), (kc.U16, 0, 0), (kc.U16, 0, 1))}
    assert all(c.n == 3 and c.form["sched"] == 1 for c in by["lines"])
    assert {c.params["mode"] for c in by["lines"]} == {0, 1}


def test_bm_cases_are_in_the_lanes_kernels_range():
    """bm-tile runs bm_match_kernel where bm_device would pick the lanes kernel: blockSize 5..21, D <= 128."""
    bm = [c for c in kc.all_cases() if c.kind == "bm"]
    assert len(bm) == 12
    for c in bm:
        assert c.opts["bm2"] == 0 and 5 <= c.params["block_size"] <= 21 and c.params["num_disparities"] <= 128
    assert sum(c.params["disp12_max_diff"] >= 0 and c.params["speckle_window_size"] > 0 for c in bm) >= 1
