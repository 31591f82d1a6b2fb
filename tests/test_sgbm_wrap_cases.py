"""The table of tests/sgbm_wrap_cases.py on the CPU (no GPU): every case reaches the form it
states, the table covers every form the general recurrence takes, and every input really
leaves int16 and tells the two cost-row updates apart.

tests/cpp/kernel_forms_check.cpp ("wide" lines) runs sgbm_make_plan of the real header at
256 CUs; the input conditions are computed with the numpy twin's closed-form cost volume
(int32: the true sums) and the C oracle under both updates."""
import os
import subprocess

import numpy as np
import pytest

from tests import sgbm_wrap_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    """plan_of(lines) -> the printed plan fields of every "wide" line, as dicts."""
    exe = tmp_path_factory.mktemp("kfw") / "kfc"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "kernel_forms_check.cpp"),
                    "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe), "wide"], input="".join(x + "\n" for x in lines), capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows = r.stdout.split("\n")[:-1]
        assert len(rows) == len(lines)
        return [dict(zip(wc.PLAN_FIELDS, map(int, row.split()))) for row in rows]

    return run


def test_every_case_reaches_its_form(plan_of):
    cases = wc.all_cases()
    bad = []
    for c, got in zip(cases, plan_of([wc.check_line(c) for c in cases])):
        stated = {k: int(v) for k, v in c.form.items() if k in wc.PLAN_FIELDS}
        assert "no_wrap" in stated and "nw" in stated
        print(f"{c.name:44s} {' '.join(f'{k}={got[k]}' for k in wc.PLAN_FIELDS)}")
        diff = {k: (v, got[k]) for k, v in stated.items() if got[k] != v}
        if diff:
            bad.append((c.name, diff))
    assert not bad, f"{len(bad)} cases miss their form, (stated, plan): {bad[:8]}"


def test_env_and_options_name_the_same_choice():
    for c in wc.all_cases():
        want = dict(wc.OPTION_DEFAULTS)
        for w in filter(None, c.env.get("MVSV_KERNELS", "").split(",")):
            want[wc.kc.KERNEL_WORDS[w]] = 0
        for k, v in c.env.items():
            assert k in wc.kc.ENV_ALL
            if k != "MVSV_KERNELS":
                want[wc.ENV_INTS[k]] = int(v)
        assert c.opts == want, c.name


def test_table_covers_every_form_of_the_general_recurrence(plan_of):
    """sgbm_make_plan over FORM_AXES at 256 CUs, plans with no_wrap == false: every distinct
    (cost2, ppc, family, sched, acc, split, lpc, waves) is the form of a case."""
    enum = wc.enumeration()
    plans = plan_of([line for _, line in enum])
    occur = {}
    for (axes, _), p in zip(enum, plans):
        if not p["no_wrap"]:
            assert not p["nw"] and not p["residual"] and p["family"] != wc.BITSLICE, axes
            occur.setdefault(wc.form_key(p), axes)
    assert len(occur) >= 40
    cases = wc.all_cases()
    table = {wc.form_key(p): c.name for c, p in zip(cases, plan_of([wc.check_line(c) for c in cases]))}
    missing = {k: a for k, a in occur.items() if k not in table}
    assert not missing, f"{len(missing)} of {len(occur)} forms have no case: {list(missing.items())[:6]}"


def test_cases_that_must_be_there():
    cs = wc.all_cases()
    P = lambda c, k: c.params[k]  # noqa: E731
    # both cost kernels: register ring at D 64 / 128 / 256, LDS ring at 17 .. 21 and at 15 by switch
    ring = [c for c in cs if c.form["cost2"]]
    assert {P(c, "num_disparities") for c in ring} >= {64, 128, 256} and all(P(c, "block_size") <= 15 for c in ring)
    lds = [c for c in cs if not c.form["cost2"] and c.kind == "sgbm"]
    assert {P(c, "block_size") for c in lds} >= {15, 17, 19, 21}
    # a forced tile height across H = 51, the default at H > 16
    assert {(c.form["cost2"], c.H) for c in cs if c.opts["cost_ty"] == 24} == {(1, 51), (0, 51)}
    assert all(c.H > 16 for c in cs)
    # the four variant words in both modes; uniquenessRatio, disp12MaxDiff, minDisparity
    assert {(P(c, "mode"), c.variant) for c in cs} == {(m, v) for m in (0, 1) for v in range(4)}
    assert {P(c, "uniqueness_ratio") > 0 for c in cs} == {False, True}
    assert {P(c, "disp12_max_diff") for c in cs} == {-1, 1}
    assert {P(c, "min_disparity") for c in cs} == {-2, 0, 3}
    # odd heights at D >= 128 on the fused final kernel
    assert {P(c, "num_disparities") for c in cs if c.H % 2 and c.form["sched"] == 2 and not c.form["split"]} >= {128, 256}
    # a batch with a plain middle frame; a colour case at blockSize 15 / P2 9000
    assert [c.n for c in cs if c.recipe == "saw_rand_saw"] == [3]
    assert [(P(c, "block_size"), P(c, "p2")) for c in cs if c.kind == "bgr"] == [(15, 9000)]
    # P2 <= 5 over wrapped costs
    assert any(P(c, "p2") <= 5 for c in cs)
    # every frame small
    assert all(c.W <= (520 if P(c, 'num_disparities') == 256 else 260) and c.H <= 51 for c in cs)


def measure(c, oracle):
    """Per sawtooth frame of the case: the twin's true cost volume T, the flagged oracle's C,
    and the maps under both updates."""
    from oracle import twin
    out = []
    for (L, R, saw), (flagged, plain) in zip(wc.frames(c), wc.references(c.name)):
        T = twin.sgbm_cost_volume(L, R, c.params, c.variant)
        C = oracle.sgbm_cost_volume(L, R, c.params, c.variant | wc.F_COST_WRAP)
        out.append((saw, T, C, flagged, plain))
    return out


@pytest.mark.parametrize("name", wc.names())
def test_input_conditions(oracle, plan_of, name):
    """The conditions that make a case a test of wrapped costs (conditions, not measurements):
    C is int16; at least 3 % of the true volume is above 32767; the maps of the wrapping and
    the saturating update differ in at least 1 % of the pixels; 20 % - 90 % of the map is valid
    and holds at least 3 distinct disparities; the plan says no_wrap == false.  The flagged
    oracle's volume is the true volume modulo 2^16."""
    c = wc.case(name)
    assert plan_of([wc.check_line(c)])[0]["no_wrap"] == 0
    invalid = (c.params["min_disparity"] - 1) * 16
    for k, (saw, T, C, flagged, plain) in enumerate(measure(c, oracle)):
        assert C.dtype == np.int16 and flagged.dtype == np.int16
        assert np.array_equal(C, T.astype(np.int16)), "flagged oracle volume != twin volume mod 2^16"
        wrapped = float((T > 32767).mean())
        differ = float((flagged != plain).mean())
        valid = flagged != invalid
        ndisp = len(np.unique(flagged[valid] >> 4))
        print(f"{name} frame {k}: largest T {T.max()}, wrapped {wrapped:.3f}, maps differ {differ:.3f}, "
              f"valid {valid.mean():.2f}, disparities {ndisp}")
        if not saw:
            assert T.max() <= 32767 and differ == 0.0  # the plain middle frame of the batch
            continue
        assert wrapped >= 0.03
        assert differ >= 0.01
        assert 0.2 <= valid.mean() <= 0.9
        assert ndisp >= 3


def test_table_holds_a_double_wrap(oracle):
    from oracle import twin
    c = wc.case("double-wrap")
    L, R, _ = wc.frames(c)[0]
    T = twin.sgbm_cost_volume(L, R, c.params, c.variant)
    assert (T > 65535).mean() >= 0.01
