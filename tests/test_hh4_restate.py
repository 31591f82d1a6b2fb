"""The MODE_HH4 reference (tests/hh4_restate.py) checked on the CPU, and the host-side
rules of the mode: what tests/test_gpu_hh4.py compares the device with must itself be
right, must tell MODE_HH4 from the other two modes on the inputs used there, and must
not move unnoticed (tests/golden/hh4_fixtures.npz).
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import twin
from tests import hh4_restate as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mvstereovision3_amd", "libmvsv.so")
FIXTURES = os.path.join(ROOT, "tests", "golden", "hh4_fixtures.npz")

built = pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")


def path_scalar(C, dx, dy, P1, P2):
    """SURVEY Appendix A.4, cell by cell: L(p, d) = C(p, d) + min(Lp(d), Lp(d -+ 1) + P1,
    min Lp + P2) - (min Lp + P2) in int16 arithmetic, Lp the path cost at p - (dx, dy),
    zero outside cost space, MAX_COST beyond the disparity range."""
    H, W1, D = C.shape
    sat = lambda v: max(-32768, min(32767, v))  # noqa: E731
    L = np.zeros((H, W1, D), np.int64)
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
    xs = range(W1) if dx >= 0 else range(W1 - 1, -1, -1)
    for y in ys:
        for x in xs:
            yp, xp = y - dy, x - dx
            Lp = [int(v) for v in L[yp, xp]] if 0 <= yp < H and 0 <= xp < W1 else [0] * D
            delta = (min(Lp) + P2 + 32768) % 65536 - 32768  # the (short) cast
            for d in range(D):
                lm = sat(Lp[d - 1] + P1) if d > 0 else sat(twin.MAX_COST + P1)
                lq = sat(Lp[d + 1] + P1) if d < D - 1 else sat(twin.MAX_COST + P1)
                m = min(Lp[d], lm, lq, delta)
                L[y, x, d] = sat(sat(m - delta) + int(C[y, x, d]))
    return L


def test_four_path_sum_equals_a_scalar_loop():
    W, H = 40, 9
    p = hr.params(num_disparities=16, block_size=3, p1=8, p2=40, mode=hr.MODE_HH4)
    L, R = hr.rand_pair(np.random.default_rng(5), H, W, 4, 0)
    C = hr.clean_volume(L, R, dict(p, mode=0))
    assert C.shape == (H, W - 16, 16)
    S = np.zeros(C.shape, np.int64)
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        S += path_scalar(C, dx, dy, 8, 40)
    assert np.array_equal(hr.aggregate(C, 8, 40), np.minimum(S, 32767))
    assert sorted(hr.DIRECTIONS) == sorted(((1, 0), (-1, 0), (0, 1), (0, -1)))


def test_clean_volume_is_the_quirked_one_outside_the_quirks():
    built_oracle = None
    try:
        from oracle import pyoracle
        pyoracle.lib()
        built_oracle = pyoracle
    except Exception:
        pass
    for seed in hr.RANDOM_SEEDS:
        L, R, p, _ = hr.random_case(seed)
        H, W = L.shape
        e = twin.sgbm_effective(p, W)
        clean = hr.clean_volume(L, R, dict(p, mode=0))
        quirked = twin.sgbm_cost_volume(L, R, dict(p, mode=1))
        inside = np.zeros(clean.shape, bool)
        inside[1:, 0, :] = True
        inside[[y for y in range(1, H) if y + e["SH2"] >= H]] = True
        assert np.array_equal(clean[~inside], quirked[~inside]), seed
        assert (clean != quirked)[inside].sum() > 0, seed  # and the quirks are real on these inputs
        if built_oracle is not None:
            assert np.array_equal(clean[~inside], built_oracle.sgbm_cost_volume(L, R, dict(p, mode=1))[~inside]), seed


@pytest.mark.parametrize("W,H,D,bs,P1,P2,s", hr.SHIFT_CASES)
def test_known_answer_on_a_constant_shift(W, H, D, bs, P1, P2, s):
    L, R = hr.shift_pair(W, H, s)
    p = hr.params(num_disparities=D, block_size=bs, p1=P1, p2=P2, mode=hr.MODE_HH4)
    d = hr.compute(L, R, p).astype(np.int32)
    m = bs // 2 + 1
    minX1 = twin.sgbm_effective(p, W)["minX1"]
    interior = d[m:H - m, minX1 + m:W - m]
    assert interior.size > 0
    wrong = np.argwhere((interior + 8) >> 4 != s)
    assert wrong.size == 0, f"{len(wrong)} of {interior.size} interior pixels are not {s}"


@pytest.mark.parametrize("seed", hr.RANDOM_SEEDS)
def test_random_cases_tell_the_modes_apart(seed):
    L, R, p, _ = hr.random_case(seed)
    e = twin.sgbm_effective(p, L.shape[1])
    assert e["W1"] > e["SW2"]  # mvsv_sgbm_validate accepts the case
    hh4 = hr.core(L, R, p)
    assert not np.array_equal(hh4, twin.sgbm_core(L, R, dict(p, mode=0))), "equals MODE_SGBM"
    assert not np.array_equal(hh4, twin.sgbm_core(L, R, dict(p, mode=1))), "equals MODE_HH"


def test_period7_pair_exercises_the_tie_rule():
    L, R, p = hr.period7_pair()
    a, b = hr.compute(L, R, p, 0), hr.compute(L, R, p, twin.F_WTA_MIN_D)
    assert (a != b).sum() > 100
    # FIRSTCOL_FIX changes nothing in this mode
    assert np.array_equal(hr.compute(L, R, p, twin.F_FIRSTCOL_FIX), a)


def test_golden_fixtures_pin_the_restatement():
    """Inputs and maps of known-answer case (a) and of the period-7 pair, recorded when
    the helper was written: an edit of the helper cannot move the target unnoticed."""
    g = np.load(FIXTURES)
    W, H, D, bs, P1, P2, s = hr.SHIFT_CASES[0]
    L, R = hr.shift_pair(W, H, s)
    assert np.array_equal(L, g["shift_L"]) and np.array_equal(R, g["shift_R"])
    p = hr.params(num_disparities=D, block_size=bs, p1=P1, p2=P2, mode=hr.MODE_HH4)
    assert np.array_equal(hr.compute(g["shift_L"], g["shift_R"], p), g["shift_map"])
    L, R, p = hr.period7_pair()
    assert np.array_equal(L, g["period7_L"]) and np.array_equal(R, g["period7_R"])
    assert np.array_equal(hr.compute(g["period7_L"], g["period7_R"], p, 0), g["period7_map_v0"])
    assert np.array_equal(hr.compute(g["period7_L"], g["period7_R"], p, 2), g["period7_map_v2"])
    assert g["shift_map"].dtype == np.int16 and not np.array_equal(g["period7_map_v0"], g["period7_map_v2"])


@built
@pytest.mark.parametrize("mode,ok", [(0, True), (1, True), (3, True), (2, False), (4, False), (-1, False)])
def test_validate_accepts_hh4_and_refuses_the_rest(mvsv, mode, ok):
    from mvstereovision3_amd import _lib
    m = mvsv.StereoSGBM.create(0, 64, 9, 648, 2592)
    m.setMode(mode)
    assert (_lib.lib().mvsv_sgbm_validate(ctypes.byref(m._params), 640, 480) == 0) == ok


@built
def test_python_mirrors_name_the_mode(mvsv):
    from mvstereovision3_amd import _lib
    assert mvsv.MODE_HH4 == 3 == _lib.MODE_HH4 == mvsv.StereoSGBM.MODE_HH4 == hr.MODE_HH4
    assert (mvsv.MODE_SGBM, mvsv.MODE_HH) == (0, 1)
    m = mvsv.StereoSGBM.create(0, 16, 3, mode=mvsv.MODE_HH4)
    assert m.getMode() == 3 and m.params()["mode"] == 3
    hdr = open(os.path.join(ROOT, "include", "mvsv.h")).read()
    assert "MVSV_MODE_HH4 = 3" in hdr and "MVSV_MODE_SGBM_3WAY = 2" in hdr


@built
def test_workspace_bytes_of_an_hh4_call(mvsv):
    """mvsv_sgbm_workspace_bytes (no device): a valid MODE_HH4 call has a plan, a
    MODE_SGBM_3WAY call has none."""
    from mvstereovision3_amd import _lib
    fn = _lib.lib().mvsv_sgbm_workspace_bytes
    fn.restype = ctypes.c_size_t
    m = mvsv.StereoSGBM.create(0, 64, 9, 648, 2592)
    m.setMode(3)
    hh4 = fn(1, 640, 480, ctypes.byref(m._params))
    m.setMode(0)
    sgbm = fn(1, 640, 480, ctypes.byref(m._params))
    # three direction planes instead of four; every other buffer is the same
    plane = (640 - 64) * 480 * 64 * 2
    assert hh4 > 0 and sgbm - hh4 == plane
    m.setMode(2)
    assert fn(1, 640, 480, ctypes.byref(m._params)) == 0
