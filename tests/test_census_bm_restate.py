"""The census StereoBM reference itself (tests/census_bm_restate.py), on the CPU: the two
window-cost restatements against each other, the known answer, radiometric invariance
(and its absence in the SAD matcher), the parameters without effect, the committed
fixture, and mvsv_bm_census_validate's rules (no device needed)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import twin
from tests import census_bm_restate as cb
from tests import census_restate as cs
from tests.conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "census_bm_fixtures.npz")


@pytest.mark.parametrize("minD", (-5, 0, 3, -16))
@pytest.mark.parametrize("window", [(9, 7), (5, 5), (3, 3), (1, 3), (3, 1), (13, 5)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_the_two_window_costs_agree(window, minD):
    """Pairs <= 40 x 24, D 16.  The right clamp fires at every minDisparity (the first virtual
    columns are negative), the left clamp's upper end at 0 and +3 (lofs 15 / 18: the last
    virtual columns pass W - 1 - lofs); -16 adds rofs = 1 and the left clamp's lower end."""
    H, W = 11, 34 + (minD % 3)
    L, R = cs.grey_pair(sum(window) + minD + 50, H, W, 3)
    p = cb.params(min_disparity=minD, num_disparities=16, block_size=5)
    g = cb.geometry(p, W, H)
    cl, cr = cb.column_pairs(g, W)
    j = np.arange(-g["w2"], g["width1"] + g["w2"])
    assert (cr != g["rofs"] + j).any(), "the right clamp does not fire"
    assert (cl != g["lofs"] + j).any() == (minD != -5), "the left clamp"
    a = cb.window_cost(L, R, p, window)
    b = cb.window_cost_scalar(L, R, p, window)
    assert a.shape == b.shape == (H - 4, g["width1"], 16)
    assert np.array_equal(a, b)
    assert 0 < a.max() <= 25 * (window[0] * window[1] - 1)


@pytest.fixture(scope="module")
def known():
    """Per (seed, window, blockSize): (pair, census map, census map of the transformed pair)."""
    out = {}
    for seed in cb.KNOWN_SEEDS:
        for bs in cb.KNOWN_BLOCKS:
            L, R = cb.known_pair(seed, bs)
            L2, R2 = cs.radiometric(L, R)
            p = cb.known_params(bs)
            for window in cb.KNOWN_WINDOWS:
                out[seed, window, bs] = (L, R, cb.compute(L, R, p, window), cb.compute(L2, R2, p, window))
    return out


@pytest.mark.parametrize("bs", cb.KNOWN_BLOCKS)
@pytest.mark.parametrize("window", cb.KNOWN_WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("seed", cb.KNOWN_SEEDS)
def test_known_answer_and_invariance_on_the_restatement(known, seed, window, bs):
    """Every pixel of the region rounds to the true shift 5 ((disp + 8) >> 4; the parabola
    term moves a share of the pixels to 79 or 81), no exceptions; v -> 2 v on the left and
    v -> v + 100 on the right leave the whole map as it is."""
    L, R, m, m2 = known[seed, window, bs]
    rows, cols = cb.known_region(*L.shape, bs, window)
    region = m[rows, cols].astype(np.int32)
    assert region.size > 0
    assert (((region + 8) >> 4) == cb.KNOWN_SHIFT).all()
    assert np.array_equal(m, m2)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_low_contrast_gain_changes_sad_and_not_census(seed):
    """Noise in 0..15, L -> 4 L, R -> R + 100, blockSize 5, texture 0: the census map is the
    same, the SAD matcher's (the prefilter cancels the offset, not the gain) is not."""
    (L, R), (L2, R2) = cb.low_contrast_pair(seed)
    p = cb.params(num_disparities=16, block_size=5, uniqueness_ratio=15, texture_threshold=0)
    for window in ((9, 7), (5, 5)):
        assert np.array_equal(cb.compute(L, R, p, window), cb.compute(L2, R2, p, window))
    sad, sad2 = twin.bm_compute(L, R, p), twin.bm_compute(L2, R2, p)
    assert not np.array_equal(sad, sad2)
    rows, cols = cb.known_region(*L.shape, 5, (9, 7))
    hit = lambda m: float((((m[rows, cols].astype(np.int32) + 8) >> 4) == 5).mean())  # noqa: E731
    print(f"seed {seed}: rounded known answer: SAD {hit(sad):.4f} -> {hit(sad2):.4f} under the gains, "
          f"census {hit(cb.compute(L2, R2, p, (9, 7))):.4f}")


def test_prefilter_and_texture_fields_have_no_effect():
    L, R = cs.grey_pair(31, 24, 64, 4)
    base = cb.params(num_disparities=16, block_size=7, uniqueness_ratio=10, disp12_max_diff=1)
    want = cb.compute(L, R, base, (5, 5))
    for kw in (dict(texture_threshold=0), dict(texture_threshold=100000), dict(pre_filter_cap=1),
               dict(pre_filter_cap=63), dict(pre_filter_type=0, pre_filter_size=51)):
        assert np.array_equal(cb.compute(L, R, dict(base, **kw), (5, 5)), want), kw
    # ... while the SAD matcher reads them
    assert not np.array_equal(twin.bm_compute(L, R, dict(base, texture_threshold=100000)), twin.bm_compute(L, R, base))


def test_fixture_is_the_restatement():
    z = np.load(FIXTURE)
    n = int(z["count"])
    assert n >= 6
    for k in range(n):
        L, R, want = z[f"L{k}"], z[f"R{k}"], z[f"map{k}"]
        assert L.shape[0] <= 24 and L.shape[1] <= 64
        p = dict(zip(cb.PARAM_NAMES, (int(v) for v in z[f"params{k}"])))
        window = tuple(int(v) for v in z[f"window{k}"])
        assert np.array_equal(cb.compute(L, R, p, window), want), f"fixture {k}"
        assert (want != twin.bm_compute(L, R, p)).any(), f"fixture {k} does not tell census from SAD"
        assert (want != (p["min_disparity"] - 1) * 16).any(), f"fixture {k} is all FILTERED"


# ---- mvsv_bm_census_validate (no device) -----------------------------------------
def _validate(m, W, H, cw, ch):
    from mvstereovision3_amd import _lib
    return _lib.lib().mvsv_bm_census_validate(ctypes.byref(m._params), W, H, cw, ch)


def test_validate_window_rules(mvsv):
    m = mvsv.StereoBM.create(64, 9)
    for cw, ch in ((9, 7), (7, 9), (5, 5), (3, 3), (1, 3), (3, 1), (13, 5), (5, 13), (65, 1), (1, 65), (21, 3)):
        assert _validate(m, 640, 480, cw, ch) == 0, (cw, ch)
        assert m.census_validate(640, 480, (cw, ch))
    for cw, ch in ((0, 0), (1, 1), (8, 7), (9, 6), (-3, 3), (3, -3), (9, 9), (67, 1), (11, 7), (2, 2), (4, 1)):
        assert _validate(m, 640, 480, cw, ch) == -1, (cw, ch)
        assert not m.census_validate(640, 480, (cw, ch))


# each rule of mvsv_bm_validate, by the field it reads: (field, a value it refuses)
BM_RULES = (("pre_filter_type", 2), ("pre_filter_size", 4), ("pre_filter_size", 257), ("pre_filter_size", 8),
            ("pre_filter_cap", 0), ("pre_filter_cap", 64), ("block_size", 3), ("block_size", 8), ("block_size", 257),
            ("num_disparities", 0), ("num_disparities", 24), ("texture_threshold", -1), ("uniqueness_ratio", -1))


@pytest.mark.parametrize("field,value", BM_RULES)
def test_validate_inherits_every_bm_rule(mvsv, field, value):
    from mvstereovision3_amd import _lib
    m = mvsv.StereoBM.create(64, 9)
    assert _validate(m, 640, 480, 9, 7) == 0
    setattr(m._params, field, value)
    assert _lib.lib().mvsv_bm_validate(ctypes.byref(m._params), 640, 480) == -1
    assert _validate(m, 640, 480, 9, 7) == -1


def test_validate_image_rules_and_bm_yml(mvsv):
    m = mvsv.StereoBM.create(64, 9)
    assert _validate(m, 0, 480, 9, 7) == -1      # empty image
    assert _validate(m, 640, 9, 9, 7) == -1      # blockSize not smaller than the image
    assert _validate(m, 640, 10, 9, 7) == 0
    # the struct loaded from bm.yml passes as it is (the prefilter fields are only checked)
    b = mvsv.StereoBM.create(0, 0)
    assert mvsv.Disparity.loadBMParameters(os.path.join(GOLDEN, "configs", "bm.yml"), b)
    assert b.getNumDisparities() == 80 and _validate(b, 160, 120, 9, 7) == 0


def test_colour_input_is_refused(mvsv):
    m = mvsv.StereoBM.create(16, 5)
    bgr = np.zeros((24, 64, 3), np.uint8)
    with pytest.raises(mvsv.MvsvError):
        m.compute_census(bgr, bgr)
    with pytest.raises(mvsv.MvsvError):
        mvsv.Disparity.binary_bm(mvsv.Stereopair(bgr, bgr), None, m)
