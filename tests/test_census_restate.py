"""The census reference itself (tests/census_restate.py), on the CPU: bit order, the two
pixel-cost restatements against each other, radiometric invariance, the known answer,
the committed fixture, and mvsv_sgbm_census_validate's rules (no device needed)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import twin
from tests import census_restate as cs
from tests.conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "census_fixtures.npz")


def test_hand_written_3x3_descriptor_pins_the_bit_order():
    I = np.array([[9, 1, 9],
                  [1, 5, 9],
                  [9, 9, 1]], np.uint8)
    # centre (1, 1) = 5; offsets in order (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1):
    # neighbours 9 1 9 1 9 9 9 1 -> darker than 5 at k = 1, 3, 7
    T = cs.census(I, 3, 3)
    assert T.dtype == np.uint64
    assert int(T[1, 1]) == (1 << 1) | (1 << 3) | (1 << 7)
    # corner (0, 0) = 9, neighbours clamped: rows (0, 0, 1), columns (0, 0, 1):
    # 9 9 1 / 9 . 1 / 1 1 5 -> darker at k = 2, 4, 5, 6, 7
    assert int(T[0, 0]) == (1 << 2) | (1 << 4) | (1 << 5) | (1 << 6) | (1 << 7)
    # a 3 x 1 window (width 3, height 1) has the two bits (0,-1), (0,1); 1 x 3 has (-1,0), (1,0)
    assert int(cs.census(I, 3, 1)[1, 1]) == 0b01  # left neighbour 1 < 5, right 9 is not
    assert int(cs.census(I, 1, 3)[1, 1]) == 0b01  # upper neighbour 1 < 5, lower 9 is not
    assert int(cs.census(I, 1, 3)[2, 2]) == 0b00 and int(cs.census(I, 3, 1)[2, 0]) == 0b00
    assert cs.offsets(3, 3)[:3] == [(-1, -1), (-1, 0), (-1, 1)]


@pytest.mark.parametrize("window", [(13, 5), (5, 13), (65, 1), (1, 65), (21, 3)])
def test_widest_windows_fill_their_bits(window):
    cw, ch = window
    rng = np.random.default_rng(cw * 100 + ch)
    I = rng.integers(0, 256, (9, 11)).astype(np.uint8)
    T = cs.census(I, cw, ch)
    bits = cw * ch - 1
    if bits < 64:
        assert int(T.max()) < (1 << bits)
    # the brightest pixel sees every other value as darker or equal; bit k set iff strictly darker
    y, x = np.unravel_index(np.argmax(I), I.shape)
    want = 0
    for k, (dy, dx) in enumerate(cs.offsets(cw, ch)):
        if I[min(max(y + dy, 0), 8), min(max(x + dx, 0), 10)] < I[y, x]:
            want |= 1 << k
    assert int(T[y, x]) == want


@pytest.mark.parametrize("window,minD,D", [((9, 7), 0, 16), ((5, 5), -3, 16), ((3, 3), 5, 16), ((7, 9), 0, 32),
                                           ((13, 5), -2, 16), ((1, 3), 0, 16)])
def test_the_two_pixel_costs_agree(window, minD, D):
    L, R = cs.grey_pair(sum(window) + D + minD, 9, D + 30)
    e = twin.sgbm_effective(cs.params(min_disparity=minD, num_disparities=D), L.shape[1])
    a = cs.pixel_cost(L, R, e, window)
    b = cs.pixel_cost_scalar(L, R, e, window)
    assert a.shape == b.shape == (9, e["W1"], D)
    assert np.array_equal(a, b)
    assert a.max() <= window[0] * window[1] - 1 and a.max() > 0


@pytest.fixture(scope="module")
def known():
    """Per (seed, window, mode): (pair, transformed pair, census maps of both, BT map of the transformed pair)."""
    out = {}
    for seed in cs.KNOWN_SEEDS:
        L, R = cs.noise_shift_pair(seed)
        L2, R2 = cs.radiometric(L, R)
        for mode in cs.KNOWN_MODES:
            p = cs.params(mode=mode, **cs.KNOWN_PARAMS)
            bt = cs.compute_bt(L2, R2, p)
            for window in cs.KNOWN_WINDOWS:
                out[seed, window, mode] = (L, R, L2, R2, cs.compute(L, R, p, window), cs.compute(L2, R2, p, window), bt)
    return out


@pytest.mark.parametrize("mode", cs.KNOWN_MODES)
@pytest.mark.parametrize("window", cs.KNOWN_WINDOWS)
@pytest.mark.parametrize("seed", cs.KNOWN_SEEDS)
def test_known_answer_and_invariance_on_the_restatement(known, seed, window, mode):
    L, R, L2, R2, m, m2, bt = known[seed, window, mode]
    # both maps are strictly increasing: every descriptor, hence the whole map, is the same
    assert np.array_equal(cs.census(L, *window), cs.census(L2, *window))
    assert np.array_equal(cs.census(R, *window), cs.census(R2, *window))
    assert np.array_equal(m, m2)
    rows, cols = cs.known_region(*L.shape)
    assert (m[rows, cols] == 16 * 5).all()
    # the BT cost on raw intensities does not survive the two gains
    share = float((bt[rows, cols] == 16 * 5).mean())
    print(f"seed {seed} window {window} mode {mode}: BT reaches 80 on {share:.3f} of the region")
    assert share < 1.0, share


def test_fixture_is_the_restatement():
    z = np.load(FIXTURE)
    n = int(z["count"])
    assert n >= 6
    modes = set()
    for k in range(n):
        L, R, want = z[f"L{k}"], z[f"R{k}"], z[f"map{k}"]
        assert L.shape[0] <= 24 and L.shape[1] <= 64
        p = dict(zip(cs.cr.PARAM_NAMES, (int(v) for v in z[f"params{k}"])))
        window = tuple(int(v) for v in z[f"window{k}"])
        modes.add(p["mode"])
        assert np.array_equal(cs.compute(L, R, p, window), want), f"fixture {k}"
        assert (want != cs.compute_bt(L, R, p)).any(), f"fixture {k} does not tell census from BT"
    assert modes == {0, 1, 3}


# ---- mvsv_sgbm_census_validate (no device) --------------------------------------
def _validate(mvsv, m, W, H, cw, ch):
    from mvstereovision3_amd import _lib
    return _lib.lib().mvsv_sgbm_census_validate(ctypes.byref(m._params), W, H, cw, ch)


def test_validate_window_rules(mvsv):
    m = mvsv.StereoSGBM.create(0, 16, 3, 10, 120)
    for cw, ch in ((9, 7), (7, 9), (5, 5), (3, 3), (1, 3), (3, 1), (13, 5), (5, 13), (65, 1), (1, 65), (21, 3)):
        assert _validate(mvsv, m, 640, 480, cw, ch) == 0, (cw, ch)
        assert m.census_validate(640, 480, (cw, ch))
    for cw, ch in ((0, 0), (1, 1), (8, 7), (9, 6), (-3, 3), (3, -3), (9, 9), (67, 1), (11, 7), (2, 2), (4, 1)):
        assert _validate(mvsv, m, 640, 480, cw, ch) == -1, (cw, ch)
        assert not m.census_validate(640, 480, (cw, ch))
    # mvsv_sgbm_validate's own rules still apply, MODE_SGBM_3WAY among them
    assert _validate(mvsv, mvsv.StereoSGBM.create(0, 24, 3), 640, 480, 9, 7) == -1
    assert _validate(mvsv, mvsv.StereoSGBM.create(0, 16, 3, mode=2), 640, 480, 9, 7) == -1
    assert _validate(mvsv, mvsv.StereoSGBM.create(0, 16, 3, mode=3), 640, 480, 9, 7) == 0
    assert _validate(mvsv, m, 0, 480, 9, 7) == -1  # empty image


def test_validate_int16_bound_on_both_sides(mvsv):
    # blockSize 21, window (9, 7): 441 * 62 = 27342; P2 = 5425 reaches 32767 exactly
    assert 5425 + 441 * 62 == 32767
    ok = mvsv.StereoSGBM.create(0, 16, 21, 10, 5425)
    bad = mvsv.StereoSGBM.create(0, 16, 21, 10, 5426)
    assert _validate(mvsv, ok, 640, 480, 9, 7) == 0
    assert _validate(mvsv, bad, 640, 480, 9, 7) == -1
    # the same parameters with a smaller window are fine, and with BT they are mvsv_sgbm's business
    assert _validate(mvsv, bad, 640, 480, 5, 5) == 0
    # effective values: blockSize 0 means 5, P2 0 means max(5, P1 + 1)
    assert _validate(mvsv, mvsv.StereoSGBM.create(0, 16, 0, 32717, 0), 640, 480, 1, 3) == -1  # 32718 + 25 * 2
    assert _validate(mvsv, mvsv.StereoSGBM.create(0, 16, 0, 32716, 0), 640, 480, 1, 3) == 0   # 32717 + 50 = 32767
    # the 64-bit window at the largest block that fits: 21 * 21 * 64 + P2
    assert _validate(mvsv, mvsv.StereoSGBM.create(0, 16, 21, 10, 32767 - 441 * 64), 640, 480, 13, 5) == 0
    assert _validate(mvsv, mvsv.StereoSGBM.create(0, 16, 23, 10, 11), 640, 480, 13, 5) == -1
