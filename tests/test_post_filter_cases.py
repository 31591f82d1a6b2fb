"""The cases of tests/post_filter_cases.py, checked on the CPU (no GPU).

A case that cannot tell a wrong speckle filter from a right one fails here, before
anyone looks at a GPU result: the C oracle (raster flood fill) must agree with the
numpy twin (union-find) on every case at every max_size, and under the oracle alone
the exact-size pairs must flip one whole component, the noise cases must have both
outcomes well represented and the checkerboards must do what they state."""
import numpy as np
import pytest

from tests import post_filter_cases as pfc

CASES = pfc.all_cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def results(oracle):
    """{(case name, max_size): oracle result}, computed once."""
    return {(c.name, s): oracle.filter_speckles(c.map, c.new_val, s, c.max_diff) for c in CASES for s in c.sizes}


def test_case_list_is_what_the_gpu_tests_expect():
    assert len(CASES) >= 40
    assert {c.check for c in CASES} == {"flip", "noise", "noise_sparse", "checker", "parity"}
    for c in CASES:
        assert c.map.dtype == np.int16 and c.map.ndim == 2 and not c.map.flags.writeable
        assert -32768 <= c.new_val <= 32767 and c.sizes
        if c.check == "flip":
            assert len(c.sizes) % 2 == 0 and all(b == a + 1 for a, b in zip(c.sizes[::2], c.sizes[1::2]))
    # the shapes that must be there
    shapes = {c.map.shape for c in CASES if c.check == "parity"}
    assert {(1, 1), (65, 1), (1, 65), (32, 32), (33, 33)} <= shapes and len(shapes) >= 12
    assert len(pfc.MEDIAN_SHAPES) == len(set(pfc.MEDIAN_SHAPES))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_equals_twin(results, c):
    from oracle import twin
    assert c.map.size <= pfc.TWIN_MAX_PIXELS
    ok, size = twin.speckle_components(c.map, c.new_val, c.max_diff)
    assert np.array_equal(ok, c.map != c.new_val)
    for s in c.sizes:
        want = np.where(ok & (size <= s), c.new_val, c.map).astype(np.int16)
        got = results[c.name, s]
        assert np.array_equal(got, want), f"max_size {s}: {np.count_nonzero(got != want)} pixels differ"


def test_twin_components_are_the_twin_filter():
    from oracle import twin
    c = pfc.case("shape_33x33")
    ok, size = twin.speckle_components(c.map, c.new_val, c.max_diff)
    want = np.where(ok & (size <= 10), c.new_val, c.map).astype(np.int16)
    assert np.array_equal(twin.filter_speckles(c.map, c.new_val, 10, c.max_diff), want)


@pytest.mark.parametrize("c", [c for c in CASES if c.check == "flip"], ids=lambda c: c.name)
def test_exact_size_pairs_flip_one_whole_component(results, c):
    for below, n in zip(c.sizes[::2], c.sizes[1::2]):
        kept, gone = results[c.name, below], results[c.name, n]
        flipped = kept != gone
        assert np.count_nonzero(flipped) == n, f"max_size {below} -> {n} flips {np.count_nonzero(flipped)} pixels"
        assert np.array_equal(kept[flipped], c.map[flipped])  # n - 1: kept whole
        assert np.all(gone[flipped] == c.new_val)             # n: removed whole
        assert np.all(c.map[flipped] != c.new_val)


@pytest.mark.parametrize("name", ["serpentine_167x203", "serpentine_64x64", "serpentine_33x65", "comb_167x203",
                                  "comb_t_167x203", "comb_65x33", "comb_t_65x33", "spiral_97x130", "ramp_newval_-16",
                                  "ramp_newval_0", "ramp_newval_32767", "extremes_65535"])
def test_single_component_cases_are_one_component(results, name):
    """All valid pixels of these maps are one component: kept whole at n - 1, and nothing left at n."""
    c = pfc.case(name)
    below, n = c.sizes
    assert n == np.count_nonzero(c.map != c.new_val)
    assert np.array_equal(results[name, below], c.map)
    assert np.all(results[name, n] == c.new_val)


def test_single_component_cases_reach_every_tile():
    for name in ("serpentine_167x203", "serpentine_far_167x203", "comb_167x203", "comb_t_167x203", "spiral_97x130"):
        c = pfc.case(name)
        H, W = c.map.shape
        value = c.map[0, 0]
        for y0 in range(0, H, 32):
            for x0 in range(0, W, 32):
                assert np.any(c.map[y0:y0 + 32, x0:x0 + 32] == value), f"{name}: tile ({x0}, {y0})"


def test_serpentine_separators_are_components_of_their_own(oracle):
    c = pfc.case("serpentine_far_167x203")
    H, W = c.map.shape
    far = c.map != c.map[0, 0]
    assert np.count_nonzero(far) == (H // 2) * (W - 1) and not np.any(c.map == c.new_val)
    # W - 2 keeps the separators and the snake, W - 1 removes the separators only
    keep = oracle.filter_speckles(c.map, c.new_val, W - 2, c.max_diff)
    drop = oracle.filter_speckles(c.map, c.new_val, W - 1, c.max_diff)
    assert np.array_equal(keep, c.map)
    assert np.all(drop[far] == c.new_val) and np.array_equal(drop[~far], c.map[~far])


@pytest.mark.parametrize("c", [c for c in CASES if c.check in ("noise", "noise_sparse")], ids=lambda c: c.name)
def test_noise_cases_have_both_outcomes(results, c):
    """>= 10 % of the valid pixels removed and >= 10 % kept at every max_size.

    The form with 10 % holes at max_diff = 64 ("noise_sparse") meets this at max_size 10,
    50 and 200 (its seeds are chosen for 200, see post_filter_cases.all_cases) but cannot
    at 1000: the holes take the lattice below its threshold, and at these shapes the
    oracle removes every valid pixel at 1000 with each of the seeds 0..399.  At 1000 it
    is held to the removed share only; the holes form with five levels connected
    (max_diff = 80) is held to both bounds at all four sizes."""
    assert c.sizes == pfc.NOISE_SIZES
    valid = c.map != c.new_val
    nvalid = np.count_nonzero(valid)
    assert nvalid >= 0.85 * c.map.size
    if "holes" in c.name:
        assert 0.08 <= 1 - nvalid / c.map.size <= 0.12
    for s in c.sizes:
        removed = np.count_nonzero(valid & (results[c.name, s] == c.new_val))
        frac = removed / nvalid
        print(f"{c.name} max_size {s}: {frac:.3f} of the valid pixels removed")
        hi = 1.0 if c.check == "noise_sparse" and s == 1000 else 0.90
        assert 0.10 <= frac <= hi, f"max_size {s}: {frac:.3f} removed"
        kept = valid & (results[c.name, s] != c.new_val)
        assert np.array_equal(results[c.name, s][kept], c.map[kept])


@pytest.mark.parametrize("c", [c for c in CASES if c.check == "checker"], ids=lambda c: c.name)
def test_checkerboards_do_what_is_stated(results, c):
    assert c.sizes == [0, 1] and not np.any(c.map == c.new_val)
    assert np.array_equal(results[c.name, 0], c.map)
    assert np.all(results[c.name, 1] == c.new_val)
    if c.max_diff >= 0 and c.name.startswith("checker"):  # the two values are further apart than max_diff
        v = np.unique(c.map)
        assert len(v) == 2 and int(v[1]) - int(v[0]) > c.max_diff


def test_threshold_cases_sit_on_max_diff():
    for name, step_at in (("threshold_edge", (31, 34)), ("threshold_inner", (36, 31))):
        c = pfc.case(name)
        row = c.map[0].astype(int)
        exact, above = step_at
        assert row[exact + 1] - row[exact] == c.max_diff and row[above + 1] - row[above] == c.max_diff + 1
        assert c.max_diff % 16 != 0
        assert np.array_equal(pfc.case(name + "_t").map, c.map.T)


def test_median_maps_cover_the_range():
    full = pfc.median_map(37, 131, "full")
    assert full.min() < -32000 and full.max() > 32000
    corners = pfc.median_map(37, 131, "corners")
    assert set(np.unique(corners)) == {-32768, -16, 0, 32767}
    assert np.array_equal(full, pfc.median_map(37, 131, "full"))
