"""StereoSGBM MODE_HH4 on the device, bit for bit.

Reference: tests/hh4_restate.py (the twin's pipeline on the clean cost volume and
the four axis directions; valid while no int16 cost wraps, which it asserts).  Every
comparison is a whole-map array_equal; nothing is masked.

The shapes are the smallest at which each kernel form can go wrong: widths and
heights that are no multiple of the lines per block (16 lines of 16 lanes, 32 of 8
for D = 16), of the rows per wave of the final kernels (4, 8, or 2 for D >= 128) or
of the cost tile (16 rows), and more than one block in every direction.
"""
import functools

import numpy as np
import pytest

from tests import hh4_restate as hr

pytestmark = pytest.mark.gpu

HH4 = hr.MODE_HH4


def report(a, b):
    bad = np.argwhere(a != b)
    if bad.size == 0:
        return ""
    pts = [(int(y), int(x), int(a[y, x]), int(b[y, x])) for y, x in bad[:10]]
    return f"{len(bad)} mismatches of {a.size}; first (y, x, gpu, restatement): {pts}"


def matcher(mvsv, p, variant=0):
    m = mvsv.StereoSGBM.create(p["min_disparity"], p["num_disparities"], p["block_size"], p["p1"], p["p2"],
                               p["disp12_max_diff"], p["pre_filter_cap"], p["uniqueness_ratio"],
                               p["speckle_window_size"], p["speckle_range"], p["mode"])
    m.setVariant(variant)
    return m


@pytest.fixture
def schedule(mvsv):
    """set(value): MVSV_OPT_PATH_SCHEDULE for the test, back to 0 afterwards."""
    yield lambda v: mvsv.set_option(mvsv.OPT_PATH_SCHEDULE, v)
    mvsv.set_option(mvsv.OPT_PATH_SCHEDULE, 0)


# ---- the random cases (tests/test_hh4_restate.py: each tells the modes apart) ------
@functools.lru_cache(maxsize=None)
def random_ref(seed):
    L, R, p, variant = hr.random_case(seed)
    return L, R, p, variant, hr.compute(L, R, p, variant)


@pytest.mark.parametrize("seed", hr.RANDOM_SEEDS)
def test_random_small(gpu, mvsv, seed):
    L, R, p, variant, want = random_ref(seed)
    got = matcher(mvsv, p, variant).compute(L, R)
    assert got.dtype == np.int16 and np.array_equal(got, want), f"{p} variant={variant}: " + report(got, want)
    # FIRSTCOL_FIX has no effect in this mode: variants 1 and 3 are 0 and 2
    other = matcher(mvsv, p, variant ^ 1).compute(L, R)
    assert np.array_equal(other, want), f"{p} variant={variant ^ 1}: " + report(other, want)
    assert np.array_equal(hr.compute(L, R, p, variant ^ 1), want)


# ---- one case per kernel form, under every path schedule ---------------------------
# name: (W, H, parameters)
FORMS = {
    "a-packed8-u16": (101, 37, dict(num_disparities=16, block_size=5, p1=200, p2=800, uniqueness_ratio=10)),
    "b-packed8-nibble": (101, 37, dict(num_disparities=16, block_size=3, uniqueness_ratio=5)),
    "c-nibble-residual": (120, 40, dict(num_disparities=32, block_size=9)),
    "d-live-u16": (150, 45, dict(num_disparities=64, block_size=9, p1=648, p2=2592, uniqueness_ratio=10)),
    "e-u8": (150, 45, dict(num_disparities=64, block_size=5, p1=8, p2=40)),
    "f-sgbm-yml": (200, 40, dict(min_disparity=1, num_disparities=128, block_size=13, speckle_window_size=150,
                                 speckle_range=2)),
    "g-u16-d128": (200, 40, dict(num_disparities=128, block_size=13, p1=1352, p2=5408, uniqueness_ratio=5)),
    "h-config5-d256": (300, 24, dict(num_disparities=256, block_size=9, p1=648, p2=2592)),
    "i-generic-d48": (110, 30, dict(num_disparities=48, block_size=5, p1=8, p2=32, uniqueness_ratio=10)),
    "j-generic-d272": (330, 20, dict(num_disparities=272, block_size=3, p1=8, p2=32)),
    "k-general-recurrence": (100, 40, dict(num_disparities=32, block_size=17, p1=2312, p2=9248, uniqueness_ratio=10)),
}


@functools.lru_cache(maxsize=None)
def form_ref(name):
    W, H, kw = FORMS[name]
    p = hr.params(mode=HH4, **kw)
    D = p["num_disparities"]
    L, R = hr.rand_pair(np.random.default_rng(9100 + D + H), H, W, D // 3, 0)
    return L, R, p, hr.compute(L, R, p)


@pytest.mark.parametrize("sched", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(FORMS))
def test_kernel_forms(gpu, mvsv, schedule, name, sched):
    from mvstereovision3_amd import _lib
    L, R, p, want = form_ref(name)
    H, W = L.shape
    m = matcher(mvsv, p)
    schedule(sched)
    bits = _lib.sgbm_plan(_lib.context(0), 1, W, H, m._params)
    # no MODE_HH4 launch is bit-sliced or runs strips, whatever the option says
    assert not bits & (_lib.PLAN_BITSLICE | _lib.PLAN_STRIPS), bits
    D, P2 = p["num_disparities"], max(p["p2"], 5)
    packed = D in (16, 32, 64, 128, 256)
    if sched == 2 and packed:
        assert bits & _lib.PLAN_SIDE
    if sched == 1:
        assert not bits & _lib.PLAN_SIDE
    if sched == 0 and packed:
        assert bits & _lib.PLAN_SIDE  # one small frame: side by side on every plane type
    if name in ("c-nibble-residual", "f-sgbm-yml") and sched != 1:
        assert bits & _lib.PLAN_RESIDUAL
    if name == "k-general-recurrence":
        # an int16 could wrap by the bound, so the general recurrence runs; the costs themselves fit
        bs = p["block_size"]
        assert 2 * P2 + bs * bs * (2 * 15 + 63) > 32767
    got = m.compute(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()).cpu().numpy()
    assert np.array_equal(got, want), f"{name} schedule {sched}: " + report(got, want)


# ---- edge cases ----------------------------------------------------------------------
EDGES = {
    "H1-all-bottom-rows": (90, 1, dict(num_disparities=32, block_size=9)),
    "H3-all-bottom-rows": (90, 3, dict(num_disparities=32, block_size=9, p1=8, p2=32)),
    "H3-d16": (70, 3, dict(num_disparities=16, block_size=9, p1=200, p2=800)),
    "W1-is-SW2+1": (32 + 5, 21, dict(num_disparities=32, block_size=9)),
    "W1-is-SW2+1-d16": (16 + 3, 35, dict(num_disparities=16, block_size=5, p1=200, p2=800)),
    "minD-5": (120, 23, dict(min_disparity=-5, num_disparities=32, block_size=5, p1=8, p2=32)),
    "minD+3": (120, 23, dict(min_disparity=3, num_disparities=64, block_size=5)),
    "uniq15": (120, 23, dict(num_disparities=32, block_size=5, uniqueness_ratio=15)),
    "uniq15-u16": (120, 23, dict(num_disparities=64, block_size=5, p1=72, p2=288, uniqueness_ratio=15)),
    "disp12-1": (120, 23, dict(num_disparities=32, block_size=5, p1=8, p2=32, disp12_max_diff=-1)),
    "disp12+3": (120, 23, dict(num_disparities=32, block_size=5, p1=8, p2=32, disp12_max_diff=3)),
    "bs0": (100, 19, dict(num_disparities=16, block_size=0, p1=8, p2=32)),
    "bs1": (100, 19, dict(num_disparities=64, block_size=1)),
    "odd-H-d128": (190, 33, dict(num_disparities=128, block_size=5, uniqueness_ratio=10)),
    "odd-H-d128-u16": (190, 17, dict(num_disparities=128, block_size=7, p1=392, p2=1568)),
    "odd-H-d256": (300, 9, dict(num_disparities=256, block_size=3)),
}


@functools.lru_cache(maxsize=None)
def edge_ref(name):
    W, H, kw = EDGES[name]
    p = hr.params(mode=HH4, pre_filter_cap=31, **kw)
    L, R = hr.rand_pair(np.random.default_rng(9500 + W + H), H, W, 4, 0 if H > 1 else 2)
    return L, R, p, hr.compute(L, R, p)


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_cases(gpu, mvsv, name):
    L, R, p, want = edge_ref(name)
    got = matcher(mvsv, p).compute(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()).cpu().numpy()
    assert np.array_equal(got, want), f"{name}: " + report(got, want)


def test_host_entry_with_strided_roi_views(gpu, mvsv):
    L, R, p, want = form_ref("e-u8")
    H, W = L.shape
    m = matcher(mvsv, p)
    bigL = np.full((H + 5, W + 11), 77, np.uint8)
    bigR = np.full((H + 3, W + 6), 33, np.uint8)
    bigL[2:2 + H, 7:7 + W] = L
    bigR[1:1 + H, 4:4 + W] = R
    out = np.full((H + 2, W + 3), -12345, np.int16)
    got = m.compute(bigL[2:2 + H, 7:7 + W], bigR[1:1 + H, 4:4 + W], out[1:1 + H, 2:2 + W])
    assert np.array_equal(got, want), report(got, want)
    assert np.shares_memory(got, out) and (out[0] == -12345).all() and (out[:, :2] == -12345).all()
    got = mvsv.Disparity.sgbm(mvsv.Stereopair(bigL[2:2 + H, 7:7 + W], bigR[1:1 + H, 4:4 + W]), None, m)
    assert np.array_equal(got, want), report(got, want)


@pytest.mark.parametrize("variant", [0, 2])
def test_period7_pair_tie_rule(gpu, mvsv, variant):
    L, R, p = hr.period7_pair()
    want = hr.compute(L, R, p, variant)
    assert not np.array_equal(want, hr.compute(L, R, p, variant ^ 2))  # the pair exercises the rule
    got = matcher(mvsv, p, variant).compute(L, R)
    assert np.array_equal(got, want), report(got, want)


@pytest.mark.parametrize("W,H,kw", [
    (120, 40, dict(num_disparities=32, block_size=9)),
    (200, 40, dict(num_disparities=128, block_size=5, p1=8, p2=32, uniqueness_ratio=10)),
], ids=["120x40-D32", "200x40-D128"])
def test_device_batch_of_three_pairs(gpu, mvsv, W, H, kw):
    p = hr.params(mode=HH4, **kw)
    pairs = [hr.rand_pair(np.random.default_rng(9700 + k), H, W, 5 + 3 * k, k) for k in range(3)]
    Ls = gpu.from_numpy(np.stack([a for a, _ in pairs])).cuda()
    Rs = gpu.from_numpy(np.stack([b for _, b in pairs])).cuda()
    got = matcher(mvsv, p).compute(Ls, Rs).cpu().numpy()
    assert got.shape == (3, H, W)
    for k, (L, R) in enumerate(pairs):
        want = hr.compute(L, R, p)
        assert np.array_equal(got[k], want), f"frame {k}: " + report(got[k], want)


def test_colour_pair(gpu, mvsv):
    from mvstereovision3_amd import _lib
    rng = np.random.default_rng(9800)
    H, W = 30, 64
    L = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    L = ((L.astype(int) + np.roll(L, 1, axis=1) + np.roll(L, 2, axis=1)) // 3).astype(np.uint8)
    R = np.clip(np.roll(L, -3, axis=1).astype(int) + rng.integers(-4, 5, L.shape), 0, 255).astype(np.uint8)
    p = hr.params(mode=HH4, num_disparities=32, block_size=5, p1=8, p2=32, uniqueness_ratio=10,
                  speckle_window_size=20, speckle_range=2)
    want = hr.compute_bgr(L, R, p)
    assert not np.array_equal(want, hr.compute(L[:, :, 1], R[:, :, 1], p))  # colour matters to the map
    m = matcher(mvsv, p)
    bits = _lib.sgbm_plan(_lib.context(0), 1, W, H, m._params, channels=3)
    assert not bits & (_lib.PLAN_BITSLICE | _lib.PLAN_STRIPS | _lib.PLAN_RESIDUAL)
    got = m.compute_bgr(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda()).cpu().numpy()
    assert np.array_equal(got, want), report(got, want)
    got = m.compute_bgr(L, R)  # the host entry
    assert np.array_equal(got, want), report(got, want)


def test_mode_3way_is_refused_by_name(gpu, mvsv):
    L, R, p, _ = form_ref("b-packed8-nibble")
    m = matcher(mvsv, dict(p, mode=2))
    with pytest.raises(mvsv.MvsvError, match="MODE_SGBM_3WAY"):
        m.compute(L, R)
    with pytest.raises(mvsv.MvsvError, match="MODE_SGBM_3WAY"):
        m.compute(gpu.from_numpy(L).cuda(), gpu.from_numpy(R).cuda())


# ---- frame streams ---------------------------------------------------------------------
STREAM_W, STREAM_H = 96, 40


def stream_pairs():
    return [hr.rand_pair(np.random.default_rng(9900 + k), STREAM_H, STREAM_W, 4 + k, 0) for k in range(3)]


def test_stream_with_an_hh4_matcher(gpu, mvsv):
    p = hr.params(mode=HH4, num_disparities=32, block_size=5, p1=8, p2=32, uniqueness_ratio=10,
                  speckle_window_size=20, speckle_range=2)
    m = matcher(mvsv, p)
    pairs = stream_pairs()
    st = mvsv.DisparityStream(m, STREAM_W, STREAM_H, depth=3, batch=2)
    try:
        for L, R in pairs:
            st.push(L, R)
        for k, (L, R) in enumerate(pairs):
            d = st.pop()[0]
            one = m.compute(L, R)
            want = hr.compute(L, R, p)
            assert np.array_equal(one, want), f"compute, frame {k}: " + report(one, want)
            assert np.array_equal(d, one), f"stream, frame {k}: " + report(d, one)
    finally:
        st.close()


def test_stream_switches_modes_between_frames(gpu, mvsv):
    from oracle import twin
    base = hr.params(num_disparities=32, block_size=5, p1=8, p2=32, uniqueness_ratio=10)
    pairs = stream_pairs()
    modes = (mvsv.MODE_SGBM, mvsv.MODE_HH4, mvsv.MODE_HH)
    want = []
    for (L, R), mode in zip(pairs, modes):
        p = dict(base, mode=mode)
        want.append(hr.compute(L, R, p) if mode == HH4 else twin.sgbm_compute(L, R, p))
    # each mode's map is its own on these frames
    L1, R1 = pairs[1]
    assert not np.array_equal(want[1], twin.sgbm_compute(L1, R1, dict(base, mode=0)))
    assert not np.array_equal(want[1], twin.sgbm_compute(L1, R1, dict(base, mode=1)))
    st = mvsv.DisparityStream(matcher(mvsv, dict(base, mode=modes[0])), STREAM_W, STREAM_H, depth=3)
    try:
        for (L, R), mode in zip(pairs, modes):
            st.set_params(matcher(mvsv, dict(base, mode=mode)))
            st.push(L, R)
        for k in range(3):
            d = st.pop()[0]
            assert np.array_equal(d, want[k]), f"frame {k} (mode {modes[k]}): " + report(d, want[k])
    finally:
        st.close()
