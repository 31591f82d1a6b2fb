"""Chosen int16 maps for the speckle filter and the 3x3 median (no GPU, pure numpy,
fixed seeds).

The disparity cores only ever hand the post filters large smooth regions with a
few specks.  These maps are built to reach what such inputs never do: one
component through every 32x32 tile, a component whose size lands exactly on
maxSpeckleSize, a tile in which every pixel is its own root, thresholds that sit
exactly on maxDiff, the ends of the int16 range, and every width / height around
the tile size.

Every generator returns ``(map, new_val, max_diff, [max_size, ...])``.  An
exact-size generator counts its component's pixels itself (n) and returns
n - 1 and n as max_size: cv::filterSpeckles removes a component of size <=
maxSpeckleSize, so n - 1 keeps it whole and n removes it whole.  Shapes are given
as (W, H).  tests/test_post_filter_cases.py checks, on the CPU, that each case
can tell a wrong filter from a right one; tests/test_gpu_post_filters.py runs
them on the device.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

# check: what tests/test_post_filter_cases.py demands of the case under the oracle
#   "flip"    sizes are pairs (n - 1, n): each pair flips one whole component of n pixels
#   "noise"   at every size >= 10 % of the valid pixels are removed and >= 10 % kept
#   "noise_sparse" the same at max_size 10, 50 and 200; at 1000 everything is removed (see all_cases)
#   "checker" sizes (0, 1): 0 changes nothing, 1 makes everything new_val
#   "parity"  oracle == twin only
Case = namedtuple("Case", "name check map new_val max_diff sizes")

NOISE_SIZES = [10, 50, 200, 1000]
TWIN_MAX_PIXELS = 35000  # the numpy twin is pure Python


def _valid_count(m, new_val):
    return int(np.count_nonzero(m != new_val))


# ---- one component through every tile ------------------------------------------------
def serpentine(W, H, far_separators=False, value=320, new_val=-16, max_diff=16):
    """Even rows carry `value`; an odd row holds one pixel of it at alternating ends, the
    rest is new_val -- or, far_separators, a value further than max_diff away, so that the
    separators are components of their own (W - 1 pixels each, smaller than the snake)."""
    m = np.full((H, W), value + 10 * max_diff + 7 if far_separators else new_val, np.int16)
    m[0::2] = value
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = value
    n = int(np.count_nonzero(m == value))
    assert n == ((H + 1) // 2) * W + H // 2
    return m, new_val, max_diff, [n - 1, n]


def comb(W, H, transpose=False, value=480, new_val=-16, max_diff=16):
    """Every second column is valid; only the last image row joins them, so the components
    of every tile but the bottom ones are lone columns."""
    m = np.full((H, W), new_val, np.int16)
    m[:, 0::2] = value
    m[H - 1] = value
    n = ((W + 1) // 2) * (H - 1) + W
    assert n == _valid_count(m, new_val)
    if transpose:
        m = np.ascontiguousarray(m.T)
    return m, new_val, max_diff, [n - 1, n]


def spiral(W=97, H=130, value=160, new_val=-16, max_diff=16):
    """One-pixel-wide square spiral from the top-left corner inwards, one pixel of new_val
    between its turns."""
    m = np.full((H, W), new_val, np.int16)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = value
    n = 1

    def free(px, py):
        return 0 <= px < W and 0 <= py < H and m[py, px] == new_val

    def can_go(ddx, ddy):
        # the next pixel is free, and the one after it is not an earlier turn of the spiral
        nx, ny = x + ddx, y + ddy
        ax, ay = nx + ddx, ny + ddy
        return free(nx, ny) and (not (0 <= ax < W and 0 <= ay < H) or m[ay, ax] == new_val)

    while True:
        if not can_go(dx, dy):
            dx, dy = -dy, dx  # turn right (y grows downwards)
            if not can_go(dx, dy):
                break
        x, y = x + dx, y + dy
        m[y, x] = value
        n += 1
    assert n == _valid_count(m, new_val)
    return m, new_val, max_diff, [n - 1, n]


# ---- every pixel its own root ----------------------------------------------------------
def checkerboard(W, H, max_diff=16, new_val=-16):
    """Two values further apart than max_diff: W * H components of one pixel, 1024 roots in
    every full tile.  max_size 0 removes nothing, 1 removes everything."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.where((xx + yy) % 2 == 0, 0, 1000).astype(np.int16)
    return m, new_val, max_diff, [0, 1]


def constant(W, H, max_diff=-1, value=48, new_val=-16):
    """One value everywhere under max_diff = -1: no two pixels connect, although all are equal."""
    return np.full((H, W), value, np.int16), new_val, max_diff, [0, 1]


# ---- near-critical noise ------------------------------------------------------------
def noise(W, H, seed, holes=False, step=16, max_diff=64, new_val=-16, sizes=NOISE_SIZES):
    """16 levels `step` apart, neighbours connected when at most 4 levels apart: a bond
    probability of (16 + 2 * (15 + 14 + 13 + 12)) / 256 = 0.484, just under the square
    lattice's threshold of 1 / 2, so components of every size up to thousands of pixels
    occur.  holes: 10 % of the pixels are new_val."""
    rng = np.random.default_rng(seed)
    m = (rng.integers(0, 16, (H, W)) * step).astype(np.int16)
    if holes:
        m[rng.random((H, W)) < 0.10] = new_val
    return m, new_val, max_diff, list(sizes)


def noise_unscaled(W, H, seed):
    """The same statistics with a max_diff that is no multiple of 16 (StereoBM passes
    speckleRange unscaled): levels 5 apart, 4 levels = 20 <= 22 < 25 = 5 levels."""
    m, new_val, _, sizes = noise(W, H, seed, step=5)
    return (m + 1).astype(np.int16), new_val, 22, sizes


# ---- thresholds and the ends of the range --------------------------------------------
def threshold(at_tile_edge, transpose=False, max_diff=37, new_val=-16):
    """Three bands along x: the step that is exactly max_diff connects, the one of
    max_diff + 1 does not.  at_tile_edge: the exact step lies on the tile edge x = 31 | 32
    and the larger one inside the tile, otherwise the other way round."""
    W, H = 40, 5
    m = np.zeros((H, W), np.int16)
    if at_tile_edge:
        m[:, 32:35] = max_diff
        m[:, 35:] = 2 * max_diff + 1
        a, b = 35 * H, 5 * H  # bands 0 + 1 | band 2
    else:
        m[:, 32:37] = max_diff + 1
        m[:, 37:] = 2 * max_diff + 1
        a, b = 32 * H, 8 * H  # band 0 | bands 1 + 2
    if transpose:
        m = np.ascontiguousarray(m.T)
    return m, new_val, max_diff, sorted([a - 1, a, b - 1, b])


def ramp(new_val, W=203, H=3):
    """0, 1, 2, ... along every row with max_diff = 1: connected end to end although the
    ends differ by W - 1.  Pixels equal to new_val (new_val = 0: the first column) drop out."""
    m = np.tile(np.arange(W, dtype=np.int16), (H, 1))
    n = _valid_count(m, new_val)
    return m, new_val, 1, [n - 1, n]


def extremes(max_diff, new_val):
    """-32768 beside 32767 in four blocks (split at the tile edge x = 32 and inside the tile
    at y = 20).  max_diff 65535 joins them all, 65534 none; new_val = 32767 takes two of the
    blocks out.  The block sizes are pairwise different."""
    W, H = 40, 41
    m = np.full((H, W), -32768, np.int16)
    m[:20, 32:] = 32767
    m[20:, :32] = 32767
    blocks = {"tl": 32 * 20, "tr": 8 * 20, "bl": 32 * 21, "br": 8 * 21}
    if new_val == 32767:
        ns = [blocks["tl"], blocks["br"]]
    elif max_diff >= 65535:
        ns = [W * H]
    else:
        ns = list(blocks.values())
    return m, new_val, max_diff, sorted(s for n in ns for s in (n - 1, n))


# ---- every width and height around the tile size -------------------------------------
SHAPES = [(1, 1), (1, 65), (65, 1), (2, 2), (2, 33), (33, 2), (32, 32), (33, 33), (31, 64), (64, 31),
          (63, 65), (65, 63), (64, 64)]  # (W, H)


def shape_noise(W, H):
    return noise(W, H, seed=9000 + 100 * W + H, sizes=[10])


@lru_cache(maxsize=None)
def all_cases():
    """Every case, built once; the maps are read-only."""
    cs = []

    def add(name, check, gen):
        m, new_val, max_diff, sizes = gen
        m = np.ascontiguousarray(m, np.int16)
        m.setflags(write=False)
        cs.append(Case(name, check, m, int(new_val), int(max_diff), [int(s) for s in sizes]))

    for W, H in ((167, 203), (64, 64), (33, 65)):
        add(f"serpentine_{W}x{H}", "flip", serpentine(W, H))
        add(f"serpentine_far_{W}x{H}", "flip", serpentine(W, H, far_separators=True))
    for W, H in ((167, 203), (65, 33)):
        add(f"comb_{W}x{H}", "flip", comb(W, H))
        add(f"comb_t_{W}x{H}", "flip", comb(W, H, transpose=True))
    add("spiral_97x130", "flip", spiral())
    for W, H in ((167, 203), (64, 64)):
        add(f"checker_{W}x{H}", "checker", checkerboard(W, H))
        add(f"checker_negdiff_{W}x{H}", "checker", checkerboard(W, H, max_diff=-1))
    add("constant_negdiff_33x33", "checker", constant(33, 33))
    for (W, H), holes_seed in (((167, 203), 183), ((97, 130), 251)):
        add(f"noise_{W}x{H}", "noise", noise(W, H, seed=2))
        # 10 % holes take the lattice well below its threshold.  At max_diff = 64 the oracle leaves
        # no component above 1000 pixels at these shapes (all removed with each of the seeds
        # 0..399), and components above 200 pixels hold >= 10 % of the valid pixels with few seeds
        # only (7 of 400 at 167x203, 34 of 400 at 97x130): the seeds are the ones that keep most
        # at 200 (0.877 and 0.827 removed).  So this form has both outcomes at max_size 10, 50 and
        # 200; with five levels connected (bond probability 0.57) it has them at all four sizes
        add(f"noise_holes_{W}x{H}", "noise_sparse", noise(W, H, seed=holes_seed, holes=True))
        add(f"noise_holes_md80_{W}x{H}", "noise", noise(W, H, seed=5, holes=True, max_diff=80))
    add("noise_unscaled_97x130", "noise", noise_unscaled(97, 130, seed=3))
    for edge in (True, False):
        for t in (False, True):
            add(f"threshold_{'edge' if edge else 'inner'}{'_t' if t else ''}", "flip", threshold(edge, t))
    for nv in (-16, 0, 32767):
        add(f"ramp_newval_{nv}", "flip", ramp(nv))
    add("extremes_65535", "flip", extremes(65535, 0))
    add("extremes_65534", "flip", extremes(65534, 0))
    add("extremes_newval_32767", "flip", extremes(65534, 32767))
    for W, H in SHAPES:
        add(f"shape_{W}x{H}", "parity", shape_noise(W, H))
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


def case(name):
    return next(c for c in all_cases() if c.name == name)


def case_sizes():
    """(case name, max_size) of every case: the parametrisation of the tests."""
    return [(c.name, s) for c in all_cases() for s in c.sizes]


# ---- median inputs ------------------------------------------------------------------
MEDIAN_SHAPES = [(H, W) for W, H in SHAPES] + [(5, 2), (2, 5), (37, 130), (37, 131)]  # (H, W)


def median_map(H, W, kind, seed=0):
    """kind "full": uniform over all of int16; "corners": only {-32768, -16, 0, 32767}."""
    rng = np.random.default_rng(5000 + 1000 * seed + 10 * H + W)
    if kind == "full":
        return rng.integers(-32768, 32768, (H, W)).astype(np.int16)
    return np.array([-32768, -16, 0, 32767], np.int16)[rng.integers(0, 4, (H, W))]
