"""Plain numpy restatement of the detection view: what the reference's detection
programs show per frame (trgt/demo.cpp:280-298),

    cv::normalize(dMap, norm, 0, 255, NORM_MINMAX, CV_8U); cv::cvtColor(GRAY2BGR);
    View::drawSubimageGrid / View::drawObstacleGrid          (src/view.cpp)
    drawFoundObstacles                                       (filled tiles / circles)

painted the way OpenCV paints it: layer after layer, each over what is there, by
slice assignment.  A restatement of OpenCV 3.4's cv::line (thickness 1, axis
parallel), filled cv::rectangle (both corners included) and filled cv::circle
(drawing.cpp Circle(), the non-antialiased path), not pinned against cv2.

The `miss` variants are the mistakes a gather kernel can fall into.  MISSES are
the ones a pixel can show: rectangles with an exclusive br, the grids drawn
over the found obstacles (blue over red), and grid lines that stop one row or
column short.  "tiles_over_circles" swaps the two found layers; both are
(0, 0, 255) in the reference (trgt/demo.cpp:119,126), so that order cannot show
in any pixel -- it is offered so that a test can say so.
"""
import numpy as np

from tests import display_restate

SUBIMAGE_GRID, OBSTACLE_GRID, FOUND_TILES, FOUND_POINTS = 1, 2, 4, 8
ALL = 15
BLUE = (100, 0, 0)
RED = (0, 0, 255)
MISSES = ("exclusive_br", "grids_over_found", "short_lines")
INVISIBLE_MISSES = ("tiles_over_circles",)


def layout(W, H):
    """(step_x, step_y, nx, ny) of SamplepointDetection's lattice (src/SamplePointDetection.cpp:38-47)."""
    dX, dY = W // 8, H // 8
    return (W // dX if dX else 0, H // dY if dY else 0, max(dX - 1, 0), max(dY - 1, 0))


def circle_spans(radius):
    """Circle() for a centre far from every border: {row offset: half-width} of the filled spans."""
    spans = {}

    def fill(dy, dx):
        for s in (-dy, dy):
            spans[s] = max(spans.get(s, -1), dx)
    err, dx, dy, plus, minus = 0, radius, 0, 1, 2 * radius - 1
    while dx >= dy:
        fill(dy, dx)
        fill(dx, dy)
        dy += 1
        err += plus
        plus += 2
        mask = (1 if err <= 0 else 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return spans


def half_widths(radius):
    s = circle_spans(radius)
    assert sorted(s) == list(range(-radius, radius + 1)) and all(s[k] == s[-k] for k in s)
    return [s[k] for k in range(radius + 1)]


def found(v, rng):
    """value < first && value > second in float32; a NaN bound finds nothing."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return (v < np.float32(rng[0])) & (v > np.float32(rng[1]))


def paint(img, layers, means=None, mean_range=(0, 0), values=None, sample_range=(0, 0), radius=3, miss=None):
    """The layers over the BGR image img (H, W, 3), in place, in drawing order."""
    assert miss is None or miss in MISSES + INVISIBLE_MISSES
    H, W = img.shape[:2]
    short = 1 if miss == "short_lines" else 0

    def lines(xs, ys, colour):
        for c in xs:  # cv::line((c, 0), (c, H)) clipped: column c in every row
            if c < W:
                img[:H - short, c] = colour
        for r in ys:
            if r < H:
                img[r, :W - short] = colour

    def tiles():
        dx, dy = W // 9, H // 9
        f = found(means, mean_range).reshape(81)
        edge = 0 if miss == "exclusive_br" else 1
        for i in np.flatnonzero(f):
            c, r = i % 9, i // 9
            img[r * dy:r * dy + dy + edge, c * dx:c * dx + dx + edge] = RED  # slices clip at the border

    def circles():
        sx, sy, nx, ny = layout(W, H)
        if nx * ny == 0:
            return
        f = found(values, sample_range).reshape(nx, ny)  # point (c, r) at (c - 1) * ny + (r - 1)
        spans = circle_spans(radius)
        for c, r in np.argwhere(f) + 1:
            cx, cy = c * sx, r * sy
            for off, h in spans.items():
                assert 0 <= cy + off < H and 0 <= cx - h and cx + h < W  # never clipped
                img[cy + off, cx - h:cx + h + 1] = RED

    def subimage_grid():
        x, y = W // 9, H // 9
        lines([x * k for k in (1, 2, 4, 5, 7, 8)], [y * k for k in (1, 2, 4, 5, 7, 8)], BLUE)

    def obstacle_grid():
        x, y = W // 3, H // 3
        lines([x, 2 * x], [y, 2 * y], RED)

    order = [(SUBIMAGE_GRID, subimage_grid), (OBSTACLE_GRID, obstacle_grid), (FOUND_TILES, tiles),
             (FOUND_POINTS, circles)]
    if miss == "tiles_over_circles":
        order = [order[0], order[1], order[3], order[2]]
    if miss == "grids_over_found":
        order = [order[2], order[3], order[0], order[1]]
    for bit, draw in order:
        if layers & bit:
            draw()
    return img


def view(d, layers, means=None, mean_range=(0, 0), values=None, sample_range=(0, 0), radius=3, alpha=0.0, beta=255.0,
         miss=None):
    """(BGR image (H, W, 3) uint8, (smin, smax)) of one int16 map."""
    base, mm = display_restate.normalize(d, alpha, beta)
    img = np.repeat(base[:, :, None], 3, axis=2)
    return paint(img, layers, means, mean_range, values, sample_range, radius, miss), mm


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------
MEAN_RANGE = (500.0, 100.0)     # found: 100 < mean < 500
SAMPLE_RANGE = (800.0, 200.0)


SHAPES = [(63, 47),     # 9 * dx == W: tile 8's br is clipped
          (100, 70),    # a remainder column that tile 8's inclusive edge reaches
          (127, 31),    # lattice steps 8 and 10
          (17, 16),     # one lattice point
          (15, 9),      # no lattice
          (2072, 48),   # a row longer than one pass of a wave
          (24, 1500)]   # more rows than blocks x waves


def host_map(W, H, seed=0):
    """Values 100..1999 with zeros and SGBM's invalid marker -16 sprinkled in."""
    rng = np.random.default_rng(9000 + seed + W * 7 + H)
    d = rng.integers(100, 2000, (H, W)).astype(np.int16)
    d[rng.random((H, W)) < 0.1] = -16
    d[rng.random((H, W)) < 0.05] = 0
    return d


def all_layers_case(W, H, seed=0):
    """(map, keyword arguments of view()) of the all-layers input of a shape."""
    return host_map(W, H, seed), dict(layers=ALL, means=checker_means(seed), mean_range=MEAN_RANGE,
                                      values=edge_values(W, H, seed), sample_range=SAMPLE_RANGE)


def checker_means(phase=0):
    """81 means, found and not found in a checkerboard: with phase 0 the corner tiles 0, 8, 72, 80 are found."""
    i = np.arange(81)
    f = ((i % 9) + (i // 9) + phase) % 2 == 0
    return np.where(f, 300.0, 700.0).astype(np.float32)


def edge_values(W, H, phase=0):
    """Lattice values with found points in the first and last lattice row and column
    and at two direct neighbours in the middle (where the lattice has them)."""
    _, _, nx, ny = layout(W, H)
    v = np.full((max(nx, 0), max(ny, 0)), 1000.0, np.float32)
    if nx * ny == 0:
        return v.reshape(-1)
    v[0, :] = 400.0
    v[-1, :] = 400.0
    v[::2, 0] = 400.0
    v[(1 + phase) % 2::2, -1] = 400.0
    if nx > 3 and ny > 2:
        v[nx // 2, ny // 2] = 400.0
        v[nx // 2 + 1, ny // 2] = 400.0
        v[nx // 2, ny // 2 - 1] = 400.0
    return v.reshape(-1)
