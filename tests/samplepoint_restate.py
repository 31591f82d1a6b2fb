"""Plain-loop restatement of SamplepointDetection (src/SamplePointDetection.cpp:29-178,
inc/Samplepoint.h:17-40, Utility::calcMeanDisparity src/utility.cpp:265-285), shared by
the sample point tests.  Deliberately a double loop over c and r, not vectorised the
way the product is."""
import numpy as np


def layout(W, H):
    """(step_x, step_y, nx, ny) of a W x H map."""
    dX, dY = W // 8, H // 8
    return (W // dX if dX else 0, H // dY if dY else 0, max(dX - 1, 0), max(dY - 1, 0))


def centres(W, H):
    """[(cx, cy)] in the reference's order: c outside, r inside."""
    dX, dY = W // 8, H // 8
    out = []
    for c in range(1, dX):
        for r in range(1, dY):
            out.append((c * (W // dX), r * (H // dY)))
    return out


def values(dmap, radius):
    """float32 value of every lattice point of a 2-D int16 map."""
    H, W = dmap.shape
    out = []
    for cx, cy in centres(W, H):
        if radius > 0:
            total = count = 0
            for y in range(cy - radius, cy + radius + 1):
                for x in range(cx - radius, cx + radius + 1):
                    v = int(dmap[y, x])
                    if v > 1:
                        total += v
                        count += 1
            out.append(0.0 if total == 0 or count == 0 else float(total // count))
        else:
            out.append(float(dmap[cy, cx]))
    return np.array(out, np.float32)


def hits(vals, first, second):
    """indices of the points with value < first && value > second (float32 compares)."""
    first, second = np.float32(first), np.float32(second)
    return [i for i, v in enumerate(np.asarray(vals, np.float32)) if v < first and v > second]


def make_map(rng, H, W):
    """int16 map with the cases the value rule distinguishes: -16 (invalid), 0, 1, 2,
    small positives whose total / count truncates, 32767, and 5x5 patches (and their
    surroundings) with no value > 1."""
    d = rng.choice(np.array([-16, 0, 1, 2, 3, 5, 7, 10, 100, 333, 1999, 32767], np.int16), size=(H, W),
                   p=[.15, .05, .05, .1, .1, .1, .1, .1, .1, .05, .05, .05]).astype(np.int16)
    cs = centres(W, H)
    for k, (cx, cy) in enumerate(cs):
        if k % 7 == 3:  # nothing > 1 in reach of radius 3
            d[max(cy - 3, 0):cy + 4, max(cx - 3, 0):cx + 4] = rng.choice(np.array([-16, 0, 1], np.int16),
                                                                         size=d[max(cy - 3, 0):cy + 4,
                                                                                max(cx - 3, 0):cx + 4].shape)
        elif k % 7 == 5:  # negative centre: radius 0 keeps it
            d[cy, cx] = -16
    return d
