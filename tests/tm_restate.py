"""Numpy restatement of Disparity::tm (src/disparity.cpp:25-58; include/mvsv.h,
DESIGN.md §4n) in exact integers, and a brute force written straight from the
reference's loops with Fraction scores.  Shared by the CPU and GPU tests.

tm(): shift-major.  For a shift x the products L(y, c) * R(y, c + x) are box-summed
over k x k (N_x at every template position at once), the squared right image is
box-summed once (sum S^2 of every window), and the running best (N, sum S^2, x) of
every pixel is updated where N_x^2 * SS_b > N_b^2 * SS_x -- in Python integers
(object arrays): the products reach 2^78."""
from fractions import Fraction

import numpy as np


def _box(a, k):
    """Sums over every k x k window of a 2-D int64 array: (h - k + 1, w - k + 1)."""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def tm_index(left, right, k):
    """(H, W) int64: the unwrapped arg-max shift of every pixel, 0 where none is written."""
    L = np.asarray(left).astype(np.int64)
    R = np.asarray(right).astype(np.int64)
    assert L.ndim == 2 and L.shape == R.shape
    H, W = L.shape
    assert 1 <= k <= 31 and k < min(H, W)
    hh, ww = H - k, W - k  # template positions i < hh, j < ww
    ss = _box(R * R, k)  # ss[i, r]: the window of R at (i, r)
    best_n = np.zeros((hh, ww), object)  # a score of 0 ...
    best_s = np.ones((hh, ww), object)   # ... (N = 0, SS = 1) ...
    best_x = np.zeros((hh, ww), np.int64)  # ... at x = 0
    for x in range(0, W - k):  # column j has the shifts x < W - j - k
        nj = W - k - x  # the columns j < nj have this shift
        n = _box(L[:, :nj + k - 1] * R[:, x:x + nj + k - 1], k)[:hh, :nj].astype(object)
        s = ss[:hh, x:x + nj].astype(object)
        s = np.where(s == 0, 1, s)  # a window of zeros: N = 0, SS = 1
        bn, bs = best_n[:, :nj], best_s[:, :nj]
        win = (n * n * bs) > (bn * bn * s)
        bn[win] = n[win]
        bs[win] = s[win]
        best_x[:, :nj][win] = x
    out = np.zeros((H, W), np.int64)
    out[:hh, :ww] = best_x
    return out


def tm(left, right, k, wide=False):
    """The map Disparity::tm stores: uint8, the shift truncated to 8 bits
    (output.at<char>); wide: the shift itself as uint16."""
    idx = tm_index(left, right, k)
    return idx.astype(np.uint16) if wide else (idx & 0xFF).astype(np.uint8)


def tm_brute(left, right, k):
    """src/disparity.cpp:39-56 as written: per pixel, the template, the search strip
    of width cols - j - 1, one CCORR_NORMED score per position as a Fraction of the
    squared score (N^2 / (sum T^2 * sum S^2); N >= 0, so the order is the score's),
    0 where the denominator is 0, and minMaxLoc's first maximum."""
    L = [[int(v) for v in row] for row in np.asarray(left)]
    R = [[int(v) for v in row] for row in np.asarray(right)]
    rows, cols = len(L), len(L[0])
    out = np.zeros((rows, cols), np.uint8)
    for i in range(rows - k):
        for j in range(cols - k):
            T = [L[i + y][j:j + k] for y in range(k)]
            dest_width = cols - j - 1
            strip = [R[i + y][j:j + dest_width] for y in range(k)]
            tt = sum(v * v for row in T for v in row)
            best, loc = None, 0
            for x in range(dest_width - k + 1):
                n = sum(T[y][c] * strip[y][x + c] for y in range(k) for c in range(k))
                s2 = sum(strip[y][x + c] ** 2 for y in range(k) for c in range(k))
                score = Fraction(n * n, tt * s2) if tt * s2 else Fraction(0)
                if best is None or score > best:
                    best, loc = score, x
            out[i, j] = loc & 0xFF
    return out
