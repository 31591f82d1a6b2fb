"""numpy restatement of the camera set-up primitives, written from the formulas
in include/mvsv.h (not from the C code): the focus measure of
Utility::checkSharpness and the maps / remap of cv::undistort.

    sum4(img, roi)            S4: the two integer 3x3 kernels on the reflect-padded parent
    sharpness(img, roi)       (S4 / 4.0) * (1.0 / N), cv::mean's double
    undistort_maps(...)       cv::undistort's CV_16SC2 + CV_16UC1 stripe maps, float64
    near_ties(...)            how many entries of those maps sit within eps of a rounding tie
    remap_fixed(src, xy, frac) cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on such maps
"""
import numpy as np

KX = np.outer([1, 2, 1], [-1, 2, -1]).astype(np.int64)   # 4 Lx: kernelX = M along x, kernelY = G along y
KY = np.outer([-1, 2, -1], [1, 2, 1]).astype(np.int64)   # 4 Ly


def _roi(img, roi):
    h, w = img.shape
    return (0, 0, w, h) if roi is None else tuple(int(v) for v in roi)


def responses(img, roi=None):
    """(KX (*) s, KY (*) s) over the roi, s the BORDER_REFLECT_101 extension of the
    parent image (np.pad's "reflect"; an axis of length 1 repeats its only element)."""
    img = np.asarray(img)
    assert img.ndim == 2 and img.dtype == np.uint8
    x0, y0, x1, y1 = _roi(img, roi)
    P = np.pad(img.astype(np.int64), 1, mode="reflect")
    rx = np.zeros((y1 - y0, x1 - x0), np.int64)
    ry = np.zeros_like(rx)
    for dy in range(3):
        for dx in range(3):
            win = P[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            rx += KX[dy, dx] * win
            ry += KY[dy, dx] * win
    return rx, ry


def sum4(img, roi=None) -> int:
    rx, ry = responses(img, roi)
    return int(np.abs(rx).sum() + np.abs(ry).sum())


def value_of(s4: int, n: int) -> float:
    """cv::mean: sum * (1.0 / N) -- a reciprocal and a product, each rounded."""
    return float((np.float64(s4) / np.float64(4.0)) * (np.float64(1.0) / np.float64(n)))


def sharpness(img, roi=None) -> float:
    x0, y0, x1, y1 = _roi(np.asarray(img), roi)
    return value_of(sum4(img, roi), (x1 - x0) * (y1 - y0))


def separable_float64(img, roi=None) -> float:
    """The literal transcription of the reference: sepFilter2D's row filter, then its
    column filter, in float64, |.|, sum -- times 4.  Exact: every value is a multiple
    of 0.25 far below 2^53."""
    img = np.asarray(img)
    x0, y0, x1, y1 = _roi(img, roi)
    P = np.pad(img.astype(np.float64), 1, mode="reflect")
    M = np.array([-1.0, 2.0, -1.0])
    G = np.array([0.25, 0.5, 0.25])

    def sep(kx, ky):
        rows = kx[0] * P[:, 0:-2] + kx[1] * P[:, 1:-1] + kx[2] * P[:, 2:]       # along x, every padded row
        full = ky[0] * rows[0:-2] + ky[1] * rows[1:-1] + ky[2] * rows[2:]       # along y
        return full[y0:y1, x0:x1]

    fm = np.abs(sep(M, G)) + np.abs(sep(G, M))
    return float(fm.sum() * 4.0)


def _stripe_uv(K, k, Ar, W, rows):
    """initUndistortRectifyMap's doubles (u, v) for `rows` rows of width W with R = I
    and new camera matrix Ar: the inverse by cofactors, then the walk along a row by
    repeated addition (cumsum adds one element after the other)."""
    a, b, c, d, e, f, g, h, i = (np.float64(v) for v in np.asarray(Ar, np.float64).reshape(9))
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    ir = [(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
          (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
          (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det]
    row = np.arange(rows, dtype=np.float64)[:, None]

    def walk(c_row, c_one, c_col):
        first = row * c_row + c_one
        return np.cumsum(np.concatenate([first, np.full((rows, W - 1), c_col)], axis=1), axis=1)

    _x, _y, _w = walk(ir[1], ir[2], ir[0]), walk(ir[4], ir[5], ir[3]), walk(ir[7], ir[8], ir[6])
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    fx, fy, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    w = 1.0 / _w
    x, y = _x * w, _y * w
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0
    v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0
    return u, v


def undistort_uv32(K, dist, new_K, W, H):
    """(u * 32, v * 32) of cv::undistort's stripes, float64 (H, W) each."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    A = K if new_K is None else np.asarray(new_K, np.float64).reshape(3, 3)
    k = np.zeros(8)
    d = np.asarray([] if dist is None else dist, np.float64).reshape(-1)
    assert d.size in (0, 4, 5, 8)
    k[:d.size] = d
    stripe = min(max(1, 4096 // W), H)
    U, V = np.empty((H, W)), np.empty((H, W))
    for y0 in range(0, H, stripe):
        rows = min(stripe, H - y0)
        Ar = A.copy()
        Ar[1, 2] = A[1, 2] - y0
        u, v = _stripe_uv(K, k, Ar, W, rows)
        U[y0:y0 + rows], V[y0:y0 + rows] = u * 32, v * 32
    return U, V


def undistort_maps(K, dist, new_K, W, H):
    """(xy int16 (H, W, 2), frac uint16 (H, W)): iu = cvRound(u * 32) (half to even),
    xy = plain short casts of iu >> 5, iv >> 5, frac = (iv & 31) * 32 + (iu & 31)."""
    U, V = undistort_uv32(K, dist, new_K, W, H)
    iu, iv = np.rint(U).astype(np.int64), np.rint(V).astype(np.int64)
    xy = np.stack([(iu >> 5).astype(np.int16), (iv >> 5).astype(np.int16)], axis=2)
    frac = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return xy, frac


def near_ties(K, dist, new_K, W, H, eps=1e-6):
    """Boolean (H, W): u * 32 or v * 32 lies within eps of a rounding tie (x.5)."""
    U, V = undistort_uv32(K, dist, new_K, W, H)
    return (np.abs(U - np.floor(U) - 0.5) < eps) | (np.abs(V - np.floor(V) - 0.5) < eps)


def remap_fixed(src, xy, frac):
    """cv::remap with CV_16SC2 / CV_16UC1 maps, INTER_LINEAR, BORDER_CONSTANT 0, CV_8UC1:
    weights (32-ay)(32-ax)*32 ... (sum 2^15), out = (sum + 2^14) >> 15; taps outside the
    source read 0."""
    src = np.asarray(src)
    sh, sw = src.shape
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    fr = frac.astype(np.int64) & 1023
    ax, ay = fr & 31, fr >> 5
    P = np.zeros((sh + 2, sw + 2), np.int64)  # a zero frame: index + 1
    P[1:-1, 1:-1] = src

    def tap(x, y):
        ok = (x >= -1) & (x <= sw) & (y >= -1) & (y <= sh)
        return np.where(ok, P[np.clip(y, -1, sh) + 1, np.clip(x, -1, sw) + 1], 0)

    acc = (tap(sx, sy) * ((32 - ay) * (32 - ax) * 32) + tap(sx + 1, sy) * ((32 - ay) * ax * 32) +
           tap(sx, sy + 1) * (ay * (32 - ax) * 32) + tap(sx + 1, sy + 1) * (ay * ax * 32))
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)
