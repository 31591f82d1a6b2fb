"""Numpy restatement of the grey pair preparation (include/mvsv.h):
cv::resize(.., 0.5, 0.5, INTER_AREA) of an interleaved 8-bit BGR image, then
cv::cvtColor(BGR2GRAY), in int64 arithmetic.  Shared by the CPU and GPU tests."""
import numpy as np

Q14, Q15 = 0, 1


def cv_round(v):
    """cvRound of a non-negative double: round half to even."""
    return int(np.rint(v))


def prepare_size(w, h, halve):
    return (cv_round(w * 0.5), cv_round(h * 0.5)) if halve else (w, h)


def halve_plane(p):
    """INTER_AREA at exactly 0.5 on one channel: (a+b+c+d+2) >> 2 on whole 2 x 2
    blocks; on blocks clipped by an odd width or height the float32 mean of the
    pixels that exist, rounded half to even.  A clipped last row takes the float
    rule in every column."""
    p = np.asarray(p).astype(np.int64)
    sh, sw = p.shape
    dw, dh = prepare_size(sw, sh, True)
    out = np.zeros((dh, dw), np.int64)
    wh, ww = sh // 2, sw // 2  # whole blocks
    q = p[:2 * wh, :2 * ww]
    out[:wh, :ww] = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2
    for dy in range(dh):
        for dx in range(dw):
            if dy < wh and dx < ww:
                continue
            blk = p[2 * dy:2 * dy + 2, 2 * dx:2 * dx + 2]
            assert 0 < blk.size < 4
            mean = np.float32(int(blk.sum())) / np.float32(blk.size)
            out[dy, dx] = min(max(int(np.rint(mean)), 0), 255)
    return out.astype(np.uint8)


def gray(bgr, variant=Q14):
    c = np.asarray(bgr).astype(np.int64)
    b, g, r = c[..., 0], c[..., 1], c[..., 2]
    if variant == Q15:
        v = (b * 3735 + g * 19235 + r * 9798 + 16384) >> 15
    else:
        v = (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def prepare(bgr, halve=True, variant=Q14):
    """(H, W, 3) uint8 -> the grey image; every channel is rounded to 8 bits by the
    halving before the conversion."""
    bgr = np.asarray(bgr)
    assert bgr.ndim == 3 and bgr.shape[2] == 3 and bgr.dtype == np.uint8
    if halve:
        bgr = np.stack([halve_plane(bgr[..., c]) for c in range(3)], axis=-1)
    return gray(bgr, variant)
