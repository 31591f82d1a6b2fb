"""Rectification before the path.

Mirrors Stereosystem::initRectification (src/Stereosystem.cpp:193-237: maps from
cv::initUndistortRectifyMap, CV_32FC1) and Stereosystem::getRectifiedImagepair
(:243-262: cv::remap INTER_LINEAR on both images, then the mDisplayROI crop)
and its resizing overload (:279-315: cv::resize INTER_LINEAR by a factor).
The remap runs in a HIP kernel with OpenCV 3.4's fixed-point arithmetic
(bit-exact for given maps); the map construction is a host double-precision
restatement (OpenCV inverts P*R by SVD, so a map may differ in the last bit).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import MvsvError, Rect, check, device_context, host_context, lib


def init_undistort_rectify_map(K, dist, R, P, size):
    """cv::initUndistortRectifyMap(K, dist, R, P, (w, h), CV_32FC1) -> (map_x, map_y)."""
    w, h = size
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
    d = np.ascontiguousarray(np.asarray(dist if dist is not None else [], np.float64).reshape(-1))
    Rm = np.ascontiguousarray(np.asarray(R if R is not None else np.eye(3), np.float64).reshape(3, 3))
    Pm = np.asarray(P, np.float64)
    Pm = np.ascontiguousarray(Pm.reshape(3, -1)[:, :3])
    mx = np.empty((h, w), np.float32)
    my = np.empty((h, w), np.float32)
    rc = lib().mvsv_init_undistort_rectify_map(K.ctypes.data, d.ctypes.data if d.size else None,
                                               int(d.size), Rm.ctypes.data, Pm.ctypes.data, w, h,
                                               mx.ctypes.data, my.ctypes.data, w)
    check(rc)
    return mx, my


def remap(src, map_x, map_y):
    """cv::remap(src, dst, map_x, map_y, INTER_LINEAR) for uint8 device tensors.

    src: (H, W) or (N, H, W) uint8 torch tensor on a HIP device; maps: float32
    device tensors of the output size.  Returns uint8 of shape (..., mh, mw).
    """
    import torch
    if not (type(src).__module__.startswith("torch") and src.is_cuda and src.dtype == torch.uint8):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "remap: uint8 device tensor expected")
    mx = map_x.contiguous()
    my = map_y.contiguous()
    if mx.shape != my.shape or mx.dtype != torch.float32 or mx.dim() != 2:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "remap: two float32 maps of one size expected")
    batched = src.dim() == 3
    s = src if batched else src.unsqueeze(0)
    if s.stride(2) != 1:
        s = s.contiguous()
    n, sh, sw = s.shape
    dh, dw = mx.shape
    out = torch.empty((n, dh, dw), dtype=torch.uint8, device=src.device)
    ctx = device_context(src)
    check(lib().mvsv_remap_device(ctx.handle, n, s.data_ptr(), s.stride(1), s.stride(0), sw, sh,
                                  mx.data_ptr(), my.data_ptr(), dw, out.data_ptr(), dw, dh * dw,
                                  dw, dh), ctx.handle)
    return out if batched else out[0]


def convert_maps(map_x, map_y):
    """cv::convertMaps(map_x, map_y, CV_16SC2, CV_16UC1) -> (xy int16 (H, W, 2), frac uint16 (H, W)).

    The fixed-point form in which cv::remap (and the raw frame stream's kernel)
    consumes float maps: xy = (X >> 5, Y >> 5) saturated to short and
    frac = (Y & 31) * 32 + (X & 31) with X = cvRound(map_x * 32), Y likewise.
    Host only; maps must be finite with |value * 32| < 2^31.
    """
    mx = np.asarray(map_x, np.float32)
    my = np.asarray(map_y, np.float32)
    if mx.ndim != 2 or mx.shape != my.shape or mx.size == 0:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "convert_maps: two float32 maps of one size expected")
    if mx.strides[1] != 4 or mx.strides[0] % 4 or mx.strides[0] < 4 * mx.shape[1] or mx.strides != my.strides:
        mx, my = np.ascontiguousarray(mx), np.ascontiguousarray(my)
    h, w = mx.shape
    xy = np.empty((h, w, 2), np.int16)
    frac = np.empty((h, w), np.uint16)
    check(lib().mvsv_convert_maps(mx.ctypes.data, my.ctypes.data, mx.strides[0] // 4, w, h,
                                  xy.ctypes.data, w, frac.ctypes.data, w))
    return xy, frac


def rectify_pair(left, right, maps, roi):
    """Stereosystem::getRectifiedImagepair on host images.

    maps = (left_x, left_y, right_x, right_y) float32 arrays of the image size;
    roi = (x0, y0, x1, y1) display ROI.  Returns the cropped rectified pair.
    """
    L = np.ascontiguousarray(left, np.uint8)
    R = np.ascontiguousarray(right, np.uint8)
    if L.shape != R.shape or L.ndim != 2:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "rectify_pair: two uint8 images of one size expected")
    H, W = L.shape
    ms = [np.ascontiguousarray(m, np.float32) for m in maps]
    if len(ms) != 4 or any(m.shape != (H, W) for m in ms):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "rectify_pair: four maps of the image size expected")
    x0, y0, x1, y1 = roi
    oL = np.empty((y1 - y0, x1 - x0), np.uint8)
    oR = np.empty_like(oL)
    arr = (ctypes.c_void_p * 4)(*[m.ctypes.data for m in ms])
    r = Rect(x0, y0, x1, y1)
    ctx = host_context()
    check(lib().mvsv_rectify_pair(ctx.handle, L.ctypes.data, W, R.ctypes.data, W, W, H, arr,
                                  ctypes.byref(r), oL.ctypes.data, oL.shape[1], oR.ctypes.data,
                                  oR.shape[1]), ctx.handle)
    return oL, oR


def resize_size(width, height, fx, fy=None):
    """Output size of cv::resize(src, dst, Size(0, 0), fx, fy): (cvRound(w fx), cvRound(h fy))."""
    fy = fx if fy is None else fy
    w, h = ctypes.c_int(), ctypes.c_int()
    check(lib().mvsv_resize_size(int(width), int(height), float(fx), float(fy), ctypes.byref(w),
                                 ctypes.byref(h)))
    return w.value, h.value


def resize(src, fx, fy=None):
    """cv::resize(src, dst, Size(0, 0), fx, fy, INTER_LINEAR) of a uint8 image
    (OpenCV 3.4 fixed-point arithmetic, on the GPU).

    src: (H, W) uint8 numpy array (host path), or a (H, W) / (N, H, W) uint8
    torch tensor on a HIP device (device path, stream-ordered like compute()).
    """
    fy = fx if fy is None else fy
    if type(src).__module__.startswith("torch"):
        import torch
        if not (src.is_cuda and src.dtype == torch.uint8 and src.dim() in (2, 3)):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "resize: uint8 device tensor expected")
        batched = src.dim() == 3
        s = src if batched else src.unsqueeze(0)
        if s.stride(2) != 1:
            s = s.contiguous()
        n, sh, sw = s.shape
        dw, dh = resize_size(sw, sh, fx, fy)
        out = torch.empty((n, dh, dw), dtype=torch.uint8, device=src.device)
        ctx = device_context(src)
        check(lib().mvsv_resize_device(ctx.handle, n, s.data_ptr(), s.stride(1), s.stride(0), sw, sh,
                                       float(fx), float(fy), out.data_ptr(), dw, dh * dw), ctx.handle)
        return out if batched else out[0]
    a = np.ascontiguousarray(src, np.uint8)
    if a.ndim != 2:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "resize: a 2-D uint8 image expected")
    sh, sw = a.shape
    dw, dh = resize_size(sw, sh, fx, fy)
    out = np.empty((dh, dw), np.uint8)
    ctx = host_context()
    check(lib().mvsv_resize(ctx.handle, a.ctypes.data, sw, sw, sh, float(fx), float(fy),
                            out.ctypes.data, dw), ctx.handle)
    return out


def undistort_maps(K, dist, size, new_K=None):
    """The CV_16SC2 + CV_16UC1 maps cv::undistort(src, dst, K, dist[, new_K]) builds
    stripe by stripe (mvsv_undistort_maps, host only): (xy int16 (H, W, 2),
    frac uint16 (H, W)) for size = (w, h); dist None or empty: no distortion."""
    w, h = (int(v) for v in size)
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
    d = np.ascontiguousarray(np.asarray(dist if dist is not None else [], np.float64).reshape(-1))
    nk = None if new_K is None else np.ascontiguousarray(np.asarray(new_K, np.float64).reshape(3, 3))
    if w <= 0 or h <= 0:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "undistort_maps: empty size")
    xy = np.empty((h, w, 2), np.int16)
    frac = np.empty((h, w), np.uint16)
    check(lib().mvsv_undistort_maps(K.ctypes.data, d.ctypes.data if d.size else None, int(d.size),
                                    nk.ctypes.data if nk is not None else None, w, h, xy.ctypes.data, w,
                                    frac.ctypes.data, w))
    return xy, frac


def remap_fixed(src, xy, frac):
    """cv::remap(src, dst, xy, frac, INTER_LINEAR) with CV_16SC2 + CV_16UC1 maps for
    uint8 device tensors (mvsv_remap_fixed_device): pure integer, bit-exact.

    src: (H, W) or (N, H, W) uint8 device tensor, any view with unit column stride;
    xy: int16 device tensor (h, w, 2), frac: uint16 / int16 device tensor (h, w) (rows
    may be strided).  Returns uint8 (..., h, w)."""
    import torch
    if not (type(src).__module__.startswith("torch") and src.is_cuda and src.dtype == torch.uint8 and
            src.dim() in (2, 3)):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "remap_fixed: uint8 device tensor expected")
    if not (xy.is_cuda and xy.dtype == torch.int16 and xy.dim() == 3 and xy.shape[2] == 2 and
            frac.is_cuda and frac.element_size() == 2 and frac.dim() == 2 and frac.shape == xy.shape[:2]):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "remap_fixed: int16 (h, w, 2) and 16-bit (h, w) device maps expected")
    if xy.stride(2) != 1 or xy.stride(1) != 2 or xy.stride(0) % 2:
        xy = xy.contiguous()
    if frac.stride(1) != 1:
        frac = frac.contiguous()
    batched = src.dim() == 3
    s = src if batched else src.unsqueeze(0)
    if s.stride(2) != 1:
        s = s.contiguous()
    n, sh, sw = s.shape
    dh, dw = frac.shape
    out = torch.empty((n, dh, dw), dtype=torch.uint8, device=src.device)
    ctx = device_context(src)
    check(lib().mvsv_remap_fixed_device(ctx.handle, n, s.data_ptr(), s.stride(1), s.stride(0), sw, sh,
                                        xy.data_ptr(), xy.stride(0) // 2, frac.data_ptr(), frac.stride(0),
                                        out.data_ptr(), dw, dh * dw, dw, dh), ctx.handle)
    return out if batched else out[0]


def undistort_pair(left, right, K_left, dist_left, K_right, dist_right, out=None):
    """Stereosystem::getUndistortedImagepair on host images (mvsv_undistort_pair):
    cv::undistort of each side with its camera matrix and distortion coefficients.
    out = (left, right) arrays to write into -- the inputs themselves are allowed."""
    L, R = np.asarray(left), np.asarray(right)
    if L.ndim != 2 or L.shape != R.shape or L.dtype != np.uint8 or R.dtype != np.uint8 or L.size == 0:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "undistort_pair: two uint8 images of one size expected")
    if L.strides[1] != 1:
        L = np.ascontiguousarray(L)
    if R.strides[1] != 1:
        R = np.ascontiguousarray(R)
    H, W = L.shape
    oL, oR = (np.empty((H, W), np.uint8), np.empty((H, W), np.uint8)) if out is None else out
    for o in (oL, oR):
        if not (isinstance(o, np.ndarray) and o.dtype == np.uint8 and o.shape == (H, W) and o.strides[1] == 1):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "undistort_pair: out must be uint8 arrays of the images' shape")
    KL = np.ascontiguousarray(np.asarray(K_left, np.float64).reshape(3, 3))
    KR = np.ascontiguousarray(np.asarray(K_right, np.float64).reshape(3, 3))
    dl = np.ascontiguousarray(np.asarray(dist_left if dist_left is not None else [], np.float64).reshape(-1))
    dr = np.ascontiguousarray(np.asarray(dist_right if dist_right is not None else [], np.float64).reshape(-1))
    ctx = host_context()
    check(lib().mvsv_undistort_pair(ctx.handle, L.ctypes.data, L.strides[0], R.ctypes.data, R.strides[0], W, H,
                                    KL.ctypes.data, dl.ctypes.data if dl.size else None, int(dl.size),
                                    KR.ctypes.data, dr.ctypes.data if dr.size else None, int(dr.size),
                                    oL.ctypes.data, oL.strides[0], oR.ctypes.data, oR.strides[0]), ctx.handle)
    return oL, oR
