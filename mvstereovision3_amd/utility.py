"""Host mirror of the reference's Utility:: reprojection helpers and ply writer.

Reference: src/utility.cpp:176-303 (calcCoordinate, calcDistance,
calcDMapValues, dmap2pcl, calcMeanDisparity, calcMinMaxDisparity) and
src/ply.cpp:37-133 (ply::write).  The per-pixel work (reproject) runs in the
HIP kernel behind mvsv_reproject_device; the single-point helpers and the PLY
text writer are host code in libmvsv.so (include/mvsv.h).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from ._lib import MvsvError, check, device_context, host_context, lib

PLY_PLAIN = 0
PLY_WITH_COLOR = 1
PLY_WITH_COLOR_SHADING = 2

# one record of a point cloud (mvsv_cloud_point)
CLOUD_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("grey", "i4")])


def _q16(Q) -> np.ndarray:
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float32).reshape(16))
    return q


class dMapValues:  # noqa: N801 - reference name (inc/utility.h:50-55)
    def __init__(self, dValue=0.0, image_x=0.0, image_y=0.0):
        self.dValue = float(dValue)
        self.image_x = float(image_x)
        self.image_y = float(image_y)


class Utility:
    """Static mirror of namespace Utility (inc/utility.h:57-82)."""

    @staticmethod
    def calcCoordinate(v: dMapValues, Q) -> np.ndarray:
        """src/utility.cpp:176-198 -> float32 (X, Y, Z, 1)."""
        q = _q16(Q)
        out = np.empty(4, np.float32)
        lib().mvsv_calc_coordinate(v.image_x, v.image_y, v.dValue, q.ctypes.data, out.ctypes.data)
        return out

    @staticmethod
    def calcDistance(v: dMapValues, Q, binning: int = 0) -> float:
        """src/utility.cpp:200-222 (binning is unused, as in the reference)."""
        q = _q16(Q)
        return float(lib().mvsv_calc_distance(v.image_x, v.image_y, v.dValue, q.ctypes.data))

    @staticmethod
    def calcDMapValues(c, Q) -> dMapValues:
        """src/utility.cpp:224-240: metric (x, y, z) -> image position and disparity * 16."""
        q = _q16(Q)
        c3 = np.ascontiguousarray(np.asarray(c, np.float32).reshape(-1)[:3])
        x = ctypes.c_float()
        y = ctypes.c_float()
        d = ctypes.c_float()
        lib().mvsv_calc_dmap_values(c3.ctypes.data, q.ctypes.data, ctypes.byref(x), ctypes.byref(y),
                                    ctypes.byref(d))
        return dMapValues(d.value, x.value, y.value)

    @staticmethod
    def dmap2pcl(filename: str, dMap, Q) -> None:
        """src/utility.cpp:242-262: PLY of every pixel with disparity > 0 (WITH_COLOR).
        An int16 device tensor (H, W) is compacted on the GPU (point_cloud): the map
        stays there and only the count and the valid points come to the host."""
        if _is_device_map(dMap):
            if dMap.dim() != 2:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "dmap2pcl: 2-D int16 map expected")
            pts, count, mm = point_cloud(dMap, Q, return_minmax=True)
            k = int(count)
            if k == 0:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "dmap2pcl: map has no positive disparity")
            xyzg = pts[:k].cpu().numpy()
            # the writer takes min / max from its map: a two-pixel map holding them gives the same
            w = ply("Hagen Hiller", "disparity pointcloud", mm.cpu().numpy().astype(np.int16).reshape(1, 2))
            if not w.write(filename, xyzg[:, :3], ply.WITH_COLOR):
                raise MvsvError(_lib.MVSV_E_IO, f"cannot write {filename}")
            return
        d = _host_map(dMap, "dmap2pcl")
        q = _q16(Q)
        ctx = host_context()
        check(lib().mvsv_dmap2pcl(ctx.handle, os.fsencode(filename), d.ctypes.data, d.strides[0] // 2,
                                  d.shape[1], d.shape[0], q.ctypes.data), ctx.handle)

    @staticmethod
    def calcMeanDisparity(matrix) -> float:
        """src/utility.cpp:265-285: integer mean of values > 1 (0 when none)."""
        m = np.asarray(matrix).astype(np.int64)
        v = m[m > 1]
        if v.size == 0 or int(v.sum()) == 0:
            return 0.0
        t, n = int(v.sum()), int(v.size)
        q = abs(t) // n * (1 if t >= 0 else -1)  # C++ int division truncates toward 0
        return float(np.float32(q))

    @staticmethod
    def calcMinMaxDisparity(matrix):
        """src/utility.cpp:286-303: min / max of the positive values.  An int16
        device tensor is reduced on the GPU (mvsv_minmax_device)."""
        if _is_device_map(matrix):
            lo, hi = (int(x) for x in minmax(matrix, positive_only=True).cpu())
            if lo > hi:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "calcMinMaxDisparity: no positive value")
            return lo, hi
        m = np.asarray(matrix)
        v = m[m > 0]
        if v.size == 0:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "calcMinMaxDisparity: no positive value")
        return int(v.min()), int(v.max())

    @staticmethod
    def checkSharpness(src, roi=None) -> float:
        """src/utility.cpp:163-174: cv::mean(|Lx| + |Ly|) of the two cv::sepFilter2D
        responses, computed on the GPU (mvsv_sharpness).  src: a uint8 image, a numpy
        array or a device tensor (H, W).  roi = (x0, y0, x1, y1) stands for the
        reference's view src(viewArea): its 1-pixel halo comes from src, as OpenCV's
        filter engine takes it from a view's parent image."""
        if (src.dim() if type(src).__module__.startswith("torch") else np.asarray(src).ndim) != 2:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "checkSharpness: a 2-D uint8 image expected")
        return float(sharpness(src, roi))


def _rect(roi):
    return _lib.Rect(*(int(v) for v in roi)) if roi is not None else None


def sharpness_value(sum4, n_pixels) -> float:
    """The double cv::mean returns for the integer sum S4 over n_pixels pixels:
    (S4 / 4.0) * (1.0 / N), a reciprocal and a product, each rounded."""
    return (float(int(sum4)) / 4.0) * (1.0 / float(int(n_pixels)))


def sharpness(frames, roi=None, return_sums=False):
    """Utility::checkSharpness of one uint8 image (H, W) or a batch (N, H, W), all
    over the same roi = (x0, y0, x1, y1) (default: the whole image), on the GPU.

    A torch device tensor (any view with unit column stride) is measured where it
    is, asynchronously up to the read-back of the N sums; a numpy array goes
    through mvsv_sharpness frame by frame.  Returns a float, or a float64 array
    (N,) for a batch; return_sums: also the exact integer sums S4 (int, or int64
    array), with value = (S4 / 4.0) * (1.0 / roi pixels)."""
    r = _rect(roi)
    if type(frames).__module__.startswith("torch"):
        import torch
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (2, 3)):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "sharpness: 2-D or 3-D uint8 device tensor expected")
        batched = frames.dim() == 3
        d = frames if batched else frames.unsqueeze(0)
        if d.stride(2) != 1:
            d = d.contiguous()
        n, H, W = d.shape
        ctx = device_context(frames)
        out = torch.empty((n,), dtype=torch.int64, device=frames.device)
        check(lib().mvsv_sharpness_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                          ctypes.byref(r) if r is not None else None, out.data_ptr()), ctx.handle)
        sums = out.cpu().numpy()
    else:
        a = np.asarray(frames)
        if a.ndim not in (2, 3) or a.dtype != np.uint8:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "sharpness: 2-D or 3-D uint8 image expected")
        if a.strides[-1] != 1:
            a = np.ascontiguousarray(a)
        batched = a.ndim == 3
        H, W = a.shape[-2:]
        ctx = host_context()
        sums = np.empty(len(a) if batched else 1, np.int64)
        for i, f in enumerate(a if batched else a[None]):
            s4 = ctypes.c_int64(0)
            check(lib().mvsv_sharpness(ctx.handle, f.ctypes.data, f.strides[0], W, H,
                                       ctypes.byref(r) if r is not None else None, None, ctypes.byref(s4)),
                  ctx.handle)
            sums[i] = s4.value
    npx = W * H if r is None else (r.x1 - r.x0) * (r.y1 - r.y0)
    values = np.array([sharpness_value(s, npx) for s in sums], np.float64)
    if not batched:
        return (float(values[0]), int(sums[0])) if return_sums else float(values[0])
    return (values, sums) if return_sums else values


def prepare_size(src_width, src_height, halve=True):
    """(width, height) of the grey image prepare_gray makes (mvsv_prepare_size):
    cvRound of half of each side when halving, half to even."""
    w, h = ctypes.c_int(), ctypes.c_int()
    check(lib().mvsv_prepare_size(int(src_width), int(src_height), 1 if halve else 0, ctypes.byref(w),
                                  ctypes.byref(h)))
    return w.value, h.value


def prepare_gray(bgr, halve=True, variant=_lib.GRAY_Q14):
    """What trgt/disparityTest.cpp does to a colour image ahead of the matchers
    (:201-211), on the GPU in one kernel: with halve, cv::resize(.., 0.5, 0.5,
    INTER_AREA) of the 3-channel image, then cv::cvtColor(BGR2GRAY); variant
    GRAY_Q14 (OpenCV up to the early 3.4 releases) or GRAY_Q15 (later ones).

    bgr: uint8 interleaved BGR, (H, W, 3) or a batch (N, H, W, 3).  A torch device
    tensor (any view whose pixels are 3 contiguous bytes, columns 3 bytes apart)
    gives a uint8 device tensor (h, w) / (N, h, w), asynchronously on the current
    stream; a numpy array gives a numpy array."""
    hv = 1 if halve else 0
    if type(bgr).__module__.startswith("torch"):
        import torch
        if not (bgr.is_cuda and bgr.dtype == torch.uint8 and bgr.dim() in (3, 4) and bgr.shape[-1] == 3):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "prepare_gray: uint8 device tensor (H, W, 3) or (N, H, W, 3) expected")
        batched = bgr.dim() == 4
        d = bgr if batched else bgr.unsqueeze(0)
        if d.stride(3) != 1 or d.stride(2) != 3:
            d = d.contiguous()
        n, H, W, _ = d.shape
        w, h = prepare_size(W, H, halve)
        ctx = device_context(bgr)
        out = torch.empty((n, h, w), dtype=torch.uint8, device=bgr.device)
        check(lib().mvsv_prepare_gray_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H, hv,
                                             int(variant), out.data_ptr(), w, h * w), ctx.handle)
        return out if batched else out[0]
    a = np.asarray(bgr)
    if a.ndim not in (3, 4) or a.dtype != np.uint8 or a.shape[-1] != 3:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "prepare_gray: uint8 image (H, W, 3) or (N, H, W, 3) expected")
    if a.strides[-2:] != (3, 1):
        a = np.ascontiguousarray(a)
    batched = a.ndim == 4
    H, W = a.shape[-3:-1]
    w, h = prepare_size(W, H, halve)
    frames = a if batched else a[None]
    out = np.empty((len(frames), h, w), np.uint8)
    ctx = host_context()
    for f, o in zip(frames, out):
        check(lib().mvsv_prepare_gray(ctx.handle, f.ctypes.data, f.strides[0], W, H, hv, int(variant), o.ctypes.data,
                                      w), ctx.handle)
    return out if batched else out[0]


def reproject(dmap, Q):
    """Utility::calcCoordinate for every pixel of an int16 device map, on the GPU.

    dmap: (H, W) or (N, H, W) int16 torch tensor on a HIP device.  Returns a
    float32 tensor (..., H, W, 4) = (X, Y, Z, valid) with valid = (d > 0).
    """
    import torch
    d, batched, ctx = _device_frames(dmap, "reproject", any_rank=True)
    n, H, W = d.shape
    out = torch.empty((n, H, W, 4), dtype=torch.float32, device=dmap.device)
    q = _q16(Q)
    check(lib().mvsv_reproject_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                      q.ctypes.data, out.data_ptr(), W, H * W), ctx.handle)
    return out if batched else out[0]


def _is_device_map(d) -> bool:
    if not type(d).__module__.startswith("torch"):
        return False
    import torch
    return d.is_cuda and d.dtype == torch.int16 and d.dim() in (2, 3)


def _host_map(dmap, what, dims=(2,)):
    """An int16 host map, 2-D (or a batch, with dims=(2, 3)), as an array with unit column stride."""
    d = np.asarray(dmap)
    if d.ndim not in dims or d.dtype != np.int16:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: {'2-D or 3-D' if 3 in dims else '2-D'} int16 map expected")
    return d if d.strides[-1] == 2 else np.ascontiguousarray(d)


def _device_frames(dmap, what, any_rank=False):
    """(frames view (N, H, W) with unit column stride, batched, context bound to the
    current stream) of an int16 device map, 2-D or 3-D; any_rank: the rank is not checked."""
    import torch
    ok = type(dmap).__module__.startswith("torch") and dmap.is_cuda and dmap.dtype == torch.int16
    if not (ok and (any_rank or dmap.dim() in (2, 3))):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: {'' if any_rank else '2-D or 3-D '}int16 device tensor expected")
    batched = dmap.dim() == 3
    d = dmap if batched else dmap.unsqueeze(0)
    if d.stride(2) != 1:
        d = d.contiguous()
    return d, batched, device_context(dmap)


def minmax(dmap, positive_only=False):
    """(min, max) of every frame of an int16 device map (any view with unit column
    stride), on the GPU: int16 tensor (2,) or (N, 2).  positive_only: over the
    values > 0 (Utility::calcMinMaxDisparity), (32767, -32768) where there is none."""
    import torch
    d, batched, ctx = _device_frames(dmap, "minmax")
    n, H, W = d.shape
    out = torch.empty((n, 2), dtype=torch.int16, device=dmap.device)
    check(lib().mvsv_minmax_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                   1 if positive_only else 0, out.data_ptr()), ctx.handle)
    return out if batched else out[0]


def normalize_minmax(dmap, alpha=0, beta=255, out=None, return_minmax=False):
    """cv::normalize(dmap, out, alpha, beta, NORM_MINMAX, CV_8U) in OpenCV 3.4's
    arithmetic, on the GPU: the display map of the reference's loops
    (trgt/liveDisparity.cpp:92).

    dmap: int16, (H, W) or a batch (N, H, W) whose frames are normalised each with
    its own min / max.  A torch device tensor (any view with unit column stride)
    gives a uint8 device tensor, asynchronously on the current stream; a numpy
    array gives a numpy array.  out: a uint8 tensor / array of the same shape to
    write into (device tensors: any view with unit column stride).
    return_minmax: also return the (smin, smax) int16 pairs, (2,) or (N, 2)."""
    if type(dmap).__module__.startswith("torch") and dmap.is_cuda:
        import torch
        d, batched, ctx = _device_frames(dmap, "normalize_minmax")
        n, H, W = d.shape
        if out is None:
            out = torch.empty(tuple(dmap.shape), dtype=torch.uint8, device=dmap.device)
        elif not (type(out).__module__.startswith("torch") and out.is_cuda and out.dtype == torch.uint8 and
                  out.shape == dmap.shape and out.stride(-1) == 1):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG,
                            "normalize_minmax: out must be a uint8 device tensor of dmap's shape, unit column stride")
        o = out if batched else out.unsqueeze(0)
        mm = torch.empty((n, 2), dtype=torch.int16, device=dmap.device) if return_minmax else None
        check(lib().mvsv_normalize_minmax_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                                 float(alpha), float(beta), o.data_ptr(), o.stride(1), o.stride(0),
                                                 mm.data_ptr() if return_minmax else None), ctx.handle)
        if return_minmax:
            return out, (mm if batched else mm[0])
        return out
    d = _host_map(dmap, "normalize_minmax", dims=(2, 3))
    if out is None:
        out = np.empty(d.shape, np.uint8)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == d.shape and out.strides[-1] == 1):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG,
                        "normalize_minmax: out must be a uint8 array of dmap's shape, unit column stride")
    frames = d if d.ndim == 3 else d[None]
    outs = out if d.ndim == 3 else out[None]
    mm = np.empty((len(frames), 2), np.int16)
    ctx = host_context()
    for f, o, m in zip(frames, outs, mm):
        check(lib().mvsv_normalize_minmax(ctx.handle, f.ctypes.data, f.strides[0] // 2, f.shape[1], f.shape[0],
                                          float(alpha), float(beta), o.ctypes.data, o.strides[0], m.ctypes.data),
              ctx.handle)
    if return_minmax:
        return out, (mm if d.ndim == 3 else mm[0])
    return out


VIEW_SUBIMAGE_GRID = 1
VIEW_OBSTACLE_GRID = 2
VIEW_FOUND_TILES = 4
VIEW_FOUND_POINTS = 8


def _view_layer_input(given, rng, built_attr, what):
    """(float32 array or device tensor or None, (first, second)) of a layer's input:
    raw values and a range, or a detector whose mRangeDisparity and built values are taken."""
    if hasattr(given, "mRangeDisparity"):
        if rng is None:
            rng = given.mRangeDisparity
        built = getattr(given, built_attr)
        given = np.asarray(built, np.float32) if len(built) else None
    if rng is None:
        rng = (0.0, 0.0)
    if len(rng) != 2:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"detection_view: {what} range must be (first, second)")
    return given, (float(rng[0]), float(rng[1]))


def view_spec(layers, mean_range=None, sample_range=None, point_radius=3, alpha=0, beta=255):
    """An mvsv_view_spec without pointers."""
    s = _lib.ViewSpec()
    s.layers = int(layers)
    s.alpha, s.beta = float(alpha), float(beta)
    s.tile_first, s.tile_second = mean_range if mean_range is not None else (0.0, 0.0)
    s.point_first, s.point_second = sample_range if sample_range is not None else (0.0, 0.0)
    s.point_radius = int(point_radius)
    return s


def detection_view(dmap, layers, means=None, mean_range=None, values=None, sample_range=None, point_radius=3,
                   alpha=0, beta=255, out=None, return_minmax=False):
    """The annotated BGR frame of the reference's detection programs
    (trgt/demo.cpp:280-298): cv::normalize(NORM_MINMAX, CV_8U), GRAY2BGR, View's
    grids and drawFoundObstacles, in one pass on the GPU (mvsv_view_device).

    dmap: int16, (H, W) or a batch (N, H, W), at least 9 x 9.  A torch device tensor
    (any view with unit column stride) gives a uint8 device tensor (..., H, W, 3) in
    B, G, R order, asynchronously on the current stream; a numpy map gives a numpy
    image.  layers: VIEW_* bits.  means: 81 (or N x 81) tile means and mean_range =
    (first, second) for VIEW_FOUND_TILES, or a MeanDisparityDetection (its
    mRangeDisparity, and its means if built).  values: the lattice values and
    sample_range for VIEW_FOUND_POINTS, or a SamplepointDetection.  point_radius:
    0..3.  out: an image of that shape to write into (unit channel stride, pixels 3
    bytes apart).  return_minmax: also return (smin, smax), (2,) or (N, 2)."""
    means, mean_range = _view_layer_input(means, mean_range, "mMeanMap", "mean")
    values, sample_range = _view_layer_input(values, sample_range, "mDistanceVec", "sample")
    spec = view_spec(layers, mean_range, sample_range, point_radius, alpha, beta)
    if type(dmap).__module__.startswith("torch") and dmap.is_cuda:
        import torch
        d, batched, ctx = _device_frames(dmap, "detection_view")
        n, H, W = d.shape
        shape = tuple(dmap.shape) + (3,)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dmap.device)
        elif not (type(out).__module__.startswith("torch") and out.is_cuda and out.dtype == torch.uint8 and
                  tuple(out.shape) == shape and out.stride(-1) == 1 and out.stride(-2) == 3):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG,
                            "detection_view: out must be a uint8 device tensor (..., H, W, 3) with dense pixels")
        o = out if batched else out.unsqueeze(0)

        def flat(a):  # float32 on the device, frames back to back
            if a is None:
                return None
            return torch.as_tensor(a, dtype=torch.float32, device=dmap.device).reshape(-1).contiguous()
        tm, tv = flat(means), flat(values)
        if tm is not None and tm.numel() != 81 * n:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "detection_view: 81 means per frame expected")
        if tv is not None:
            from .disparity import samplepoint_layout
            _, _, nx, ny = samplepoint_layout(W, H)
            if tv.numel() != nx * ny * n:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "detection_view: one value per lattice point and frame expected")
            if tv.numel() == 0:
                tv = torch.zeros(1, dtype=torch.float32, device=dmap.device)  # no lattice: never read
        spec.means = tm.data_ptr() if tm is not None else None
        spec.values = tv.data_ptr() if tv is not None else None
        mm = torch.empty((n, 2), dtype=torch.int16, device=dmap.device) if return_minmax else None
        check(lib().mvsv_view_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H, ctypes.byref(spec),
                                     o.data_ptr(), o.stride(1), o.stride(0),
                                     mm.data_ptr() if return_minmax else None), ctx.handle)
        if return_minmax:
            return out, (mm if batched else mm[0])
        return out
    d = _host_map(dmap, "detection_view", dims=(2, 3))
    if out is None:
        out = np.empty(d.shape + (3,), np.uint8)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == d.shape + (3,) and
              out.strides[-1] == 1 and out.strides[-2] == 3):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG,
                        "detection_view: out must be a uint8 array (..., H, W, 3) with dense pixels")
    frames = d if d.ndim == 3 else d[None]
    outs = out if d.ndim == 3 else out[None]
    n = len(frames)
    hm = np.ascontiguousarray(np.asarray(means, np.float32).reshape(n, 81)) if means is not None else None
    hv = np.ascontiguousarray(np.asarray(values, np.float32).reshape(n, -1)) if values is not None else None
    if hv is not None:
        from .disparity import samplepoint_layout
        _, _, nx, ny = samplepoint_layout(d.shape[-1], d.shape[-2])
        if hv.shape[1] != nx * ny:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "detection_view: one value per lattice point and frame expected")
        if hv.shape[1] == 0:
            hv = np.zeros((n, 1), np.float32)  # no lattice: a pointer that is never read
    mm = np.empty((n, 2), np.int16)
    ctx = host_context()
    for k, (f, o, m) in enumerate(zip(frames, outs, mm)):
        spec.means = hm[k].ctypes.data if hm is not None else None
        spec.values = hv[k].ctypes.data if hv is not None else None
        check(lib().mvsv_view(ctx.handle, f.ctypes.data, f.strides[0] // 2, f.shape[1], f.shape[0], ctypes.byref(spec),
                              o.ctypes.data, o.strides[0], m.ctypes.data), ctx.handle)
    if return_minmax:
        return out, (mm if d.ndim == 3 else mm[0])
    return out


class View:
    """Static mirror of namespace View (inc/view.h, src/view.cpp): the two grids,
    painted in place over a host BGR image (H, W, 3) by the library's host painter
    (mvsv_view_draw), whose rules are the device view's."""

    @staticmethod
    def _draw(img, layer):
        if not (isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and
                img.strides[2] == 1 and img.strides[1] == 3 and img.flags.writeable):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "View: a writeable uint8 BGR image (H, W, 3) with dense pixels expected")
        spec = view_spec(layer)
        rc = lib().mvsv_view_draw(img.ctypes.data, img.strides[0], img.shape[1], img.shape[0], ctypes.byref(spec))
        if rc:
            raise MvsvError(rc, "View: the image must be at least 9 x 9")

    @staticmethod
    def drawObstacleGrid(img, binning=0):
        """src/view.cpp: the 3 x 3 grid, red (binning is unused, as in the reference)."""
        View._draw(img, VIEW_OBSTACLE_GRID)

    @staticmethod
    def drawSubimageGrid(img, binning=0):
        """src/view.cpp: the lines of the 9 x 9 grid that are no obstacle grid lines, (100, 0, 0)."""
        View._draw(img, VIEW_SUBIMAGE_GRID)


def point_cloud(dmap, Q, max_points=None, return_minmax=False, out=None):
    """The valid pixels (v > 0) of an int16 map as a point cloud, compacted on the
    GPU in raster order -- what Utility::dmap2pcl makes of a map (src/utility.cpp:
    248-259), with the grey ply::write prints (mvsv_point_cloud_device).

    A torch device tensor (H, W) or (N, H, W) (any view with unit column stride)
    gives (records, counts), asynchronously on the current stream: records float32
    (cap, 4) / (N, cap, 4) = (x, y, z, grey bits) -- read the int32 grey as
    records.view(torch.int32)[..., 3] -- and counts int32, scalar / (N,).  cap =
    max_points, default H * W.  Frame f's first min(counts[f], cap) records are
    written and nothing else; counts holds the number of valid pixels even beyond
    cap.  out: a contiguous float32 device tensor (cap, 4) / (N, cap, 4) to write into.

    A numpy map (H, W) gives the records as a structured array of CLOUD_DTYPE,
    trimmed to min(count, max_points).

    return_minmax: also the int32 (min, max) over the valid values, (2,) / (N, 2);
    (32767, -32768) where there is none."""
    q = _q16(Q)
    if type(dmap).__module__.startswith("torch") and dmap.is_cuda:
        import torch
        d, batched, ctx = _device_frames(dmap, "point_cloud")
        n, H, W = d.shape
        if out is None:
            cap = H * W if max_points is None else int(max_points)
            if cap < 1:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "point_cloud: max_points must be at least 1")
            out = torch.empty((n, cap, 4) if batched else (cap, 4), dtype=torch.float32, device=dmap.device)
        elif not (type(out).__module__.startswith("torch") and out.is_cuda and out.dtype == torch.float32 and
                  out.is_contiguous() and out.dim() == (3 if batched else 2) and out.shape[-1] == 4 and
                  out.shape[-2] >= 1 and (not batched or out.shape[0] == n)):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG,
                            "point_cloud: out must be a contiguous float32 device tensor (cap, 4) or (N, cap, 4)")
        cap = out.shape[-2]
        counts = torch.empty((n,), dtype=torch.int32, device=dmap.device)
        mm = torch.empty((n, 2), dtype=torch.int32, device=dmap.device) if return_minmax else None
        check(lib().mvsv_point_cloud_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                            q.ctypes.data, out.data_ptr(), cap, counts.data_ptr(),
                                            mm.data_ptr() if return_minmax else None), ctx.handle)
        c = counts if batched else counts[0]
        if return_minmax:
            return out, c, (mm if batched else mm[0])
        return out, c
    d = _host_map(dmap, "point_cloud")
    cap = d.size if max_points is None else int(max_points)
    if cap < 1:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "point_cloud: max_points must be at least 1")
    cap = min(cap, d.size)
    rec = np.empty(cap, CLOUD_DTYPE)
    count = ctypes.c_int(0)
    mm = np.zeros(2, np.int32)
    ctx = host_context()
    check(lib().mvsv_point_cloud(ctx.handle, d.ctypes.data, d.strides[0] // 2, d.shape[1], d.shape[0],
                                 q.ctypes.data, rec.ctypes.data, cap, ctypes.byref(count), mm.ctypes.data),
          ctx.handle)
    rec = rec[:min(count.value, cap)]
    if return_minmax:
        return rec, mm
    return rec


class ply:  # noqa: N801 - reference name (inc/ply.h)
    """src/ply.cpp: ASCII PLY writer with the reference's three modes."""

    PLAIN = PLY_PLAIN
    WITH_COLOR = PLY_WITH_COLOR
    WITH_COLOR_SHADING = PLY_WITH_COLOR_SHADING

    def __init__(self, author: str = "", object_name: str = "", disparity_map=None):
        self.mAuthor = author
        self.mObjectName = object_name
        self.mDMap = None if disparity_map is None else np.asarray(disparity_map)

    def write(self, filename: str, to_write, mode: int) -> bool:
        """ply::write: to_write = sequence of (x, y, z[, ...]) points."""
        pts = np.ascontiguousarray(np.asarray(to_write, np.float32).reshape(len(to_write), -1))
        if pts.size and pts.shape[1] < 3:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "ply.write: 3 coordinates per vertex")
        stride = pts.shape[1] if pts.size else 3
        d = self.mDMap
        if mode != PLY_PLAIN and (d is None or d.size == 0):
            return False  # "if(mDMap.rows == 0 || mDMap.cols == 0) return false;"
        dp, ds, W, H = None, 0, 0, 0
        if d is not None and d.size:
            d = np.ascontiguousarray(d.astype(np.int16, copy=False))
            dp, ds, W, H = d.ctypes.data, d.strides[0] // 2, d.shape[1], d.shape[0]
        rc = lib().mvsv_write_ply(os.fsencode(filename), self.mAuthor.encode(),
                                  self.mObjectName.encode(), pts.ctypes.data if pts.size else None,
                                  len(pts), stride, mode, dp, ds, W, H)
        if rc == _lib.MVSV_E_INVALID_ARG and mode != PLY_PLAIN:
            raise MvsvError(rc, "ply.write: the disparity map has no positive value")
        check(rc)
        return True
