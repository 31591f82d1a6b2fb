"""Host-side mirror of the reference's disparity interface, on libmvsv.

Reference surface (hG3n/mvStereoVision3):

* ``struct Stereopair``                inc/utility.h:31-41
* ``Disparity::sgbmParameters``        inc/disparity.h:17-27
* ``Disparity::sgbm(Stereopair const&, cv::Mat&, cv::Ptr<cv::StereoSGBM>)``
                                       src/disparity.cpp:6-10
* ``Disparity::bm(Stereopair const&, cv::Mat&, cv::Ptr<cv::StereoBM>)``
                                       src/disparity.cpp:18-22
* ``Disparity::loadSGBMParameters(std::string, cv::Ptr<cv::StereoSGBM>&,
  sgbmParameters&) -> bool``           src/disparity.cpp:60-108
* the matcher objects themselves: ``cv::StereoSGBM::create(...)`` /
  ``cv::StereoBM::create(...)`` plus their setters (src/disparity.cpp:83-95,
  trgt/liveDisparity.cpp:61, trgt/captureDisparity.cpp:196).

Same names, same argument meaning, same error behaviour: invalid matcher state
raises (OpenCV raises ``cv::Exception``; here :class:`MvsvError`), the loader
returns ``False``.  Images are host ``numpy`` uint8 arrays (ROI views with
stride > width are accepted, like the cropped ``cv::Mat`` of
src/Stereosystem.cpp:255-256) or HBM-resident ``torch`` uint8 tensors; the
result is int16 disparity x 16 (CV_16S).  All compute runs in the HIP kernels
of libmvsv.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import logging
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import (MODE_HH, MODE_HH4, MODE_SGBM, PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL,
                   BmParams, MvsvError, SgbmParams, SgbmYamlValues, check, device_context, host_context, lib)
from .utility import _device_frames

log = logging.getLogger("mvsv.disparity")

DISP_SHIFT = 4
DISP_SCALE = 1 << DISP_SHIFT


@dataclass
class Stereopair:
    """inc/utility.h:31-41 — a rectified left/right pair plus a log tag."""
    mLeft: object = None
    mRight: object = None
    mTag: str = field(default="STEREOPAIR\t")


@dataclass
class sgbmParameters:  # noqa: N801 - reference name
    """Disparity::sgbmParameters, inc/disparity.h:17-27."""
    minDisp: int = 0
    numDisp: int = 0
    blockSize: int = 0
    disp12MaxDiff: int = 0
    preFilterCap: int = 0
    uniquenessRatio: int = 0
    speckleWindowSize: int = 0
    speckleRange: int = 0
    disparityMode: int = 0


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def _host_pair(left, right, what):
    """Two 2-D uint8 arrays of one size, with unit column stride."""
    L, R = np.asarray(left), np.asarray(right)
    if L.ndim != 2 or R.ndim != 2 or L.dtype != np.uint8 or R.dtype != np.uint8:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: inputs must be 2-D CV_8UC1 (uint8)")
    if L.shape != R.shape:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: left and right sizes differ")
    return tuple(a if a.strides[1] == 1 else np.ascontiguousarray(a) for a in (L, R))


def _device_pair(left, right, what, channels=1):
    """Two uint8 device tensors of one shape, (H, W) or (N, H, W) -- with channels = 3 a
    last dimension of 3 behind it -- as frames (N, ...) with dense rows:
    (left, right, whether they came as a batch)."""
    import torch
    nd, c = (2, "") if channels == 1 else (3, ",3")
    if left.dtype != torch.uint8 or right.dtype != torch.uint8:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: inputs must be uint8")
    if left.shape != right.shape or left.dim() not in (nd, nd + 1) or (channels == 3 and left.shape[-1] != 3):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: inputs must be (H,W{c}) or (N,H,W{c}), equal")
    if not left.is_cuda or not right.is_cuda or left.device != right.device:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: device tensors on one GPU expected")
    batched = left.dim() == nd + 1
    frames = [t if batched else t.unsqueeze(0) for t in (left, right)]
    dense = (lambda t: t.stride(2) == 1) if channels == 1 else (lambda t: t.stride(3) == 1 and t.stride(2) == 3)
    Lt, Rt = (t if dense(t) else t.contiguous() for t in frames)
    return Lt, Rt, batched


def _run_host(fn, params, left, right, out, what):
    L, R = _host_pair(left, right, what)
    H, W = L.shape
    if out is None or not isinstance(out, np.ndarray) or out.shape != (H, W) \
            or out.dtype != np.int16 or out.strides[1] != 2:
        out = np.empty((H, W), np.int16)  # cv::Mat::create semantics: reallocate
    ctx = host_context()
    rc = fn(ctx.handle, L.ctypes.data, L.strides[0], R.ctypes.data, R.strides[0], W, H,
            ctypes.byref(params), out.ctypes.data, out.strides[0] // 2)
    check(rc, ctx.handle)
    return out


def _run_device(fn, params, left, right, out, what):
    import torch
    Lt, Rt, batched = _device_pair(left, right, what)
    n, H, W = Lt.shape
    if out is None or tuple(out.shape) != tuple(left.shape) or out.dtype != torch.int16 \
            or out.device != left.device or out.stride(-1) != 1:
        out = torch.empty(left.shape, dtype=torch.int16, device=left.device)
    Ot = out if batched else out.unsqueeze(0)
    ctx = device_context(left)
    rc = fn(ctx.handle, n, Lt.data_ptr(), Lt.stride(1), Lt.stride(0), Rt.data_ptr(), Rt.stride(1),
            Rt.stride(0), W, H, ctypes.byref(params), Ot.data_ptr(), Ot.stride(1), Ot.stride(0))
    check(rc, ctx.handle)
    return out


def _run_host_bgr(fn, params, left, right, out, what):
    """(H, W, 3) or (N, H, W, 3) uint8 host arrays through the host colour entry."""
    L = np.asarray(left)
    R = np.asarray(right)
    if L.ndim not in (3, 4) or L.shape[-1] != 3 or L.dtype != np.uint8 or R.dtype != np.uint8:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: inputs must be (H,W,3) or (N,H,W,3) CV_8UC3 (uint8)")
    if L.shape != R.shape:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: left and right sizes differ")
    if L.strides[-1] != 1 or L.strides[-2] != 3:
        L = np.ascontiguousarray(L)
    if R.strides[-1] != 1 or R.strides[-2] != 3:
        R = np.ascontiguousarray(R)
    batched = L.ndim == 4
    H, W = L.shape[-3], L.shape[-2]
    if out is None or not isinstance(out, np.ndarray) or out.shape != L.shape[:-1] \
            or out.dtype != np.int16 or out.strides[-1] != 2:
        out = np.empty(L.shape[:-1], np.int16)  # cv::Mat::create semantics: reallocate
    ctx = host_context()
    for Lf, Rf, Of in (zip(L, R, out) if batched else ((L, R, out),)):
        rc = fn(ctx.handle, Lf.ctypes.data, Lf.strides[0], Rf.ctypes.data, Rf.strides[0], W, H,
                ctypes.byref(params), Of.ctypes.data, Of.strides[0] // 2)
        check(rc, ctx.handle)
    return out


def _run_device_bgr(fn, params, left, right, out, what):
    """(H, W, 3) or (N, H, W, 3) uint8 device tensors on the current torch stream."""
    import torch
    Lt, Rt, batched = _device_pair(left, right, what, channels=3)
    n, H, W, _ = Lt.shape
    oshape = tuple(left.shape[:-1])
    if out is None or tuple(out.shape) != oshape or out.dtype != torch.int16 \
            or out.device != left.device or out.stride(-1) != 1:
        out = torch.empty(oshape, dtype=torch.int16, device=left.device)
    Ot = out if batched else out.unsqueeze(0)
    ctx = device_context(left)
    rc = fn(ctx.handle, n, Lt.data_ptr(), Lt.stride(1), Lt.stride(0), Rt.data_ptr(), Rt.stride(1),
            Rt.stride(0), W, H, ctypes.byref(params), Ot.data_ptr(), Ot.stride(1), Ot.stride(0))
    check(rc, ctx.handle)
    return out


class StereoMatcher:
    DISP_SHIFT = DISP_SHIFT
    DISP_SCALE = DISP_SCALE

    def compute(self, left, right, disparity=None):
        """cv::StereoMatcher::compute: returns the CV_16S disparity map."""
        if _is_torch(left):
            return _run_device(self._dev_fn(), self._params, left, right, disparity,
                               type(self).__name__)
        return _run_host(self._host_fn(), self._params, left, right, disparity,
                         type(self).__name__)

    # common setters / getters of cv::StereoMatcher
    def setMinDisparity(self, v): self._params.min_disparity = int(v)      # noqa: E704
    def getMinDisparity(self): return self._params.min_disparity            # noqa: E704
    def setNumDisparities(self, v): self._params.num_disparities = int(v)  # noqa: E704
    def getNumDisparities(self): return self._params.num_disparities        # noqa: E704
    def setBlockSize(self, v): self._params.block_size = int(v)            # noqa: E704
    def getBlockSize(self): return self._params.block_size                  # noqa: E704
    def setSpeckleWindowSize(self, v): self._params.speckle_window_size = int(v)  # noqa: E704
    def getSpeckleWindowSize(self): return self._params.speckle_window_size       # noqa: E704
    def setSpeckleRange(self, v): self._params.speckle_range = int(v)       # noqa: E704
    def getSpeckleRange(self): return self._params.speckle_range            # noqa: E704
    def setDisp12MaxDiff(self, v): self._params.disp12_max_diff = int(v)   # noqa: E704
    def getDisp12MaxDiff(self): return self._params.disp12_max_diff         # noqa: E704

    def params(self) -> dict:
        return self._params.as_dict()


class StereoSGBM(StereoMatcher):
    """cv::StereoSGBM (OpenCV 3.4 semantics) backed by the MI355X kernels."""
    MODE_SGBM = MODE_SGBM
    MODE_HH = MODE_HH
    MODE_HH4 = MODE_HH4

    def __init__(self, params: SgbmParams):
        self._params = params

    @staticmethod
    def create(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0,
               preFilterCap=0, uniquenessRatio=0, speckleWindowSize=0, speckleRange=0,
               mode=MODE_SGBM):
        p = SgbmParams()
        lib().mvsv_sgbm_params_create(ctypes.byref(p), int(minDisparity), int(numDisparities),
                                      int(blockSize), int(P1), int(P2), int(disp12MaxDiff),
                                      int(preFilterCap), int(uniquenessRatio),
                                      int(speckleWindowSize), int(speckleRange), int(mode))
        return StereoSGBM(p)

    def _host_fn(self): return lib().mvsv_sgbm         # noqa: E704
    def _dev_fn(self): return lib().mvsv_sgbm_device   # noqa: E704

    def compute_bgr(self, left, right, disparity=None):
        """cv::StereoSGBM::compute on a CV_8UC3 pair: the Birchfield-Tomasi cost
        summed over the three channels.  (H, W, 3) or (N, H, W, 3) uint8, numpy
        arrays or torch device tensors, otherwise as :meth:`compute` (which reads
        a 3-D array as a batch of grey frames, so the colour form has its own
        name).  Rows may be padded; pixels must be 3 contiguous bytes."""
        if _is_torch(left) != _is_torch(right):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "StereoSGBM: left and right must both be numpy or both torch")
        if _is_torch(left):
            return _run_device_bgr(lib().mvsv_sgbm_bgr_device, self._params, left, right, disparity, "StereoSGBM")
        return _run_host_bgr(lib().mvsv_sgbm_bgr, self._params, left, right, disparity, "StereoSGBM")

    def compute_census(self, left, right, disparity=None, window=(9, 7)):
        """StereoSGBM on the census cost (mvsv_sgbm_census): the pixel cost is the Hamming
        distance of the two views' census descriptors over the ``window`` = (width,
        height) neighbourhood (:func:`census_transform`); everything after the pixel
        cost is :meth:`compute`'s.  Inputs and result as :meth:`compute`: (H, W) numpy
        arrays, or (H, W) / (N, H, W) torch device tensors on the current stream.
        preFilterCap has no effect; the cost is invariant under any strictly increasing
        map of either image's intensities."""
        cw, ch = (int(v) for v in window)
        if _is_torch(left) != _is_torch(right):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "StereoSGBM: left and right must both be numpy or both torch")
        if _is_torch(left):
            return _run_device(lambda *a: lib().mvsv_sgbm_census_device(*a, cw, ch), self._params, left, right,
                               disparity, "StereoSGBM")
        return _run_host(lambda *a: lib().mvsv_sgbm_census(*a, cw, ch), self._params, left, right, disparity,
                         "StereoSGBM")

    def census_validate(self, width, height, window=(9, 7)) -> bool:
        """mvsv_sgbm_census_validate: whether :meth:`compute_census` accepts these
        parameters and this window for a width x height pair (no device needed)."""
        return lib().mvsv_sgbm_census_validate(ctypes.byref(self._params), int(width), int(height),
                                               int(window[0]), int(window[1])) == 0

    def setPreFilterCap(self, v): self._params.pre_filter_cap = int(v)      # noqa: E704
    def getPreFilterCap(self): return self._params.pre_filter_cap            # noqa: E704
    def setUniquenessRatio(self, v): self._params.uniqueness_ratio = int(v)  # noqa: E704
    def getUniquenessRatio(self): return self._params.uniqueness_ratio       # noqa: E704
    def setP1(self, v): self._params.p1 = int(v)                             # noqa: E704
    def getP1(self): return self._params.p1                                  # noqa: E704
    def setP2(self, v): self._params.p2 = int(v)                             # noqa: E704
    def getP2(self): return self._params.p2                                  # noqa: E704
    def setMode(self, v): self._params.mode = int(v)                         # noqa: E704
    def getMode(self): return self._params.mode                              # noqa: E704
    def setVariant(self, v): self._params.variant = int(v)                   # noqa: E704


class StereoBM(StereoMatcher):
    """cv::StereoBM (OpenCV 3.4 semantics, CV_16S output) on the MI355X kernels."""
    PREFILTER_NORMALIZED_RESPONSE = PREFILTER_NORMALIZED_RESPONSE
    PREFILTER_XSOBEL = PREFILTER_XSOBEL

    def __init__(self, params: BmParams):
        self._params = params

    @staticmethod
    def create(numDisparities=0, blockSize=21):
        p = BmParams()
        lib().mvsv_bm_params_default(ctypes.byref(p), int(numDisparities), int(blockSize))
        return StereoBM(p)

    def _host_fn(self): return lib().mvsv_bm           # noqa: E704
    def _dev_fn(self): return lib().mvsv_bm_device     # noqa: E704

    def compute_census(self, left, right, disparity=None, window=(9, 7)):
        """StereoBM on the census cost (mvsv_bm_census): the pixel cost is the Hamming
        distance of the two views' census descriptors over the ``window`` = (width,
        height) neighbourhood (:func:`census_transform`) in place of the SAD of the
        prefiltered views; everything after the pixel cost is :meth:`compute`'s.
        Inputs and result as :meth:`compute`: (H, W) numpy arrays, or (H, W) / (N, H, W)
        torch device tensors on the current stream.  The prefilter fields and the
        texture threshold have no effect; the map is invariant under any strictly
        increasing map of either image's intensities."""
        cw, ch = (int(v) for v in window)
        if _is_torch(left) != _is_torch(right):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "StereoBM: left and right must both be numpy or both torch")
        if _is_torch(left):
            return _run_device(lambda *a: lib().mvsv_bm_census_device(*a, cw, ch), self._params, left, right,
                               disparity, "StereoBM")
        return _run_host(lambda *a: lib().mvsv_bm_census(*a, cw, ch), self._params, left, right, disparity,
                         "StereoBM")

    def census_validate(self, width, height, window=(9, 7)) -> bool:
        """mvsv_bm_census_validate: whether :meth:`compute_census` accepts these
        parameters and this window for a width x height pair (no device needed)."""
        return lib().mvsv_bm_census_validate(ctypes.byref(self._params), int(width), int(height),
                                             int(window[0]), int(window[1])) == 0

    def setPreFilterType(self, v): self._params.pre_filter_type = int(v)     # noqa: E704
    def getPreFilterType(self): return self._params.pre_filter_type          # noqa: E704
    def setPreFilterSize(self, v): self._params.pre_filter_size = int(v)     # noqa: E704
    def getPreFilterSize(self): return self._params.pre_filter_size          # noqa: E704
    def setPreFilterCap(self, v): self._params.pre_filter_cap = int(v)       # noqa: E704
    def getPreFilterCap(self): return self._params.pre_filter_cap            # noqa: E704
    def setTextureThreshold(self, v): self._params.texture_threshold = int(v)  # noqa: E704
    def getTextureThreshold(self): return self._params.texture_threshold       # noqa: E704
    def setUniquenessRatio(self, v): self._params.uniqueness_ratio = int(v)    # noqa: E704
    def getUniquenessRatio(self): return self._params.uniqueness_ratio         # noqa: E704


class Disparity:
    """namespace Disparity (inc/disparity.h:15-36)."""

    sgbmParameters = sgbmParameters

    @staticmethod
    def sgbm(inputImages: Stereopair, output, dispCompute: StereoSGBM):
        """src/disparity.cpp:6-10: forwards to compute(); returns the (re)allocated map."""
        return dispCompute.compute(inputImages.mLeft, inputImages.mRight, output)

    @staticmethod
    def sgbm_bgr(inputImages: Stereopair, output, dispCompute: StereoSGBM):
        """Disparity::sgbm on a CV_8UC3 pair (cv::StereoSGBM::compute matches in colour)."""
        return dispCompute.compute_bgr(inputImages.mLeft, inputImages.mRight, output)

    @staticmethod
    def binary_sgbm(inputImages: Stereopair, output, dispCompute: StereoSGBM, window=(9, 7)):
        """Disparity::binary_sgbm (inc/disparity.h:30, src/disparity.cpp:12-15; commented out in
        the reference as "currently not working"): SGBM on a census cost, on this engine's
        own contract (StereoSGBM.compute_census)."""
        return dispCompute.compute_census(inputImages.mLeft, inputImages.mRight, output, window)

    @staticmethod
    def bm(inputImages: Stereopair, output, dispCompute: StereoBM):
        """src/disparity.cpp:18-22."""
        return dispCompute.compute(inputImages.mLeft, inputImages.mRight, output)

    @staticmethod
    def binary_bm(inputImages: Stereopair, output, dispCompute: StereoBM, window=(9, 7)):
        """StereoBM on a census cost (StereoBM.compute_census), the counterpart of
        binary_sgbm for the fast matcher (trgt/disparityTest.cpp:267-268 runs both
        matchers side by side), on this engine's own contract."""
        return dispCompute.compute_census(inputImages.mLeft, inputImages.mRight, output, window)

    @staticmethod
    def tm(inputImages: Stereopair, output, kernelSize: int):
        """src/disparity.cpp:25-58; returns the (re)allocated 8-bit map."""
        return tm(inputImages.mLeft, inputImages.mRight, kernelSize)

    @staticmethod
    def loadSGBMParameters(filename: str, disparityObj: StereoSGBM,
                           para: sgbmParameters) -> bool:
        """src/disparity.cpp:60-108: reads configs/sgbm.yml, applies 8 setters + mode.

        P1/P2 are left untouched (programs create the matcher with P1 = P2 = 0,
        so OpenCV's effective P1 = 2, P2 = 5 apply).
        """
        vals = SgbmYamlValues()
        rc = lib().mvsv_load_sgbm_yaml(str(filename).encode(), ctypes.byref(disparityObj._params),
                                       ctypes.byref(vals))
        if rc == _lib.MVSV_E_PARSE:
            log.error("Node in %s is empty", filename)
            return False
        if rc < 0:
            log.error("Unable to open disparity parameters")
            return False
        for f in _lib.YAML_FIELDS:
            setattr(para, f, int(getattr(vals, f)))
        log.info("Successfully loaded disparity parameters")
        return True

    @staticmethod
    def loadBMParameters(filename: str, disparityObj: StereoBM) -> bool:
        """New: reads configs/bm.yml:2-7 (shipped by the reference, read by nothing)."""
        rc = lib().mvsv_load_bm_yaml(str(filename).encode(), ctypes.byref(disparityObj._params))
        if rc < 0:
            log.error("Unable to load BM parameters from %s", filename)
            return False
        return True


def tm_validate(kernel_size: int, width: int, height: int) -> bool:
    """mvsv_tm_validate: 1 <= kernel_size <= 31 and kernel_size < min(width, height)."""
    return lib().mvsv_tm_validate(int(kernel_size), int(width), int(height)) == 0


def tm(left, right, kernel_size: int, wide: bool = False):
    """Disparity::tm (src/disparity.cpp:25-58): for every pixel (i, j) with
    i < H - k and j < W - k, cv::matchTemplate(CV_TM_CCORR_NORMED) of the k x k
    template of ``left`` along the row of ``right`` (to the right, up to column
    W - 2); the first shift with the largest score is stored, 0 elsewhere.
    Scores are compared in exact integers (include/mvsv.h).

    numpy uint8 (H, W) arrays give a numpy uint8 map through the host entry.
    torch uint8 device tensors (H, W) or (N, H, W) run on the current torch
    stream and give a device tensor: uint8 (the shift's low byte, as the
    reference's ``output.at<char>`` stores it) or, with ``wide``, the shift
    itself as uint16."""
    what = "tm"
    k = int(kernel_size)
    if _is_torch(left) != _is_torch(right):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: left and right must both be numpy or both torch")
    if _is_torch(left):
        import torch
        Lt, Rt, batched = _device_pair(left, right, what)
        n, H, W = Lt.shape
        if not tm_validate(k, W, H):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: kernel size {k} not within 1..31 and below min(W, H)")
        eb = 2 if wide else 1
        out = torch.empty((n, H, W), dtype=torch.uint16 if wide else torch.uint8, device=left.device)
        ctx = device_context(left)
        check(lib().mvsv_tm_device(ctx.handle, n, Lt.data_ptr(), Lt.stride(1), Lt.stride(0), Rt.data_ptr(),
                                   Rt.stride(1), Rt.stride(0), W, H, k, out.data_ptr(), W * eb, H * W * eb, eb),
              ctx.handle)
        return out if batched else out[0]
    L, R = _host_pair(left, right, what)
    if wide:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: the 16-bit map is for device tensors (the host entry is 8 bit)")
    H, W = L.shape
    if not tm_validate(k, W, H):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: kernel size {k} not within 1..31 and below min(W, H)")
    out = np.empty((H, W), np.uint8)
    ctx = host_context()
    check(lib().mvsv_tm(ctx.handle, L.ctypes.data, L.strides[0], R.ctypes.data, R.strides[0], W, H, k,
                        out.ctypes.data, out.strides[0]), ctx.handle)
    return out


def census_transform(img, window=(9, 7)):
    """The census descriptors :meth:`StereoSGBM.compute_census` matches on (mvsv_census):
    uint64 per pixel, bit k = 1 iff the k-th window offset's pixel (row-major over the
    ``window`` = (width, height) neighbourhood, centre skipped, clamped into the image)
    is darker than the centre.  (H, W) uint8 numpy array -> numpy uint64; (H, W) or
    (N, H, W) uint8 torch device tensor -> device tensor of int64 holding the same bits
    (torch has no general uint64), on the current stream."""
    cw, ch = (int(v) for v in window)
    if _is_torch(img):
        import torch
        if img.dtype != torch.uint8 or not img.is_cuda or img.dim() not in (2, 3):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "census_transform: (H, W) or (N, H, W) uint8 device tensor expected")
        t = img if img.dim() == 3 else img.unsqueeze(0)
        if t.stride(2) != 1:
            t = t.contiguous()
        n, H, W = t.shape
        out = torch.empty((n, H, W), dtype=torch.int64, device=img.device)
        ctx = device_context(img)
        check(lib().mvsv_census_device(ctx.handle, n, t.data_ptr(), t.stride(1), t.stride(0), W, H, cw, ch,
                                       out.data_ptr(), W, H * W), ctx.handle)
        return out if img.dim() == 3 else out[0]
    a = np.asarray(img)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "census_transform: a 2-D uint8 image expected")
    if a.strides[1] != 1:
        a = np.ascontiguousarray(a)
    H, W = a.shape
    out = np.empty((H, W), np.uint64)
    ctx = host_context()
    check(lib().mvsv_census(ctx.handle, a.ctypes.data, a.strides[0], W, H, cw, ch, out.ctypes.data, W), ctx.handle)
    return out


def synth_pair(seed: int, width: int, height: int, min_disparity: int, num_disparities: int):
    """Deterministic synthetic rectified pair; host uint8 arrays."""
    L = np.empty((height, width), np.uint8)
    R = np.empty((height, width), np.uint8)
    check(lib().mvsv_synth_pair(ctypes.c_uint32(seed & 0xFFFFFFFF), width, height,
                                min_disparity, num_disparities, L.ctypes.data, R.ctypes.data))
    return L, R


def mean_disparity_grid(dmap):
    """MeanDisparityDetection::build(MEAN_VALUE) on device: (N,81) or (81,) float32."""
    import torch
    d, batched, ctx = _device_frames(dmap, "mean_disparity_grid", any_rank=True)
    n, H, W = d.shape
    out = torch.empty((n, 81), dtype=torch.float32, device=dmap.device)
    check(lib().mvsv_mean_disparity_grid_device(ctx.handle, n, d.data_ptr(), d.stride(1),
                                                d.stride(0), W, H, out.data_ptr()), ctx.handle)
    return out if batched else out[0]


def _post_map(t, what):
    """(N, H, W) view of an (H, W) or (N, H, W) int16 device map, and whether it was batched; the
    callers check the column stride."""
    import torch
    if not _is_torch(t) or not t.is_cuda or t.dtype != torch.int16 or t.dim() not in (2, 3):
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: (H, W) or (N, H, W) int16 device tensor expected")
    return (t if t.dim() == 3 else t.unsqueeze(0)), t.dim() == 3


def median_blur3(dmap, out=None):
    """cv::medianBlur(dmap, out, 3) on device: the 3x3 median (replicate border) of an
    (H, W) or (N, H, W) int16 device tensor.  Views reach the kernels as views (row and
    frame strides, storage offset); `out`, if given, is a tensor of the same shape that
    does not overlap `dmap` and may be a view too."""
    import torch
    s, batched = _post_map(dmap, "median_blur3")
    if s.stride(2) != 1:
        s = s.contiguous()
    n, H, W = s.shape
    if out is None:
        out = torch.empty(dmap.shape, dtype=torch.int16, device=dmap.device)
    d, _ = _post_map(out, "median_blur3")
    if out.shape != dmap.shape or out.device != dmap.device or d.stride(2) != 1:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "median_blur3: out must match the map and have unit column stride")
    ctx = device_context(dmap)
    check(lib().mvsv_median_blur3_device(ctx.handle, n, s.data_ptr(), s.stride(1), s.stride(0), d.data_ptr(),
                                         d.stride(1), d.stride(0), W, H), ctx.handle)
    return out


def filter_speckles(dmap, new_val, max_size, max_diff):
    """cv::filterSpeckles(dmap, new_val, max_size, max_diff) on device, in place on an
    (H, W) or (N, H, W) int16 device tensor (a view is filtered as a view); returns dmap."""
    d, _ = _post_map(dmap, "filter_speckles")
    if d.stride(2) != 1:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "filter_speckles: unit column stride expected (in place)")
    n, H, W = d.shape
    ctx = device_context(dmap)
    check(lib().mvsv_filter_speckles_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                            int(new_val), int(max_size), int(max_diff)), ctx.handle)
    return dmap


# mvsv_sample_hit (include/mvsv.h): a lattice point inside the range and its calcCoordinate
SAMPLE_HIT_DTYPE = np.dtype([("index", "<i4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4")])


def samplepoint_layout(width, height):
    """SamplepointDetection::init's lattice of a width x height map:
    (step_x, step_y, nx, ny); point (c, r) is at ((c + 1) * step_x, (r + 1) * step_y)
    and has index c * ny + r.  nx * ny == 0 for a map narrower or lower than 16."""
    v = [ctypes.c_int() for _ in range(4)]
    check(lib().mvsv_samplepoint_layout(int(width), int(height), *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def samplepoint_values(dmap, radius=2):
    """SamplepointDetection::build on device: the value of every lattice point of
    an int16 device map, (N, nx * ny) or (nx * ny,) float32 in the reference's
    (column-major) point order."""
    import torch
    d, batched, ctx = _device_frames(dmap, "samplepoint_values", any_rank=True)
    n, H, W = d.shape
    _, _, nx, ny = samplepoint_layout(W, H)
    out = torch.empty((n, nx * ny), dtype=torch.float32, device=dmap.device)
    check(lib().mvsv_samplepoint_values_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                               int(radius), out.data_ptr()), ctx.handle)
    return out if batched else out[0]


def samplepoint_detect(values, shape, Q, range_disparity, max_hits=None):
    """SamplepointDetection::detectObstacles on device.  values: (N, nx * ny) or
    (nx * ny,) float32 device tensor of a map of shape = (rows, cols);
    range_disparity = (first, second): a hit has second < value < first.
    Returns (counts, hits): int32 (N,) and uint8 (N, max_hits, 16) device tensors,
    hits holding mvsv_sample_hit records (view the host copy as SAMPLE_HIT_DTYPE),
    the first min(count, max_hits) of each frame in index order; max_hits=None:
    room for every point.  Without the batch dimension: (count, hits[max_hits, 16])."""
    import torch
    if not _is_torch(values) or not values.is_cuda or values.dtype != torch.float32:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "samplepoint_detect: float32 device tensor expected")
    batched = values.dim() == 2
    v = (values if batched else values.unsqueeze(0)).contiguous()
    H, W = int(shape[0]), int(shape[1])
    _, _, nx, ny = samplepoint_layout(W, H)
    if v.shape[1] != nx * ny:
        raise MvsvError(_lib.MVSV_E_INVALID_ARG, "samplepoint_detect: values do not match the map's lattice")
    n = v.shape[0]
    cap = nx * ny if max_hits is None else int(max_hits)
    counts = torch.zeros((n,), dtype=torch.int32, device=values.device)
    hits = torch.zeros((n, cap, 16), dtype=torch.uint8, device=values.device)
    q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(16))
    ctx = device_context(values)
    check(lib().mvsv_samplepoint_detect_device(ctx.handle, n, v.data_ptr(), W, H, q.ctypes.data,
                                               float(range_disparity[0]), float(range_disparity[1]), cap,
                                               counts.data_ptr(), hits.data_ptr() if cap else None),
          ctx.handle)
    return (counts, hits) if batched else (counts[0], hits[0])
