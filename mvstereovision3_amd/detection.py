"""MeanDisparityDetection, SamplepointDetection and the camera-loop frame stream.

Mirrors src/MeanDisparityDetection.cpp:71-266, inc/Subimage.h:17-47,
trgt/mean_test.cpp:80-106 (createDMapROIS) and replaces the disparity worker
thread of trgt/mean_test.cpp:61-70 with DisparityStream (mvsv_stream_*: upload,
SGBM + 9x9 mean grid on the device, download, overlapped on HIP streams).
The 81 tile means are computed on the GPU (mean_grid_kernel); the 81-element
decisions stay on the host, exactly as the reference orders them.
SamplepointDetection (src/SamplePointDetection.cpp:29-178, inc/Samplepoint.h:17-40) is
the lattice detector: its values come from sample_grid_kernel, its decisions from the
host or, on a stream, from sample_detect_kernel's hit records.
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref

import numpy as np

from . import _lib
from ._lib import MvsvError, Rect, check, context, host_context, lib
from .utility import PLY_WITH_COLOR, Utility, _host_map, dMapValues, ply

MEAN_DISTANCE = 0
MEAN_VALUE = 1

# src/MeanDisparityDetection.cpp:21-66 (note: key 10 is absent, 81 is present)
POSITIONS = {}
_groups = ["TOP LEFT", "TOP", "TOP RIGHT", "LEFT", "CENTER", "RIGHT", "BOTTOM LEFT", "BOTTOM",
           "BOTTOM RIGHT"]
for _k in range(9):
    POSITIONS[_k] = f"TOP LEFT - {_k}"
POSITIONS.update({9: "TOP - 0"})
for _k in range(1, 9):
    POSITIONS[10 + _k] = f"TOP - {_k}"
for _g, _base in zip(_groups[2:], range(19, 82, 9)):
    for _k in range(9):
        POSITIONS[_base + _k] = f"{_g} - {_k}"


def create_dmap_rois(reference_shape, num_disp, binning=0, reload=False):
    """createDMapROIS (trgt/mean_test.cpp:80-106) -> (roi_u, roi_b) as (x0, y0, x1, y1)."""
    rows, cols = reference_shape
    shift = num_disp // 2
    if shift % 2 == 1:
        shift = shift + 1
        if (cols - shift) % 8 != 0:
            shift = shift + (cols - shift % 8)  # sic: operator precedence as in the reference
    roi_u = (shift, 0, cols, rows)
    roi_b = (shift // 2, 0, cols // 2, rows // 2)
    return roi_u, roi_b


class Subimage:
    """inc/Subimage.h: a tile with its centre and mean disparity value."""

    def __init__(self, tl=(0, 0), br=(0, 0)):
        self.tl = tuple(tl)
        self.br = tuple(br)
        tx, ty = br[0] - tl[0], br[1] - tl[1]
        self.roi_center = (tl[0] + int(tx / 2), tl[1] + int(ty / 2))
        self.value = 0.0

    def calculateSubimageValue(self, dMap):
        self.value = Utility.calcMeanDisparity(np.asarray(dMap)[self.tl[1]:self.br[1],
                                                                self.tl[0]:self.br[0]])


class MeanDisparityDetection:
    """src/MeanDisparityDetection.cpp with the 9x9 means computed on the GPU."""

    MEAN_DISTANCE = MEAN_DISTANCE
    MEAN_VALUE = MEAN_VALUE

    def __init__(self, pcl_dir="pcl/subimage_detection"):
        self.mSubimageVec: list[Subimage] = []
        self.mFoundObstacles: list[Subimage] = []
        self.mMeanMap: list[float] = []
        self.mMeanDistanceMap: list[float] = []
        self.mFoundPoints: list[np.ndarray] = []
        self.mObstacleCounter = 0
        self.mRange = (0.0, 0.0)
        self.mRangeDisparity = (0.0, 0.0)
        self.mDetectionMode = None
        self.mQ_32F = None
        self.mDMap = None
        self.pcl_dir = pcl_dir

    def init(self, reference, Q, min_distance, max_distance):
        """:71-112 — 9x9 tiles of (cols/9) x (rows/9) and the disparity range of [min, max] m."""
        shape = reference if isinstance(reference, tuple) else np.asarray(reference).shape
        rows, cols = shape[0], shape[1]
        self.mSubimageVec = []
        self.mQ_32F = np.asarray(Q, np.float32).reshape(4, 4)
        dx, dy = cols // 9, rows // 9
        for r in range(9):
            for c in range(9):
                tl = (c * dx, r * dy)
                br = (c * dx + dx, r * dy + dy)
                self.mSubimageVec.append(Subimage(tl, br))
                self.mFoundObstacles.append(Subimage(tl, br))
        # detectObstacles' batched coordinate call: tile centres and Q as float32
        self._centers = np.array([s.roi_center for s in self.mSubimageVec], np.float32).reshape(81, 2)
        self._q16 = np.ascontiguousarray(self.mQ_32F.reshape(16))
        lo = Utility.calcDMapValues([0, 0, np.float32(min_distance) * np.float32(1000)], self.mQ_32F)
        hi = Utility.calcDMapValues([0, 0, np.float32(max_distance) * np.float32(1000)], self.mQ_32F)
        self.mRangeDisparity = (lo.dValue, hi.dValue)

    def setRange(self, min_distance, max_distance):
        self.mRange = (float(np.float32(min_distance)), float(np.float32(max_distance)))

    def getRange(self):
        # ObstacleDetection::mRange is pair<float,float>; the derived getter returns pair<int,int>
        return int(self.mRange[0]), int(self.mRange[1])

    def getSubimageVec(self):
        return self.mSubimageVec

    def getMeanMap(self):
        return self.mMeanMap

    def getMeanDistanceMap(self):
        return self.mMeanDistanceMap

    def getFoundObstacles(self):
        return self.mFoundObstacles

    def getObstacleCounter(self):
        return self.mObstacleCounter

    def build(self, dMap, binning=0, mode=MEAN_VALUE, means=None):
        """:159-206.  dMap: host int16 map (or torch tensor on a HIP device).

        The tile means come from the GPU grid kernel (or `means`, e.g. from a
        DisparityStream pop).  MEAN_DISTANCE falls through into MEAN_VALUE, as the
        reference's switch does (no break), so the mode ends as MEAN_VALUE.
        """
        self.mDMap = dMap
        m = self._grid(dMap) if means is None else np.asarray(means, np.float32).reshape(81)
        if mode == MEAN_DISTANCE:
            self.mDetectionMode = MEAN_DISTANCE
            self.mMeanDistanceMap = []
            for i, s in enumerate(self.mSubimageVec):
                v = dMapValues(m[i], s.roi_center[0], s.roi_center[1])
                self.mMeanDistanceMap.append(Utility.calcDistance(v, self.mQ_32F, 0))
            mode = MEAN_VALUE
        if mode == MEAN_VALUE:
            self.mDetectionMode = MEAN_VALUE
            self.mMeanMap = m.tolist()
            for s, v in zip(self.mSubimageVec, self.mMeanMap):
                s.value = v

    def _grid(self, dMap):
        if type(dMap).__module__.startswith("torch"):
            from .disparity import mean_disparity_grid
            return mean_disparity_grid(dMap).cpu().numpy()
        d = _host_map(dMap, "build")
        out = np.empty(81, np.float32)
        ctx = host_context()
        check(lib().mvsv_mean_disparity_grid(ctx.handle, d.ctypes.data, d.strides[0] // 2,
                                             d.shape[1], d.shape[0], out.ctypes.data), ctx.handle)
        return out

    def detectObstacles(self, write_pcl=True):
        """:211-266.  Returns the list of position strings printed in MEAN_DISTANCE mode."""
        printed = []
        if self.mDetectionMode == MEAN_DISTANCE:
            for i, dist in enumerate(self.mMeanDistanceMap):
                if self.mRange[1] > dist > self.mRange[0]:
                    printed.append(POSITIONS.get(i, ""))
            return printed
        if self.mDetectionMode != MEAN_VALUE:
            return printed
        lo, hi = np.float32(self.mRangeDisparity[0]), np.float32(self.mRangeDisparity[1])
        # the reference's per-tile test (float32 compares) over all 81 means at
        # once, then every found tile's coordinate in one native call
        means = np.asarray(self.mMeanMap, np.float32)
        found = np.flatnonzero((means < lo) & (means > hi))
        self.mFoundObstacles = [self.mSubimageVec[i] for i in found]
        self.mFoundPoints = []
        if found.size:
            xyd = np.empty((found.size, 3), np.float32)
            xyd[:, 0] = self._centers[found, 0]
            xyd[:, 1] = self._centers[found, 1]
            xyd[:, 2] = means[found]
            pts = np.empty((found.size, 4), np.float32)
            lib().mvsv_calc_coordinates(int(found.size), xyd.ctypes.data, self._q16.ctypes.data, pts.ctypes.data)
            self.mFoundPoints = list(pts)
        if self.mFoundPoints and write_pcl:
            c = self.mObstacleCounter
            prefix = "000" if c < 10 else ("00" if c < 100 else "0")
            path = os.path.join(self.pcl_dir, f"pcl_{prefix}{c}.ply")
            dm = self.mDMap.cpu().numpy() if type(self.mDMap).__module__.startswith("torch") \
                else np.asarray(self.mDMap)
            ply("Hagen Hiller", "obstacle pointcloud", dm).write(path, np.stack(self.mFoundPoints),
                                                                 PLY_WITH_COLOR)
            self.mObstacleCounter += 1
        return printed


class Samplepoint:
    """inc/Samplepoint.h: a (2 * radius + 1)^2 patch around a lattice point."""

    def __init__(self, center=(0, 0), radius=0):
        self.center = (int(center[0]), int(center[1]))
        self.radius = int(radius)
        # cv::Rect(p1, p2) as (x, y, width, height)
        self.roi = (self.center[0] - self.radius, self.center[1] - self.radius, 2 * self.radius + 1,
                    2 * self.radius + 1)
        self.value = 0.0

    def calculateSamplepointValue(self, dMap):
        d = np.asarray(dMap)
        if self.radius > 0:
            x, y, w, h = self.roi
            self.value = Utility.calcMeanDisparity(d[y:y + h, x:x + w])
        else:
            self.value = float(d[self.center[1], self.center[0]])


class SamplepointDetection:
    """src/SamplePointDetection.cpp with the lattice values computed on the GPU.

    A lattice of 5x5 patches, one every step_x x step_y pixels (8 for most
    sizes), in the reference's order: columns in the outer loop, rows inside.
    build() fills the values (sample_grid_kernel, or `values` from a
    DisparityStream frame); detectObstacles() keeps the points whose value lies
    inside the disparity range of [min, max] metres and reprojects them.
    """

    RADIUS = 2  # src/SamplePointDetection.cpp:43

    def __init__(self, pcl_dir="pcl/samplepoint_detection"):
        self.mSPVec: list[Samplepoint] = []
        self.mFoundObstacles: list[Samplepoint] = []
        self.mDistanceVec: list[float] = []
        self.mFoundPoints: list[np.ndarray] = []
        self.mCenterVec = np.array([0.0, 0.0, 1.0, 0.0], np.float32)
        self.mImageCenter = (0, 0)
        self.mObstacleCounter = 0
        self.mRange = (0.0, 0.0)
        self.mRangeDisparity = (0.0, 0.0)
        self.mQ_32F = None
        self.mDMap = None
        self.pcl_dir = pcl_dir
        self._shape = None
        self._centers = np.empty((0, 2), np.float32)
        self._q16 = None

    def init(self, reference, Q, min_distance, max_distance):
        """:29-75 — the lattice of `reference`'s size and the disparity range of [min, max] m."""
        shape = reference if isinstance(reference, tuple) else np.asarray(reference).shape
        rows, cols = int(shape[0]), int(shape[1])
        self._shape = (rows, cols)
        self.mSPVec = []
        self.mQ_32F = np.asarray(Q, np.float32).reshape(4, 4)
        distance_x, distance_y = cols // 8, rows // 8
        for c in range(1, distance_x):
            for r in range(1, distance_y):
                center = (c * (cols // distance_x), r * (rows // distance_y))
                self.mSPVec.append(Samplepoint(center, self.RADIUS))
                # the layout, for the visualisation, until the first detectObstacles
                self.mFoundObstacles.append(Samplepoint(center, self.RADIUS))
        self.mCenterVec = np.array([0.0, 0.0, 1.0, 0.0], np.float32)
        self.mImageCenter = (int(self.mQ_32F[0, 3]), int(self.mQ_32F[1, 3]))  # cv::Point = Point2i
        self._centers = np.array([s.center for s in self.mSPVec], np.float32).reshape(len(self.mSPVec), 2)
        self._q16 = np.ascontiguousarray(self.mQ_32F.reshape(16))
        lo = Utility.calcDMapValues([0, 0, np.float32(min_distance) * np.float32(1000)], self.mQ_32F)
        hi = Utility.calcDMapValues([0, 0, np.float32(max_distance) * np.float32(1000)], self.mQ_32F)
        self.mRangeDisparity = (lo.dValue, hi.dValue)

    def setRange(self, min_distance, max_distance):
        """Stored only: detection uses the disparity range set by init, as in the reference."""
        self.mRange = (float(np.float32(min_distance)), float(np.float32(max_distance)))

    def getRange(self):
        return int(self.mRange[0]), int(self.mRange[1])

    def getRangeDisparity(self):
        return self.mRangeDisparity

    def getSamplepointVec(self):
        return self.mSPVec

    def getCenterPoint(self):
        return self.mCenterVec

    def getFoundObstacles(self):
        return self.mFoundObstacles

    def getFoundPoints(self):
        return self.mFoundPoints

    def getObstacleCounter(self):
        return self.mObstacleCounter

    def build(self, dMap, binning=0, mode=0, values=None):
        """:117-129 (binning and mode are ignored there too).  dMap: host int16 map
        or torch device tensor of init's size; values: the lattice values if they
        are at hand already (DisparityStream.front_samples)."""
        self.mDMap = dMap
        n = len(self.mSPVec)
        if values is not None:
            v = np.asarray(values, np.float32).reshape(-1)
            if v.size != n:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "build: one value per sample point expected")
        else:
            shape = tuple(dMap.shape)
            if shape != self._shape:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "build: a map of init's size expected")
            v = self._values(dMap, n)
        self.mDistanceVec = v.tolist()
        for s, x in zip(self.mSPVec, self.mDistanceVec):
            s.value = x

    def _values(self, dMap, n):
        if type(dMap).__module__.startswith("torch"):
            from .disparity import samplepoint_values
            return samplepoint_values(dMap, self.RADIUS).cpu().numpy()
        d = _host_map(dMap, "build")
        out = np.empty(n, np.float32)
        if n:
            ctx = host_context()
            check(lib().mvsv_samplepoint_values(ctx.handle, d.ctypes.data, d.strides[0] // 2, d.shape[1],
                                                d.shape[0], self.RADIUS, out.ctypes.data), ctx.handle)
        return out

    def detectObstacles(self, write_pcl=True, hits=None):
        """:134-178.  hits: the (count, records) a DisparityStream frame brought
        back (front_samples) instead of the host decision; records beyond the
        stream's max_hits are not in it, so neither in the result."""
        values = np.asarray(self.mDistanceVec, np.float32)
        if hits is not None:
            if values.size != len(self.mSPVec):
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "detectObstacles: build() has not run")
            count, rec = hits
            rec = np.asarray(rec)[:int(count)]
            found = rec["index"].astype(np.int64)
            if found.size and (found.min() < 0 or found.max() >= values.size):
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "detectObstacles: hit outside the lattice")
            pts = np.empty((found.size, 4), np.float32)
            pts[:, 0], pts[:, 1], pts[:, 2] = rec["x"], rec["y"], rec["z"]
            # calcCoordinate's fourth element W * (float)(1 / W), which a record does
            # not carry: Q's last row in mvsv_calc_coordinate's arithmetic
            q = self._q16[12:].astype(np.float64)
            c = self._centers[found].astype(np.float64)
            d = (values[found] / np.float32(16)).astype(np.float64)
            w = (((0.0 + q[0] * c[:, 0]) + q[1] * c[:, 1]) + q[2] * d + q[3]).astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                pts[:, 3] = w * (1.0 / w.astype(np.float64)).astype(np.float32)
        else:
            lo, hi = np.float32(self.mRangeDisparity[0]), np.float32(self.mRangeDisparity[1])
            # the reference's per-point test (float32 compares) over the lattice at
            # once, then every found point's coordinate in one native call
            found = np.flatnonzero((values < lo) & (values > hi))
            pts = np.empty((found.size, 4), np.float32)
            if found.size:
                xyd = np.empty((found.size, 3), np.float32)
                xyd[:, :2] = self._centers[found]
                xyd[:, 2] = values[found]
                lib().mvsv_calc_coordinates(int(found.size), xyd.ctypes.data, self._q16.ctypes.data,
                                            pts.ctypes.data)
        self.mFoundObstacles = []
        for i in found:
            s = Samplepoint(self.mSPVec[i].center, self.mSPVec[i].radius)
            s.value = float(values[i])
            self.mFoundObstacles.append(s)
        self.mFoundPoints = list(pts)
        if self.mFoundPoints and write_pcl:
            c = self.mObstacleCounter
            prefix = "000" if c < 10 else ("00" if c < 100 else "0")
            path = os.path.join(self.pcl_dir, f"pcl_{prefix}{c}.ply")
            dm = self.mDMap.cpu().numpy() if type(self.mDMap).__module__.startswith("torch") \
                else np.asarray(self.mDMap)
            ply("Hagen Hiller", "obstacle pointcloud", dm).write(path, pts, PLY_WITH_COLOR)
            self.mObstacleCounter += 1


class _DeviceSpan:
    """Device memory owned by someone else (float32 by default), for torch.as_tensor (no copy)."""

    def __init__(self, ptr, shape, owner, typestr="<f4"):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class DisparityStream:
    """Double-buffered camera-loop pipeline over mvsv_stream (include/mvsv.h).

    push(left, right) uploads a rectified pair and enqueues SGBM (+ the 9x9
    mean grid of grid_roi); pop() returns (disparity int16, means[81] or None)
    in push order.  `depth` frames may be in flight; with batch > 1 they are
    computed in groups of `batch` frames (frame-batch kernels); with inflight > 1
    up to that many groups run concurrently on the stream's compute lanes.
    DisparityStream.raw(...) opens the same pipeline for raw camera pairs
    (push_raw): rectification, crop and resize run on the device too.
    matcher: a StereoSGBM or a StereoBM (mvsv_stream_create_bm), here and in
    set_params, which may switch between the two; anything else raises.
    enable_bgr / push_bgr: colour pairs, halved and converted on the device.
    Device ends: push / push_raw / push_bgr also take torch uint8 tensors on the
    stream's device, one frame or N frames with a leading axis, ordered against
    torch's current stream by events (no synchronisation; the source may be
    overwritten or freed on that stream right after the call).
    pop(copy_map="device"), front_map(device=True), front_display(copy="device"),
    front_view(copy="device") and front_rectified() hand the results out on the
    device; host_outputs(...) switches the per-frame downloads off; fence() is for
    zero-copy readers.
    """

    @staticmethod
    def _matcher_kind(matcher):
        """MATCHER_SGBM / MATCHER_BM of a matcher object, by its parameter block."""
        p = getattr(matcher, "_params", None)
        if isinstance(p, _lib.SgbmParams):
            return _lib.MATCHER_SGBM
        if isinstance(p, _lib.BmParams):
            return _lib.MATCHER_BM
        raise MvsvError(_lib.MVSV_E_INVALID_ARG,
                        f"DisparityStream: a StereoSGBM or StereoBM matcher expected, not {type(matcher).__name__}")

    def __init__(self, matcher, width, height, depth=3, grid_roi=None, device=0, batch=1,
                 inflight=1):
        self._h = None
        self._close_pending = False
        kind = self._matcher_kind(matcher)
        self._ctx = context(device)
        self.width, self.height = width, height
        self._params = matcher._params
        self._grid = grid_roi is not None
        roi = Rect(*grid_roi) if grid_roi is not None else None
        h = ctypes.c_void_p()
        create = lib().mvsv_stream_create_bm if kind == _lib.MATCHER_BM else lib().mvsv_stream_create
        check(create(self._ctx.handle, width, height, ctypes.byref(self._params),
                     depth, ctypes.byref(roi) if roi is not None else None,
                     ctypes.byref(h)), self._ctx.handle)
        self._raw_shape = None
        self._keep = False
        self._opened(h, batch, inflight)

    @classmethod
    def raw(cls, matcher, stereosystem_or_maps, roi=None, factor=None, depth=3, grid_roi=None,
            batch=1, inflight=1, keep_rectified=False, device=0):
        """A stream that takes the raw camera pair (mvsv_stream_create_raw): the
        camera loop of trgt/liveDisparity.cpp:82-101 as push_raw / pop.

        stereosystem_or_maps: a calibration.Stereosystem (initialised here if it
        is not yet; its mMap1 / mMap2 / mDisplayROI are used), or the four float32
        maps (left x, left y, right x, right y) of the raw frame's size with
        roi = (x0, y0, x1, y1) (default: the whole frame).  The maps are converted
        once to fixed point and stay on the device; each push_raw uploads the raw
        pair only, and remap, crop and (with factor) cv::resize run on the device
        ahead of SGBM.  The stream's frames (.width x .height) are the ROI, or
        resize_size(ROI, factor) with a factor (taken as a float, like the
        reference's parameter).  Every frame is resized: the reference's quirk
        that the *initialising* call of getRectifiedImagepair(pair, factor)
        returns the unresized crop (src/Stereosystem.cpp:298-311) does not apply
        here.  keep_rectified: pop(rectified=True) also returns the rectified pair.
        """
        kind = cls._matcher_kind(matcher)
        s = stereosystem_or_maps
        if hasattr(s, "initRectification"):
            if not s.mIsInit and not s.initRectification():
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "raw stream: the rectification cannot be initialised")
            maps = (s.mMap1[0], s.mMap2[0], s.mMap1[1], s.mMap2[1])
            roi = s.mDisplayROI if roi is None else roi
        else:
            maps = tuple(s)
        if len(maps) != 4 or any(m is None for m in maps):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "raw stream: four maps expected")
        ms = [np.ascontiguousarray(m, np.float32) for m in maps]
        if ms[0].ndim != 2 or any(m.shape != ms[0].shape for m in ms):
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "raw stream: four maps of the raw frame's size expected")
        rh, rw = ms[0].shape
        roi = (0, 0, rw, rh) if roi is None else tuple(int(v) for v in roi)
        r = _lib.Rectification()
        r.raw_width, r.raw_height, r.map_stride = rw, rh, rw
        for i, m in enumerate(ms):
            r.maps[i] = m.ctypes.data
        r.roi = Rect(*roi)
        r.factor = 0.0 if factor is None else float(np.float32(factor))
        r.keep_rectified = 1 if keep_rectified else 0
        self = cls.__new__(cls)
        self._ctx = context(device)
        self._params = matcher._params
        self._grid = grid_roi is not None
        g = Rect(*grid_roi) if grid_roi is not None else None
        h = ctypes.c_void_p()
        self._h = None
        self._close_pending = False
        create = lib().mvsv_stream_create_raw_bm if kind == _lib.MATCHER_BM else lib().mvsv_stream_create_raw
        check(create(self._ctx.handle, ctypes.byref(r), ctypes.byref(self._params),
                     depth, ctypes.byref(g) if g is not None else None,
                     ctypes.byref(h)), self._ctx.handle)
        w, hh = ctypes.c_int(), ctypes.c_int()
        check(lib().mvsv_stream_size(h, ctypes.byref(w), ctypes.byref(hh)), self._ctx.handle)
        self.width, self.height = w.value, hh.value
        self._raw_shape = (rh, rw)
        self._keep = bool(keep_rectified)
        self._opened(h, batch, inflight)
        return self

    def _opened(self, h, batch, inflight):
        self._h = h
        # pinned host slots stay allocated while pop views are alive: a view's
        # buffer references the stream, and close() defers the destroy until
        # the last view is gone (use-after-free otherwise)
        self._live_views = 0
        self._close_pending = False
        # pop views are released by weakref finalizers, which may run from GC on
        # any thread: the view count, the pending close and the destroy share a lock
        self._views_lock = threading.RLock()
        if batch != 1:
            self.set_batch(batch)
        if inflight != 1:
            self.set_inflight(inflight)

    def set_inflight(self, n):
        """Up to n frame-batch launches in flight (mvsv_stream_set_inflight)."""
        check(lib().mvsv_stream_set_inflight(self._h, int(n)), self._ctx.handle)

    def set_batch(self, batch):
        """Compute frames `batch` at a time (mvsv_stream_set_batch)."""
        check(lib().mvsv_stream_set_batch(self._h, int(batch)), self._ctx.handle)

    def set_params(self, matcher):
        """New parameters -- and the matcher, StereoSGBM or StereoBM -- for the frames
        pushed from now on (mvsv_stream_set_params / mvsv_stream_set_bm_params)."""
        kind = self._matcher_kind(matcher)
        setter = lib().mvsv_stream_set_bm_params if kind == _lib.MATCHER_BM else lib().mvsv_stream_set_params
        check(setter(self._live(), ctypes.byref(matcher._params)), self._ctx.handle)
        self._params = matcher._params

    def matcher(self):
        """MATCHER_SGBM or MATCHER_BM: what computes the frames pushed from now on."""
        return int(lib().mvsv_stream_matcher(self._live()))

    def enable_bgr(self, src_shape, halve=True, variant=_lib.GRAY_Q14):
        """The stream (of rectified pairs) also takes colour pairs from now on:
        src_shape = (height, width) of the BGR frames, whose prepare_size must be the
        stream's size; each pushed pair is uploaded as BGR and utility.prepare_gray
        runs on the device ahead of the matcher (mvsv_stream_enable_bgr).  Only while
        no frame is pending.  A BGR frame's sharpness is that of its prepared pair."""
        h, w = int(src_shape[0]), int(src_shape[1])
        check(lib().mvsv_stream_enable_bgr(self._live(), w, h, 1 if halve else 0, int(variant)), self._ctx.handle)
        self._bgr_shape = (h, w, 3)

    def disable_bgr(self):
        check(lib().mvsv_stream_disable_bgr(self._live()), self._ctx.handle)
        self._bgr_shape = None

    def bgr_match(self, on=True):
        """The maps of the colour pairs pushed from now on come from the colour matcher
        (StereoSGBM.compute_bgr) on the pair at the stream's size -- the halved BGR
        pair, or the pushed one without halving -- instead of the prepared grey pair,
        which still feeds sharpness and the rectified pair (mvsv_stream_set_bgr_match).
        After enable_bgr, only while no frame is pending, SGBM only; grey pushes keep
        working and never share a launch with colour-matched frames."""
        check(lib().mvsv_stream_set_bgr_match(self._live(), 1 if on else 0), self._ctx.handle)

    def census(self, window=(9, 7)):
        """Every frame pushed from now on is matched on the census cost with this
        ``window`` = (width, height) (StereoSGBM.compute_census; mvsv_stream_set_census);
        ``None`` switches back to the Birchfield-Tomasi cost.  Only while no frame is
        pending, SGBM only, and not together with colour matching; every optional stage
        follows the census map."""
        cw, ch = (0, 0) if window is None else (int(window[0]), int(window[1]))
        check(lib().mvsv_stream_set_census(self._live(), cw, ch), self._ctx.handle)

    def bm_census(self, window=(9, 7)):
        """The same for a StereoBM stream (StereoBM.compute_census;
        mvsv_stream_set_bm_census): every frame pushed from now on is matched on the
        census cost with this ``window``; ``None`` switches back to the SAD cost.  Only
        while no frame is pending and with the StereoBM matcher; while it is on a switch
        to SGBM is refused."""
        cw, ch = (0, 0) if window is None else (int(window[0]), int(window[1]))
        check(lib().mvsv_stream_set_bm_census(self._live(), cw, ch), self._ctx.handle)

    def push_bgr(self, left, right):
        """Push a colour pair: uint8 (height, width, 3) BGR arrays of enable_bgr's shape."""
        self._live()
        shape = getattr(self, "_bgr_shape", None)
        if shape is None:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "push_bgr: enable_bgr first (a stream of rectified pairs)")
        if self._on_device(left) or self._on_device(right):
            return self._push_device(lib().mvsv_stream_push_bgr_device, left, right, shape, "push_bgr")
        L = np.asarray(left)
        R = np.asarray(right)
        if L.shape != shape or R.shape != shape or L.dtype != np.uint8 or R.dtype != np.uint8:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "push_bgr: uint8 BGR pair of enable_bgr's shape expected")
        if L.strides[1:] != (3, 1):
            L = np.ascontiguousarray(L)
        if R.strides[1:] != (3, 1):
            R = np.ascontiguousarray(R)
        check(lib().mvsv_stream_push_bgr(self._h, L.ctypes.data, L.strides[0], R.ctypes.data, R.strides[0]),
              self._ctx.handle)

    def pending(self):
        return int(lib().mvsv_stream_pending(self._h))

    def _live(self):
        if self.closed:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "stream is closed")
        return self._h

    @staticmethod
    def _on_device(x):
        """A torch tensor in device memory (numpy arrays and CPU tensors take the host path)."""
        return getattr(x, "is_cuda", False) is True

    def _push_device(self, fn, left, right, shape, what):
        """One frame (`shape`) or N frames (N, *shape) from torch device tensors
        (mvsv_stream_push*_device), ordered against torch's current stream."""
        import torch
        bad = MvsvError(_lib.MVSV_E_INVALID_ARG,
                        f"{what}: a pair of uint8 tensors of shape {shape} or (N, *{shape}) on the stream's device expected")
        if not (self._on_device(left) and self._on_device(right)):
            raise bad
        dev = torch.device("cuda", self._ctx.device)
        nd = len(shape)
        inner = (3, 1) if nd == 3 else (1,)
        pair = []
        for t in (left, right):
            if t.device != dev or t.dtype != torch.uint8 or t.dim() not in (nd, nd + 1) \
                    or tuple(t.shape[-nd:]) != tuple(shape) or t.shape != left.shape:
                raise bad
            if tuple(t.stride()[-len(inner):]) != inner:
                t = t.contiguous()
            pair.append(t)
        L, R = pair
        n = L.shape[0] if L.dim() == nd + 1 else 1
        fs = (lambda t: t.stride(0)) if L.dim() == nd + 1 else (lambda t: 0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(fn(self._h, n, L.data_ptr(), L.stride(-nd), fs(L), R.data_ptr(), R.stride(-nd), fs(R), stream),
              self._ctx.handle)

    def host_outputs(self, map=True, rectified=True, display=True, view=True):
        """Which per-frame products are also downloaded to the host (default: all;
        mvsv_stream_set_host_outputs).  Only while no frame is pending.  The host
        getters of a product that is switched off raise; the device getters work."""
        mask = (_lib.MVSV_HOST_MAP if map else 0) | (_lib.MVSV_HOST_RECTIFIED if rectified else 0) | \
               (_lib.MVSV_HOST_DISPLAY if display else 0) | (_lib.MVSV_HOST_VIEW if view else 0)
        check(lib().mvsv_stream_set_host_outputs(self._live(), mask), self._ctx.handle)

    def fence(self):
        """Everything the stream enqueues from now on waits for what is queued on
        torch's current stream now (mvsv_stream_fence): call it after the last read of
        a zero-copy tensor whose frame is popped while that read may still run."""
        import torch
        stream = torch.cuda.current_stream(torch.device("cuda", self._ctx.device)).cuda_stream
        check(lib().mvsv_stream_fence(self._live(), stream), self._ctx.handle)

    def _span(self, ptr, shape, typestr):
        import torch
        dev = torch.device("cuda", self._ctx.device)
        return torch.as_tensor(_DeviceSpan(ptr.value, shape, self, typestr), device=dev)

    def front_map(self, device=True):
        """(map, means) of the oldest pending frame, which stays pending: the int16
        map as a zero-copy device tensor viewing the stream's ring, read-only by
        contract and valid until the frame is popped (mvsv_stream_front_map_device)."""
        self._live()
        if not device:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "front_map: device=True expected (pop returns the host map)")
        ptr = ctypes.c_void_p()
        means = np.empty(81, np.float32) if self._grid else None
        check(lib().mvsv_stream_front_map_device(self._h, ctypes.byref(ptr),
                                                 means.ctypes.data if means is not None else None),
              self._ctx.handle)
        return self._span(ptr, (self.height, self.width), "<i2"), means

    def front_rectified(self):
        """(left, right) of the oldest pending frame of a keep_rectified stream, which
        stays pending: the rectified pair as zero-copy uint8 device tensors, read-only
        by contract and valid until the frame is popped."""
        self._live()
        pl, pr = ctypes.c_void_p(), ctypes.c_void_p()
        check(lib().mvsv_stream_front_rectified_device(self._h, ctypes.byref(pl), ctypes.byref(pr)),
              self._ctx.handle)
        shape = (self.height, self.width)
        return self._span(pl, shape, "|u1"), self._span(pr, shape, "|u1")

    def push(self, left, right):
        self._live()
        if self._on_device(left) or self._on_device(right):
            if self._raw_shape is not None:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "push: a raw stream takes push_raw")
            return self._push_device(lib().mvsv_stream_push_device, left, right, (self.height, self.width), "push")
        L = np.asarray(left)
        R = np.asarray(right)
        if L.shape != (self.height, self.width) or R.shape != L.shape or L.dtype != np.uint8 \
                or R.dtype != np.uint8:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "push: uint8 pair of the stream's size expected")
        if L.strides[1] != 1:
            L = np.ascontiguousarray(L)
        if R.strides[1] != 1:
            R = np.ascontiguousarray(R)
        check(lib().mvsv_stream_push(self._h, L.ctypes.data, L.strides[0], R.ctypes.data,
                                     R.strides[0]), self._ctx.handle)

    def push_raw(self, left, right):
        """Push a raw camera pair (a stream made by DisparityStream.raw)."""
        self._live()
        if self._raw_shape is None:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "push_raw: a stream of rectified pairs takes push")
        if self._on_device(left) or self._on_device(right):
            return self._push_device(lib().mvsv_stream_push_raw_device, left, right, self._raw_shape, "push_raw")
        L = np.asarray(left)
        R = np.asarray(right)
        if L.shape != self._raw_shape or R.shape != L.shape or L.dtype != np.uint8 or R.dtype != np.uint8:
            raise MvsvError(_lib.MVSV_E_INVALID_ARG, "push_raw: uint8 pair of the raw frame's size expected")
        if L.strides[1] != 1:
            L = np.ascontiguousarray(L)
        if R.strides[1] != 1:
            R = np.ascontiguousarray(R)
        check(lib().mvsv_stream_push_raw(self._h, L.ctypes.data, L.strides[0], R.ctypes.data,
                                         R.strides[0]), self._ctx.handle)

    def pop(self, copy_map=True, rectified=False):
        """(map, means) of the oldest frame; copy_map=False returns (None, means);
        copy_map="view" returns a read-only view of the map in the stream's pinned
        host slot (no host copy), valid until the next push.  rectified=True (a raw
        stream with keep_rectified) returns (map, means, (left, right)) with the
        frame's rectified pair.  copy_map="device": the map as a fresh int16 tensor on
        the stream's device, filled on torch's current stream (mvsv_stream_pop_device)."""
        self._live()
        if isinstance(copy_map, str) and copy_map == "device":
            import torch
            if rectified:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "pop(copy_map='device'): front_rectified() hands out the pair")
            dev = torch.device("cuda", self._ctx.device)
            out = torch.empty((self.height, self.width), dtype=torch.int16, device=dev)
            means = np.empty(81, np.float32) if self._grid else None
            check(lib().mvsv_stream_pop_device(self._h, out.data_ptr(), self.width,
                                               means.ctypes.data if means is not None else None,
                                               torch.cuda.current_stream(dev).cuda_stream), self._ctx.handle)
            return out, means
        if rectified:
            if not self._keep or copy_map == "view":
                raise MvsvError(_lib.MVSV_E_INVALID_ARG,
                                "pop(rectified=True): a raw stream with keep_rectified and a copied map expected")
            out = np.empty((self.height, self.width), np.int16) if copy_map else None
            means = np.empty(81, np.float32) if self._grid else None
            rl = np.empty((self.height, self.width), np.uint8)
            rr = np.empty_like(rl)
            check(lib().mvsv_stream_pop_pair(self._h, out.ctypes.data if out is not None else None, self.width,
                                             means.ctypes.data if means is not None else None,
                                             rl.ctypes.data, self.width, rr.ctypes.data, self.width),
                  self._ctx.handle)
            return out, means, (rl, rr)
        if copy_map == "view":
            ptr = ctypes.c_void_p()
            means = np.empty(81, np.float32) if self._grid else None
            check(lib().mvsv_stream_pop_view(self._h, ctypes.byref(ptr),
                                             means.ctypes.data if means is not None else None),
                  self._ctx.handle)
            buf = (ctypes.c_int16 * (self.width * self.height)).from_address(ptr.value)
            buf._owner = self  # numpy's base chain keeps the stream (and its slots) alive
            with self._views_lock:
                self._live_views += 1
            fin = weakref.finalize(buf, DisparityStream._view_released, self)
            fin.atexit = False  # no library calls during interpreter shutdown
            view = np.ctypeslib.as_array(buf).reshape(self.height, self.width)
            view.flags.writeable = False
            return view, means
        out = np.empty((self.height, self.width), np.int16) if copy_map else None
        means = np.empty(81, np.float32) if self._grid else None
        check(lib().mvsv_stream_pop(self._h, out.ctypes.data if out is not None else None, self.width,
                                    means.ctypes.data if means is not None else None),
              self._ctx.handle)
        return out, means

    def enable_samplepoints(self, detector_or_args, roi=None, max_hits=None):
        """SamplepointDetection's lattice on every frame from now on, computed
        after SGBM on the device (mvsv_stream_enable_samplepoints); only while
        no frame is pending.  detector_or_args: an initialised SamplepointDetection
        (its Q, radius and disparity range), or (Q, range_first, range_second[,
        radius]).  roi = (x0, y0, x1, y1): the part of the map the lattice is
        laid over -- the detector's init size (default: the whole map).
        max_hits: at most that many hit records per frame (default: all)."""
        self._live()
        d = detector_or_args
        if hasattr(d, "mRangeDisparity"):
            Q, first, second, radius = d._q16, d.mRangeDisparity[0], d.mRangeDisparity[1], d.RADIUS
            if Q is None:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, "enable_samplepoints: init() the detector first")
        else:
            Q, first, second = d[0], d[1], d[2]
            radius = d[3] if len(d) > 3 else SamplepointDetection.RADIUS
        q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(16))
        r = Rect(*(int(v) for v in roi)) if roi is not None else None
        check(lib().mvsv_stream_enable_samplepoints(self._h, ctypes.byref(r) if r is not None else None,
                                                    int(radius), q.ctypes.data, float(first), float(second),
                                                    0 if max_hits is None else int(max_hits)), self._ctx.handle)
        w, h = (self.width, self.height) if roi is None else (r.x1 - r.x0, r.y1 - r.y0)
        from .disparity import samplepoint_layout
        _, _, nx, ny = samplepoint_layout(w, h)
        self._sp_npts = nx * ny
        self._sp_cap = self._sp_npts if max_hits is None or max_hits <= 0 else min(int(max_hits), self._sp_npts)

    def disable_samplepoints(self):
        self._live()
        check(lib().mvsv_stream_disable_samplepoints(self._h), self._ctx.handle)
        self._sp_npts = None

    def front_samples(self):
        """(values, count, hits) of the oldest pending frame, which stays pending
        (pop it afterwards): the lattice values (float32), the number of hits
        and the first min(count, max_hits) hit records as a structured array
        (index, x, y, z) in index order."""
        self._live()
        from .disparity import SAMPLE_HIT_DTYPE
        npts = getattr(self, "_sp_npts", None)
        cap = self._sp_cap if npts is not None else 0
        values = np.empty(npts or 0, np.float32)
        hits = np.empty(cap, SAMPLE_HIT_DTYPE)
        count = ctypes.c_int(0)
        check(lib().mvsv_stream_front_samples(self._h, values.ctypes.data if values.size else None,
                                              ctypes.byref(count), hits.ctypes.data if cap else None, cap),
              self._ctx.handle)
        return values, count.value, hits[:min(count.value, cap)]

    def enable_display(self, roi=None, alpha=0, beta=255):
        """The 8-bit display map of every frame from now on:
        cv::normalize(dMap(roi), out, alpha, beta, NORM_MINMAX, CV_8U), computed
        after SGBM on the device (mvsv_stream_enable_display); only while no frame
        is pending.  roi = (x0, y0, x1, y1), default the whole map."""
        self._live()
        self._display_views_gone("enable_display")
        r = Rect(*(int(v) for v in roi)) if roi is not None else None
        check(lib().mvsv_stream_enable_display(self._h, ctypes.byref(r) if r is not None else None,
                                               float(alpha), float(beta)), self._ctx.handle)
        self._disp_shape = (self.height, self.width) if r is None else (r.y1 - r.y0, r.x1 - r.x0)

    def disable_display(self):
        self._live()
        self._display_views_gone("disable_display")
        check(lib().mvsv_stream_disable_display(self._h), self._ctx.handle)
        self._disp_shape = None

    def _display_views_gone(self, what):
        # the pinned display slots are reallocated: no view may point into them
        with self._views_lock:
            if getattr(self, "_disp_views", 0) > 0:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: a front_display view is still alive")

    def front_display(self, copy=True):
        """(map, (smin, smax)) of the oldest pending frame, which stays pending (pop
        it afterwards): the uint8 display map of the enabled roi and the min / max
        it was normalised with.  copy="view": a read-only view of the map in the
        stream's pinned host slot, valid until the next push.  copy="device": a
        zero-copy device tensor viewing the stream's ring, read-only by contract and
        valid until the frame is popped."""
        self._live()
        shape = getattr(self, "_disp_shape", None) or (0, 0)
        mm = np.zeros(2, np.int16)
        if copy == "device":
            ptr = ctypes.c_void_p()
            check(lib().mvsv_stream_front_display_device(self._h, ctypes.byref(ptr), mm.ctypes.data),
                  self._ctx.handle)
            return self._span(ptr, shape, "|u1"), (int(mm[0]), int(mm[1]))
        if copy == "view":
            ptr = ctypes.c_void_p()
            check(lib().mvsv_stream_front_display_view(self._h, ctypes.byref(ptr), mm.ctypes.data),
                  self._ctx.handle)
            buf = (ctypes.c_uint8 * (shape[0] * shape[1])).from_address(ptr.value)
            buf._owner = self
            with self._views_lock:
                self._live_views += 1
                self._disp_views = getattr(self, "_disp_views", 0) + 1
            fin = weakref.finalize(buf, DisparityStream._display_view_released, self)
            fin.atexit = False
            view = np.ctypeslib.as_array(buf).reshape(shape)
            view.flags.writeable = False
            return view, (int(mm[0]), int(mm[1]))
        out = np.empty(shape, np.uint8)
        check(lib().mvsv_stream_front_display(self._h, out.ctypes.data if out.size else None, shape[1],
                                              mm.ctypes.data), self._ctx.handle)
        return out, (int(mm[0]), int(mm[1]))

    def enable_view(self, layers, roi=None, mean_detector_or_range=None, point_radius=3, alpha=0, beta=255):
        """The detection view of every frame from now on (utility.detection_view of
        dMap(roi): display bytes as BGR, View's grids, the found tiles and points),
        computed on the device after the frame's mean grid and lattice
        (mvsv_stream_enable_view); only while no frame is pending.
        VIEW_FOUND_TILES needs a stream whose grid_roi equals roi and
        mean_detector_or_range: a MeanDisparityDetection (its mRangeDisparity) or
        (first, second).  VIEW_FOUND_POINTS needs enable_samplepoints with the same
        roi and uses its range."""
        self._live()
        self._view_views_gone("enable_view")
        from .utility import view_spec
        rng = mean_detector_or_range
        if hasattr(rng, "mRangeDisparity"):
            rng = rng.mRangeDisparity
        spec = view_spec(layers, rng, None, point_radius, alpha, beta)
        r = Rect(*(int(v) for v in roi)) if roi is not None else None
        check(lib().mvsv_stream_enable_view(self._h, ctypes.byref(r) if r is not None else None, ctypes.byref(spec)),
              self._ctx.handle)
        self._view_shape = (self.height, self.width, 3) if r is None else (r.y1 - r.y0, r.x1 - r.x0, 3)

    def disable_view(self):
        self._live()
        self._view_views_gone("disable_view")
        check(lib().mvsv_stream_disable_view(self._h), self._ctx.handle)
        self._view_shape = None

    def _view_views_gone(self, what):
        # the pinned view slots are reallocated: no view may point into them
        with self._views_lock:
            if getattr(self, "_view_views", 0) > 0:
                raise MvsvError(_lib.MVSV_E_INVALID_ARG, f"{what}: a front_view view is still alive")

    def front_view(self, copy=True):
        """(image, (smin, smax)) of the oldest pending frame, which stays pending (pop
        it afterwards): the uint8 BGR detection view (h, w, 3) of the enabled roi and
        the min / max it was normalised with.  copy="view": a read-only view of the
        image in the stream's pinned host slot, valid until the next push.
        copy="device": a zero-copy device tensor viewing the stream's ring, read-only
        by contract and valid until the frame is popped."""
        self._live()
        shape = getattr(self, "_view_shape", None) or (0, 0, 3)
        mm = np.zeros(2, np.int16)
        if copy == "device":
            ptr = ctypes.c_void_p()
            check(lib().mvsv_stream_front_view_device(self._h, ctypes.byref(ptr), mm.ctypes.data), self._ctx.handle)
            return self._span(ptr, shape, "|u1"), (int(mm[0]), int(mm[1]))
        if copy == "view":
            ptr = ctypes.c_void_p()
            check(lib().mvsv_stream_front_view_view(self._h, ctypes.byref(ptr), mm.ctypes.data), self._ctx.handle)
            buf = (ctypes.c_uint8 * (shape[0] * shape[1] * 3)).from_address(ptr.value)
            buf._owner = self
            with self._views_lock:
                self._live_views += 1
                self._view_views = getattr(self, "_view_views", 0) + 1
            fin = weakref.finalize(buf, DisparityStream._view_view_released, self)
            fin.atexit = False
            view = np.ctypeslib.as_array(buf).reshape(shape)
            view.flags.writeable = False
            return view, (int(mm[0]), int(mm[1]))
        out = np.empty(shape, np.uint8)
        check(lib().mvsv_stream_front_view(self._h, out.ctypes.data if out.size else None, 3 * shape[1],
                                           mm.ctypes.data), self._ctx.handle)
        return out, (int(mm[0]), int(mm[1]))

    def enable_cloud(self, Q, roi=None, max_points=None):
        """The point cloud of every frame from now on: the pixels with v > 0 of
        dMap(roi) in raster order, as Utility::dmap2pcl writes them
        (mvsv_stream_enable_cloud), compacted after SGBM into a device ring; only
        while no frame is pending.  roi = (x0, y0, x1, y1), default the whole map;
        x / y count from its corner.  max_points: the records kept per frame,
        default every pixel of the roi."""
        self._live()
        q = np.ascontiguousarray(np.asarray(Q, np.float32).reshape(16))
        r = Rect(*(int(v) for v in roi)) if roi is not None else None
        check(lib().mvsv_stream_enable_cloud(self._h, ctypes.byref(r) if r is not None else None, q.ctypes.data,
                                             0 if max_points is None else int(max_points)), self._ctx.handle)
        px = self.width * self.height if r is None else (r.x1 - r.x0) * (r.y1 - r.y0)
        self._cloud_max = px if max_points is None or max_points <= 0 else min(int(max_points), px)

    def disable_cloud(self):
        self._live()
        check(lib().mvsv_stream_disable_cloud(self._h), self._ctx.handle)
        self._cloud_max = None

    def front_cloud(self, copy=True, return_minmax=False):
        """(records, count) of the oldest pending frame, which stays pending (pop it
        afterwards).  count: the frame's number of valid pixels; records: the first
        min(count, max_points) of them as a structured array of CLOUD_DTYPE, copied
        from the device now that the count is known.  copy=False: no copy -- a
        float32 device tensor (min(count, max_points), 4) viewing the frame's slot
        of the ring ((x, y, z, grey bits), as point_cloud returns), valid until the
        frame is popped.  return_minmax: also (min, max) over the valid values."""
        self._live()
        from .utility import CLOUD_DTYPE
        cap = getattr(self, "_cloud_max", None) or 0
        count = ctypes.c_int(0)
        mm = np.zeros(2, np.int32)
        if copy:
            # the header first (the frame is waited for here), then the records that exist
            check(lib().mvsv_stream_front_cloud(self._h, None, 0, ctypes.byref(count), mm.ctypes.data),
                  self._ctx.handle)
            rec = np.empty(min(count.value, cap), CLOUD_DTYPE)
            if rec.size:
                check(lib().mvsv_stream_front_cloud(self._h, rec.ctypes.data, rec.size, None, None),
                      self._ctx.handle)
        else:
            import torch
            ptr = ctypes.c_void_p()
            check(lib().mvsv_stream_front_cloud_device(self._h, ctypes.byref(ptr), ctypes.byref(count),
                                                       mm.ctypes.data), self._ctx.handle)
            k = min(count.value, cap)
            dev = torch.device("cuda", self._ctx.device)
            if k == 0:
                rec = torch.empty((0, 4), dtype=torch.float32, device=dev)
            else:
                rec = torch.as_tensor(_DeviceSpan(ptr.value, (k, 4), self), device=dev)
        if return_minmax:
            return rec, count.value, (int(mm[0]), int(mm[1]))
        return rec, count.value

    def enable_sharpness(self, roi_left=None, roi_right=None):
        """Utility::checkSharpness of every pushed pair from now on, each side over
        its own roi = (x0, y0, x1, y1) (default: the whole image), on the device
        beside the frame's other passes (mvsv_stream_enable_sharpness); only while
        no frame is pending.  The pushed images are measured: on a raw stream the
        raw camera pair, as trgt/liveView.cpp measures what getImagepair returned."""
        self._live()
        rl = Rect(*(int(v) for v in roi_left)) if roi_left is not None else None
        rr = Rect(*(int(v) for v in roi_right)) if roi_right is not None else None
        check(lib().mvsv_stream_enable_sharpness(self._h, ctypes.byref(rl) if rl is not None else None,
                                                 ctypes.byref(rr) if rr is not None else None), self._ctx.handle)

    def disable_sharpness(self):
        self._live()
        check(lib().mvsv_stream_disable_sharpness(self._h), self._ctx.handle)

    def front_sharpness(self, return_sums=False):
        """(left, right) focus values of the oldest pending frame, which stays
        pending (pop it afterwards); return_sums: also the exact integer sums S4."""
        self._live()
        values = np.zeros(2, np.float64)
        sums = np.zeros(2, np.int64)
        check(lib().mvsv_stream_front_sharpness(self._h, values.ctypes.data, sums.ctypes.data), self._ctx.handle)
        v = (float(values[0]), float(values[1]))
        return (v, (int(sums[0]), int(sums[1]))) if return_sums else v

    @staticmethod
    def _display_view_released(stream):
        with stream._views_lock:
            stream._disp_views -= 1
        DisparityStream._view_released(stream)

    @staticmethod
    def _view_view_released(stream):
        with stream._views_lock:
            stream._view_views -= 1
        DisparityStream._view_released(stream)

    @staticmethod
    def _view_released(stream):
        with stream._views_lock:
            stream._live_views -= 1
            if stream._close_pending and stream._live_views == 0:
                stream._destroy()

    def _destroy(self):
        with self._views_lock:
            if self._h:
                lib().mvsv_stream_destroy(self._h)
                self._h = None
            self._close_pending = False

    def close(self):
        """Destroys the stream; with pop views still alive, when the last one goes."""
        with self._views_lock:
            if self._live_views > 0:
                self._close_pending = True
                return
            self._destroy()

    @property
    def closed(self):
        return self._h is None or self._close_pending

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
