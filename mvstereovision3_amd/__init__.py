"""mvstereovision3_amd — MI355X-native stereo disparity engine.

Drop-in for the disparity hot path of hG3n/mvStereoVision3
(Disparity::sgbm / Disparity::bm / Disparity::loadSGBMParameters,
src/disparity.cpp:6-108).  Compute lives in hand-written HIP kernels for
gfx950 behind the C ABI of libmvsv.so (include/mvsv.h); this package is the
host-side mirror of the reference interface.
"""
from ._lib import (GRAY_Q14, GRAY_Q15, MATCHER_BM, MATCHER_SGBM, MODE_HH, MODE_HH4, MODE_SGBM, MVSV_E_TIMEOUT, MVSV_HOST_ALL,
                   MVSV_HOST_DISPLAY, MVSV_HOST_MAP, MVSV_HOST_RECTIFIED, MVSV_HOST_VIEW, OPT_BITSLICE, OPT_BM_TILE_ROWS, OPT_PATH_SCHEDULE,
                   OPT_STRIP_SPIN_LIMIT, OPT_STRIP_WAVES,
                   PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL, VARIANT_FIRSTCOL_FIX,
                   VARIANT_WTA_MIN_D, MvsvError, set_option, synchronize)
from .disparity import (SAMPLE_HIT_DTYPE, Disparity, StereoBM, StereoSGBM, Stereopair, census_transform, filter_speckles,
                        mean_disparity_grid, median_blur3, samplepoint_detect, samplepoint_layout,
                        samplepoint_values, sgbmParameters, synth_pair, tm, tm_validate)
from .detection import (DisparityStream, MeanDisparityDetection, Samplepoint, SamplepointDetection, Subimage,
                        create_dmap_rois)
from .calibration import Stereosystem, read_matrix, stereo_rectify, write_matrices
from .rectify import (convert_maps, init_undistort_rectify_map, rectify_pair, remap, remap_fixed, undistort_maps,
                      undistort_pair)
from .utility import (CLOUD_DTYPE, VIEW_FOUND_POINTS, VIEW_FOUND_TILES, VIEW_OBSTACLE_GRID, VIEW_SUBIMAGE_GRID, Utility,
                      View, dMapValues, detection_view, minmax, normalize_minmax, ply, point_cloud, prepare_gray, prepare_size,
                      reproject, sharpness)

__all__ = [
    "Disparity", "StereoBM", "StereoSGBM", "Stereopair", "sgbmParameters", "MvsvError",
    "synth_pair", "mean_disparity_grid", "median_blur3", "filter_speckles", "MODE_SGBM", "MODE_HH", "MODE_HH4", "PREFILTER_XSOBEL",
    "PREFILTER_NORMALIZED_RESPONSE", "VARIANT_FIRSTCOL_FIX", "VARIANT_WTA_MIN_D",
    "DisparityStream", "MeanDisparityDetection", "Subimage", "create_dmap_rois", "Utility",
    "dMapValues", "ply", "reproject", "init_undistort_rectify_map", "rectify_pair", "remap",
    "synchronize", "set_option", "Stereosystem", "read_matrix", "write_matrices",
    "stereo_rectify", "convert_maps", "MVSV_E_TIMEOUT", "OPT_STRIP_SPIN_LIMIT", "OPT_STRIP_WAVES", "OPT_BM_TILE_ROWS",
    "OPT_PATH_SCHEDULE", "OPT_BITSLICE", "Samplepoint", "SamplepointDetection", "samplepoint_layout",
    "samplepoint_values", "samplepoint_detect", "SAMPLE_HIT_DTYPE",
    "normalize_minmax", "minmax", "point_cloud", "CLOUD_DTYPE",
    "sharpness", "undistort_maps", "remap_fixed", "undistort_pair",
    "detection_view", "View", "VIEW_SUBIMAGE_GRID", "VIEW_OBSTACLE_GRID", "VIEW_FOUND_TILES", "VIEW_FOUND_POINTS",
    "prepare_gray", "prepare_size", "GRAY_Q14", "GRAY_Q15", "MATCHER_SGBM", "MATCHER_BM",
    "tm", "tm_validate", "census_transform", "MVSV_HOST_MAP", "MVSV_HOST_RECTIFIED", "MVSV_HOST_DISPLAY", "MVSV_HOST_VIEW", "MVSV_HOST_ALL",
]
__version__ = "1.0.0"
