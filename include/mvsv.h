/*
 * mvsv.h — C ABI of the MI355X-native stereo disparity engine (libmvsv.so).
 *
 * This is the drop-in boundary for the reference's disparity hot path.  Every
 * entry point replaces one reference interface (hG3n/mvStereoVision3):
 *
 *   mvsv_sgbm / mvsv_sgbm_device      Disparity::sgbm        src/disparity.cpp:6-10,
 *                                     decl inc/disparity.h:29 (forwards to
 *                                     cv::StereoSGBM::compute, also called
 *                                     directly at trgt/liveDisparity.cpp:91);
 *                                     modes MODE_SGBM, MODE_HH and MODE_HH4
 *                                     (MODE_SGBM_3WAY is refused by name)
 *   mvsv_sgbm_census(_device) /       Disparity::binary_sgbm src/disparity.cpp:12-15,
 *   mvsv_census(_device)              decl inc/disparity.h:30 (commented out in the
 *                                     reference, "currently not working"): SGBM on a
 *                                     census cost, on this engine's own contract
 *   mvsv_bm / mvsv_bm_device          Disparity::bm          src/disparity.cpp:18-22,
 *                                     decl inc/disparity.h:31
 *   mvsv_bm_census(_device)           Disparity::binary_bm: StereoBM on a census cost
 *                                     (the StereoBinaryBM of inc/disparity.h:13's
 *                                     module), on this engine's own contract
 *   mvsv_load_sgbm_yaml               Disparity::loadSGBMParameters
 *                                     src/disparity.cpp:60-108, inc/disparity.h:34
 *   mvsv_load_bm_yaml                 (new) loader for configs/bm.yml:2-7, which
 *                                     the reference ships but never reads
 *   mvsv_sgbm_params / mvsv_bm_params cv::StereoSGBM / cv::StereoBM state set by
 *                                     create() + setters (src/disparity.cpp:83-95,
 *                                     trgt/liveDisparity.cpp:61); field meaning and
 *                                     defaults are OpenCV 3.4's
 *   mvsv_sgbm_yaml_values             struct Disparity::sgbmParameters
 *                                     inc/disparity.h:17-27
 *   mvsv_mean_disparity_grid_device   MeanDisparityDetection::build(MEAN_VALUE)
 *                                     src/MeanDisparityDetection.cpp:159-206 +
 *                                     Utility::calcMeanDisparity src/utility.cpp:265-285
 *   mvsv_mean_disparity_grid          same, host map (MeanDisparityDetection::build)
 *   mvsv_median_blur3_device /        cv::medianBlur(.., 3) and cv::filterSpeckles on CV_16S
 *   mvsv_filter_speckles_device       maps: the post filters of cv::StereoSGBM::compute /
 *                                     cv::StereoBM::compute, callable on their own
 *   mvsv_samplepoint_layout /         SamplepointDetection::init / build /
 *   _values(_device) / _detect_device detectObstacles src/SamplePointDetection.cpp:29-178,
 *                                     Samplepoint inc/Samplepoint.h:17-40
 *   mvsv_stream_enable_samplepoints / both detectors on every frame of a stream
 *   _front_samples                    (trgt/demo.cpp:206-209,271-276)
 *   mvsv_normalize_minmax(_device)    cv::normalize(dMap, dMapNorm, 0, 255, NORM_MINMAX, CV_8U)
 *                                     trgt/liveDisparity.cpp:92, trgt/mean_test.cpp:307 and
 *                                     the other loops' display step
 *   mvsv_minmax_device                Utility::calcMinMaxDisparity src/utility.cpp:287-304
 *   mvsv_stream_enable_display /      the display map with every frame of a stream
 *   _front_display(_view)             (trgt/liveDisparity.cpp:88-95)
 *   mvsv_view(_device) / _view_draw   the annotated frame of the detection programs: normalize,
 *                                     cvtColor(GRAY2BGR), View::drawSubimageGrid / drawObstacleGrid
 *                                     (src/view.cpp), drawFoundObstacles (trgt/demo.cpp:116-128,280-298)
 *   mvsv_stream_enable_view /         that frame with every frame of a stream
 *   _front_view(_view)
 *   mvsv_stream_*                     the disparity worker thread + main loop of
 *                                     trgt/mean_test.cpp:61-70,258-318 (condvar
 *                                     hand-off, Disparity::sgbm, build(MEAN_VALUE))
 *                                     as a double-buffered device pipeline
 *   mvsv_stream_create_raw /          the same loop from the raw camera pair
 *   _push_raw / _pop_pair             (trgt/liveDisparity.cpp:82-101): rectification,
 *                                     crop and resize on the device, ahead of SGBM
 *   mvsv_convert_maps                 cv::convertMaps(CV_16SC2, CV_16UC1)
 *   mvsv_remap_device / mvsv_rectify  cv::remap(INTER_LINEAR) + ROI crop of
 *                                     Stereosystem::getRectifiedImagepair
 *                                     src/Stereosystem.cpp:243-262
 *   mvsv_init_undistort_rectify_map   cv::initUndistortRectifyMap (CV_32FC1) as
 *                                     called by Stereosystem::initRectification
 *                                     src/Stereosystem.cpp:193-237
 *   mvsv_reproject_device             Utility::calcCoordinate src/utility.cpp:176-198,
 *                                     per pixel (the loop of Utility::dmap2pcl :242-262)
 *   mvsv_calc_coordinate(s) / _distance  Utility::calcCoordinate / calcDistance
 *   / _dmap_values                    src/utility.cpp:176-240 (host, one point)
 *   mvsv_write_ply                    ply::write src/ply.cpp:37-133 (MODE PLAIN,
 *                                     WITH_COLOR, WITH_COLOR_SHADING)
 *   mvsv_dmap2pcl                     Utility::dmap2pcl src/utility.cpp:242-262
 *   mvsv_point_cloud(_device)         the loop of Utility::dmap2pcl src/utility.cpp:248-259
 *                                     (pixels with v > 0 in raster order) with the grey
 *                                     of ply::write src/ply.cpp:90, compacted on the device
 *   mvsv_stream_enable_cloud /        the point cloud with every frame of a stream (the
 *   _front_cloud(_device)             dmap2pcl call of trgt/demo.cpp:394 and the other loops)
 *   mvsv_sharpness(_device)           Utility::checkSharpness src/utility.cpp:163-174, the
 *                                     focusing loop of trgt/liveView.cpp:94-117
 *   mvsv_stream_enable_sharpness /    the focus measure of the pushed pair with every frame
 *   _front_sharpness                  of a stream
 *   mvsv_undistort_maps /             cv::undistort's CV_16SC2 stripe maps, cv::remap on such
 *   mvsv_remap_fixed_device /         maps, and Stereosystem::getUndistortedImagepair
 *   mvsv_undistort_pair               src/Stereosystem.cpp:179-191 (trgt/liveUndistortion.cpp:58,
 *                                     example/images.cpp:95)
 *   mvsv_prepare_gray(_device)        cv::resize(.., 0.5, 0.5, INTER_AREA) + cv::cvtColor(BGR2GRAY)
 *                                     of trgt/disparityTest.cpp:201-211, one kernel
 *   mvsv_stream_create_bm /           Disparity::bm (trgt/disparityTest.cpp:268) as a stream's
 *   _create_raw_bm / _set_bm_params   matcher, beside Disparity::sgbm (:267)
 *   mvsv_stream_enable_bgr /          colour pairs into a stream: uploaded as BGR, prepared on
 *   _push_bgr                         the device ahead of the matcher
 *   mvsv_stream_push*_device /        the same loops for a producer and a consumer on the GPU:
 *   _pop_device / _front_*_device /   frames from device memory, results read where they lie (no
 *   _set_host_outputs / _fence        counterpart in the reference, whose images live in cv::Mat)
 *   mvsv_tm(_device) / _tm_validate   Disparity::tm          src/disparity.cpp:25-58,
 *                                     decl inc/disparity.h:32 (cv::matchTemplate
 *                                     CV_TM_CCORR_NORMED along the row, per pixel)
 *
 * Conventions
 *   - Plain C types only; no exceptions cross this boundary.
 *   - Every function returns MVSV_OK (0) or a negative MVSV_E_* code; the
 *     context's message is available through mvsv_last_error().
 *   - Parameter validation follows OpenCV's CV_Assert/CV_Error rules for the
 *     same call (invalid -> MVSV_E_INVALID_ARG instead of cv::Exception).
 *   - Output is CV_16S-compatible: int16 disparity * 16 (DISP_SHIFT = 4);
 *     invalid pixels are (minDisparity - 1) * 16.
 *   - A context owns one HIP stream and its cached device buffers; it is not
 *     thread-safe: use one context per host thread (the reference runs one
 *     matcher per worker thread, trgt/mean_test.cpp:61-70).
 *   - Host-pointer calls (mvsv_sgbm, mvsv_bm) are synchronous.  Device-pointer
 *     calls (*_device) enqueue on the context stream and return immediately;
 *     call mvsv_synchronize() before reading results on the host.
 */
#ifndef MVSV_H
#define MVSV_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define MVSV_API __attribute__((visibility("default")))
#else
#define MVSV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MVSV_VERSION 100 /* 1.0.0 */

enum {
    MVSV_OK = 0,
    MVSV_E_INVALID_ARG = -1, /* OpenCV would throw cv::Exception (StsOutOfRange / assert) */
    MVSV_E_HIP = -2,         /* HIP runtime error (launch, copy, device) */
    MVSV_E_OOM = -3,         /* device or host allocation failed */
    MVSV_E_IO = -4,          /* cannot open file */
    MVSV_E_PARSE = -5,       /* missing / malformed YAML key */
    MVSV_E_NODEV = -6,       /* no HIP device available */
    MVSV_E_TIMEOUT = -7      /* a strip-to-strip hand-off of the SGBM path kernel was
                                given up: the affected maps are all INVALID */
};

/* Context options (mvsv_set_option). */
enum {
    /* polls a strip-boundary wait of the SGBM path kernel makes before it gives
     * up (default 1 << 20, ~1 s); 0 gives up at the first poll that finds the
     * producer's data not yet written (fault injection for tests) */
    MVSV_OPT_STRIP_SPIN_LIMIT = 1,
    /* rows per block of the StereoBM disparities-on-lanes kernel (0 = chosen
     * per launch from the shape; 1..128 forces it -- tests, A/B runs) */
    MVSV_OPT_BM_TILE_ROWS = 2,
    /* compute waves per strip of the SGBM sheared-strip kernel: 0 = by launch
     * size (narrow strips when the wide ones would leave CUs idle), 8 (4 for
     * numDisparities > 128) = narrow, 15 (7) = wide; other values = 0 */
    MVSV_OPT_STRIP_WAVES = 3,
    /* SGBM path schedule (numDisparities 32 / 64 / 128 / 256): 0 = by launch
     * size -- all line directions side by side for launches that would fill
     * at most half the GPU with sheared strips (one camera frame; needs
     * P2 <= 15),
     * sheared strips otherwise; 1 = strips; 2 = directions side by side.
     * MODE_HH4 has no diagonal path and never runs strips: 0 = side by side
     * (nibble planes for P2 <= 15, byte / u16 planes while the three planes
     * stay small), else one launch per direction; 1 = one launch per
     * direction on byte / u16 planes; 2 = side by side */
    MVSV_OPT_PATH_SCHEDULE = 4,
    /* which strip a block of the sheared-strip kernel runs: 1 (default) = a
     * ticket drawn on arrival, so a strip only waits on a strip already
     * running or done whatever the dispatch order and whatever else shares
     * the GPU (every launch size); 0 = its blockIdx (relies on in-order
     * dispatch, A/B runs only). */
    MVSV_OPT_STRIP_TICKETS = 5,
    /* SGBM direction passes read the cost residual plane
     * R = min(C - min_d C, 2*P2) + P2 (one nibble per cost, 4x fewer bytes
     * than C) instead of C where that is exact: no int16 wrap is possible,
     * 3*P2 <= 15 and numDisparities <= 128 (configs/sgbm.yml).  1 (default)
     * = on, 0 = always read C (A/B runs); results are identical either way. */
    MVSV_OPT_COST_RESIDUAL = 6,
    /* Bit-sliced MODE_HH path aggregation (round 5, mvsv_bsgm.hip): 1 (default)
     * = where it applies (MODE_HH, numDisparities 128, P1 2 / P2 5 -- the
     * sgbm.yml regime --, uniquenessRatio 0, no int16 wrap); 0 = the packed
     * int16 kernels.  Results are identical either way. */
    MVSV_OPT_BITSLICE = 7
};

/* StereoSGBM modes (cv::StereoSGBM::MODE_SGBM / MODE_HH / MODE_HH4).
 * MODE_HH4: four paths (L->R, R->L, down, up) on the cost volume without
 * OpenCV 3.4's cost-row quirks (MVSV_VARIANT_FIRSTCOL_FIX has no effect); the
 * WTA tie rule is MODE_SGBM's.  MVSV_MODE_SGBM_3WAY is named only so that it
 * can be refused by name: its result depends on OpenCV's stripe split, which
 * this library does not restate (MVSV_E_INVALID_ARG). */
enum { MVSV_MODE_SGBM = 0, MVSV_MODE_HH = 1, MVSV_MODE_SGBM_3WAY = 2, MVSV_MODE_HH4 = 3 };
/* StereoBM prefilter types (cv::StereoBM::PREFILTER_*). */
enum { MVSV_PREFILTER_NORMALIZED_RESPONSE = 0, MVSV_PREFILTER_XSOBEL = 1 };

/* Semantic variants of OpenCV releases (bit flags in mvsv_sgbm_params.variant).
 * 0 = OpenCV 3.4.x CV_SIMD128 behaviour (the pinned default). */
enum {
    MVSV_VARIANT_FIRSTCOL_FIX = 1, /* later releases refresh cost column x=0 */
    MVSV_VARIANT_WTA_MIN_D = 2     /* later releases: MODE_SGBM ties -> smallest d */
};

typedef struct {
    int min_disparity;       /* setMinDisparity */
    int num_disparities;     /* setNumDisparities, must be > 0 and % 16 == 0 */
    int block_size;          /* setBlockSize (<= 0 -> 5) */
    int p1, p2;              /* setP1 / setP2 (<= 0 -> 2 / 5, P2 = max(P2, P1+1)) */
    int disp12_max_diff;     /* setDisp12MaxDiff (<= 0 -> 1) */
    int pre_filter_cap;      /* setPreFilterCap (ftzero = max(cap,15)|1) */
    int uniqueness_ratio;    /* setUniquenessRatio (< 0 -> 10) */
    int speckle_window_size; /* setSpeckleWindowSize (0 disables speckle filter) */
    int speckle_range;       /* setSpeckleRange (multiplied by 16) */
    int mode;                /* MVSV_MODE_SGBM (5 paths), MVSV_MODE_HH (8) or MVSV_MODE_HH4 (4) */
    int variant;             /* MVSV_VARIANT_* bits, 0 = OpenCV 3.4 */
} mvsv_sgbm_params;

typedef struct {
    int pre_filter_type;     /* MVSV_PREFILTER_XSOBEL (default) or _NORMALIZED_RESPONSE */
    int pre_filter_size;     /* odd, 5..255 */
    int pre_filter_cap;      /* 1..63 */
    int block_size;          /* odd, 5..255, < min(W, H) */
    int min_disparity;
    int num_disparities;     /* > 0, % 16 == 0 */
    int texture_threshold;   /* >= 0 */
    int uniqueness_ratio;    /* >= 0 */
    int speckle_window_size;
    int speckle_range;
    int disp12_max_diff;     /* < 0 disables the left-right check */
} mvsv_bm_params;

/* Disparity::sgbmParameters (inc/disparity.h:17-27): the raw YAML values. */
typedef struct {
    int minDisp, numDisp, blockSize, disp12MaxDiff, preFilterCap, uniquenessRatio,
        speckleWindowSize, speckleRange, disparityMode;
} mvsv_sgbm_yaml_values;

typedef struct mvsv_ctx mvsv_ctx;

MVSV_API int mvsv_version(void);

/* StereoSGBM::create() defaults: (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, MODE_SGBM). */
MVSV_API void mvsv_sgbm_params_default(mvsv_sgbm_params* p);
/* StereoSGBM::create(minDisparity, numDisparities, blockSize, P1, P2, ...). */
MVSV_API void mvsv_sgbm_params_create(mvsv_sgbm_params* p, int min_disparity,
                                      int num_disparities, int block_size, int p1, int p2,
                                      int disp12_max_diff, int pre_filter_cap,
                                      int uniqueness_ratio, int speckle_window_size,
                                      int speckle_range, int mode);
/* StereoBM::create(numDisparities, blockSize) defaults. */
MVSV_API void mvsv_bm_params_default(mvsv_bm_params* p, int num_disparities, int block_size);

/* Validation only (no device needed): MVSV_OK or MVSV_E_INVALID_ARG. */
MVSV_API int mvsv_sgbm_validate(const mvsv_sgbm_params* p, int W, int H);
MVSV_API int mvsv_bm_validate(const mvsv_bm_params* p, int W, int H);

MVSV_API int mvsv_create(mvsv_ctx** out, int hip_device);
MVSV_API void mvsv_destroy(mvsv_ctx* ctx);
MVSV_API const char* mvsv_last_error(const mvsv_ctx* ctx);
/* Enqueue on an external hipStream_t (e.g. the caller's current stream).
 * NULL selects the HIP null (default) stream, which is what torch's default
 * current stream is; mvsv_use_own_stream() returns to the context's own
 * non-blocking stream. */
MVSV_API int mvsv_set_stream(mvsv_ctx* ctx, void* hip_stream);
MVSV_API int mvsv_use_own_stream(mvsv_ctx* ctx);
MVSV_API void* mvsv_get_stream(mvsv_ctx* ctx);
/* Waits for the context stream; MVSV_E_TIMEOUT if an SGBM launch since the last
 * check gave up a strip hand-off (its maps were written as all INVALID).  The
 * device calls also return MVSV_E_TIMEOUT, without enqueueing, when an earlier
 * launch that has completed by then gave up. */
MVSV_API int mvsv_synchronize(mvsv_ctx* ctx);
MVSV_API int mvsv_set_option(mvsv_ctx* ctx, int option, long long value);
/* Release cached device buffers. */
MVSV_API int mvsv_trim(mvsv_ctx* ctx);

/* Host pointers, synchronous.  Strides are in elements (bytes for u8, int16
 * elements for out); stride >= W allows ROI views (src/Stereosystem.cpp:255-256).
 *
 * mvsv_sgbm and costs above 32767.  P2 + blockSize^2 pixel costs can pass int16 on
 * high-contrast pairs (blockSize 21, or 15 with P2 in the thousands).  OpenCV's own map then
 * depends on its build: the SIMD build's cost-row update saturates, the scalar (non-SIMD)
 * build's wraps modulo 2^16, and a wrapped -- negative -- cost wins the WTA in both.  The
 * engine reproduces the scalar build bit for bit: modular cost rows, signed path costs, a
 * signed S saturated on both sides (tests/test_gpu_sgbm_wrap.py).  The
 * test oracle's default flags restate the saturating update, ORC_F_COST_WRAP the wrapping
 * one; on the tests' inputs the two differ in 27 % of the map pixels.  MODE_HH4 and three
 * live colour channels have no reference in this regime. */
MVSV_API int mvsv_sgbm(mvsv_ctx* ctx, const uint8_t* left, size_t left_stride,
                       const uint8_t* right, size_t right_stride, int width, int height,
                       const mvsv_sgbm_params* p, int16_t* out, size_t out_stride);
MVSV_API int mvsv_bm(mvsv_ctx* ctx, const uint8_t* left, size_t left_stride,
                     const uint8_t* right, size_t right_stride, int width, int height,
                     const mvsv_bm_params* p, int16_t* out, size_t out_stride);

/* Device pointers (HBM-resident), asynchronous on the context stream.
 * A batch of n frames: frame i starts at base + i * frame_stride (elements). */
MVSV_API int mvsv_sgbm_device(mvsv_ctx* ctx, int n, const uint8_t* left, size_t left_stride,
                              size_t left_frame_stride, const uint8_t* right,
                              size_t right_stride, size_t right_frame_stride, int width,
                              int height, const mvsv_sgbm_params* p, int16_t* out,
                              size_t out_stride, size_t out_frame_stride);
MVSV_API int mvsv_bm_device(mvsv_ctx* ctx, int n, const uint8_t* left, size_t left_stride,
                            size_t left_frame_stride, const uint8_t* right,
                            size_t right_stride, size_t right_frame_stride, int width,
                            int height, const mvsv_bm_params* p, int16_t* out,
                            size_t out_stride, size_t out_frame_stride);

/* Device bytes the context will cache for one SGBM call of this shape: the buffer
 * sizes of the launch plan the library makes for it, plus the speckle filter's
 * buffers.  The figure is for a context with default options (no MVSV_*
 * environment, no mvsv_set_option) on a 256-CU device; 0 for invalid parameters
 * and for an empty column range (such a call only fills the map). */
MVSV_API size_t mvsv_sgbm_workspace_bytes(int n, int width, int height,
                                          const mvsv_sgbm_params* p);

/* The pipeline this context would run for an SGBM call of this shape and these
   parameters (no reference counterpart: introspection for byte models and
   tests), as MVSV_PLAN_* bits in *plan. */
enum {
    MVSV_PLAN_BITSLICE = 1,  /* bit-sliced path aggregation (MODE_HH or MODE_SGBM, sgbm.yml regime) */
    MVSV_PLAN_SIDE = 2,      /* every direction on its own chains (small launches) */
    MVSV_PLAN_STRIPS = 4,    /* sheared strips + row directions (frame batches) */
    MVSV_PLAN_RESIDUAL = 8   /* packed passes read the nibble cost residual plane */
};
MVSV_API int mvsv_sgbm_plan(mvsv_ctx* ctx, int n, int width, int height, const mvsv_sgbm_params* p,
                            int* plan);

/* StereoSGBM on 3-channel pairs, as cv::StereoSGBM::compute takes CV_8UC3: images
 * are interleaved 8-bit, 3 bytes per pixel (channel c of pixel x = byte 3x + c),
 * and the Birchfield-Tomasi pixel cost is the sum of the three channels' costs
 * ([OpenCV] calcPixelCostBT, cn == 3); everything after the pixel cost is that of
 * mvsv_sgbm.  width is in pixels; the input strides are in bytes (row stride
 * >= 3 * width), out_stride / out_frame_stride in int16 elements.  Arguments,
 * mvsv_sgbm_validate's rules and error codes otherwise as mvsv_sgbm /
 * mvsv_sgbm_device.  The channel order does not matter to the result. */
MVSV_API int mvsv_sgbm_bgr(mvsv_ctx* ctx, const uint8_t* left, size_t left_stride,
                           const uint8_t* right, size_t right_stride, int width, int height,
                           const mvsv_sgbm_params* p, int16_t* out, size_t out_stride);
MVSV_API int mvsv_sgbm_bgr_device(mvsv_ctx* ctx, int n, const uint8_t* left, size_t left_stride,
                                  size_t left_frame_stride, const uint8_t* right,
                                  size_t right_stride, size_t right_frame_stride, int width,
                                  int height, const mvsv_sgbm_params* p, int16_t* out,
                                  size_t out_stride, size_t out_frame_stride);
/* mvsv_sgbm_workspace_bytes / mvsv_sgbm_plan for a pair of `channels` (1 or 3)
 * channels: a colour launch never runs the bit-sliced or residual pipelines. */
MVSV_API size_t mvsv_sgbm_workspace_bytes_cn(int n, int width, int height,
                                             const mvsv_sgbm_params* p, int channels);
MVSV_API int mvsv_sgbm_plan_cn(mvsv_ctx* ctx, int n, int width, int height, const mvsv_sgbm_params* p,
                               int channels, int* plan);

/* StereoSGBM on a census matching cost: Disparity::binary_sgbm (inc/disparity.h:30,
 * src/disparity.cpp:12-15, commented out in the reference as "currently not working").
 * The contract is this engine's own, not opencv_contrib's
 * StereoBinarySGBM.
 *
 * Census transform of an 8-bit image I (height x width) with an odd
 * census_width x census_height window, 3 <= census_width * census_height <= 65:
 * the window offsets run dy = -ch/2 .. ch/2 (outer) and dx = -cw/2 .. cw/2 (inner),
 * the centre is skipped and the others are numbered k = 0 .. cw*ch - 2 in that order;
 * bit k of T(y, x) is 1 iff I(clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)) < I(y, x).
 * T is a uint64 whose bits above cw*ch - 1 are 0.
 *
 * Pixel cost: popcount(T_left(y, x) ^ T_right(y, x - d)).  Everything after the
 * pixel cost is mvsv_sgbm's for the same parameters and mode (box sum, + P2, the
 * OpenCV 3.4 cost rows in modes 0 and 1, paths, WTA, uniqueness, sub-pixel fit, LR
 * check, medianBlur(3), speckle filter).  pre_filter_cap has no effect.
 *
 * mvsv_sgbm_census_validate: mvsv_sgbm_validate's rules, the window rule above, and
 * P2 + blockSize^2 * (cw*ch - 1) <= 32767 with the effective values (no cost leaves
 * int16).  Grey pairs only.  The calls return MVSV_E_INVALID_ARG with a message that
 * names the broken rule.  Other arguments as mvsv_sgbm / mvsv_sgbm_device. */
MVSV_API int mvsv_sgbm_census_validate(const mvsv_sgbm_params* p, int W, int H, int census_width,
                                       int census_height);
MVSV_API int mvsv_sgbm_census(mvsv_ctx* ctx, const uint8_t* left, size_t left_stride,
                              const uint8_t* right, size_t right_stride, int width, int height,
                              const mvsv_sgbm_params* p, int16_t* out, size_t out_stride,
                              int census_width, int census_height);
MVSV_API int mvsv_sgbm_census_device(mvsv_ctx* ctx, int n, const uint8_t* left, size_t left_stride,
                                     size_t left_frame_stride, const uint8_t* right,
                                     size_t right_stride, size_t right_frame_stride, int width,
                                     int height, const mvsv_sgbm_params* p, int16_t* out,
                                     size_t out_stride, size_t out_frame_stride, int census_width,
                                     int census_height);
/* mvsv_sgbm_workspace_bytes / mvsv_sgbm_plan of a census call: it always takes the
 * LDS-ring cost kernel and never the bit-sliced or residual pipelines. */
MVSV_API size_t mvsv_sgbm_workspace_bytes_census(int n, int width, int height, const mvsv_sgbm_params* p,
                                                 int census_width, int census_height);
MVSV_API int mvsv_sgbm_plan_census(mvsv_ctx* ctx, int n, int width, int height, const mvsv_sgbm_params* p,
                                   int census_width, int census_height, int* plan);
/* The census transform alone.  stride / frame_stride in bytes, out_stride /
 * out_frame_stride in uint64 elements (>= width); only the width descriptors of a
 * row are written. */
MVSV_API int mvsv_census(mvsv_ctx* ctx, const uint8_t* img, size_t stride, int width, int height,
                         int census_width, int census_height, uint64_t* out, size_t out_stride);
MVSV_API int mvsv_census_device(mvsv_ctx* ctx, int n, const uint8_t* img, size_t stride, size_t frame_stride,
                                int width, int height, int census_width, int census_height, uint64_t* out,
                                size_t out_stride, size_t out_frame_stride);

/* StereoBM on a census matching cost: Disparity::binary_bm.  The reference's file loop
 * runs both matchers side by side (trgt/disparityTest.cpp:267-268) and the module its
 * header names (inc/disparity.h:13, opencv_contrib stereo) pairs StereoBinarySGBM with
 * StereoBinaryBM.  The contract is this engine's own, not opencv_contrib's.
 *
 * Descriptors: the census transform above, unchanged.  Pixel cost: wherever StereoBM
 * takes |Lf(y, xl) - Rf(y, xr)| on prefiltered bytes, popcount(T_left(y, xl) ^
 * T_right(y, xr)) for the same column pairs (virtual column j = x - lofs, left column
 * lofs + clamp(j, -lofs, W - 1 - lofs), right column rofs + clamp(j, -rofs,
 * W - numDisparities - rofs) + k).  Everything after the pixel cost is mvsv_bm's for the
 * same parameters: blockSize^2 window sum, argmin (ties -> smallest index), uniqueness
 * test, parabola fit, FILTERED = (minDisparity - 1) * 16, validateDisparity when
 * disp12MaxDiff >= 0, the valid rectangle, filterSpeckles.  pre_filter_type,
 * pre_filter_size, pre_filter_cap and texture_threshold have no effect (they are still
 * checked by mvsv_bm_validate's rules); there is no texture test.  A map does not change
 * under a strictly increasing map of either view's intensities.
 *
 * mvsv_bm_census_validate: mvsv_bm_validate's rules and the window rule.  Grey pairs only.
 * The calls return MVSV_E_INVALID_ARG with a message that names the broken rule, also
 * for a blockSize / numDisparities whose descriptor tiles no kernel form can hold.  Other
 * arguments as mvsv_bm / mvsv_bm_device. */
MVSV_API int mvsv_bm_census_validate(const mvsv_bm_params* p, int W, int H, int census_width,
                                     int census_height);
MVSV_API int mvsv_bm_census(mvsv_ctx* ctx, const uint8_t* left, size_t left_stride, const uint8_t* right,
                            size_t right_stride, int width, int height, const mvsv_bm_params* p,
                            int16_t* out, size_t out_stride, int census_width, int census_height);
MVSV_API int mvsv_bm_census_device(mvsv_ctx* ctx, int n, const uint8_t* left, size_t left_stride,
                                   size_t left_frame_stride, const uint8_t* right, size_t right_stride,
                                   size_t right_frame_stride, int width, int height,
                                   const mvsv_bm_params* p, int16_t* out, size_t out_stride,
                                   size_t out_frame_stride, int census_width, int census_height);

/* MeanDisparityDetection post-pass on device: 9x9 tile means of an int16 map
 * (tile = (W/9)x(H/9), remainder ignored; mean over values > 1 with integer
 * division, 0 for an empty tile).  means: 81 floats per frame (device ptr). */
MVSV_API int mvsv_mean_disparity_grid_device(mvsv_ctx* ctx, int n, const int16_t* dmap,
                                             size_t stride, size_t frame_stride, int width,
                                             int height, float* means);

/* The post filters of the disparity path on their own, on device maps.
 *
 * mvsv_median_blur3_device: cv::medianBlur(src, dst, 3) for CV_16S (replicate
 * border), what StereoSGBM::compute applies after its core.  n frames, strides
 * in int16 elements (stride >= width), any 2-byte-aligned views: an even width
 * with even strides and 4-byte-aligned views takes the packed kernel, every
 * other form the scalar one.  The extents of src and dst ([first, last] element
 * of the n frames) must not intersect: MVSV_E_INVALID_ARG, there is no in-place
 * form.
 *
 * mvsv_filter_speckles_device: cv::filterSpeckles(img, new_val,
 * max_speckle_size, max_diff) for CV_16S, in place on n frames; the frames are
 * filtered independently.  new_val must be an int16 value.  max_speckle_size
 * <= 0 removes nothing and max_diff < 0 makes every pixel a component of its
 * own, as in OpenCV.  StereoSGBM passes ((minDisparity - 1) * 16,
 * speckleWindowSize, 16 * speckleRange), StereoBM the same new_val and window
 * with speckleRange unscaled. */
MVSV_API int mvsv_median_blur3_device(mvsv_ctx* ctx, int n, const int16_t* src, size_t src_stride,
                                      size_t src_frame_stride, int16_t* dst, size_t dst_stride,
                                      size_t dst_frame_stride, int width, int height);
MVSV_API int mvsv_filter_speckles_device(mvsv_ctx* ctx, int n, int16_t* img, size_t stride,
                                         size_t frame_stride, int width, int height, int new_val,
                                         int max_speckle_size, int max_diff);

/* Same grid for a host map (synchronous). means: 81 floats, row-major 9x9. */
MVSV_API int mvsv_mean_disparity_grid(mvsv_ctx* ctx, const int16_t* dmap, size_t stride,
                                      int width, int height, float* means);

/* ---- SamplepointDetection: the lattice detector (src/SamplePointDetection.cpp) ----
 * Layout (init, :38-47): dX = width / 8, dY = height / 8, step_x = width / dX,
 * step_y = height / dY (integer divisions: steps of 8..15), centres
 * (c * step_x, r * step_y) for c = 1..dX-1 (outer loop), r = 1..dY-1 (inner), so
 * nx = dX - 1, ny = dY - 1 and point (c, r) has index (c - 1) * ny + (r - 1).
 * A map narrower or lower than 16 has no point (nx * ny == 0; a step is 0 where
 * its dX / dY is): valid, the calls below then return MVSV_OK and do nothing.
 * Host only, no device needed. */
MVSV_API int mvsv_samplepoint_layout(int width, int height, int* step_x, int* step_y, int* nx,
                                     int* ny);

/* Samplepoint::calculateSamplepointValue (inc/Samplepoint.h:32-40) of every
 * lattice point of n int16 maps (device pointers, strides in elements; any
 * 2-byte-aligned view): the patch [cx - radius, cx + radius] x [cy - radius,
 * cy + radius] through Utility::calcMeanDisparity (mean of the values > 1 with
 * integer division, 0 for none) for radius > 0, the raw centre value for
 * radius 0.  The reference's radius is 2; 0 .. min(step_x, step_y) - 1 keeps the
 * patches inside the map, anything else is MVSV_E_INVALID_ARG.
 * values: nx * ny floats per frame (device pointer), frames back to back. */
MVSV_API int mvsv_samplepoint_values_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t stride,
                                            size_t frame_stride, int width, int height, int radius,
                                            float* values);
/* Same for one host map into a host array (synchronous). */
MVSV_API int mvsv_samplepoint_values(mvsv_ctx* ctx, const int16_t* dmap, size_t stride, int width,
                                     int height, int radius, float* values);

/* SamplepointDetection::detectObstacles (:134-178) on the device: a point is a
 * hit when value < range_first && value > range_second (float compares); each
 * hit carries Utility::calcCoordinate(value, centre x, centre y, Q) -- the
 * arithmetic of mvsv_calc_coordinate, bit for bit.  Per frame: counts[f] = the
 * number of hits (it may exceed max_hits), hits[f * max_hits ..] = the first
 * min(count, max_hits) of them in index order.  values as written by
 * mvsv_samplepoint_values_device for a width x height map; all device
 * pointers; max_hits >= 0 (0: count only, hits may be NULL). */
typedef struct {
    int32_t index; /* lattice point, (c - 1) * ny + (r - 1) */
    float x, y, z; /* calcCoordinate's X, Y, Z */
} mvsv_sample_hit;
MVSV_API int mvsv_samplepoint_detect_device(mvsv_ctx* ctx, int n, const float* values, int width,
                                            int height, const float* Q, float range_first,
                                            float range_second, int max_hits, int* counts,
                                            mvsv_sample_hit* hits);

/* ---- point clouds: the valid pixels of a disparity map, compacted in raster order ----
 * Utility::dmap2pcl's loop (src/utility.cpp:248-259) keeps the pixels with v > 0,
 * row by row, and ply::write greys them (src/ply.cpp:90).  A record is that point:
 *   x, y, z   mvsv_calc_coordinate(col, row, v) bit for bit, col / row relative to
 *             the view
 *   grey      int((z - (float)mn) / (float)(mx - mn) * 255.0) with mn / mx the frame's
 *             min / max over v > 0: float difference and quotient, double product,
 *             truncation -- what mvsv_write_ply prints in MVSV_PLY_WITH_COLOR mode.
 *             Not clamped to 0..255 (z is in millimetres; the reference does not
 *             clamp either).  INT32_MIN where the double is NaN or outside int32,
 *             notably for every point of a frame with mx == mn.
 * Record k of frame f is its k-th valid pixel in raster order, at
 * records[f * capacity + k]; positions come from a prefix sum, so two runs give the
 * same bytes.  At most capacity records per frame are written and nothing behind
 * them; counts[f] is the number of valid pixels even where it exceeds capacity;
 * minmax[2 f] = (mn, mx), or (32767, -32768) for a frame without a positive value
 * (count 0, nothing written).
 *
 * dmap as for mvsv_normalize_minmax_device (any 2-byte-aligned view, packed loads
 * where the strides allow); records 16-byte aligned; width * height < 2^31; all
 * device pointers, asynchronous on the context's stream; minmax may be NULL. */
typedef struct {
    float x, y, z;
    int32_t grey;
} mvsv_cloud_point;
MVSV_API int mvsv_point_cloud_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t stride, size_t frame_stride,
                                     int width, int height, const float* Q, mvsv_cloud_point* records, int capacity,
                                     int* counts, int32_t* minmax);
/* Same for one host map into host records (synchronous): *count and minmax[2] (may
 * be NULL) are read back first, then only min(*count, capacity) records. */
MVSV_API int mvsv_point_cloud(mvsv_ctx* ctx, const int16_t* dmap, size_t stride, int width, int height,
                              const float* Q, mvsv_cloud_point* records, int capacity, int* count, int32_t* minmax);

/* ---- display maps: cv::normalize(NORM_MINMAX, CV_8U) of a disparity map ---------
 * OpenCV 3.4's arithmetic (normalize -> Mat::convertTo, CV_16S -> CV_8U, no mask;
 * its SSE2 / scalar form, where product and sum round separately):
 *   smin, smax  the minimum / maximum over all values of the view (the invalid
 *               marker (minDisparity - 1) * 16 included)
 *   in double   dmin = min(alpha, beta), dmax = max(alpha, beta),
 *               scale = (dmax - dmin) * (smax - smin > DBL_EPSILON ? 1 / (smax - smin) : 0),
 *               shift = dmin - smin * scale, every operation rounded on its own
 *   in float    out = saturate_u8(round_half_even((float)v * (float)scale + (float)shift)),
 *               product and sum each rounded
 * A constant map gives scale 0 and every pixel saturate(dmin).
 *
 * dmap: n int16 views (device pointers, strides in elements; any 2-byte-aligned
 * view with stride >= width -- no byte outside [row, row + width) is touched).
 * Row and frame strides that are multiples of 8 elements take packed 16-byte
 * loads around narrow head / tail elements, other strides narrow loads; the
 * results are the same.  All calls are asynchronous on the context's stream.
 *
 * minmax: [n][2] int16 (min, max) per frame.  positive_only != 0: over the
 * values > 0 only (Utility::calcMinMaxDisparity's rule); a frame without one
 * gives (32767, -32768). */
MVSV_API int mvsv_minmax_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t stride, size_t frame_stride,
                                int width, int height, int positive_only, int16_t* minmax);
/* out: n uint8 maps (device pointer, strides in bytes, any alignment); minmax:
 * device pointer, [n][2] (smin, smax) of every frame, or NULL.  Each frame is
 * normalised with its own min / max. */
MVSV_API int mvsv_normalize_minmax_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t stride,
                                          size_t frame_stride, int width, int height, double alpha, double beta,
                                          uint8_t* out, size_t out_stride, size_t out_frame_stride,
                                          int16_t* minmax);
/* Same for one host map into a host image (synchronous); minmax: 2 int16 on the
 * host, or NULL. */
MVSV_API int mvsv_normalize_minmax(mvsv_ctx* ctx, const int16_t* dmap, size_t stride, int width, int height,
                                   double alpha, double beta, uint8_t* out, size_t out_stride, int16_t* minmax);

/* ---- detection view: the annotated BGR frame of the detection programs ------------
 * What trgt/demo.cpp:280-298 (and mean_test, sample_test, obstacle, ...) show per
 * frame: cv::normalize(NORM_MINMAX, CV_8U), cv::cvtColor(GRAY2BGR), View's grids
 * (src/view.cpp) and drawFoundObstacles, in one device pass.  The view of a
 * width x height map (both >= 9) is uint8 [height][width][3] in B, G, R order.
 * Every pixel starts as its display byte in all three channels (exactly what
 * mvsv_normalize_minmax_device writes for alpha, beta); then the layers of
 * `layers` are drawn in this order, each over everything before it, all
 * relative to the view and clipped to it (a restatement of OpenCV 3.4's
 * cv::line, filled cv::rectangle and filled cv::circle, thickness 1, no
 * antialiasing):
 *   SUBIMAGE_GRID  View::drawSubimageGrid: colour (100, 0, 0), whole columns
 *                  (width / 9) * k and whole rows (height / 9) * k, k in {1, 2, 4, 5, 7, 8}
 *   OBSTACLE_GRID  View::drawObstacleGrid: colour (0, 0, 255), columns width / 3
 *                  and 2 * (width / 3), rows height / 3 and 2 * (height / 3)
 *   FOUND_TILES    drawFoundObstacles(Subimage): tile (c, r), index r * 9 + c, is
 *                  found when means[i] < tile_first && means[i] > tile_second
 *                  (float compares, MeanDisparityDetection::detectObstacles) and
 *                  paints (0, 0, 255) on c * dx <= x <= c * dx + dx,
 *                  r * dy <= y <= r * dy + dy with dx = width / 9, dy = height / 9:
 *                  both corners included, as a filled cv::rectangle does
 *   FOUND_POINTS   drawFoundObstacles(Samplepoint): a lattice point of
 *                  mvsv_samplepoint_layout(width, height) is found when
 *                  values[i] < point_first && values[i] > point_second and paints
 *                  cv::circle(centre, point_radius, (0, 0, 255), -1); the
 *                  reference's radius is 3, accepted are 0..3 (lattice steps are
 *                  >= 8, so circles neither overlap nor leave the view).  A map
 *                  without lattice points has no circles.
 * A NaN or infinite range bound is valid: the compares decide. */
enum {
    MVSV_VIEW_SUBIMAGE_GRID = 1,
    MVSV_VIEW_OBSTACLE_GRID = 2,
    MVSV_VIEW_FOUND_TILES = 4,
    MVSV_VIEW_FOUND_POINTS = 8
};
typedef struct {
    int layers;                      /* MVSV_VIEW_* bits */
    double alpha, beta;              /* as mvsv_normalize_minmax; finite */
    const float* means;              /* [n][81], needed by FOUND_TILES */
    float tile_first, tile_second;
    const float* values;             /* [n][nx * ny], needed by FOUND_POINTS */
    float point_first, point_second;
    int point_radius;                /* 0..3 */
} mvsv_view_spec;
/* dmap as for mvsv_normalize_minmax_device (any 2-byte-aligned view, packed
 * 16-byte loads where the strides allow); out: n images (device pointer, strides
 * in bytes, any alignment, out_stride >= 3 * width) -- no byte outside
 * [row, row + 3 * width) is touched; the store width (16, 8, 4, 2 or 1 bytes)
 * follows the alignment of out and its strides, the bytes are the same; dense
 * 16-byte-aligned images are the fast case.  FOUND_POINTS needs width < 2^20.
 * spec->means / values: device
 * pointers, frames back to back.  minmax: device pointer, [n][2] (smin, smax), or
 * NULL.  Asynchronous on the context's stream.  Unknown layer bits, a layer
 * whose pointer is NULL, a radius outside 0..3, a non-finite alpha / beta,
 * width or height < 9, or out_stride < 3 * width: MVSV_E_INVALID_ARG before any
 * launch. */
MVSV_API int mvsv_view_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t stride, size_t frame_stride,
                              int width, int height, const mvsv_view_spec* spec, uint8_t* out, size_t out_stride,
                              size_t out_frame_stride, int16_t* minmax);
/* Same for one host map into a host image (synchronous); spec->means / values
 * are host pointers, minmax: 2 int16 on the host, or NULL. */
MVSV_API int mvsv_view(mvsv_ctx* ctx, const int16_t* dmap, size_t stride, int width, int height,
                       const mvsv_view_spec* spec, uint8_t* out, size_t out_stride, int16_t* minmax);
/* The layers alone, painted over an existing host BGR image the way View::draw*Grid
 * and drawFoundObstacles do it (one after the other; alpha / beta play no part but
 * must be finite).  Host only, no device needed; the same argument rules. */
MVSV_API int mvsv_view_draw(uint8_t* bgr, size_t stride, int width, int height, const mvsv_view_spec* spec);

/* ---- frame stream ------------------------------------------
 * A camera loop pushes rectified pairs from host memory and pops int16 maps in
 * push order.  Up to `depth` frames are in flight: the upload of one frame, the
 * SGBM of the previous one (on the context stream) and the download of the one
 * before overlap.  With grid_roi, each frame's 9x9 MeanDisparityDetection grid
 * over that ROI of the map (createDMapROIS, trgt/mean_test.cpp:80-106) is
 * computed on the device and returned by pop. */
typedef struct mvsv_stream mvsv_stream;
typedef struct { int x0, y0, x1, y1; } mvsv_rect; /* half-open [x0,x1) x [y0,y1) */
MVSV_API int mvsv_stream_create(mvsv_ctx* ctx, int width, int height, const mvsv_sgbm_params* p,
                                int depth, const mvsv_rect* grid_roi, mvsv_stream** out);
/* new parameters for frames pushed from now on (the reference's setters between frames) */
MVSV_API int mvsv_stream_set_params(mvsv_stream* s, const mvsv_sgbm_params* p);
/* compute pushed frames `batch` at a time (1..depth, default 1): one frame-batch
 * launch per group of consecutive frames -- the sustained rate of the batch
 * kernels for up to batch-1 frames of extra latency; pop / set_params launch a
 * partial group when they need its frames */
MVSV_API int mvsv_stream_set_batch(mvsv_stream* s, int batch);
/* up to n (1..4, default 1) frame-batch launches in flight at once: launches go
 * round-robin to the caller's context and n-1 contexts the stream creates on the
 * same device (own HIP stream and scratch each; kernel options copied from the
 * caller's context) -- one launch's latency-bound kernels overlap the next's */
MVSV_API int mvsv_stream_set_inflight(mvsv_stream* s, int n);
/* MVSV_E_INVALID_ARG when depth frames are already pending (pop first) */
MVSV_API int mvsv_stream_push(mvsv_stream* s, const uint8_t* left, size_t left_stride,
                              const uint8_t* right, size_t right_stride);
/* waits for the oldest pending frame; out (int16, stride in elements) and means
 * (81 floats) may be NULL */
MVSV_API int mvsv_stream_pop(mvsv_stream* s, int16_t* out, size_t out_stride, float* means);
/* pop without the map copy: *map points at the frame's int16 map in the stream's
 * pinned host slot (width elements per row, rows contiguous), valid until the
 * next push (which may reuse the slot); means (81 floats) may be NULL */
MVSV_API int mvsv_stream_pop_view(mvsv_stream* s, const int16_t** map, float* means);
MVSV_API int mvsv_stream_pending(const mvsv_stream* s);
MVSV_API void mvsv_stream_destroy(mvsv_stream* s);

/* ---- raw frame stream: camera pairs in, rectified on the device ------------------
 * The loop of trgt/liveDisparity.cpp:82-101 / trgt/mean_test.cpp:258-318:
 * Stereosystem::getRectifiedImagepair (two cv::remap + the mDisplayROI crop,
 * src/Stereosystem.cpp:244-315), optionally cv::resize by a factor, then
 * Disparity::sgbm and the detection grid.  A raw stream owns the rectification:
 * the four float maps are converted once, at creation, to cv::convertMaps'
 * fixed-point form (cropped to roi, device resident); a pushed raw pair is
 * uploaded once and rectified (and resized) by kernels ahead of its SGBM launch,
 * so the rectified pair never visits the host unless keep_rectified asks for it.
 * The maps are only read during mvsv_stream_create_raw.  Map values follow
 * mvsv_convert_maps' contract. */
typedef struct {
    int raw_width, raw_height; /* the camera frame, each 1..32767 */
    const float* maps[4];      /* left x, left y, right x, right y: host, raw size */
    size_t map_stride;         /* floats per row, >= raw_width */
    mvsv_rect roi;             /* mDisplayROI: non-empty, inside the raw frame */
    double factor;             /* 0 or 1: none; else cv::resize(.., factor, factor) of the crop */
    int keep_rectified;        /* mvsv_stream_pop_pair can also return the rectified pair */
} mvsv_rectification;
/* The stream's frames (what SGBM sees and pop returns) have the roi's size, or
 * mvsv_resize_size(roi width, roi height, factor, factor) with a factor; p and
 * grid_roi are validated against that size (mvsv_stream_size reports it).
 * set_params / set_batch / set_inflight / pop / pop_view / pending / destroy work
 * as on a stream of rectified pairs. */
MVSV_API int mvsv_stream_create_raw(mvsv_ctx* ctx, const mvsv_rectification* rect,
                                    const mvsv_sgbm_params* p, int depth, const mvsv_rect* grid_roi,
                                    mvsv_stream** out);
/* size of the maps a stream returns (either kind of stream) */
MVSV_API int mvsv_stream_size(const mvsv_stream* s, int* width, int* height);
/* a raw_width x raw_height pair; MVSV_E_INVALID_ARG on a stream of rectified pairs
 * (as mvsv_stream_push is on a raw stream) and when depth frames are pending */
MVSV_API int mvsv_stream_push_raw(mvsv_stream* s, const uint8_t* left, size_t left_stride,
                                  const uint8_t* right, size_t right_stride);
/* mvsv_stream_pop that can also hand out the frame's rectified (cropped, resized)
 * pair -- what the reference's loops display or save
 * (trgt/captureDisparity.cpp:270-271).  Every output may be NULL; non-NULL
 * rect_left / rect_right on a stream without keep_rectified is
 * MVSV_E_INVALID_ARG (the frame stays pending). */
MVSV_API int mvsv_stream_pop_pair(mvsv_stream* s, int16_t* out, size_t out_stride, float* means,
                                  uint8_t* rect_left, size_t rect_left_stride, uint8_t* rect_right,
                                  size_t rect_right_stride);

/* The lattice detector in the stream (either kind): every frame's sample point
 * values and hits are computed after its SGBM, on the same device stream as the
 * mean grid, and come back with the frame -- the reference's loop with both
 * detectors (trgt/demo.cpp:206-209,271-276) without the map visiting the host
 * first.  roi: the part of the map the lattice is laid over (NULL: the whole map;
 * it must lie inside the stream's frame), radius as for
 * mvsv_samplepoint_values_device, Q / range_first / range_second as for
 * mvsv_samplepoint_detect_device; max_hits <= 0: room for every point.  Allowed
 * only while no frame is pending (MVSV_E_INVALID_ARG otherwise); a second call
 * replaces the first.  A stream that never enables it enqueues nothing extra. */
MVSV_API int mvsv_stream_enable_samplepoints(mvsv_stream* s, const mvsv_rect* roi, int radius,
                                             const float* Q, float range_first, float range_second,
                                             int max_hits);
MVSV_API int mvsv_stream_disable_samplepoints(mvsv_stream* s);
/* Waits for the oldest pending frame and copies its lattice results out without
 * popping it (so it composes with pop, pop_view and pop_pair): values (nx * ny
 * floats of the roi's layout), *count (all hits) and the first min(count,
 * max_hits, capacity) hit records.  Every output may be NULL.
 * MVSV_E_INVALID_ARG when the lattice is not enabled or no frame is pending; the
 * frame's own error when its launch failed (as pop reports it).  The frame stays
 * pending either way. */
MVSV_API int mvsv_stream_front_samples(mvsv_stream* s, float* values, int* count,
                                       mvsv_sample_hit* hits, int capacity);

/* The display map in the stream (either kind): every frame's
 * cv::normalize(dMap(roi), out, alpha, beta, NORM_MINMAX, CV_8U) is computed after
 * its SGBM on the same device stream and comes back with the frame, next to the
 * int16 map -- the last step of the reference's loops (trgt/liveDisparity.cpp:92;
 * the detector loops normalise the work ROI, trgt/mean_test.cpp:307).  roi: NULL
 * for the whole map; it must lie inside the stream's frame.  alpha, beta finite.
 * Allowed only while no frame is pending (MVSV_E_INVALID_ARG otherwise); a second
 * call replaces the first.  A stream that never enables it enqueues nothing extra. */
MVSV_API int mvsv_stream_enable_display(mvsv_stream* s, const mvsv_rect* roi, double alpha, double beta);
MVSV_API int mvsv_stream_disable_display(mvsv_stream* s);
/* Waits for the oldest pending frame and copies its display map (roi height rows
 * of roi width bytes, out_stride bytes apart) and minmax[2] = (smin, smax) out
 * without popping it, so it composes with pop, pop_view, pop_pair and
 * front_samples.  Either output may be NULL.  MVSV_E_INVALID_ARG when the display
 * is not enabled or no frame is pending; the frame's own error when its launch
 * failed (as pop reports it).  The frame stays pending either way. */
MVSV_API int mvsv_stream_front_display(mvsv_stream* s, uint8_t* out, size_t out_stride, int16_t* minmax);
/* Same without the copy: *map points at the frame's dense map (stride = roi
 * width) in the stream's pinned slot, valid until the next push. */
MVSV_API int mvsv_stream_front_display_view(mvsv_stream* s, const uint8_t** map, int16_t* minmax);

/* The detection view in the stream (either kind): every frame's mvsv_view_device
 * over roi (NULL: the whole map; at least 9 x 9) is computed after the frame's
 * mean grid and lattice passes and comes back with the frame, in buffers of its
 * own (independent of the display).  spec's layers, alpha, beta, tile range and
 * point_radius are used; its means / values pointers and point range are ignored:
 *   FOUND_TILES   needs a stream created with a grid_roi equal to roi; the means
 *                 are the frame's own, on the device
 *   FOUND_POINTS  needs mvsv_stream_enable_samplepoints with the same ROI; its
 *                 range and the frame's device values are used.  While the view
 *                 uses them, mvsv_stream_disable_samplepoints and a change of
 *                 their ROI are refused.
 * Allowed only while no frame is pending; a second call replaces the first.
 * MVSV_E_INVALID_ARG with a message otherwise. */
MVSV_API int mvsv_stream_enable_view(mvsv_stream* s, const mvsv_rect* roi, const mvsv_view_spec* spec);
MVSV_API int mvsv_stream_disable_view(mvsv_stream* s);
/* As mvsv_stream_front_display: the oldest pending frame's view (roi height rows of
 * 3 * roi width bytes, out_stride bytes apart) and minmax[2], without popping. */
MVSV_API int mvsv_stream_front_view(mvsv_stream* s, uint8_t* out, size_t out_stride, int16_t* minmax);
/* Same without the copy: *view points at the frame's dense image (stride = 3 * roi
 * width) in the stream's pinned slot, valid until the next push. */
MVSV_API int mvsv_stream_front_view_view(mvsv_stream* s, const uint8_t** view, int16_t* minmax);

/* The point cloud in the stream (either kind): every frame's
 * mvsv_point_cloud_device of dMap(roi) is computed after its SGBM on the same
 * device stream -- what Utility::dmap2pcl("pointcloud.ply", dMapRaw, Q_32F) makes of
 * a frame (trgt/demo.cpp:394).  roi: NULL for the whole map; it must lie inside the
 * stream's frame, and x / y count from its corner, as for dMapRaw(roi).
 * max_points <= 0: room for every pixel of the roi.  The records stay on the device,
 * in a ring of depth x max_points; only (count, min, max) come back with the frame.
 * Allowed only while no frame is pending (MVSV_E_INVALID_ARG otherwise); a second
 * call replaces the first.  A stream that never enables it enqueues and allocates
 * nothing extra. */
MVSV_API int mvsv_stream_enable_cloud(mvsv_stream* s, const mvsv_rect* roi, const float* Q, int max_points);
MVSV_API int mvsv_stream_disable_cloud(mvsv_stream* s);
/* Waits for the oldest pending frame and copies the first min(count, max_points,
 * capacity) records from the device, *count = the number of pixels with v > 0 (it
 * may exceed both), minmax[2] = (min, max) over them, without popping the frame, so
 * it composes with pop, pop_view, pop_pair, front_samples and front_display.  Every
 * output may be NULL.  MVSV_E_INVALID_ARG when the cloud is not enabled or no frame
 * is pending; the frame's own error when its launch failed (as pop reports it). */
MVSV_API int mvsv_stream_front_cloud(mvsv_stream* s, mvsv_cloud_point* records, int capacity, int* count,
                                     int32_t* minmax);
/* Same without the copy: *records_dev is the device pointer of the frame's slot
 * (max_points records, the first min(count, max_points) written), valid until the
 * frame is popped -- for consumers that stay on the GPU. */
MVSV_API int mvsv_stream_front_cloud_device(mvsv_stream* s, const mvsv_cloud_point** records_dev, int* count,
                                            int32_t* minmax);

/* ---- camera set-up: the focus measure (Utility::checkSharpness, src/utility.cpp:163-174) ----
 * OpenCV 3.4: Lx = sepFilter2D(src, CV_64F, kernelX = M, kernelY = G), Ly =
 * sepFilter2D(src, CV_64F, kernelX = G, kernelY = M) with M = (-1, 2, -1) and
 * G = getGaussianKernel(3, -1) = (0.25, 0.5, 0.25); the result is cv::mean(|Lx| + |Ly|).
 *   border   BORDER_REFLECT_101 (index i of n: 0 for n == 1, else -i below 0 and
 *            2n - 2 - i from n on)
 *   ROI      the filter engine does not isolate a view: the 1-pixel halo of a roi
 *            comes from the parent image and is reflected only at the parent's border
 *   mean     sum * (1.0 / N): a reciprocal and a product, each rounded
 * Every intermediate is a multiple of 0.25 far below 2^53, so the doubles are exact
 * and
 *   S4 = sum over the roi of |KX (*) s| + |KY (*) s|,  KX = (1,2,1)^T (-1,2,-1) = 4 Lx,
 *                                                      KY = (-1,2,-1)^T (1,2,1) = 4 Ly
 * on the reflect-extended parent s is an exact integer (at most 4080 a pixel).  The
 * device delivers S4; sharpness = (S4 / 4.0) * (1.0 / N) in host double, N the roi's
 * pixels.  No atomics: two runs give the same bytes.
 *
 * n u8 images (device), strides in bytes, any alignment (row and frame strides that
 * are multiples of 4 take packed loads, others narrow ones; no byte outside
 * [row, row + width) is read); roi NULL = whole image, else non-empty and inside it;
 * width * height < 2^31; sums: device, n int64.  Asynchronous on the context's stream. */
MVSV_API int mvsv_sharpness_device(mvsv_ctx* ctx, int n, const uint8_t* img, size_t stride, size_t frame_stride,
                                   int width, int height, const mvsv_rect* roi, int64_t* sums);
/* one host image, synchronous; value and sum4 may each be NULL */
MVSV_API int mvsv_sharpness(mvsv_ctx* ctx, const uint8_t* img, size_t stride, int width, int height,
                            const mvsv_rect* roi, double* value, int64_t* sum4);

/* The focus measure in the stream (either kind): mvsv_sharpness_device of the pushed
 * left and right image, each over its own roi (NULL: the whole image), on the frame's
 * device stream beside the other post-passes -- the value liveView prints, with every
 * frame.  The pushed images are measured: on a raw stream the raw camera pair before
 * rectification (what getImagepair returned), and the rois are validated against that
 * size.  16 bytes more come back with a frame.  Allowed only while no frame is pending
 * (MVSV_E_INVALID_ARG otherwise); a second call replaces the first.  A stream that
 * never enables it enqueues and allocates nothing extra. */
MVSV_API int mvsv_stream_enable_sharpness(mvsv_stream* s, const mvsv_rect* roi_left, const mvsv_rect* roi_right);
MVSV_API int mvsv_stream_disable_sharpness(mvsv_stream* s);
/* Waits for the oldest pending frame and hands out (left, right) values and / or S4
 * sums without popping it, so it composes with pop, pop_view, pop_pair, front_samples,
 * front_display and front_cloud.  Either output may be NULL.  MVSV_E_INVALID_ARG when
 * the measure is not enabled or no frame is pending; the frame's own error when its
 * launch failed (as pop reports it). */
MVSV_API int mvsv_stream_front_sharpness(mvsv_stream* s, double value[2], int64_t sum4[2]);

/* ---- StereoBM streams (trgt/disparityTest.cpp:267-268 runs both matchers) -----------
 * A stream computes its frames with one matcher at a time.  create_bm / create_raw_bm
 * are mvsv_stream_create / mvsv_stream_create_raw with StereoBM (mvsv_bm_device) as the
 * matcher.  mvsv_stream_set_bm_params switches a stream of either origin to StereoBM
 * for the frames pushed from now on, mvsv_stream_set_params to SGBM; each validates
 * against the stream's size and first launches the frames already pushed, so a
 * frame-batch launch never mixes matchers or parameter sets.  Everything behind the
 * matcher (mean grid, sample points, display, view, cloud, sharpness, pop*, batch,
 * inflight lanes, raw rectification) is a function of the int16 map and works alike;
 * StereoBM's FILTERED value (min_disparity - 1) * 16 goes through each product's own
 * rule.  The strip-wait report (MVSV_E_TIMEOUT) is SGBM's: a StereoBM frame never has it. */
enum { MVSV_MATCHER_SGBM = 0, MVSV_MATCHER_BM = 1 };
MVSV_API int mvsv_stream_create_bm(mvsv_ctx* ctx, int width, int height, const mvsv_bm_params* p, int depth,
                                   const mvsv_rect* grid_roi, mvsv_stream** out);
MVSV_API int mvsv_stream_create_raw_bm(mvsv_ctx* ctx, const mvsv_rectification* rect, const mvsv_bm_params* p,
                                       int depth, const mvsv_rect* grid_roi, mvsv_stream** out);
MVSV_API int mvsv_stream_set_bm_params(mvsv_stream* s, const mvsv_bm_params* p);
/* the matcher of the frames pushed from now on (MVSV_MATCHER_*); -1 for a null stream */
MVSV_API int mvsv_stream_matcher(const mvsv_stream* s);

/* ---- colour frames into a stream of rectified pairs ---------------------------------
 * mvsv_stream_enable_bgr: the stream also takes src_width x src_height interleaved BGR
 * pairs (mvsv_stream_push_bgr); each is uploaded once as BGR and mvsv_prepare_gray_device
 * (halve, variant) writes the frame's grey pair on the device ahead of its matcher, the
 * way a raw stream rectifies.  mvsv_prepare_size(src_width, src_height, halve) must equal
 * the stream's size.  Only on a stream of rectified pairs, only while no frame is pending
 * (MVSV_E_INVALID_ARG otherwise); a second call replaces the first.  mvsv_stream_push
 * (grey) stays valid, and grey and BGR frames may alternate.  The sharpness product of a
 * BGR frame is measured on its prepared grey pair (the stream's size), as for a grey frame.
 * mvsv_stream_push_bgr: strides in bytes, >= 3 * src_width; MVSV_E_INVALID_ARG on a raw
 * stream, without enable_bgr, and when depth frames are pending. */
MVSV_API int mvsv_stream_enable_bgr(mvsv_stream* s, int src_width, int src_height, int halve, int variant);
MVSV_API int mvsv_stream_disable_bgr(mvsv_stream* s);
MVSV_API int mvsv_stream_push_bgr(mvsv_stream* s, const uint8_t* left, size_t left_stride, const uint8_t* right,
                                  size_t right_stride);
/* mvsv_stream_set_bgr_match: with on != 0 the map of every BGR frame pushed from now on
 * comes from the colour matcher (mvsv_sgbm_bgr_device) on the frame's BGR pair at the
 * stream's size: the INTER_AREA half of mvsv_prepare_gray per channel, without the grey
 * conversion, or the pushed pair itself with halve 0.  The grey pair is still prepared
 * and feeds the sharpness product and every other grey product as before; every product
 * computed from the map follows the colour map.  Valid after mvsv_stream_enable_bgr,
 * while no frame is pending and with the SGBM matcher (MVSV_E_INVALID_ARG otherwise);
 * while it is on, mvsv_stream_set_bm_params is MVSV_E_INVALID_ARG.  Grey pushes keep
 * working; a frame-batch launch never holds grey-matched and colour-matched frames
 * together (a frame of the other kind sends the pending ones off first, as a parameter
 * change does).  mvsv_stream_disable_bgr and a new mvsv_stream_enable_bgr switch it off. */
MVSV_API int mvsv_stream_set_bgr_match(mvsv_stream* s, int on);
/* mvsv_stream_set_census: every frame pushed from now on is matched on the census cost
 * (mvsv_sgbm_census_device) with this window; 0, 0 switches back to the Birchfield-Tomasi
 * cost.  Valid while no frame is pending, with the SGBM matcher and without colour
 * matching (MVSV_E_INVALID_ARG otherwise, also for a window or parameters that
 * mvsv_sgbm_census_validate refuses); while it is on, mvsv_stream_set_bgr_match(1) and
 * a switch to StereoBM are refused, and mvsv_stream_set_params validates against the
 * census rules.  Every stage computed from the map follows the census map. */
MVSV_API int mvsv_stream_set_census(mvsv_stream* s, int census_width, int census_height);
/* mvsv_stream_set_bm_census: the same for the StereoBM matcher (mvsv_bm_census_device);
 * 0, 0 switches back to the SAD cost.  Valid while no frame is pending and with the
 * StereoBM matcher (MVSV_E_INVALID_ARG otherwise, also for a window or parameters that
 * mvsv_bm_census_validate refuses); while it is on, mvsv_stream_set_bm_params validates
 * against the census rules and mvsv_stream_set_params (a switch to SGBM) is refused. */
MVSV_API int mvsv_stream_set_bm_census(mvsv_stream* s, int census_width, int census_height);

/* ---- device ends of a stream: frames from device memory, maps handed back there ------
 * mvsv_stream_push_device / _push_raw_device / _push_bgr_device: n >= 1 frames (strides in
 * bytes, frame strides between consecutive frames; rows of width, raw_width or
 * 3 * src_width bytes) become n consecutive pushes -- the frames, their order, the launch
 * grouping by `batch` and the behaviour at the ring's wrap are those of n single pushes.
 * n > depth - pending is MVSV_E_INVALID_ARG and pushes nothing; the kind of stream is
 * checked as by the host calls.  The sources must be memory of the stream's device or
 * device-accessible host memory (pinned, managed): anything else is MVSV_E_INVALID_ARG
 * before anything is enqueued.
 * Ordering is by events, without host synchronisation: the copy into the slots (one
 * kernel launch per contiguous piece of the ring, so at most two) waits for what is
 * queued on producer_stream (NULL: the legacy null stream) at the call, and
 * producer_stream is made to wait for the copy: what the caller enqueues on it after the
 * call may overwrite or free the sources. */
MVSV_API int mvsv_stream_push_device(mvsv_stream* s, int n, const uint8_t* left, size_t left_stride,
                                     size_t left_frame_stride, const uint8_t* right, size_t right_stride,
                                     size_t right_frame_stride, void* producer_stream);
MVSV_API int mvsv_stream_push_raw_device(mvsv_stream* s, int n, const uint8_t* left, size_t left_stride,
                                         size_t left_frame_stride, const uint8_t* right, size_t right_stride,
                                         size_t right_frame_stride, void* producer_stream);
MVSV_API int mvsv_stream_push_bgr_device(mvsv_stream* s, int n, const uint8_t* left, size_t left_stride,
                                         size_t left_frame_stride, const uint8_t* right, size_t right_stride,
                                         size_t right_frame_stride, void* producer_stream);
/* Which per-frame products are also copied to the stream's pinned host slots (default:
 * all).  Only while no frame is pending.  A host getter of a product that is switched
 * off -- pop / pop_pair with a non-NULL out, pop_view, pop_pair's rectified outputs,
 * front_display*, front_view* -- returns MVSV_E_INVALID_ARG and leaves the frame pending;
 * pop with out == NULL still pops.  The means, the sample points, the cloud header, the
 * sharpness and the display / view (min, max) always come to the host. */
#define MVSV_HOST_MAP 1
#define MVSV_HOST_RECTIFIED 2
#define MVSV_HOST_DISPLAY 4
#define MVSV_HOST_VIEW 8
#define MVSV_HOST_ALL 15
MVSV_API int mvsv_stream_set_host_outputs(mvsv_stream* s, int mask);
/* Pops the oldest frame (waiting for it on the host, status and MVSV_E_TIMEOUT as pop) and
 * enqueues the copy of its map into out_dev (device memory, stride in elements) on
 * consumer_stream (NULL: the legacy null stream); the slot's next frame waits for that copy. */
MVSV_API int mvsv_stream_pop_device(mvsv_stream* s, int16_t* out_dev, size_t out_stride, float* means,
                                    void* consumer_stream);
/* No pop, no copy: pointers into the stream's device rings (rows contiguous), complete
 * when the call returns and valid until the frame is popped -- the rule of
 * front_cloud_device.  They work whether or not the matching host output is on.
 * front_rectified_device needs a stream created with keep_rectified. */
MVSV_API int mvsv_stream_front_map_device(mvsv_stream* s, const int16_t** map_dev, float* means);
MVSV_API int mvsv_stream_front_rectified_device(mvsv_stream* s, const uint8_t** left_dev, const uint8_t** right_dev);
MVSV_API int mvsv_stream_front_display_device(mvsv_stream* s, const uint8_t** map_dev, int16_t* minmax);
MVSV_API int mvsv_stream_front_view_device(mvsv_stream* s, const uint8_t** bgr_dev, int16_t* minmax);
/* Everything the stream enqueues from now on (uploads, launches) waits for what is queued
 * on hip_stream now: for a zero-copy consumer whose reads of a front_*_device pointer may
 * still be running when it pops the frame, after which the slot may be pushed again. */
MVSV_API int mvsv_stream_fence(mvsv_stream* s, void* hip_stream);

/* ---- camera set-up: undistorted pairs (Stereosystem::getUndistortedImagepair) -------
 * cv::undistort(src, dst, K, dist) of OpenCV 3.4 (no new camera matrix: Ar = K) works
 * in stripes of min(max(1, 4096 / W), H) rows; for the stripe starting at row y0 it
 * calls initUndistortRectifyMap(K, dist, I, Ar with Ar(1,2) = cy - y0, CV_16SC2) and
 * remap(INTER_LINEAR, BORDER_CONSTANT 0).  CV_16SC2 maps come straight from the doubles
 * u, v: iu = cvRound(u * 32), iv = cvRound(v * 32) (half to even), xy = ((short)(iu >> 5),
 * (short)(iv >> 5)) -- plain casts, not saturated as in mvsv_convert_maps --,
 * frac = (iv & 31) * 32 + (iu & 31).
 *
 * mvsv_undistort_maps: those maps for a whole width x height image (host only).  K
 * 3x3, dist as for mvsv_init_undistort_rectify_map (ndist 0: all zeros, dist may be
 * NULL), new_K 3x3 or NULL for K; xy_stride in int16 pairs, frac_stride in elements.
 * The double arithmetic is mvsv_init_undistort_rectify_map's (shared code, the
 * incremental walk along a row included), and so is its caveat: Ar is inverted by its
 * adjugate where OpenCV uses LU, so u, v may differ in the last bit and a map entry by
 * one 1/32 step where u * 32 or v * 32 lies that close to a rounding tie. */
MVSV_API int mvsv_undistort_maps(const double* K, const double* dist, int ndist, const double* new_K, int width,
                                 int height, int16_t* xy, size_t xy_stride, uint16_t* frac, size_t frac_stride);
/* cv::remap(src, dst, xy, frac, INTER_LINEAR, BORDER_CONSTANT 0) for CV_8UC1 images and
 * CV_16SC2 + CV_16UC1 maps on the device: pure integer (mvsv_remap_device's arithmetic
 * behind its rounding step), bit-exact for given maps.  n frames share one map pair of
 * the destination's size; image strides in bytes, xy_stride in int16 pairs, frac_stride
 * in elements; maps 2-byte aligned. */
MVSV_API int mvsv_remap_fixed_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t src_stride,
                                     size_t src_frame_stride, int src_width, int src_height, const int16_t* xy,
                                     size_t xy_stride, const uint16_t* frac, size_t frac_stride, uint8_t* dst,
                                     size_t dst_stride, size_t dst_frame_stride, int dst_width, int dst_height);
/* Stereosystem::getUndistortedImagepair on host buffers (synchronous): cv::undistort of
 * the left image with (K_left, dist_left) and of the right one with (K_right,
 * dist_right).  out_left / out_right may be left / right (the reference copies the
 * result back into the pair).  The context keeps the device maps of the last
 * calibration it was called with (size, K and dist of both sides): a camera loop builds
 * and uploads them once; mvsv_trim releases them. */
MVSV_API int mvsv_undistort_pair(mvsv_ctx* ctx, const uint8_t* left, size_t left_stride, const uint8_t* right,
                                 size_t right_stride, int width, int height, const double* K_left,
                                 const double* dist_left, int ndist_left, const double* K_right,
                                 const double* dist_right, int ndist_right, uint8_t* out_left,
                                 size_t out_left_stride, uint8_t* out_right, size_t out_right_stride);

/* ---- before the path: rectification ---------------------------
 * cv::remap(src, dst, map_x, map_y, INTER_LINEAR) with BORDER_CONSTANT 0 for CV_8UC1
 * images and CV_32FC1 maps, in OpenCV 3.4's fixed-point arithmetic (INTER_BITS 5,
 * 15-bit weights): bit-exact for given maps.  n frames (device pointers) share one
 * map pair (dst_width x dst_height floats each, map_stride floats per row). */
MVSV_API int mvsv_remap_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t src_stride,
                               size_t src_frame_stride, int src_width, int src_height,
                               const float* map_x, const float* map_y, size_t map_stride,
                               uint8_t* dst, size_t dst_stride, size_t dst_frame_stride,
                               int dst_width, int dst_height);

/* cv::convertMaps(map_x, map_y, xy, frac, CV_16SC2, false): the fixed-point form
 * in which cv::remap consumes CV_32FC1 maps (host only, no device needed).  Per
 * pixel X = cvRound(map_x * 32), Y = cvRound(map_y * 32) (float product, round
 * half to even); xy = (saturate_cast<short>(X >> 5), saturate_cast<short>(Y >> 5));
 * frac = (Y & 31) * 32 + (X & 31).  Strides per row: map_stride in floats,
 * xy_stride in int16 pairs, frac_stride in elements.  The same arithmetic as
 * the first lines of the remap kernel; as for mvsv_remap_device, the result is
 * undefined for map values that are not finite or have |value * 32| >= 2^31. */
MVSV_API int mvsv_convert_maps(const float* map_x, const float* map_y, size_t map_stride, int width,
                               int height, int16_t* xy, size_t xy_stride, uint16_t* frac,
                               size_t frac_stride);

/* Stereosystem::getRectifiedImagepair on host buffers: remap both images of a
 * W x H pair with their map pairs (maps: left x, left y, right x, right y, host,
 * W x H floats each), then crop to roi (mDisplayROI) into out_left / out_right
 * ((roi.x1 - roi.x0) x (roi.y1 - roi.y0) bytes). */
MVSV_API int mvsv_rectify_pair(mvsv_ctx* ctx, const uint8_t* left, size_t left_stride,
                               const uint8_t* right, size_t right_stride, int width, int height,
                               const float* const* maps, const mvsv_rect* roi, uint8_t* out_left,
                               size_t out_left_stride, uint8_t* out_right, size_t out_right_stride);

/* cv::resize(src, dst, Size(0, 0), fx, fy, INTER_LINEAR) for CV_8UC1 -- the resize
 * step of Stereosystem::getRectifiedImagepair(Stereopair&, float)
 * (src/Stereosystem.cpp:279-315), in OpenCV 3.4's arithmetic (11-bit fixed-point
 * taps; a factor of exactly 0.5 takes INTER_AREA's fast 2x2 path).
 * mvsv_resize_size: the output size (cvRound(width * fx), cvRound(height * fy)).
 * mvsv_resize_device: n frames, device pointers, strides in bytes.
 * mvsv_resize: one host image (dst holds the mvsv_resize_size image). */
MVSV_API int mvsv_resize_size(int src_width, int src_height, double fx, double fy, int* dst_width,
                              int* dst_height);
MVSV_API int mvsv_resize_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t src_stride,
                                size_t src_frame_stride, int src_width, int src_height, double fx,
                                double fy, uint8_t* dst, size_t dst_stride, size_t dst_frame_stride);
MVSV_API int mvsv_resize(mvsv_ctx* ctx, const uint8_t* src, size_t src_stride, int src_width,
                         int src_height, double fx, double fy, uint8_t* dst, size_t dst_stride);

/* ---- grey pair preparation: colour frames in (trgt/disparityTest.cpp:201-211) -------
 * What the reference's file-driven harness does to an image between cv::imread and
 * the matchers, on interleaved 8-bit BGR (CV_8UC3), in one kernel:
 *   halve = 1: cv::resize(src, dst, Size(), 0.5, 0.5, INTER_AREA) -- every channel by
 *              mvsv_resize's 2x2 rule ((a+b+c+d+2) >> 2 on whole blocks, the float mean
 *              rounded half to even on blocks clipped by an odd width or height), each
 *              channel rounded to 8 bits --, then
 *   always:    cv::cvtColor(BGR2GRAY) for 8 bit:
 *              MVSV_GRAY_Q14  (B*1868 + G*9617 + R*4899 + 8192) >> 14   (OpenCV up to
 *                             the early 3.4 releases; the default)
 *              MVSV_GRAY_Q15  (B*3735 + G*19235 + R*9798 + 16384) >> 15 (later releases)
 * halve = 0 is the conversion alone; any other value is MVSV_E_INVALID_ARG.
 * mvsv_prepare_size: the grey image's size (mvsv_resize_size(w, h, 0.5, 0.5) when
 * halving: cvRound, half to even; a 1-pixel side halves to 0 and is invalid).  Host only.
 * mvsv_prepare_gray_device: n frames, device pointers, strides in bytes, any base
 * alignment and any stride >= 3 * src_width (a BGR ROI view); sources whose base and
 * strides are multiples of 4 are read with packed loads.  No byte outside
 * [row, row + 3 * src_width) is read, none outside [row, row + dst_width) written.
 * Asynchronous on the context's stream.
 * mvsv_prepare_gray: one host image, synchronous. */
enum { MVSV_GRAY_Q14 = 0, MVSV_GRAY_Q15 = 1 };
MVSV_API int mvsv_prepare_size(int src_width, int src_height, int halve, int* dst_width, int* dst_height);
MVSV_API int mvsv_prepare_gray_device(mvsv_ctx* ctx, int n, const uint8_t* bgr, size_t stride, size_t frame_stride,
                                      int src_width, int src_height, int halve, int variant, uint8_t* dst,
                                      size_t dst_stride, size_t dst_frame_stride);
MVSV_API int mvsv_prepare_gray(mvsv_ctx* ctx, const uint8_t* bgr, size_t stride, int src_width, int src_height,
                               int halve, int variant, uint8_t* dst, size_t dst_stride);

/* ---- Disparity::tm: normalised cross-correlation row search (src/disparity.cpp:25-58) ----
 * For every pixel (i, j), i < height - k and j < width - k (both exclusive, the
 * reference's loop bounds), the k x k template left[i.., j..] is matched against the
 * windows right[i.., j + x ..], x = 0 .. width - j - k - 1 (the search strip ends at
 * column width - 2 and runs to the right), by cv::matchTemplate(CV_TM_CCORR_NORMED):
 * score = N / sqrt(sum T^2 * sum S^2), N = sum T * S, and 0 where the denominator is 0.
 * The first x with the largest score (cv::minMaxLoc's scan order) is stored; every
 * other pixel of the map is 0.  Scores are compared exactly: x beats the best b so far
 * iff N_x^2 * sum S_b^2 > N_b^2 * sum S_x^2 in 128-bit integers (strict: the earliest x
 * keeps a tie; a window of zeros counts as N = 0, sum S^2 = 1), never in floating
 * point alone -- cv::matchTemplate's arithmetic without the rounding of its float DFT.
 * mvsv_tm_validate: 1 <= k <= 31, k < min(width, height), sides <= 65535; context-free.
 * mvsv_tm: host images, synchronous; dst is 8 bit: x truncated (output.at<char>), so
 *   x >= 256 wraps.
 * mvsv_tm_device: n frames, device pointers, strides in bytes (ROI views where a stride
 *   exceeds the row), asynchronous on the context's stream.  elem_bytes 1: the wrapped
 *   byte; elem_bytes 2 (new): x as uint16, dst and its strides even.  Rows >= height - k
 *   and columns >= width - k are written as 0; no byte outside [row, row + width *
 *   elem_bytes) of a destination row is written, none outside [row, row + width) read. */
MVSV_API int mvsv_tm_validate(int k, int width, int height);
MVSV_API int mvsv_tm(mvsv_ctx* ctx, const uint8_t* left, size_t left_stride, const uint8_t* right,
                     size_t right_stride, int width, int height, int k, uint8_t* dst, size_t dst_stride);
MVSV_API int mvsv_tm_device(mvsv_ctx* ctx, int n, const uint8_t* left, size_t left_stride,
                            size_t left_frame_stride, const uint8_t* right, size_t right_stride,
                            size_t right_frame_stride, int width, int height, int k, void* dst,
                            size_t dst_stride, size_t dst_frame_stride, int elem_bytes);

/* cv::initUndistortRectifyMap(K, dist, R, P, size, CV_32FC1): K 3x3, dist =
 * (k1, k2, p1, p2[, k3[, k4, k5, k6]]) with ndist in {0, 4, 5, 8}, R 3x3, P 3x3 or
 * the left 3x3 of a 3x4 projection (row-major doubles).  Double-precision
 * restatement (inverse of P*R by adjugate; OpenCV uses SVD, so maps may differ
 * in the last float bit); host only. */
MVSV_API int mvsv_init_undistort_rectify_map(const double* K, const double* dist, int ndist,
                                             const double* R, const double* P, int width,
                                             int height, float* map_x, float* map_y,
                                             size_t map_stride);

/* cv::stereoRectify(K1, D1, K2, D2, size, R, T, R1, R2, P1, P2, Q, flags, alpha,
 * size, &roi1, &roi2) as Stereosystem::initRectification calls it
 * (src/Stereosystem.cpp:209-212: flags = CALIB_ZERO_DISPARITY, alpha = 0).
 * K 3x3, D (k1, k2, p1, p2[, k3[, k4, k5, k6]]), R 3x3, T 3; outputs R1/R2 3x3,
 * P1/P2 3x4, Q 4x4 (may be NULL), valid-pixel ROIs (may be NULL); all row-major
 * doubles.  Double-precision restatement of OpenCV 3.4's cvStereoRectify (host). */
#define MVSV_CALIB_ZERO_DISPARITY 1024
MVSV_API int mvsv_stereo_rectify(const double* K1, const double* D1, int ndist1, const double* K2,
                                 const double* D2, int ndist2, int width, int height,
                                 const double* R, const double* T, int flags, double alpha,
                                 double* R1, double* R2, double* P1, double* P2, double* Q,
                                 mvsv_rect* roi1, mvsv_rect* roi2);

/* ---- calibration files -------------------------------------------
 * cv::FileStorage YAML matrices ("key: !!opencv-matrix", rows / cols / dt / data) in
 * the layout OpenCV 3.x writes (%YAML:1.0 header, data lists wrapped at column 71,
 * doubles "%.16e", floats "%.8e", integral values "%d."): the files of
 * parameters/<system>/{intrinsic,extrinsic}.yml and afterCalibrationParameters.yml.
 * Empty matrices are rows = cols = 0, dt 'u'. */
#define MVSV_MAT_MAX 16
typedef struct {
    int rows, cols;
    char dt; /* 'u' 'c' 'w' 's' 'i' 'f' 'd' (CV_8U ... CV_64F) */
    double data[MVSV_MAT_MAX];
} mvsv_mat;
/* Stereosystem's intrinsic state: the nodes saveIntrinsic writes, in order. */
typedef struct {
    mvsv_mat camera_matrix_left, camera_matrix_right, dist_coeffs_left, dist_coeffs_right,
        camera_matrix_left_new, camera_matrix_right_new, q_matrix;
} mvsv_intrinsics;
typedef struct { mvsv_mat R, T, E, F; } mvsv_extrinsics;
/* One matrix node: MVSV_E_IO (cannot open), MVSV_E_PARSE (absent / malformed / > 16). */
MVSV_API int mvsv_read_matrix_yaml(const char* path, const char* key, mvsv_mat* out);
/* n matrix nodes in order (a new file). */
MVSV_API int mvsv_write_matrices_yaml(const char* path, const char* const* keys,
                                      const mvsv_mat* mats, int n);
/* Stereosystem::loadIntrinsic (src/Stereosystem.cpp:356-386): cameraMatrixLeft,
 * cameraMatrixRight and distCoeffsRight must exist (the reference checks
 * distCoeffsRight twice, never distCoeffsLeft); the *_new and Q fields come back
 * empty (loadIntrinsic does not read them). */
MVSV_API int mvsv_load_intrinsic(const char* path, mvsv_intrinsics* out);
/* Stereosystem::loadExtrinisic (src/Stereosystem.cpp:326-354): R, T, E, F required. */
MVSV_API int mvsv_load_extrinsic(const char* path, mvsv_extrinsics* out);
/* Stereosystem::saveIntrinsic / saveExtrinsic (src/Stereosystem.cpp:388-446). */
MVSV_API int mvsv_save_intrinsic(const char* path, const mvsv_intrinsics* in);
MVSV_API int mvsv_save_extrinsic(const char* path, const mvsv_extrinsics* in);

/* ---- after the path: reprojection and point-cloud output ----
 * Q is the 4x4 CV_32F reprojection matrix of stereoRectify, 16 floats row-major
 * (e.g. afterCalibrationParameters.yml "Q"). */

/* Utility::calcCoordinate for every pixel of n int16 maps (device pointers):
 * (X, Y, Z, W) = Q * (x, y, v / 16, 1) in OpenCV's float GEMM arithmetic, divided
 * by W; Z = 0 where Z / 1000 is infinite.  xyzw[f][y][x] = (X, Y, Z, v > 0), i.e.
 * float4 per pixel, row stride / frame stride in float4 elements. */
MVSV_API int mvsv_reproject_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t stride,
                                   size_t frame_stride, int width, int height, const float* Q,
                                   float* xyzw, size_t xyzw_stride, size_t xyzw_frame_stride);

/* Utility::calcCoordinate (one point, host): out = (X, Y, Z, 1). */
MVSV_API void mvsv_calc_coordinate(float image_x, float image_y, float d_value, const float* Q,
                                   float* out4);
/* calcCoordinate of n points at once (MeanDisparityDetection::detectObstacles'
 * per-tile loop, src/MeanDisparityDetection.cpp:228-240): xyd = n x (image x,
 * image y, disparity * 16), out = n x (X, Y, Z, 1); the same arithmetic as
 * mvsv_calc_coordinate, one call instead of one per found tile. */
MVSV_API void mvsv_calc_coordinates(int n, const float* xyd, const float* Q, float* out4);
/* Utility::calcDistance: Z / 1000 of calcCoordinate, 0 when infinite. */
MVSV_API float mvsv_calc_distance(float image_x, float image_y, float d_value, const float* Q);
/* Utility::calcDMapValues: metric point (x, y, z) -> image x, y and disparity * 16. */
MVSV_API void mvsv_calc_dmap_values(const float* c3, const float* Q, float* image_x,
                                    float* image_y, float* d_value);

enum { MVSV_PLY_PLAIN = 0, MVSV_PLY_WITH_COLOR = 1, MVSV_PLY_WITH_COLOR_SHADING = 2 };

/* ply::write: ASCII PLY of count vertices (x, y, z floats, vertex_stride floats
 * apart).  WITH_COLOR greys each vertex by (z - min) / (max - min) * 255 with the
 * min / max of the positive values of the int16 map dmap (the ply's mDMap);
 * WITH_COLOR_SHADING declares colour properties but writes none (as the
 * reference does).  Colour modes need dmap (returns MVSV_E_INVALID_ARG if it is
 * empty or has no positive value).  Host-only; MVSV_E_IO if the file cannot be
 * opened. */
MVSV_API int mvsv_write_ply(const char* path, const char* author, const char* object_name,
                            const float* xyz, size_t count, size_t vertex_stride, int mode,
                            const int16_t* dmap, size_t dmap_stride, int width, int height);

/* Utility::dmap2pcl: every pixel of the host int16 map with v > 0 reprojected
 * (on the device of ctx, mvsv_point_cloud_device: only the valid points come back)
 * and written as "Hagen Hiller" / "disparity pointcloud" PLY in MODE WITH_COLOR,
 * raster order. */
MVSV_API int mvsv_dmap2pcl(mvsv_ctx* ctx, const char* path, const int16_t* dmap, size_t stride,
                           int width, int height, const float* Q);

/* Disparity::loadSGBMParameters: reads configs/sgbm.yml keys minDisp, numDisp,
 * blockSize, disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize,
 * speckleWindowRange, mode into *values and applies the 8 setters + mode to
 * *p (P1/P2 untouched, as in the reference).  Missing numDisp, blockSize,
 * speckleWindowSize or speckleWindowRange -> MVSV_E_PARSE; other keys missing
 * leave the value 0 (cv::FileNode >> int on an empty node). */
MVSV_API int mvsv_load_sgbm_yaml(const char* path, mvsv_sgbm_params* p,
                                 mvsv_sgbm_yaml_values* values);
/* configs/bm.yml keys: numDisp, blockSize, preFilterCap, preFilterSize,
 * uniquenessRatio, textureThreshold (+ optional minDisp, speckleWindowSize,
 * speckleWindowRange, disp12MaxDiff, preFilterType). numDisp and blockSize are
 * required. */
MVSV_API int mvsv_load_bm_yaml(const char* path, mvsv_bm_params* p);

/* Stage profiling with HIP events (used by bench.py to time the dominant kernel
 * live).  Stages: 0 prefilter, 1 cost volume, 2 cost fixup, 3 path aggregation
 * (span of all direction passes before the final one), 4 final direction +
 * WTA/LR, 5 post-filters (median + speckle), 6 BM match, 7 path strips (the
 * sheared-strip kernel alone, inside stage 3), 8 path lines (the L->R line
 * kernel on the second stream, overlapping stage 7). */
#define MVSV_NUM_STAGES 9
MVSV_API int mvsv_profile_enable(mvsv_ctx* ctx, int on);
MVSV_API int mvsv_profile_reset(mvsv_ctx* ctx);
/* Synchronizes, then writes accumulated milliseconds and launch counts per stage. */
MVSV_API int mvsv_profile_read(mvsv_ctx* ctx, double* stage_ms, int* stage_launches, int n);
MVSV_API const char* mvsv_profile_stage_name(int stage);

/* Deterministic synthetic rectified pair: PCG32 noise,
 * 3x3 box blur, slanted-plane + rectangle disparity field, +-1 noise.
 * Host buffers of width*height bytes each. */
MVSV_API int mvsv_synth_pair(uint32_t seed, int width, int height, int min_disparity,
                             int num_disparities, uint8_t* left, uint8_t* right);

#ifdef __cplusplus
}
#endif
#endif /* MVSV_H */
