// mvsv_stereosystem.hpp — C++ drop-in for the reference's class Stereosystem
// (inc/Stereosystem.h:16-86, src/Stereosystem.cpp) on libmvsv: calibration
// files, the rectification set-up and the rectified (optionally resized) pair.
//
// Reference surface kept (names, argument meaning, return values, quirks):
//   getFundamentalMatrix / getTranslationMatrix / getBaseline / getRotationMatrix /
//   getQMatrix / getNewKMats                         src/Stereosystem.cpp:47-80
//   getUndistortedImagepair(Stereopair&)             src/Stereosystem.cpp:179-191
//   initRectification                                src/Stereosystem.cpp:193-241
//   getRectifiedImagepair(Stereopair&)               src/Stereosystem.cpp:243-277
//   getRectifiedImagepair(Stereopair&, float)        src/Stereosystem.cpp:279-315
//   resetRectification                               src/Stereosystem.cpp:317-320
//   loadExtrinisic / loadIntrinsic / saveExtrinsic / saveIntrinsic
//                                                    src/Stereosystem.cpp:326-446
// New: RawDisparityStream, the loop of trgt/liveDisparity.cpp:82-101 from the raw
// pair to the disparity map as a device pipeline (mvsv_stream_create_raw).
// What the reference gets from its two mvIMPACT cameras (image size, binning
// mode, the raw pair of getImagepair) is given here at construction / passed
// in: getRectifiedImagepair rectifies the raw pair the Stereopair holds, in
// place, like the reference does after Stereosystem::getImagepair filled it.
// Calibration (cv::stereoCalibrate) stays out of scope.
// Compute: the remaps and the resize run in HIP kernels (mvsv_rectify_pair,
// mvsv_undistort_pair, mvsv_resize, include/mvsv.h); stereoRectify and the
// undistort maps are host restatements (mvsv_stereo_rectify,
// mvsv_init_undistort_rectify_map, mvsv_undistort_maps).  LOG(INFO) / LOG(ERROR) lines of the
// reference go to stderr with the same mTag prefix.
#ifndef MVSV_STEREOSYSTEM_HPP
#define MVSV_STEREOSYSTEM_HPP

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "mvsv.h"
#include "mvsv_detection.hpp"
#include "mvsv_disparity.hpp"

namespace mvsv {

// The small CV_64F / CV_32F matrices of the calibration state (cv::Mat subset:
// rows x cols doubles, the element type char of the file, empty = 0 x 0).
struct Matd {
    int rows = 0, cols = 0;
    char dt = 'u';
    std::vector<double> v;

    Matd() = default;
    Matd(int r, int c, char t = 'd') : rows(r), cols(c), dt(t), v((size_t)r * c, 0.0) {}
    bool empty() const { return rows == 0 || cols == 0; }
    double& at(int r, int c) { return v[(size_t)r * cols + c]; }
    double at(int r, int c) const { return v[(size_t)r * cols + c]; }
    const double* data() const { return v.data(); }
    static Matd from(const mvsv_mat& m)
    {
        Matd o(m.rows, m.cols, m.dt ? m.dt : 'u');
        for (int i = 0; i < m.rows * m.cols; i++) o.v[i] = m.data[i];
        return o;
    }
    mvsv_mat to() const
    {
        mvsv_mat m{};
        m.rows = rows;
        m.cols = cols;
        m.dt = empty() ? 'u' : dt;
        for (size_t i = 0; i < v.size() && i < MVSV_MAT_MAX; i++) m.data[i] = v[i];
        return m;
    }
    void copyTo(Matd& o) const { o = *this; }
};

class Stereosystem {
public:
    // width x height: the cameras' image size (halved by binning, like
    // Camera::getImageWidth / getImageHeight report it); binning: both cameras
    // in binning mode (the intrinsics are halved while the rectification is
    // initialised, src/Stereosystem.cpp:202-206, 232-236)
    Stereosystem(int width, int height, bool binning = false)
        : mWidth(width), mHeight(height), mBinning(binning), mTag("STEREOSYSTEM\t")
    {
        log_info("Stereosystem created\n");
    }
    ~Stereosystem() { log_info("Stereosystem destroyed\n"); }

    // --- getters (src/Stereosystem.cpp:47-80) --------------------------------
    void getFundamentalMatrix(Matd& fundamental) const { mF.copyTo(fundamental); }
    void getTranslationMatrix(Matd& translation) const { mT.copyTo(translation); }
    double getBaseline() const
    {
        return std::sqrt(std::pow(mT.at(0, 0), 2) + std::pow(mT.at(1, 0), 2) + std::pow(mT.at(2, 0), 2));
    }
    Matd getRotationMatrix() const { return mR; }
    Matd getQMatrix() const { return mQ; }
    std::vector<Matd> getNewKMats() const { return {mP0, mP1}; }

    // cv::undistort of the raw pair in sip (mWidth x mHeight CV_8UC1) with each
    // camera's matrix and distortion coefficients, written back into sip
    // (src/Stereosystem.cpp:179-191).  The fixed-point maps are built once and stay
    // on the device, in the calling thread's context, as long as the calibration
    // this instance passes does not change (mvsv_undistort_pair): loadIntrinsic with
    // other values replaces them.  An empty distCoeffs matrix means no distortion.
    bool getUndistortedImagepair(Stereopair& sip)
    {
        Mat& L = sip.mLeft;
        Mat& R = sip.mRight;
        if (mIntrinsicLeft.rows != 3 || mIntrinsicRight.rows != 3 || L.empty() || R.empty() ||
            L.type != MAT_8UC1 || R.type != MAT_8UC1 || L.cols != mWidth || L.rows != mHeight ||
            R.cols != mWidth || R.rows != mHeight)
            return false;
        mvsv_ctx* c = thread_context();
        check(mvsv_undistort_pair(c, L.data, L.step, R.data, R.step, mWidth, mHeight, mIntrinsicLeft.data(),
                                  mDistCoeffsLeft.empty() ? nullptr : mDistCoeffsLeft.data(),
                                  (int)mDistCoeffsLeft.v.size(), mIntrinsicRight.data(),
                                  mDistCoeffsRight.empty() ? nullptr : mDistCoeffsRight.data(),
                                  (int)mDistCoeffsRight.v.size(), L.data, L.step, R.data, R.step),
              c);
        return true;
    }

    // --- rectification (src/Stereosystem.cpp:193-320) --------------------------
    bool initRectification()
    {
        log_info("Called initRectifiaction()\n");
        if (mIntrinsicLeft.rows != 3 || mIntrinsicRight.rows != 3 || mR.rows != 3 || mT.empty()) {
            log_error("Unable to init rectification\n");
            return false;
        }
        Matd KL = mIntrinsicLeft, KR = mIntrinsicRight;
        if (mBinning)
            for (int i = 0; i < 9; i++) {
                KL.v[i] /= 2;
                KR.v[i] /= 2;
            }
        Matd R0(3, 3), R1(3, 3), P0(3, 4), P1(3, 4), Q(4, 4);
        mvsv_rect roi0{}, roi1{};
        if (mvsv_stereo_rectify(KL.data(), mDistCoeffsLeft.empty() ? nullptr : mDistCoeffsLeft.data(),
                                (int)mDistCoeffsLeft.v.size(), KR.data(),
                                mDistCoeffsRight.empty() ? nullptr : mDistCoeffsRight.data(),
                                (int)mDistCoeffsRight.v.size(), mWidth, mHeight, mR.data(), mT.data(),
                                MVSV_CALIB_ZERO_DISPARITY, 0.0, R0.v.data(), R1.v.data(), P0.v.data(),
                                P1.v.data(), Q.v.data(), &roi0, &roi1) != MVSV_OK) {
            log_error("Unable to init rectification\n");
            return false;
        }
        mR0 = R0;
        mR1 = R1;
        mP0 = P0;
        mP1 = P1;
        mQ = Q;
        mValidROI[0] = roi0;
        mValidROI[1] = roi1;
        const size_t px = (size_t)mWidth * mHeight;
        for (int c = 0; c < 2; c++) {
            mMap1[c].assign(px, 0.f);
            mMap2[c].assign(px, 0.f);
            const Matd& K = c ? KR : KL;
            const Matd& D = c ? mDistCoeffsRight : mDistCoeffsLeft;
            const Matd& R = c ? R1 : R0;
            const Matd& P = c ? P1 : P0;
            double P3[9];
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) P3[r * 3 + k] = P.at(r, k);
            if (mvsv_init_undistort_rectify_map(K.data(), D.empty() ? nullptr : D.data(), (int)D.v.size(),
                                                R.data(), P3, mWidth, mHeight, mMap1[c].data(),
                                                mMap2[c].data(), mWidth) != MVSV_OK) {
                log_error("Unable to init rectification\n");
                return false;
            }
        }
        // mDisplayROI = mValidROI[0] & mValidROI[1]
        mDisplayROI = {std::max(roi0.x0, roi1.x0), std::max(roi0.y0, roi1.y0), std::min(roi0.x1, roi1.x1),
                       std::min(roi0.y1, roi1.y1)};
        if (mDisplayROI.x1 <= mDisplayROI.x0 || mDisplayROI.y1 <= mDisplayROI.y0) mDisplayROI = {0, 0, 0, 0};
        log_info("Rectification successfully initialized! [" + std::to_string(mDisplayROI.x1 - mDisplayROI.x0) +
                 " x " + std::to_string(mDisplayROI.y1 - mDisplayROI.y0) + " from (" +
                 std::to_string(mDisplayROI.x0) + ", " + std::to_string(mDisplayROI.y0) + ")]\n");
        mIsInit = true;
        return true;
    }

    // remap the raw pair in sip (mWidth x mHeight CV_8UC1) and crop it to the
    // display ROI
    bool getRectifiedImagepair(Stereopair& sip)
    {
        if (!mIsInit && !initRectification()) return false;
        return rectify(sip);
    }

    // ... and resize the crop by factor -- only when the rectification was
    // already initialised: the reference's initialising call returns the
    // unresized crop (src/Stereosystem.cpp:303-312)
    bool getRectifiedImagepair(Stereopair& sip, float factor)
    {
        if (mIsInit) {
            if (!rectify(sip)) return false;
            return resize_pair(sip, factor);
        }
        if (!initRectification()) return false;
        return rectify(sip);
    }

    void resetRectification() { mIsInit = false; }

    // --- load / save (src/Stereosystem.cpp:326-446) ---------------------------
    bool loadExtrinisic(std::string const& file)  // sic: the reference's spelling
    {
        mvsv_extrinsics v;
        const int rc = mvsv_load_extrinsic(file.c_str(), &v);
        if (rc == MVSV_E_PARSE) {
            log_error("Node in " + file + "is empty.\n");
            return false;
        }
        if (rc < 0) {
            log_error("Unable to open extrinsic file: " + file + "\n");
            return false;
        }
        mR = Matd::from(v.R);
        mT = Matd::from(v.T);
        mE = Matd::from(v.E);
        mF = Matd::from(v.F);
        log_info("Successfully loaded Extrinsics.\n");
        return true;
    }
    bool loadIntrinsic(std::string const& file)
    {
        mvsv_intrinsics v;
        const int rc = mvsv_load_intrinsic(file.c_str(), &v);
        if (rc == MVSV_E_PARSE) {
            log_error("Node in " + file + " is empty.\n");
            return false;
        }
        if (rc < 0) {
            log_error("Unable to open intrinsic file: " + file + "\n");
            return false;
        }
        mIntrinsicLeft = Matd::from(v.camera_matrix_left);
        mIntrinsicRight = Matd::from(v.camera_matrix_right);
        mDistCoeffsLeft = Matd::from(v.dist_coeffs_left);
        mDistCoeffsRight = Matd::from(v.dist_coeffs_right);
        log_info("Successfully loaded Intrinsics.\n");
        return true;
    }
    bool saveExtrinsic(std::string const& file)
    {
        mvsv_extrinsics v{mR.to(), mT.to(), mE.to(), mF.to()};
        if (mvsv_save_extrinsic(file.c_str(), &v) < 0) {
            log_error("Unable to open " + file + " for saving.\n");
            return false;
        }
        log_info("Successfully saved Extrinsics to " + file + "\n");
        return true;
    }
    bool saveIntrinsic(std::string const& file)
    {
        mvsv_intrinsics v{mIntrinsicLeft.to(),  mIntrinsicRight.to(), mDistCoeffsLeft.to(),
                          mDistCoeffsRight.to(), mP0.to(),           mP1.to(),
                          mQ.to()};
        if (mvsv_save_intrinsic(file.c_str(), &v) < 0) {
            log_error("Unable to open " + file + " for saving.\n");
            return false;
        }
        log_info("Successfully saved Intrinsics to " + file + "\n");
        return true;
    }

    // the state the reference keeps private, readable for tests / tools
    int width() const { return mWidth; }
    int height() const { return mHeight; }
    bool isInit() const { return mIsInit; }
    const mvsv_rect& displayROI() const { return mDisplayROI; }
    const std::vector<float>& map1(int c) const { return mMap1[c]; }
    const std::vector<float>& map2(int c) const { return mMap2[c]; }

private:
    void log_info(const std::string& m) const { std::fprintf(stderr, "%s%s", mTag.c_str(), m.c_str()); }
    void log_error(const std::string& m) const { std::fprintf(stderr, "%s%s", mTag.c_str(), m.c_str()); }

    bool rectify(Stereopair& sip)
    {
        const Mat& L = sip.mLeft;
        const Mat& R = sip.mRight;
        if (L.empty() || R.empty() || L.type != MAT_8UC1 || R.type != MAT_8UC1 || L.cols != mWidth ||
            L.rows != mHeight || R.cols != mWidth || R.rows != mHeight)
            return false;
        const int cw = mDisplayROI.x1 - mDisplayROI.x0, ch = mDisplayROI.y1 - mDisplayROI.y0;
        if (cw <= 0 || ch <= 0) return false;
        Mat oL(ch, cw, MAT_8UC1), oR(ch, cw, MAT_8UC1);
        const float* maps[4] = {mMap1[0].data(), mMap2[0].data(), mMap1[1].data(), mMap2[1].data()};
        mvsv_ctx* c = thread_context();
        check(mvsv_rectify_pair(c, L.data, L.step, R.data, R.step, mWidth, mHeight, maps, &mDisplayROI,
                                oL.data, oL.step, oR.data, oR.step),
              c);
        sip.mLeft = oL;
        sip.mRight = oR;
        return true;
    }
    bool resize_pair(Stereopair& sip, float factor)
    {
        Mat* im[2] = {&sip.mLeft, &sip.mRight};
        mvsv_ctx* c = thread_context();
        for (Mat* m : im) {
            int dw = 0, dh = 0;
            if (mvsv_resize_size(m->cols, m->rows, factor, factor, &dw, &dh) != MVSV_OK) return false;
            Mat o(dh, dw, MAT_8UC1);
            check(mvsv_resize(c, m->data, m->step, m->cols, m->rows, factor, factor, o.data, o.step), c);
            *m = o;
        }
        return true;
    }

    int mWidth, mHeight;
    bool mBinning;
    Matd mR, mT, mE, mF;
    bool mIsInit = false;
    std::vector<float> mMap1[2], mMap2[2];
    Matd mR0, mR1, mP0, mP1, mQ;
    mvsv_rect mValidROI[2] = {};
    mvsv_rect mDisplayROI = {};
    Matd mIntrinsicLeft, mIntrinsicRight, mDistCoeffsLeft, mDistCoeffsRight;
    std::string mTag;
};

// The camera loop of trgt/liveDisparity.cpp:82-101 (getImagepair,
// getRectifiedImagepair[, factor], Disparity::sgbm) as a pipelined stream on the
// device (mvsv_stream_create_raw): push_raw(raw pair) / pop(disparity).  Opened
// from a Stereosystem that has run initRectification(); its maps are converted
// and uploaded once, here.  Every frame is resized when a factor is given (the
// reference's unresized initialising call has no counterpart).  Uses the calling
// thread's context: create, use and destroy it on one thread.
class RawDisparityStream {
public:
    RawDisparityStream(const Stereosystem& s, const StereoSGBM& matcher, float factor = 0.f, int depth = 3,
                       const mvsv_rect* grid_roi = nullptr, bool keep_rectified = false, int batch = 1,
                       int inflight = 1)
        : mRawW(s.width()), mRawH(s.height()), mKeep(keep_rectified)
    {
        open(s, &matcher.params(), nullptr, factor, depth, grid_roi, batch, inflight);
    }
    // the same loop with StereoBM as the matcher (mvsv_stream_create_raw_bm)
    RawDisparityStream(const Stereosystem& s, const StereoBM& matcher, float factor = 0.f, int depth = 3,
                       const mvsv_rect* grid_roi = nullptr, bool keep_rectified = false, int batch = 1,
                       int inflight = 1)
        : mRawW(s.width()), mRawH(s.height()), mKeep(keep_rectified)
    {
        open(s, nullptr, &matcher.p, factor, depth, grid_roi, batch, inflight);
    }
    ~RawDisparityStream() { mvsv_stream_destroy(mStream); }
    RawDisparityStream(const RawDisparityStream&) = delete;
    RawDisparityStream& operator=(const RawDisparityStream&) = delete;

    int width() const { return mW; }
    int height() const { return mH; }
    int pending() const { return mvsv_stream_pending(mStream); }
    void set_params(const StereoSGBM& matcher) { check(mvsv_stream_set_params(mStream, &matcher.params()), mCtx); }
    void set_params(const StereoBM& matcher) { check(mvsv_stream_set_bm_params(mStream, &matcher.p), mCtx); }
    int matcher() const { return mvsv_stream_matcher(mStream); }

private:
    // one of sgbm / bm is given
    void open(const Stereosystem& s, const mvsv_sgbm_params* sgbm, const mvsv_bm_params* bm, float factor, int depth,
              const mvsv_rect* grid_roi, int batch, int inflight)
    {
        if (!s.isInit()) throw Error(MVSV_E_INVALID_ARG, "RawDisparityStream: initRectification() has not run");
        mCtx = thread_context();
        mvsv_rectification r{};
        r.raw_width = mRawW;
        r.raw_height = mRawH;
        r.maps[0] = s.map1(0).data();
        r.maps[1] = s.map2(0).data();
        r.maps[2] = s.map1(1).data();
        r.maps[3] = s.map2(1).data();
        r.map_stride = (size_t)mRawW;
        r.roi = s.displayROI();
        r.factor = factor;
        r.keep_rectified = mKeep ? 1 : 0;
        check(sgbm ? mvsv_stream_create_raw(mCtx, &r, sgbm, depth, grid_roi, &mStream)
                   : mvsv_stream_create_raw_bm(mCtx, &r, bm, depth, grid_roi, &mStream),
              mCtx);
        int rc = mvsv_stream_size(mStream, &mW, &mH);
        if (rc == MVSV_OK && batch != 1) rc = mvsv_stream_set_batch(mStream, batch);
        if (rc == MVSV_OK && inflight != 1) rc = mvsv_stream_set_inflight(mStream, inflight);
        if (rc != MVSV_OK) {
            mvsv_stream_destroy(mStream);
            check(rc, mCtx);
        }
    }

public:
    void push_raw(const Mat& left, const Mat& right)
    {
        check_pair(left, right);
        if (left.cols != mRawW || left.rows != mRawH)
            throw Error(MVSV_E_INVALID_ARG, "RawDisparityStream: pair of the raw frame's size expected");
        check(mvsv_stream_push_raw(mStream, left.data, left.step, right.data, right.step), mCtx);
    }
    // the oldest frame's map (CV_16S, disparity * 16); means: 81 floats of the
    // grid_roi's 9x9 grid, or nullptr; rectified: the frame's rectified pair
    // (needs keep_rectified), or nullptr
    void pop(Mat& disparity, float* means = nullptr, Stereopair* rectified = nullptr)
    {
        if (rectified && !mKeep) throw Error(MVSV_E_INVALID_ARG, "RawDisparityStream: opened without keep_rectified");
        disparity.create(mH, mW, MAT_16SC1);
        if (rectified) {
            rectified->mLeft.create(mH, mW, MAT_8UC1);
            rectified->mRight.create(mH, mW, MAT_8UC1);
        }
        check(mvsv_stream_pop_pair(mStream, reinterpret_cast<int16_t*>(disparity.data), disparity.step / 2, means,
                                   rectified ? rectified->mLeft.data : nullptr, rectified ? rectified->mLeft.step : 0,
                                   rectified ? rectified->mRight.data : nullptr,
                                   rectified ? rectified->mRight.step : 0),
              mCtx);
    }
    // ---- device ends, as on DisparityStream (mvsv.h "device ends of a stream") ----
    // n raw pairs of device memory (strides in bytes) as n pushes, ordered against hip_stream by events
    void pushDevice(int n, const uint8_t* left, size_t left_step, size_t left_frame_step, const uint8_t* right,
                    size_t right_step, size_t right_frame_step, void* hip_stream = nullptr)
    {
        check(mvsv_stream_push_raw_device(mStream, n, left, left_step, left_frame_step, right, right_step,
                                          right_frame_step, hip_stream), mCtx);
    }
    void popDevice(int16_t* out_dev, size_t out_stride, float* means = nullptr, void* hip_stream = nullptr)
    {
        check(mvsv_stream_pop_device(mStream, out_dev, out_stride, means, hip_stream), mCtx);
    }
    const int16_t* frontMapDevice(float* means = nullptr)
    {
        const int16_t* map = nullptr;
        check(mvsv_stream_front_map_device(mStream, &map, means), mCtx);
        return map;
    }
    void hostOutputs(int mask) { check(mvsv_stream_set_host_outputs(mStream, mask), mCtx); }
    void fence(void* hip_stream = nullptr) { check(mvsv_stream_fence(mStream, hip_stream), mCtx); }
    // the lattice detector on every frame, as on DisparityStream
    void enableSamplepoints(const SamplepointDetection& d, const Rect* roi = nullptr, int max_hits = 0)
    {
        mLattice = stream_enable_samplepoints(mCtx, mStream, mW, mH, d, roi, max_hits);
    }
    void disableSamplepoints() { check(mvsv_stream_disable_samplepoints(mStream), mCtx); }
    void frontSamples(SampleFrame& out) { stream_front_samples(mCtx, mStream, mLattice, out); }
    // the 8-bit display map on every frame, as on DisparityStream
    void enableDisplay(const Rect* roi = nullptr, double alpha = 0, double beta = 255)
    {
        mDisplay = stream_enable_display(mCtx, mStream, mW, mH, roi, alpha, beta);
    }
    void disableDisplay()
    {
        check(mvsv_stream_disable_display(mStream), mCtx);
        mDisplay = {};
    }
    void frontDisplay(Mat& out, int16_t* minmax = nullptr)
    {
        stream_front_display(mCtx, mStream, mDisplay, out, minmax);
    }
    // the detection view on every frame, as on DisparityStream
    void enableView(int layers, const Rect* roi = nullptr, std::pair<float, float> meanRange = {0.0f, 0.0f},
                    int pointRadius = 3, double alpha = 0, double beta = 255)
    {
        mView = stream_enable_view(mCtx, mStream, mW, mH, layers, roi, meanRange, pointRadius, alpha, beta);
    }
    void disableView()
    {
        check(mvsv_stream_disable_view(mStream), mCtx);
        mView = {};
    }
    void frontView(Mat& out, int16_t* minmax = nullptr) { stream_front_view(mCtx, mStream, mView, out, minmax); }
    // the focus measure of every pushed raw pair (what trgt/liveView.cpp prints),
    // as on DisparityStream; the view areas lie in the raw frame
    void enableSharpness(const Rect* roi_left = nullptr, const Rect* roi_right = nullptr)
    {
        stream_enable_sharpness(mCtx, mStream, roi_left, roi_right);
    }
    void disableSharpness() { check(mvsv_stream_disable_sharpness(mStream), mCtx); }
    Sharpness frontSharpness() { return stream_front_sharpness(mCtx, mStream); }
    // the point cloud on every frame, as on DisparityStream
    void enableCloud(const QMatrix& Q, const Rect* roi = nullptr, int max_points = 0)
    {
        mCloud = stream_enable_cloud(mCtx, mStream, mW, mH, Q, roi, max_points);
    }
    void disableCloud()
    {
        check(mvsv_stream_disable_cloud(mStream), mCtx);
        mCloud = 0;
    }
    int frontCloud(std::vector<mvsv_cloud_point>& out, int32_t* minmax = nullptr)
    {
        return stream_front_cloud(mCtx, mStream, mCloud, out, minmax);
    }

private:
    mvsv_ctx* mCtx = nullptr;
    mvsv_stream* mStream = nullptr;
    int mRawW, mRawH, mW = 0, mH = 0;
    SampleLayout mLattice;
    DisplaySize mDisplay, mView;
    int mCloud = 0;
    bool mKeep;
};

}  // namespace mvsv

#endif  // MVSV_STEREOSYSTEM_HPP
