// mvsv_detection.hpp — C++ mirror of the reference's code around the disparity
// path, on libmvsv:
//
//   struct dMapValues, namespace Utility        inc/utility.h:50-82, src/utility.cpp:176-303
//   class ply (MODE PLAIN / WITH_COLOR / ...)   inc/ply.h, src/ply.cpp:37-133
//   struct Subimage                             inc/Subimage.h:17-47
//   class MeanDisparityDetection                inc/MeanDisparityDetection.h,
//                                               src/MeanDisparityDetection.cpp:71-266
//   struct Samplepoint                          inc/Samplepoint.h:17-40
//   class SamplepointDetection                  inc/SamplepointDetection.h,
//                                               src/SamplePointDetection.cpp:29-178
//   createDMapROIS                              trgt/mean_test.cpp:80-106
//   mvsv::DisparityStream                       replaces the worker thread +
//                                               condition variable of
//                                               trgt/mean_test.cpp:61-70,258-318
//
// Per-pixel work (the 9x9 tile means, reprojection) runs in the HIP kernels
// behind include/mvsv.h; the 81-element decisions stay on the host in the
// reference's order.  Matrices are the reference's CV_32F 4x4 Q (16 floats,
// row-major).
#ifndef MVSV_DETECTION_HPP
#define MVSV_DETECTION_HPP

#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "mvsv_disparity.hpp"

namespace mvsv {

using QMatrix = std::array<float, 16>;

struct dMapValues {  // inc/utility.h:50-55
    float dValue = 0, image_x = 0, image_y = 0;
};

struct Point {
    int x = 0, y = 0;
};

namespace Utility {

inline std::array<float, 4> calcCoordinate(dMapValues v, const QMatrix& Q)
{
    std::array<float, 4> c;
    mvsv_calc_coordinate(v.image_x, v.image_y, v.dValue, Q.data(), c.data());
    return c;
}
inline float calcDistance(dMapValues v, const QMatrix& Q, int /*binning*/)
{
    return mvsv_calc_distance(v.image_x, v.image_y, v.dValue, Q.data());
}
inline dMapValues calcDMapValues(const std::array<float, 3>& c, const QMatrix& Q)
{
    dMapValues v;
    mvsv_calc_dmap_values(c.data(), Q.data(), &v.image_x, &v.image_y, &v.dValue);
    return v;
}
// src/utility.cpp:242-262 (reprojection on the device, PLY WITH_COLOR)
inline void dmap2pcl(const std::string& filename, const Mat& dMap, const QMatrix& Q)
{
    if (dMap.type != MAT_16SC1) throw Error(MVSV_E_INVALID_ARG, "dmap2pcl: CV_16S map expected");
    mvsv_ctx* c = thread_context();
    check(mvsv_dmap2pcl(c, filename.c_str(), reinterpret_cast<const int16_t*>(dMap.data),
                        dMap.step / 2, dMap.cols, dMap.rows, Q.data()),
          c);
}
// src/utility.cpp:265-285 on the host: integer mean of the values > 1
inline float calcMeanDisparity(const Mat& m)
{
    int total = 0, n = 0;
    for (int r = 0; r < m.rows; r++)
        for (int c = 0; c < m.cols; c++) {
            short v = m.ptr<int16_t>(r)[c];
            if (v > 1) {
                total += v;
                ++n;
            }
        }
    if (total == 0 || n == 0) return 0.0f;
    return (float)(total / (n < 0 ? -n : n));
}
// cv::normalize(dMap, out, alpha, beta, cv::NORM_MINMAX, CV_8U) on the device --
// the display step of every loop of the reference (trgt/liveDisparity.cpp:92; the
// detector loops pass the work ROI dMap(roi), trgt/mean_test.cpp:307).
// minmax: where given, the (smin, smax) the map was normalised with.
inline void normalize(const Mat& dMap, Mat& out, double alpha = 0, double beta = 255, int16_t* minmax = nullptr)
{
    if (dMap.type != MAT_16SC1 || dMap.empty()) throw Error(MVSV_E_INVALID_ARG, "normalize: CV_16S map expected");
    out.create(dMap.rows, dMap.cols, MAT_8UC1);
    mvsv_ctx* c = thread_context();
    check(mvsv_normalize_minmax(c, reinterpret_cast<const int16_t*>(dMap.data), dMap.step / 2, dMap.cols, dMap.rows,
                                alpha, beta, out.data, out.step, minmax),
          c);
}
// What trgt/disparityTest.cpp:201-211 does to an image ahead of the matchers, on the
// device (mvsv_prepare_gray): with halve, cv::resize(.., 0.5, 0.5, INTER_AREA) of the
// CV_8UC3 image, then cv::cvtColor(BGR2GRAY) in the arithmetic of `variant`
// (MVSV_GRAY_Q14 / MVSV_GRAY_Q15).  out: CV_8UC1 of mvsv_prepare_size.
inline void prepareGray(const Mat& bgr, Mat& out, bool halve = true, int variant = MVSV_GRAY_Q14)
{
    if (bgr.type != MAT_8UC3 || bgr.empty()) throw Error(MVSV_E_INVALID_ARG, "prepareGray: CV_8UC3 image expected");
    int w = 0, h = 0;
    if (mvsv_prepare_size(bgr.cols, bgr.rows, halve ? 1 : 0, &w, &h) < 0)
        throw Error(MVSV_E_INVALID_ARG, "prepareGray: the image halves to nothing");
    out.create(h, w, MAT_8UC1);
    mvsv_ctx* c = thread_context();
    check(mvsv_prepare_gray(c, bgr.data, bgr.step, bgr.cols, bgr.rows, halve ? 1 : 0, variant, out.data, out.step), c);
}
// The frame the detection programs show (trgt/demo.cpp:280-298): normalize,
// cv::cvtColor(GRAY2BGR), View's grids and drawFoundObstacles in one device pass
// (mvsv_view).  out: CV_8UC3, B, G, R.  layers: MVSV_VIEW_* bits; means81 and
// meanRange (MeanDisparityDetection's means and mRangeDisparity) for
// MVSV_VIEW_FOUND_TILES, values and sampleRange (SamplepointDetection's) for
// MVSV_VIEW_FOUND_POINTS.
inline void detectionView(const Mat& dMap, Mat& out, int layers, const float* means81 = nullptr,
                          std::pair<float, float> meanRange = {0.0f, 0.0f}, const float* values = nullptr,
                          std::pair<float, float> sampleRange = {0.0f, 0.0f}, int pointRadius = 3, double alpha = 0,
                          double beta = 255, int16_t* minmax = nullptr)
{
    if (dMap.type != MAT_16SC1 || dMap.empty()) throw Error(MVSV_E_INVALID_ARG, "detectionView: CV_16S map expected");
    out.create(dMap.rows, dMap.cols, MAT_8UC3);
    const mvsv_view_spec spec{layers,         alpha,  beta,          means81,      meanRange.first, meanRange.second,
                              values, sampleRange.first, sampleRange.second, pointRadius};
    mvsv_ctx* c = thread_context();
    check(mvsv_view(c, reinterpret_cast<const int16_t*>(dMap.data), dMap.step / 2, dMap.cols, dMap.rows, &spec,
                    out.data, out.step, minmax),
          c);
}
// src/utility.cpp:163-174: cv::mean(|Lx| + |Ly|) of the two cv::sepFilter2D responses,
// on the device (mvsv_sharpness).  The reference passes a view, checkSharpness(
// s.mLeft(viewArea)) (trgt/liveView.cpp:107-108), and OpenCV's filter engine takes
// the view's 1-pixel halo from the parent image; an mvsv::Mat view does not know its
// parent, so the parent and the view area are passed here.  sum4: where given, the
// exact integer sum S4 (include/mvsv.h) behind the value.
inline double checkSharpness(const Mat& image, const Rect& viewArea, int64_t* sum4 = nullptr)
{
    if (image.type != MAT_8UC1 || image.empty()) throw Error(MVSV_E_INVALID_ARG, "checkSharpness: CV_8U image expected");
    const mvsv_rect r{viewArea.x, viewArea.y, viewArea.x + viewArea.width, viewArea.y + viewArea.height};
    double value = 0;
    mvsv_ctx* c = thread_context();
    check(mvsv_sharpness(c, image.data, image.step, image.cols, image.rows, &r, &value, sum4), c);
    return value;
}
inline double checkSharpness(const Mat& image) { return checkSharpness(image, Rect{0, 0, image.cols, image.rows}); }
// the loop of dmap2pcl without the file: the pixels with v > 0 of dMap in raster
// order as (x, y, z, grey) records, compacted on the device (mvsv_point_cloud).
// max_points <= 0: every valid pixel.  Returns the number of valid pixels, which may
// exceed max_points; out holds the first min(count, max_points).  minmax: where
// given, the (min, max) over the valid values.
inline int pointCloud(const Mat& dMap, const QMatrix& Q, std::vector<mvsv_cloud_point>& out, int max_points = 0,
                      int32_t* minmax = nullptr)
{
    if (dMap.type != MAT_16SC1 || dMap.empty()) throw Error(MVSV_E_INVALID_ARG, "pointCloud: CV_16S map expected");
    const size_t px = (size_t)dMap.rows * dMap.cols;
    out.resize(max_points <= 0 ? px : std::min((size_t)max_points, px));
    int count = 0;
    mvsv_ctx* c = thread_context();
    check(mvsv_point_cloud(c, reinterpret_cast<const int16_t*>(dMap.data), dMap.step / 2, dMap.cols, dMap.rows,
                           Q.data(), out.data(), (int)out.size(), &count, minmax),
          c);
    out.resize(std::min((size_t)std::max(count, 0), out.size()));
    return count;
}

}  // namespace Utility

// inc/view.h, src/view.cpp: the two grids painted over a CV_8UC3 image on the host
// (mvsv_view_draw: the device view's rules, no device needed).  binning is unused,
// as in the reference.
namespace View {

inline void draw_layer(Mat& stream, int layer)
{
    if (stream.type != MAT_8UC3 || stream.empty()) throw Error(MVSV_E_INVALID_ARG, "View: CV_8UC3 image expected");
    const mvsv_view_spec spec{layer, 0, 255, nullptr, 0, 0, nullptr, 0, 0, 3};
    check(mvsv_view_draw(stream.data, stream.step, stream.cols, stream.rows, &spec), nullptr);
}
inline void drawObstacleGrid(Mat& stream, int binning = 0)
{
    (void)binning;
    draw_layer(stream, MVSV_VIEW_OBSTACLE_GRID);
}
inline void drawSubimageGrid(Mat& stream, int binning = 0)
{
    (void)binning;
    draw_layer(stream, MVSV_VIEW_SUBIMAGE_GRID);
}

}  // namespace View

class ply {  // inc/ply.h
public:
    enum MODE { PLAIN = MVSV_PLY_PLAIN, WITH_COLOR = MVSV_PLY_WITH_COLOR,
                WITH_COLOR_SHADING = MVSV_PLY_WITH_COLOR_SHADING };
    ply() = default;
    ply(std::string author, std::string object) : mAuthor(std::move(author)), mObjectName(std::move(object)) {}
    ply(std::string author, std::string object, const Mat& dmap)
        : mAuthor(std::move(author)), mObjectName(std::move(object)), mDMap(dmap) {}
    bool write(const std::string& filename, const std::vector<std::array<float, 4>>& to_write, int mode)
    {
        if (mode != PLAIN && mDMap.empty()) return false;
        int rc = mvsv_write_ply(filename.c_str(), mAuthor.c_str(), mObjectName.c_str(),
                                to_write.empty() ? nullptr : to_write[0].data(), to_write.size(), 4,
                                mode, mDMap.empty() ? nullptr : reinterpret_cast<const int16_t*>(mDMap.data),
                                mDMap.step / 2, mDMap.cols, mDMap.rows);
        return rc == MVSV_OK;
    }

private:
    std::string mAuthor, mObjectName;
    Mat mDMap;
};

struct Subimage {  // inc/Subimage.h:17-47
    Subimage() = default;
    Subimage(Point tl_, Point br_) : tl(tl_), br(br_)
    {
        int tx = br.x - tl.x, ty = br.y - tl.y;
        roi_center = {tl.x + tx / 2, tl.y + ty / 2};
    }
    void calculateSubimageValue(const Mat& dMap)
    {
        value = Utility::calcMeanDisparity(dMap(Rect{tl.x, tl.y, br.x - tl.x, br.y - tl.y}));
    }
    Point tl, br, roi_center;
    float value = 0;
};

// trgt/mean_test.cpp:80-106 (the unbinned / binned work ROIs of the disparity map)
inline void createDMapROIS(int rows, int cols, int numDisp, Rect& roi_u, Rect& roi_b)
{
    int pixelShift = numDisp / 2;
    if (pixelShift % 2 == 1) {
        pixelShift = pixelShift + 1;
        if ((cols - pixelShift) % 8 != 0) pixelShift = pixelShift + (cols - pixelShift % 8);
    }
    roi_u = Rect{pixelShift, 0, cols - pixelShift, rows};
    roi_b = Rect{pixelShift / 2, 0, cols / 2 - pixelShift / 2, rows / 2};
}

class MeanDisparityDetection {  // src/MeanDisparityDetection.cpp
public:
    enum MODE { MEAN_DISTANCE, MEAN_VALUE };

    explicit MeanDisparityDetection(std::string pcl_dir = "pcl/subimage_detection")
        : mPclDir(std::move(pcl_dir))
    {
        for (int k = 0; k < 9; ++k) mPositions[k] = "TOP LEFT - " + std::to_string(k);
        mPositions[9] = "TOP - 0";  // the reference's table skips key 10
        for (int k = 1; k < 9; ++k) mPositions[10 + k] = "TOP - " + std::to_string(k);
        const char* groups[] = {"TOP RIGHT", "LEFT", "CENTER", "RIGHT", "BOTTOM LEFT", "BOTTOM",
                                "BOTTOM RIGHT"};
        for (int g = 0; g < 7; ++g)
            for (int k = 0; k < 9; ++k)
                mPositions[19 + 9 * g + k] = std::string(groups[g]) + " - " + std::to_string(k);
    }

    // :71-112
    void init(const Mat& reference, const QMatrix& Q, float min_distance, float max_distance)
    {
        mSubimageVec.clear();
        mQ = Q;
        int dx = reference.cols / 9, dy = reference.rows / 9;
        for (int r = 0; r < 9; ++r)
            for (int c = 0; c < 9; ++c) {
                Point tl{c * dx, r * dy}, br{c * dx + dx, r * dy + dy};
                mSubimageVec.emplace_back(tl, br);
                mFoundObstacles.emplace_back(tl, br);
            }
        dMapValues lo = Utility::calcDMapValues({0, 0, min_distance * 1000}, mQ);
        dMapValues hi = Utility::calcDMapValues({0, 0, max_distance * 1000}, mQ);
        mRangeDisparity = {lo.dValue, hi.dValue};
    }

    // :159-206; the 81 means come from the GPU (host map, or `means` from a stream pop)
    void build(const Mat& dMap, int /*binning*/, int mode, const float* means = nullptr)
    {
        mDMap = dMap;
        float m[81];
        if (!means) {
            if (dMap.type != MAT_16SC1) throw Error(MVSV_E_INVALID_ARG, "build: CV_16S map expected");
            mvsv_ctx* c = thread_context();
            check(mvsv_mean_disparity_grid(c, reinterpret_cast<const int16_t*>(dMap.data),
                                           dMap.step / 2, dMap.cols, dMap.rows, m),
                  c);
            means = m;
        }
        switch (mode) {
        case MEAN_DISTANCE:
            mDetectionMode = MEAN_DISTANCE;
            mMeanDistanceMap.clear();
            for (size_t i = 0; i < mSubimageVec.size(); ++i) {
                const Subimage& s = mSubimageVec[i];
                dMapValues v{means[i], (float)s.roi_center.x, (float)s.roi_center.y};
                mMeanDistanceMap.push_back(Utility::calcDistance(v, mQ, 0));
            }
            // falls through, as the reference's switch does
        case MEAN_VALUE:
            mDetectionMode = MEAN_VALUE;
            mMeanMap.clear();
            for (size_t i = 0; i < mSubimageVec.size(); ++i) {
                mSubimageVec[i].value = means[i];
                mMeanMap.push_back(means[i]);
            }
        }
    }

    // :211-266; returns the positions the reference prints in MEAN_DISTANCE mode
    std::vector<std::string> detectObstacles()
    {
        std::vector<std::string> printed;
        if (mDetectionMode == MEAN_DISTANCE) {
            for (size_t i = 0; i < mMeanDistanceMap.size(); ++i)
                if (mMeanDistanceMap[i] < mRange.second && mMeanDistanceMap[i] > mRange.first)
                    printed.push_back(mPositions[(int)i]);
            return printed;
        }
        if (mDetectionMode != MEAN_VALUE) return printed;
        mFoundObstacles.clear();
        std::vector<std::array<float, 4>> points;
        for (size_t i = 0; i < mMeanMap.size(); ++i) {
            if (mMeanMap[i] < mRangeDisparity.first && mMeanMap[i] > mRangeDisparity.second) {
                Subimage s = mSubimageVec[i];
                mFoundObstacles.push_back(s);
                dMapValues v{mMeanMap[i], (float)s.roi_center.x, (float)s.roi_center.y};
                points.push_back(Utility::calcCoordinate(v, mQ));
            }
        }
        if (!points.empty()) {
            ply p("Hagen Hiller", "obstacle pointcloud", mDMap);
            std::string prefix = mObstacleCounter < 10 ? "000" : (mObstacleCounter < 100 ? "00" : "0");
            p.write(mPclDir + "/pcl_" + prefix + std::to_string(mObstacleCounter) + ".ply", points,
                    ply::WITH_COLOR);
            ++mObstacleCounter;
        }
        return printed;
    }

    void setRange(float min_distance, float max_distance) { mRange = {min_distance, max_distance}; }
    std::pair<int, int> getRange() const { return {(int)mRange.first, (int)mRange.second}; }
    const std::vector<Subimage>& getSubimageVec() const { return mSubimageVec; }
    const std::vector<float>& getMeanMap() const { return mMeanMap; }
    const std::vector<float>& getMeanDistanceMap() const { return mMeanDistanceMap; }
    const std::vector<Subimage>& getFoundObstacles() const { return mFoundObstacles; }
    int getObstacleCounter() const { return mObstacleCounter; }
    std::pair<float, float> getRangeDisparity() const { return mRangeDisparity; }

private:
    std::string mPclDir;
    Mat mDMap;
    std::map<int, std::string> mPositions;
    std::vector<Subimage> mSubimageVec, mFoundObstacles;
    std::vector<float> mMeanMap, mMeanDistanceMap;
    QMatrix mQ{};
    int mDetectionMode = -1;
    int mObstacleCounter = 0;
    std::pair<float, float> mRange{0, 0}, mRangeDisparity{0, 0};
};

struct Samplepoint {  // inc/Samplepoint.h:17-40
    Samplepoint() = default;
    Samplepoint(Point center_, int radius_)
        : center(center_), radius(radius_),
          roi{center_.x - radius_, center_.y - radius_, 2 * radius_ + 1, 2 * radius_ + 1}
    {
    }
    void calculateSamplepointValue(const Mat& dMap)
    {
        if (radius > 0)
            value = Utility::calcMeanDisparity(dMap(roi));
        else
            value = dMap.ptr<int16_t>(center.y)[center.x];
    }
    Point center;
    int radius = 0;
    Rect roi{0, 0, 0, 0};
    float value = 0;
};

// A stream frame's lattice results (frontSamples of either stream class)
struct SampleFrame {
    std::vector<float> values;          // one per lattice point
    int count = 0;                      // all hits of the frame (may exceed hits.size())
    std::vector<mvsv_sample_hit> hits;  // exactly the first min(count, max_hits), index order
};

// The lattice detector: 5x5 patches every step_x x step_y pixels, in the
// reference's order (columns in the outer loop).  The values come from the GPU
// (mvsv_samplepoint_values, or a stream frame's); the decisions stay on the host
// in the reference's order, or come from the stream as hit records.
class SamplepointDetection {  // src/SamplePointDetection.cpp
public:
    static constexpr int kRadius = 2;  // :43

    explicit SamplepointDetection(std::string pcl_dir = "pcl/samplepoint_detection") : mPclDir(std::move(pcl_dir)) {}

    // :29-75
    void init(const Mat& reference, const QMatrix& Q, float min_distance, float max_distance)
    {
        mSPVec.clear();
        mQ = Q;
        mRows = reference.rows;
        mCols = reference.cols;
        int distanceX = reference.cols / 8, distanceY = reference.rows / 8;
        for (int c = 1; c < distanceX; ++c)
            for (int r = 1; r < distanceY; ++r) {
                Point center{c * (reference.cols / distanceX), r * (reference.rows / distanceY)};
                mSPVec.emplace_back(center, kRadius);
                mFoundObstacles.emplace_back(center, kRadius);  // the layout, for the visualisation
            }
        mCenterVec = {0.0f, 0.0f, 1.0f, 0.0f};
        mImageCenter = {(int)mQ[3], (int)mQ[7]};
        dMapValues lo = Utility::calcDMapValues({0, 0, min_distance * 1000}, mQ);
        dMapValues hi = Utility::calcDMapValues({0, 0, max_distance * 1000}, mQ);
        mRangeDisparity = {lo.dValue, hi.dValue};
    }

    // :117-129 (binning and mode are ignored there too); values: one float per
    // sample point where they are at hand (a stream frame's), else computed here
    void build(const Mat& dMap, int /*binning*/, int /*mode*/, const float* values = nullptr)
    {
        mDMap = dMap;
        mDistanceVec.assign(mSPVec.size(), 0.0f);
        if (values) {
            std::copy(values, values + mSPVec.size(), mDistanceVec.begin());
        } else {
            if (dMap.type != MAT_16SC1 || dMap.rows != mRows || dMap.cols != mCols)
                throw Error(MVSV_E_INVALID_ARG, "build: CV_16S map of init's size expected");
            mvsv_ctx* c = thread_context();
            check(mvsv_samplepoint_values(c, reinterpret_cast<const int16_t*>(dMap.data), dMap.step / 2, dMap.cols,
                                          dMap.rows, kRadius, mDistanceVec.data()),
                  c);
        }
        for (size_t i = 0; i < mSPVec.size(); ++i) mSPVec[i].value = mDistanceVec[i];
    }

    // :134-178
    void detectObstacles()
    {
        mFoundObstacles.clear();
        mFoundPoints.clear();
        for (size_t i = 0; i < mDistanceVec.size(); ++i) {
            if (mDistanceVec[i] < mRangeDisparity.first && mDistanceVec[i] > mRangeDisparity.second) {
                Samplepoint s = mSPVec[i];
                s.value = mDistanceVec[i];
                mFoundObstacles.push_back(s);
                dMapValues v{mDistanceVec[i], (float)s.center.x, (float)s.center.y};
                mFoundPoints.push_back(Utility::calcCoordinate(v, mQ));
            }
        }
        writeFound();
    }
    // the decisions of a stream frame (frontSamples) instead of the host's.
    // count: the number of records that hits holds -- SampleFrame::hits.size(),
    // i.e. min(the frame's hit count, the stream's max_hits), NOT SampleFrame::count
    // when the stream caps the records.  Needs build() first (the values).
    void detectObstacles(int count, const mvsv_sample_hit* hits)
    {
        if (mDistanceVec.size() != mSPVec.size())
            throw Error(MVSV_E_INVALID_ARG, "detectObstacles: build() has not run");
        if (count < 0 || (count > 0 && !hits)) throw Error(MVSV_E_INVALID_ARG, "detectObstacles: bad hit records");
        mFoundObstacles.clear();
        mFoundPoints.clear();
        for (int k = 0; k < count; ++k) {
            const mvsv_sample_hit& h = hits[k];
            if (h.index < 0 || (size_t)h.index >= mSPVec.size())
                throw Error(MVSV_E_INVALID_ARG, "detectObstacles: hit outside the lattice");
            Samplepoint s = mSPVec[h.index];
            s.value = mDistanceVec[h.index];
            mFoundObstacles.push_back(s);
            // the fourth element, which a record does not carry, from the point itself
            dMapValues v{s.value, (float)s.center.x, (float)s.center.y};
            mFoundPoints.push_back({h.x, h.y, h.z, Utility::calcCoordinate(v, mQ)[3]});
        }
        writeFound();
    }
    // the same from a frame as frontSamples filled it: the records it holds
    void detectObstacles(const SampleFrame& f) { detectObstacles((int)f.hits.size(), f.hits.data()); }

    void setRange(float min_distance, float max_distance) { mRange = {min_distance, max_distance}; }
    std::pair<int, int> getRange() const { return {(int)mRange.first, (int)mRange.second}; }
    const std::vector<Samplepoint>& getSamplepointVec() const { return mSPVec; }
    const std::array<float, 4>& getCenterPoint() const { return mCenterVec; }
    const std::vector<Samplepoint>& getFoundObstacles() const { return mFoundObstacles; }
    int getObstacleCounter() const { return mObstacleCounter; }
    std::pair<float, float> getRangeDisparity() const { return mRangeDisparity; }
    const std::vector<std::array<float, 4>>& getFoundPoints() const { return mFoundPoints; }
    const QMatrix& getQ() const { return mQ; }

private:
    void writeFound()
    {
        if (mFoundPoints.empty()) return;
        ply p("Hagen Hiller", "obstacle pointcloud", mDMap);
        std::string prefix = mObstacleCounter < 10 ? "000" : (mObstacleCounter < 100 ? "00" : "0");
        p.write(mPclDir + "/pcl_" + prefix + std::to_string(mObstacleCounter) + ".ply", mFoundPoints,
                ply::WITH_COLOR);
        ++mObstacleCounter;
    }

    std::string mPclDir;
    Mat mDMap;
    std::vector<Samplepoint> mSPVec, mFoundObstacles;
    std::vector<float> mDistanceVec;
    std::vector<std::array<float, 4>> mFoundPoints;
    std::array<float, 4> mCenterVec{0.0f, 0.0f, 1.0f, 0.0f};
    Point mImageCenter;
    QMatrix mQ{};
    int mRows = 0, mCols = 0;
    int mObstacleCounter = 0;
    std::pair<float, float> mRange{0, 0}, mRangeDisparity{0, 0};
};

// what a stream class remembers of its enabled lattice
struct SampleLayout {
    int npts = 0;  // lattice points of the roi
    int cap = 0;   // hit records a frame brings back at most (the effective max_hits)
};

// the lattice calls shared by DisparityStream and RawDisparityStream
inline SampleLayout stream_enable_samplepoints(mvsv_ctx* ctx, mvsv_stream* s, int width, int height,
                                               const SamplepointDetection& d, const Rect* roi, int max_hits)
{
    mvsv_rect r{0, 0, width, height};
    if (roi) r = {roi->x, roi->y, roi->x + roi->width, roi->y + roi->height};
    const std::pair<float, float> range = d.getRangeDisparity();
    check(mvsv_stream_enable_samplepoints(s, &r, SamplepointDetection::kRadius, d.getQ().data(), range.first,
                                          range.second, max_hits),
          ctx);
    int sx, sy, nx, ny;
    check(mvsv_samplepoint_layout(r.x1 - r.x0, r.y1 - r.y0, &sx, &sy, &nx, &ny), ctx);
    const int npts = nx * ny;
    return {npts, max_hits <= 0 ? npts : std::min(max_hits, npts)};  // as the stream sizes its records
}
inline void stream_front_samples(mvsv_ctx* ctx, mvsv_stream* s, const SampleLayout& l, SampleFrame& out)
{
    out.values.resize((size_t)l.npts);
    out.hits.resize((size_t)l.cap);
    out.count = 0;
    check(mvsv_stream_front_samples(s, out.values.data(), &out.count, out.hits.data(), l.cap), ctx);
    out.hits.resize((size_t)std::max(0, std::min(out.count, l.cap)));  // only records that were written
}

// the display calls shared by DisparityStream and RawDisparityStream: the enabled
// roi's size is what a stream class remembers
struct DisplaySize {
    int rows = 0, cols = 0;
};
inline DisplaySize stream_enable_display(mvsv_ctx* ctx, mvsv_stream* s, int width, int height, const Rect* roi,
                                         double alpha, double beta)
{
    mvsv_rect r{0, 0, width, height};
    if (roi) r = {roi->x, roi->y, roi->x + roi->width, roi->y + roi->height};
    check(mvsv_stream_enable_display(s, &r, alpha, beta), ctx);
    return {r.y1 - r.y0, r.x1 - r.x0};
}
inline void stream_front_display(mvsv_ctx* ctx, mvsv_stream* s, const DisplaySize& d, Mat& out, int16_t* minmax)
{
    if (d.rows > 0 && d.cols > 0) out.create(d.rows, d.cols, MAT_8UC1);
    check(mvsv_stream_front_display(s, d.rows > 0 ? out.data : nullptr, out.step, minmax), ctx);
}

// the detection view calls shared by DisparityStream and RawDisparityStream
inline DisplaySize stream_enable_view(mvsv_ctx* ctx, mvsv_stream* s, int width, int height, int layers, const Rect* roi,
                                      std::pair<float, float> meanRange, int pointRadius, double alpha, double beta)
{
    mvsv_rect r{0, 0, width, height};
    if (roi) r = {roi->x, roi->y, roi->x + roi->width, roi->y + roi->height};
    const mvsv_view_spec spec{layers, alpha, beta, nullptr, meanRange.first, meanRange.second, nullptr, 0, 0, pointRadius};
    check(mvsv_stream_enable_view(s, &r, &spec), ctx);
    return {r.y1 - r.y0, r.x1 - r.x0};
}
inline void stream_front_view(mvsv_ctx* ctx, mvsv_stream* s, const DisplaySize& d, Mat& out, int16_t* minmax)
{
    if (d.rows > 0 && d.cols > 0) out.create(d.rows, d.cols, MAT_8UC3);
    check(mvsv_stream_front_view(s, d.rows > 0 ? out.data : nullptr, out.step, minmax), ctx);
}

// the point cloud calls shared by DisparityStream and RawDisparityStream: the
// records kept per frame are what a stream class remembers
inline int stream_enable_cloud(mvsv_ctx* ctx, mvsv_stream* s, int width, int height, const QMatrix& Q, const Rect* roi,
                               int max_points)
{
    mvsv_rect r{0, 0, width, height};
    if (roi) r = {roi->x, roi->y, roi->x + roi->width, roi->y + roi->height};
    check(mvsv_stream_enable_cloud(s, &r, Q.data(), max_points), ctx);
    const long px = (long)(r.x1 - r.x0) * (r.y1 - r.y0);
    return (int)(max_points <= 0 ? px : std::min((long)max_points, px));
}
// the header first (the frame is waited for there), then the records that exist
inline int stream_front_cloud(mvsv_ctx* ctx, mvsv_stream* s, int cap, std::vector<mvsv_cloud_point>& out,
                              int32_t* minmax)
{
    int count = 0;
    check(mvsv_stream_front_cloud(s, nullptr, 0, &count, minmax), ctx);
    out.resize((size_t)std::max(0, std::min(count, cap)));
    if (!out.empty()) check(mvsv_stream_front_cloud(s, out.data(), (int)out.size(), nullptr, nullptr), ctx);
    return count;
}

// the focus measure calls shared by DisparityStream and RawDisparityStream
struct Sharpness {
    double left = 0, right = 0;      // Utility::checkSharpness of the pushed images
    int64_t sum4_left = 0, sum4_right = 0;
};
inline void stream_enable_sharpness(mvsv_ctx* ctx, mvsv_stream* s, const Rect* roi_left, const Rect* roi_right)
{
    mvsv_rect l{}, r{};
    if (roi_left) l = {roi_left->x, roi_left->y, roi_left->x + roi_left->width, roi_left->y + roi_left->height};
    if (roi_right) r = {roi_right->x, roi_right->y, roi_right->x + roi_right->width, roi_right->y + roi_right->height};
    check(mvsv_stream_enable_sharpness(s, roi_left ? &l : nullptr, roi_right ? &r : nullptr), ctx);
}
inline Sharpness stream_front_sharpness(mvsv_ctx* ctx, mvsv_stream* s)
{
    double v[2] = {0, 0};
    int64_t s4[2] = {0, 0};
    check(mvsv_stream_front_sharpness(s, v, s4), ctx);
    return {v[0], v[1], s4[0], s4[1]};
}

// Camera loop without the worker thread: push rectified pairs, pop maps (and the
// 9x9 means of the work ROI) in order; up to `depth` frames in flight.  The matcher
// is a StereoSGBM or a StereoBM (trgt/disparityTest.cpp:267-268 runs both); setParams
// takes either and switches the frames pushed from then on.
class DisparityStream {
public:
    DisparityStream(const StereoBM& matcher, int width, int height, int depth = 3, const Rect* grid_roi = nullptr)
        : ctx_(thread_context()), w_(width), h_(height)
    {
        mvsv_rect r{};
        if (grid_roi) r = {grid_roi->x, grid_roi->y, grid_roi->x + grid_roi->width, grid_roi->y + grid_roi->height};
        check(mvsv_stream_create_bm(ctx_, width, height, &matcher.p, depth, grid_roi ? &r : nullptr, &s_), ctx_);
    }
    DisparityStream(const StereoSGBM& matcher, int width, int height, int depth = 3,
                    const Rect* grid_roi = nullptr)
        : ctx_(thread_context()), w_(width), h_(height)
    {
        mvsv_rect r{};
        if (grid_roi) r = {grid_roi->x, grid_roi->y, grid_roi->x + grid_roi->width, grid_roi->y + grid_roi->height};
        check(mvsv_stream_create(ctx_, width, height, &matcher.params(), depth, grid_roi ? &r : nullptr, &s_),
              ctx_);
    }
    ~DisparityStream()
    {
        if (s_) mvsv_stream_destroy(s_);
    }
    DisparityStream(const DisparityStream&) = delete;
    DisparityStream& operator=(const DisparityStream&) = delete;
    void setParams(const StereoSGBM& matcher) { check(mvsv_stream_set_params(s_, &matcher.params()), ctx_); }
    void setParams(const StereoBM& matcher) { check(mvsv_stream_set_bm_params(s_, &matcher.p), ctx_); }
    // MVSV_MATCHER_SGBM / MVSV_MATCHER_BM: what computes the frames pushed from now on
    int matcher() const { return mvsv_stream_matcher(s_); }
    // colour pairs (CV_8UC3, src_width x src_height) from now on too (no frame may be
    // pending): uploaded as BGR, Utility::prepareGray on the device ahead of the matcher;
    // mvsv_prepare_size of the source must be the stream's size
    void enableBgr(int src_width, int src_height, bool halve = true, int variant = MVSV_GRAY_Q14)
    {
        check(mvsv_stream_enable_bgr(s_, src_width, src_height, halve ? 1 : 0, variant), ctx_);
    }
    void disableBgr() { check(mvsv_stream_disable_bgr(s_), ctx_); }
    // the maps of the colour pairs pushed from now on come from StereoSGBM on the halved
    // BGR pair itself, as cv::StereoSGBM matches CV_8UC3 (after enableBgr, no frame
    // pending, SGBM only; a switch to StereoBM throws while it is on)
    void bgrMatch(bool on = true) { check(mvsv_stream_set_bgr_match(s_, on ? 1 : 0), ctx_); }
    void pushBgr(const Mat& left, const Mat& right)
    {
        if (left.empty() || left.type != MAT_8UC3 || right.type != MAT_8UC3 || left.rows != right.rows ||
            left.cols != right.cols)
            throw Error(MVSV_E_INVALID_ARG, "pushBgr: CV_8UC3 pair of one size expected");
        check(mvsv_stream_push_bgr(s_, left.data, left.step, right.data, right.step), ctx_);
    }
    // frames computed `batch` at a time (frame-batch kernels, up to batch-1 frames of latency)
    void setBatch(int batch) { check(mvsv_stream_set_batch(s_, batch), ctx_); }
    // up to n frame-batch launches computed concurrently (1..4)
    void setInflight(int n) { check(mvsv_stream_set_inflight(s_, n), ctx_); }
    int pending() const { return mvsv_stream_pending(s_); }
    void push(const Stereopair& s)
    {
        check_pair(s.mLeft, s.mRight);
        check(mvsv_stream_push(s_, s.mLeft.data, s.mLeft.step, s.mRight.data, s.mRight.step), ctx_);
    }
    void pop(Mat& disparity, float* means81 = nullptr)
    {
        disparity.create(h_, w_, MAT_16SC1);
        check(mvsv_stream_pop(s_, reinterpret_cast<int16_t*>(disparity.data), disparity.step / 2, means81),
              ctx_);
    }
    // the oldest frame's map in the stream's pinned host slot (width x height
    // int16, no copy), valid until the next push
    const int16_t* popView(float* means81 = nullptr)
    {
        const int16_t* map = nullptr;
        check(mvsv_stream_pop_view(s_, &map, means81), ctx_);
        return map;
    }
    // the lattice detector on every frame pushed from now on (no frame may be
    // pending): d's Q and disparity range, over roi (d's init size; default the
    // whole map); at most max_hits hit records per frame (<= 0: all)
    void enableSamplepoints(const SamplepointDetection& d, const Rect* roi = nullptr, int max_hits = 0)
    {
        lattice_ = stream_enable_samplepoints(ctx_, s_, w_, h_, d, roi, max_hits);
    }
    void disableSamplepoints() { check(mvsv_stream_disable_samplepoints(s_), ctx_); }
    // the oldest pending frame's lattice results; the frame stays pending (pop it next)
    void frontSamples(SampleFrame& out) { stream_front_samples(ctx_, s_, lattice_, out); }
    // the 8-bit display map (Utility::normalize of dMap(roi)) with every frame pushed
    // from now on (no frame may be pending); default roi: the whole map
    void enableDisplay(const Rect* roi = nullptr, double alpha = 0, double beta = 255)
    {
        display_ = stream_enable_display(ctx_, s_, w_, h_, roi, alpha, beta);
    }
    void disableDisplay()
    {
        check(mvsv_stream_disable_display(s_), ctx_);
        display_ = {};
    }
    // the oldest pending frame's display map and (smin, smax); the frame stays pending
    void frontDisplay(Mat& out, int16_t* minmax = nullptr) { stream_front_display(ctx_, s_, display_, out, minmax); }
    // the same map in the stream's pinned host slot (dense, no copy), valid until the next push
    const uint8_t* frontDisplayView(int16_t* minmax = nullptr)
    {
        const uint8_t* map = nullptr;
        check(mvsv_stream_front_display_view(s_, &map, minmax), ctx_);
        return map;
    }
    // the detection view (Utility::detectionView of dMap(roi)) with every frame pushed
    // from now on (no frame may be pending).  MVSV_VIEW_FOUND_TILES: roi must be the
    // stream's grid_roi, meanRange a MeanDisparityDetection's mRangeDisparity;
    // MVSV_VIEW_FOUND_POINTS: enableSamplepoints over the same roi first
    void enableView(int layers, const Rect* roi = nullptr, std::pair<float, float> meanRange = {0.0f, 0.0f},
                    int pointRadius = 3, double alpha = 0, double beta = 255)
    {
        view_ = stream_enable_view(ctx_, s_, w_, h_, layers, roi, meanRange, pointRadius, alpha, beta);
    }
    void disableView()
    {
        check(mvsv_stream_disable_view(s_), ctx_);
        view_ = {};
    }
    // the oldest pending frame's view (CV_8UC3) and (smin, smax); the frame stays pending
    void frontView(Mat& out, int16_t* minmax = nullptr) { stream_front_view(ctx_, s_, view_, out, minmax); }
    // the same image in the stream's pinned host slot (dense, no copy), valid until the next push
    const uint8_t* frontViewView(int16_t* minmax = nullptr)
    {
        const uint8_t* img = nullptr;
        check(mvsv_stream_front_view_view(s_, &img, minmax), ctx_);
        return img;
    }
    // the point cloud (Utility::pointCloud of dMap(roi)) with every frame pushed from
    // now on (no frame may be pending); default roi: the whole map, max_points <= 0:
    // room for every pixel of the roi.  The records stay on the device until asked for.
    void enableCloud(const QMatrix& Q, const Rect* roi = nullptr, int max_points = 0)
    {
        cloud_ = stream_enable_cloud(ctx_, s_, w_, h_, Q, roi, max_points);
    }
    void disableCloud()
    {
        check(mvsv_stream_disable_cloud(s_), ctx_);
        cloud_ = 0;
    }
    // the oldest pending frame's records (the first min(count, max_points)); returns
    // the count of valid pixels; the frame stays pending
    int frontCloud(std::vector<mvsv_cloud_point>& out, int32_t* minmax = nullptr)
    {
        return stream_front_cloud(ctx_, s_, cloud_, out, minmax);
    }
    // Utility::checkSharpness of every pair pushed from now on (no frame may be pending),
    // each side over its own view area (default: the whole image)
    void enableSharpness(const Rect* roi_left = nullptr, const Rect* roi_right = nullptr)
    {
        stream_enable_sharpness(ctx_, s_, roi_left, roi_right);
    }
    void disableSharpness() { check(mvsv_stream_disable_sharpness(s_), ctx_); }
    // the oldest pending frame's focus values; the frame stays pending
    Sharpness frontSharpness() { return stream_front_sharpness(ctx_, s_); }
    // the same records on the device (the frame's slot of the ring), valid until the frame is popped
    const mvsv_cloud_point* frontCloudDevice(int* count, int32_t* minmax = nullptr)
    {
        const mvsv_cloud_point* p = nullptr;
        check(mvsv_stream_front_cloud_device(s_, &p, count, minmax), ctx_);
        return p;
    }
    // ---- device ends (mvsv.h "device ends of a stream") ----
    // n frames of device memory (or device-accessible host memory), strides in bytes,
    // as n pushes; ordered against hip_stream (nullptr: the null stream) by events, so
    // work queued on it after the call may overwrite the frames
    void pushDevice(int n, const uint8_t* left, size_t left_step, size_t left_frame_step, const uint8_t* right,
                    size_t right_step, size_t right_frame_step, void* hip_stream = nullptr)
    {
        check(mvsv_stream_push_device(s_, n, left, left_step, left_frame_step, right, right_step, right_frame_step,
                                      hip_stream), ctx_);
    }
    // the same for CV_8UC3 frames (enableBgr first)
    void pushBgrDevice(int n, const uint8_t* left, size_t left_step, size_t left_frame_step, const uint8_t* right,
                       size_t right_step, size_t right_frame_step, void* hip_stream = nullptr)
    {
        check(mvsv_stream_push_bgr_device(s_, n, left, left_step, left_frame_step, right, right_step,
                                          right_frame_step, hip_stream), ctx_);
    }
    // pops; the map is copied into device memory (stride in elements) on hip_stream
    void popDevice(int16_t* out_dev, size_t out_stride, float* means81 = nullptr, void* hip_stream = nullptr)
    {
        check(mvsv_stream_pop_device(s_, out_dev, out_stride, means81, hip_stream), ctx_);
    }
    // the oldest pending frame's map in the stream's device ring (dense, no copy), valid until it is popped
    const int16_t* frontMapDevice(float* means81 = nullptr)
    {
        const int16_t* map = nullptr;
        check(mvsv_stream_front_map_device(s_, &map, means81), ctx_);
        return map;
    }
    // MVSV_HOST_* bits: the per-frame products that are also downloaded (no frame may be pending)
    void hostOutputs(int mask) { check(mvsv_stream_set_host_outputs(s_, mask), ctx_); }
    // what the stream enqueues from now on waits for what is queued on hip_stream now
    void fence(void* hip_stream = nullptr) { check(mvsv_stream_fence(s_, hip_stream), ctx_); }

private:
    mvsv_ctx* ctx_;
    mvsv_stream* s_ = nullptr;
    int w_, h_;
    SampleLayout lattice_;
    DisplaySize display_, view_;
    int cloud_ = 0;
};

}  // namespace mvsv

#endif  // MVSV_DETECTION_HPP
