// What the reference's detection programs show per frame (trgt/demo.cpp:280-298):
//   cv::normalize(dMapWork, dMapNorm, 0, 255, NORM_MINMAX, CV_8U); cv::cvtColor(GRAY2BGR);
//   View::drawSubimageGrid / View::drawObstacleGrid; drawFoundObstacles
// on include/mvsv_detection.hpp.
//   view_check cpu OUT_DIR      View's grids on the host, argument checks without a device
//   view_check gpu OUT_DIR      + Utility::detectionView, the view on a stream with both detectors
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mvsv_stereosystem.hpp"  // also compiles RawDisparityStream's view methods

static const mvsv::QMatrix Q = {1.f, 0.f, 0.f, -183.390320f, 0.f, 1.f, 0.f, -120.106110f,
                                0.f, 0.f, 0.f, 303.516571f,  0.f, 0.f, 0.00842495915f, 0.f};

#define REQUIRE(cond, code)                                  \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("failed: %s (%d)\n", #cond, code);   \
            return code;                                     \
        }                                                    \
    } while (0)

static bool is(const mvsv::Mat& img, int x, int y, int b, int g, int r)
{
    const uint8_t* p = img.ptr<uint8_t>(y) + 3 * x;
    return p[0] == b && p[1] == g && p[2] == r;
}

// the frame as demo.cpp builds it on the host: grey, the grids, then red over the
// found tiles (both corners included) -- drawn here pixel by pixel
static void host_frame(const mvsv::Mat& norm, const float* means, std::pair<float, float> range, mvsv::Mat& out)
{
    out.create(norm.rows, norm.cols, mvsv::MAT_8UC3);
    for (int y = 0; y < norm.rows; y++)
        for (int x = 0; x < norm.cols; x++)
            for (int c = 0; c < 3; c++) out.ptr<uint8_t>(y)[3 * x + c] = norm.ptr<uint8_t>(y)[x];
    mvsv::View::drawSubimageGrid(out, 0);
    mvsv::View::drawObstacleGrid(out, 0);
    const int dx = norm.cols / 9, dy = norm.rows / 9;
    for (int i = 0; i < 81; i++) {
        if (!(means[i] < range.first && means[i] > range.second)) continue;
        for (int y = (i / 9) * dy; y <= (i / 9) * dy + dy && y < norm.rows; y++)
            for (int x = (i % 9) * dx; x <= (i % 9) * dx + dx && x < norm.cols; x++) {
                uint8_t* p = out.ptr<uint8_t>(y) + 3 * x;
                p[0] = 0;
                p[1] = 0;
                p[2] = 255;
            }
    }
}

static bool same(const mvsv::Mat& a, const mvsv::Mat& b)
{
    if (a.type != mvsv::MAT_8UC3 || b.type != a.type || a.rows != b.rows || a.cols != b.cols) return false;
    for (int y = 0; y < a.rows; y++)
        if (std::memcmp(a.ptr<uint8_t>(y), b.ptr<uint8_t>(y), 3 * (size_t)a.cols) != 0) return false;
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    const std::string dir = argv[2];  // the detectors' point cloud files
    try {
        // View's grids on a 100 x 70 image: x = 11, y = 7 and x = 33, y = 23
        mvsv::Mat img(70, 100, mvsv::MAT_8UC3);
        std::memset(img.data, 7, 70 * 300);
        mvsv::View::drawSubimageGrid(img, 0);
        REQUIRE(is(img, 11, 0, 100, 0, 0) && is(img, 11, 69, 100, 0, 0) && is(img, 88, 40, 100, 0, 0), 10);
        REQUIRE(is(img, 0, 7, 100, 0, 0) && is(img, 99, 56, 100, 0, 0), 11);
        REQUIRE(is(img, 33, 0, 7, 7, 7) && is(img, 66, 1, 7, 7, 7) && is(img, 0, 21, 7, 7, 7) && is(img, 99, 63, 7, 7, 7), 12);
        mvsv::View::drawObstacleGrid(img, 0);
        REQUIRE(is(img, 33, 0, 0, 0, 255) && is(img, 66, 69, 0, 0, 255) && is(img, 0, 23, 0, 0, 255) &&
                    is(img, 99, 46, 0, 0, 255), 13);
        REQUIRE(is(img, 33, 7, 0, 0, 255) && is(img, 11, 23, 0, 0, 255) && is(img, 11, 7, 100, 0, 0) && is(img, 1, 1, 7, 7, 7), 14);
        // argument checks that need no device
        mvsv_view_spec spec{MVSV_VIEW_FOUND_TILES, 0, 255, nullptr, 0, 0, nullptr, 0, 0, 3};
        REQUIRE(mvsv_view_draw(img.data, img.step, 100, 70, &spec) == MVSV_E_INVALID_ARG, 15);  // no means
        spec.layers = 16;
        REQUIRE(mvsv_view_draw(img.data, img.step, 100, 70, &spec) == MVSV_E_INVALID_ARG, 16);
        spec.layers = MVSV_VIEW_SUBIMAGE_GRID;
        REQUIRE(mvsv_view_draw(img.data, 299, 100, 70, &spec) == MVSV_E_INVALID_ARG, 17);
        REQUIRE(mvsv_view_draw(img.data, img.step, 8, 70, &spec) == MVSV_E_INVALID_ARG, 18);
        spec.point_radius = 4;
        REQUIRE(mvsv_view_draw(img.data, img.step, 100, 70, &spec) == MVSV_E_INVALID_ARG, 19);
        REQUIRE(mvsv_view(nullptr, nullptr, 0, 0, 0, &spec, nullptr, 0, nullptr) == MVSV_E_INVALID_ARG, 20);
        REQUIRE(mvsv_stream_enable_view(nullptr, nullptr, &spec) == MVSV_E_INVALID_ARG, 21);
        REQUIRE(mvsv_stream_front_view(nullptr, img.data, 300, nullptr) == MVSV_E_INVALID_ARG, 22);
        bool threw = false;
        try {
            mvsv::Mat grey(70, 100, mvsv::MAT_8UC1);
            mvsv::View::drawObstacleGrid(grey, 0);
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw, 23);
        std::printf("cpu ok\n");
        if (!gpu) return 0;

        // demo.cpp's loop: SGBM, both detectors on the work ROI, the annotated frame
        auto sgbm = mvsv::StereoSGBM::create(0, 64, 9, 8 * 81, 32 * 81);
        std::vector<uint8_t> L(320 * 96), R(320 * 96);
        REQUIRE(mvsv_synth_pair(0x5EED0000u + 90, 320, 96, 0, 64, L.data(), R.data()) == MVSV_OK, 30);
        mvsv::Mat Lm = mvsv::Mat::wrap(L.data(), 96, 320, mvsv::MAT_8UC1, 320);
        mvsv::Mat Rm = mvsv::Mat::wrap(R.data(), 96, 320, mvsv::MAT_8UC1, 320);
        Stereopair pair(Lm, Rm);
        mvsv::Rect roi_u, roi_b;
        mvsv::createDMapROIS(96, 320, 64, roi_u, roi_b);
        mvsv::Mat direct;
        sgbm->compute(Lm, Rm, direct);
        mvsv::Mat work = direct(roi_u);
        mvsv::MeanDisparityDetection m(dir);
        mvsv::SamplepointDetection sp(dir);
        m.init(work, Q, 0.1f, 30.f);
        sp.init(work, Q, 0.1f, 30.f);
        m.build(work, 0, mvsv::MeanDisparityDetection::MEAN_VALUE);
        sp.build(work, 0, 0);
        std::vector<float> values;
        for (const mvsv::Samplepoint& s : sp.getSamplepointVec()) values.push_back(s.value);
        int found_tiles = 0;
        for (float v : m.getMeanMap()) found_tiles += v < m.getRangeDisparity().first && v > m.getRangeDisparity().second;
        REQUIRE(found_tiles > 0, 31);

        // the tiles' window: the device frame == the host frame built as demo.cpp builds it
        const int grids = MVSV_VIEW_SUBIMAGE_GRID | MVSV_VIEW_OBSTACLE_GRID;
        mvsv::Mat norm, want, si, spv, both;
        int16_t mm[2], got_mm[2];
        mvsv::Utility::normalize(work, norm, 0, 255, mm);
        host_frame(norm, m.getMeanMap().data(), m.getRangeDisparity(), want);
        mvsv::Utility::detectionView(work, si, grids | MVSV_VIEW_FOUND_TILES, m.getMeanMap().data(), m.getRangeDisparity(),
                                     nullptr, {0.f, 0.f}, 3, 0, 255, got_mm);
        REQUIRE(same(si, want) && got_mm[0] == mm[0] && got_mm[1] == mm[1], 32);
        // the points' window: every found point's centre and the ends of its widest span are red
        mvsv::Utility::detectionView(work, spv, grids | MVSV_VIEW_FOUND_POINTS, nullptr, {0.f, 0.f}, values.data(),
                                     sp.getRangeDisparity());
        sp.detectObstacles();
        REQUIRE(!sp.getFoundObstacles().empty(), 33);
        for (const mvsv::Samplepoint& s : sp.getFoundObstacles())
            REQUIRE(is(spv, s.center.x, s.center.y, 0, 0, 255) && is(spv, s.center.x - 3, s.center.y, 0, 0, 255) &&
                        is(spv, s.center.x + 3, s.center.y, 0, 0, 255) && is(spv, s.center.x, s.center.y + 3, 0, 0, 255),
                    34);
        mvsv::Utility::detectionView(work, both, 15, m.getMeanMap().data(), m.getRangeDisparity(), values.data(),
                                     sp.getRangeDisparity());

        // the same frames with every frame of a stream
        mvsv::DisparityStream st(*sgbm, 320, 96, 2, &roi_u);
        st.setBatch(2);
        threw = false;
        try {
            st.enableView(MVSV_VIEW_FOUND_POINTS, &roi_u);  // no sample points on the stream
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw, 40);
        st.enableSamplepoints(sp, &roi_u);
        st.enableView(15, &roi_u, m.getRangeDisparity());
        st.push(pair);
        threw = false;
        try {
            st.disableView();  // a frame is pending
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw, 41);
        st.push(pair);
        for (int f = 0; f < 2; f++) {
            mvsv::Mat view, map;
            st.frontView(view, got_mm);
            const uint8_t* pinned = st.frontViewView();
            REQUIRE(st.pending() == 2 - f, 42);
            REQUIRE(same(view, both) && got_mm[0] == mm[0] && got_mm[1] == mm[1], 43);
            REQUIRE(std::memcmp(pinned, both.data, 3 * (size_t)both.rows * both.cols) == 0, 44);
            st.pop(map);
        }
        threw = false;
        try {
            st.disableSamplepoints();  // the view draws the found points
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw, 45);
        st.disableView();
        st.disableSamplepoints();
        st.push(pair);
        threw = false;
        try {
            mvsv::Mat view;
            st.frontView(view);
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        mvsv::Mat map;
        st.pop(map);
        REQUIRE(threw && st.pending() == 0, 46);
        std::printf("gpu ok\n");
    } catch (const mvsv::Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
