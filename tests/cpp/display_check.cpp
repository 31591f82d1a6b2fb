// The display step of the reference's loops -- cv::normalize(dMap, dMapNorm, 0, 255,
// cv::NORM_MINMAX, CV_8U), trgt/liveDisparity.cpp:92, on the work ROI in
// trgt/mean_test.cpp:307 -- on include/mvsv_detection.hpp.
//   display_check cpu      the arithmetic restated here, argument checks without a device
//   display_check gpu      + Utility::normalize on the device, the display map on a stream
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mvsv_stereosystem.hpp"  // also compiles RawDisparityStream's display methods

#define REQUIRE(cond, code)                                  \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("failed: %s (%d)\n", #cond, code);   \
            return code;                                     \
        }                                                    \
    } while (0)

// OpenCV 3.4's arithmetic, every operation rounded on its own (volatile keeps the
// compiler from fusing or widening any of them)
static void restate(const mvsv::Mat& d, double alpha, double beta, std::vector<uint8_t>& out, int16_t mm[2])
{
    int smin = 32767, smax = -32768;
    for (int y = 0; y < d.rows; y++)
        for (int x = 0; x < d.cols; x++) {
            const int v = d.ptr<int16_t>(y)[x];
            smin = v < smin ? v : smin;
            smax = v > smax ? v : smax;
        }
    const double dmin = alpha < beta ? alpha : beta, dmax = alpha < beta ? beta : alpha;
    volatile double range = (double)smax - (double)smin;
    volatile double recip = range > DBL_EPSILON ? 1.0 / range : 0.0;
    volatile double scale = (dmax - dmin) * recip;
    volatile double prod = (double)smin * scale;
    volatile double shift = dmin - prod;
    const float sf = (float)scale, hf = (float)shift;
    out.resize((size_t)d.rows * d.cols);
    for (int y = 0; y < d.rows; y++)
        for (int x = 0; x < d.cols; x++) {
            volatile float p = (float)d.ptr<int16_t>(y)[x] * sf;
            volatile float t = p + hf;
            const long r = std::lrint((double)t);  // half to even in the default rounding mode
            out[(size_t)y * d.cols + x] = (uint8_t)(r < 0 ? 0 : r > 255 ? 255 : r);
        }
    mm[0] = (int16_t)smin;
    mm[1] = (int16_t)smax;
}

static bool same(const mvsv::Mat& got, const std::vector<uint8_t>& want)
{
    if (got.type != mvsv::MAT_8UC1 || (size_t)got.rows * got.cols != want.size()) return false;
    for (int y = 0; y < got.rows; y++)
        if (std::memcmp(got.ptr<uint8_t>(y), want.data() + (size_t)y * got.cols, got.cols) != 0) return false;
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        std::vector<uint8_t> want;
        int16_t mm[2];
        // (0, 510): scale 0.5 exactly, halves go to the even neighbour
        mvsv::Mat half(1, 511, mvsv::MAT_16SC1);
        for (int x = 0; x < 511; x++) half.ptr<int16_t>(0)[x] = (int16_t)x;
        restate(half, 0, 255, want, mm);
        REQUIRE(mm[0] == 0 && mm[1] == 510, 10);
        REQUIRE(want[1] == 0 && want[2] == 1 && want[3] == 2 && want[5] == 2 && want[7] == 4 && want[510] == 255, 11);
        // SGBM's invalid marker as the minimum: the ladder (-16, 222) in a 100 x 70 map
        mvsv::Mat dmap(70, 100, mvsv::MAT_16SC1);
        for (int y = 0; y < 70; y++)
            for (int x = 0; x < 100; x++) dmap.ptr<int16_t>(y)[x] = (int16_t)((y * 100 + x) % 239 - 16);
        restate(dmap, 0, 255, want, mm);
        REQUIRE(mm[0] == -16 && mm[1] == 222 && want[0] == 0 && want[238] == 255, 12);
        // argument checks that need no device
        uint8_t byte = 0;
        REQUIRE(mvsv_normalize_minmax(nullptr, dmap.ptr<int16_t>(0), 100, 100, 70, 0, 255, &byte, 100, nullptr) ==
                    MVSV_E_INVALID_ARG, 13);
        REQUIRE(mvsv_minmax_device(nullptr, 1, dmap.ptr<int16_t>(0), 100, 7000, 100, 70, 0, mm) == MVSV_E_INVALID_ARG, 14);
        REQUIRE(mvsv_stream_enable_display(nullptr, nullptr, 0, 255) == MVSV_E_INVALID_ARG, 15);
        REQUIRE(mvsv_stream_front_display(nullptr, &byte, 1, nullptr) == MVSV_E_INVALID_ARG, 16);
        std::printf("cpu ok\n");
        if (!gpu) return 0;

        // Utility::normalize == the restatement, whole map and an odd ROI of it
        mvsv::Mat norm;
        int16_t got_mm[2] = {0, 0};
        mvsv::Utility::normalize(dmap, norm, 0, 255, got_mm);
        REQUIRE(same(norm, want) && got_mm[0] == -16 && got_mm[1] == 222, 20);
        mvsv::Mat part = dmap(mvsv::Rect{7, 3, 81, 59});
        restate(part, 32, 224, want, mm);
        mvsv::Utility::normalize(part, norm, 224, 32, got_mm);
        REQUIRE(same(norm, want) && got_mm[0] == mm[0] && got_mm[1] == mm[1], 21);
        mvsv::Utility::normalize(half, norm);
        restate(half, 0, 255, want, mm);
        REQUIRE(same(norm, want), 22);

        // liveDisparity's loop: the display map comes back with every frame of a stream
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
        mvsv::DisparityStream st(*sgbm, 320, 96, 2, &roi_u);
        st.setBatch(2);
        mvsv::Mat disp;
        st.push(pair);
        bool threw = false;
        try {
            st.frontDisplay(disp);  // not enabled
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw && st.pending() == 1, 31);
        threw = false;
        try {
            st.enableDisplay(&roi_u);  // a frame is pending
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw, 32);
        {
            mvsv::Mat map;
            st.pop(map);
        }
        for (int whole = 0; whole < 2; whole++) {
            if (whole)
                st.enableDisplay();
            else
                st.enableDisplay(&roi_u);
            st.push(pair);
            st.push(pair);
            for (int f = 0; f < 2; f++) {
                st.frontDisplay(disp, got_mm);
                const uint8_t* view = st.frontDisplayView();
                REQUIRE(st.pending() == 2 - f, 33);
                mvsv::Mat map;
                st.pop(map);
                for (int y = 0; y < 96; y++)
                    REQUIRE(std::memcmp(map.ptr<int16_t>(y), direct.ptr<int16_t>(y), 640) == 0, 34);
                mvsv::Mat w = whole ? map : map(roi_u);
                restate(w, 0, 255, want, mm);
                REQUIRE(same(disp, want) && got_mm[0] == mm[0] && got_mm[1] == mm[1], 35);
                REQUIRE(std::memcmp(view, want.data(), want.size()) == 0, 36);
                mvsv::Utility::normalize(w, norm);
                REQUIRE(same(norm, want), 37);
            }
        }
        st.disableDisplay();
        st.push(pair);
        threw = false;
        try {
            st.frontDisplay(disp);
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        mvsv::Mat map;
        st.pop(map);
        REQUIRE(threw && st.pending() == 0, 38);
        std::printf("gpu ok\n");
    } catch (const mvsv::Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
