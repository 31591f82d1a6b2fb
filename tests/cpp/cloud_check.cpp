// The point cloud of the reference's loops -- Utility::dmap2pcl("pointcloud.ply",
// dMapRaw, Q_32F), trgt/demo.cpp:394 and the other detector programs -- on
// include/mvsv_detection.hpp: Utility::pointCloud and the streams' enableCloud /
// frontCloud.
//   cloud_check cpu      the records restated here, argument checks without a device
//   cloud_check gpu      + Utility::pointCloud on the device, the cloud on a stream
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mvsv_stereosystem.hpp"  // also compiles RawDisparityStream's cloud methods

#define REQUIRE(cond, code)                                  \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("failed: %s (%d)\n", #cond, code);   \
            return code;                                     \
        }                                                    \
    } while (0)

// Q of tests/golden/q_matrix.json
static const mvsv::QMatrix Q = {1.0f, 0.0f, 0.0f, -183.390320f, 0.0f, 1.0f, 0.0f, -120.106110f,
                                0.0f, 0.0f, 0.0f, 303.516571f,  0.0f, 0.0f, 0.00842495915f, 0.0f};

// Utility::dmap2pcl's loop with ply::write's grey, every operation rounded on its
// own (volatile keeps the compiler from widening or fusing any of them)
static int restate(const mvsv::Mat& d, std::vector<mvsv_cloud_point>& out, int32_t mm[2])
{
    int mn = 32767, mx = -32768;
    for (int y = 0; y < d.rows; y++)
        for (int x = 0; x < d.cols; x++) {
            const int v = d.ptr<int16_t>(y)[x];
            if (v > 0) {
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
            }
        }
    out.clear();
    for (int y = 0; y < d.rows; y++)
        for (int x = 0; x < d.cols; x++) {
            const int v = d.ptr<int16_t>(y)[x];
            if (v <= 0) continue;
            float c[4];
            mvsv_calc_coordinate((float)x, (float)y, (float)v, Q.data(), c);
            volatile float num = c[2] - (float)mn;
            volatile float q = num / (float)(mx - mn);
            volatile double t = (double)q * 255.0;
            const double tt = t;
            const int32_t g = (tt > -2147483649.0 && tt < 2147483648.0) ? (int32_t)tt : INT32_MIN;
            out.push_back({c[0], c[1], c[2], g});
        }
    mm[0] = mn;
    mm[1] = mx;
    return (int)out.size();
}

static bool same(const std::vector<mvsv_cloud_point>& got, const std::vector<mvsv_cloud_point>& want, size_t k)
{
    return got.size() == k && want.size() >= k &&
           (k == 0 || std::memcmp(got.data(), want.data(), k * sizeof(mvsv_cloud_point)) == 0);
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        static_assert(sizeof(mvsv_cloud_point) == 16, "a cloud record is 16 bytes");
        std::vector<mvsv_cloud_point> want, got;
        int32_t mm[2], got_mm[2] = {0, 0};
        // a 100 x 70 map: every third pixel invalid or zero, values 2..600 elsewhere
        mvsv::Mat dmap(70, 100, mvsv::MAT_16SC1);
        for (int y = 0; y < 70; y++)
            for (int x = 0; x < 100; x++) {
                const int i = y * 100 + x;
                dmap.ptr<int16_t>(y)[x] = (int16_t)(i % 3 == 0 ? (i % 2 ? -16 : 0) : 1 + (i * 7) % 600);
            }
        const int n = restate(dmap, want, mm);
        REQUIRE(n == 4666 && mm[0] == 2 && mm[1] == 600, 10);
        const auto first = mvsv::Utility::calcCoordinate({(float)dmap.ptr<int16_t>(0)[1], 1.0f, 0.0f}, Q);  // pixel (1, 0)
        REQUIRE(want[0].x == first[0] && want[0].y == first[1] && want[0].z == first[2] && want[0].grey > 255, 11);
        mvsv::Mat constant(2, 3, mvsv::MAT_16SC1);
        for (int i = 0; i < 6; i++) constant.ptr<int16_t>(i / 3)[i % 3] = 77;
        std::vector<mvsv_cloud_point> cw;
        REQUIRE(restate(constant, cw, mm) == 6 && mm[0] == 77 && mm[1] == 77 && cw[5].grey == INT32_MIN, 12);
        // argument checks that need no device
        int count = 0;
        mvsv_cloud_point one;
        REQUIRE(mvsv_point_cloud(nullptr, dmap.ptr<int16_t>(0), 100, 100, 70, Q.data(), &one, 1, &count, nullptr) ==
                    MVSV_E_INVALID_ARG, 13);
        REQUIRE(mvsv_point_cloud_device(nullptr, 1, dmap.ptr<int16_t>(0), 100, 7000, 100, 70, Q.data(), &one, 1, &count,
                                        nullptr) == MVSV_E_INVALID_ARG, 14);
        REQUIRE(mvsv_stream_enable_cloud(nullptr, nullptr, Q.data(), 0) == MVSV_E_INVALID_ARG, 15);
        REQUIRE(mvsv_stream_front_cloud(nullptr, &one, 1, &count, nullptr) == MVSV_E_INVALID_ARG, 16);
        std::printf("cpu ok\n");
        if (!gpu) return 0;

        // Utility::pointCloud == the restatement: whole map, truncated, an odd ROI, a constant map
        restate(dmap, want, mm);
        REQUIRE(mvsv::Utility::pointCloud(dmap, Q, got, 0, got_mm) == n, 20);
        REQUIRE(same(got, want, (size_t)n) && got_mm[0] == 2 && got_mm[1] == 600, 21);
        REQUIRE(mvsv::Utility::pointCloud(dmap, Q, got, 100) == n && same(got, want, 100), 22);
        mvsv::Mat part = dmap(mvsv::Rect{7, 3, 81, 59});
        const int np = restate(part, want, mm);
        REQUIRE(mvsv::Utility::pointCloud(part, Q, got, 0, got_mm) == np && same(got, want, (size_t)np), 23);
        REQUIRE(got_mm[0] == mm[0] && got_mm[1] == mm[1], 24);
        REQUIRE(mvsv::Utility::pointCloud(constant, Q, got) == 6 && same(got, cw, 6), 25);

        // the detector loops: the cloud comes with every frame of a stream
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
        st.push(pair);
        bool threw = false;
        try {
            st.frontCloud(got);  // not enabled
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw && st.pending() == 1, 31);
        threw = false;
        try {
            st.enableCloud(Q, &roi_u);  // a frame is pending
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw, 32);
        {
            mvsv::Mat map;
            st.pop(map);
        }
        for (int mode = 0; mode < 3; mode++) {  // the work ROI, the whole map, the work ROI cut to 500 points
            if (mode == 1)
                st.enableCloud(Q);
            else
                st.enableCloud(Q, &roi_u, mode == 2 ? 500 : 0);
            st.push(pair);
            st.push(pair);
            for (int f = 0; f < 2; f++) {
                const int c = st.frontCloud(got, got_mm);
                int cdev = -1;
                REQUIRE(st.frontCloudDevice(&cdev) != nullptr && cdev == c, 33);
                REQUIRE(st.pending() == 2 - f, 34);
                mvsv::Mat map;
                st.pop(map);
                for (int y = 0; y < 96; y++)
                    REQUIRE(std::memcmp(map.ptr<int16_t>(y), direct.ptr<int16_t>(y), 640) == 0, 35);
                mvsv::Mat w = mode == 1 ? map : map(roi_u);
                const int wn = restate(w, want, mm);
                REQUIRE(c == wn && wn > 500 && got_mm[0] == mm[0] && got_mm[1] == mm[1], 36);
                REQUIRE(same(got, want, mode == 2 ? 500 : (size_t)wn), 37);
            }
        }
        st.disableCloud();
        st.push(pair);
        threw = false;
        try {
            st.frontCloud(got);
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
