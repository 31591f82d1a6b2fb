// The two set-up loops of the reference on include/mvsv_detection.hpp and
// include/mvsv_stereosystem.hpp:
//   trgt/liveView.cpp:94-117          Utility::checkSharpness of a view area of each raw image
//   trgt/liveUndistortion.cpp:58      Stereosystem::getUndistortedImagepair
//
//   setup_demo cpu
//       compiles the call patterns; argument checks that need no device
//   setup_demo gpu PAIR W H X Y RW RH S4L S4R VL VR S4WL INTRINSIC WANT
//       PAIR: left then right image, W x H bytes each; (X, Y, RW, RH): the view area;
//       S4L / S4R / VL / VR: the twin's sums and values of that area (values as hex
//       floats), S4WL: its sum of the whole left image; INTRINSIC: intrinsic.yml;
//       WANT: the twin's undistorted pair, left then right
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "mvsv_stereosystem.hpp"

#define REQUIRE(cond, code)                                  \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("failed: %s (%d)\n", #cond, code);   \
            return code;                                     \
        }                                                    \
    } while (0)

static bool read_file(const char* path, std::vector<uint8_t>& out, size_t bytes)
{
    std::ifstream f(path, std::ios::binary);
    out.resize(bytes);
    return f && f.read(reinterpret_cast<char*>(out.data()), (std::streamsize)bytes);
}

template <class F>
static bool throws_invalid(F f)
{
    try {
        f();
    } catch (const mvsv::Error& e) {
        return e.code() == MVSV_E_INVALID_ARG;
    }
    return false;
}

static bool same_image(const mvsv::Mat& got, const uint8_t* want)
{
    for (int y = 0; y < got.rows; y++)
        if (std::memcmp(got.ptr<uint8_t>(y), want + (size_t)y * got.cols, got.cols) != 0) return false;
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        // ---- without a device ----------------------------------------------------------
        mvsv::Mat none;
        mvsv::Mat wrong(4, 8, mvsv::MAT_16SC1);
        REQUIRE(throws_invalid([&] { mvsv::Utility::checkSharpness(none); }), 10);
        REQUIRE(throws_invalid([&] { mvsv::Utility::checkSharpness(wrong, mvsv::Rect{0, 0, 4, 4}); }), 11);
        uint8_t px[32] = {0};
        int64_t s4 = 0;
        double v = 0;
        REQUIRE(mvsv_sharpness(nullptr, px, 8, 8, 4, nullptr, &v, &s4) == MVSV_E_INVALID_ARG, 12);
        REQUIRE(mvsv_sharpness_device(nullptr, 1, px, 8, 32, 8, 4, nullptr, &s4) == MVSV_E_INVALID_ARG, 13);
        REQUIRE(mvsv_stream_enable_sharpness(nullptr, nullptr, nullptr) == MVSV_E_INVALID_ARG, 14);
        REQUIRE(mvsv_stream_disable_sharpness(nullptr) == MVSV_E_INVALID_ARG, 15);
        REQUIRE(mvsv_stream_front_sharpness(nullptr, &v, &s4) == MVSV_E_INVALID_ARG, 16);
        const double K[9] = {80, 0, 47.25, 0, 80, 31.5, 0, 0, 1};
        REQUIRE(mvsv_undistort_pair(nullptr, px, 8, px, 8, 8, 4, K, nullptr, 0, K, nullptr, 0, px, 8, px, 8) ==
                    MVSV_E_INVALID_ARG, 17);
        // no coefficients and quarter-pixel principal point: the identity map, exactly
        std::vector<int16_t> xy(2 * 96 * 64);
        std::vector<uint16_t> frac(96 * 64);
        REQUIRE(mvsv_undistort_maps(K, nullptr, 0, nullptr, 96, 64, xy.data(), 96, frac.data(), 96) == MVSV_OK, 18);
        for (int y = 0; y < 64; y++)
            for (int x = 0; x < 96; x++)
                REQUIRE(xy[2 * (y * 96 + x)] == x && xy[2 * (y * 96 + x) + 1] == y && frac[y * 96 + x] == 0, 19);
        const double three[3] = {0.1, 0.2, 0.3};
        REQUIRE(mvsv_undistort_maps(K, three, 3, nullptr, 96, 64, xy.data(), 96, frac.data(), 96) ==
                    MVSV_E_INVALID_ARG, 20);
        {
            mvsv::Stereosystem bare(8, 4);
            mvsv::Mat l(4, 8, mvsv::MAT_8UC1), r(4, 8, mvsv::MAT_8UC1);
            Stereopair p(l, r);
            REQUIRE(!bare.getUndistortedImagepair(p), 21);  // no intrinsics loaded
        }
        std::printf("cpu ok\n");
        if (!gpu) return 0;
        if (argc != 16) return 2;

        // ---- trgt/liveView.cpp: the focus values of the clicked view area ------------------
        const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
        const mvsv::Rect viewArea{std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]), std::atoi(argv[8])};
        const int64_t want_l = std::atoll(argv[9]), want_r = std::atoll(argv[10]), want_whole = std::atoll(argv[13]);
        const double want_vl = std::strtod(argv[11], nullptr), want_vr = std::strtod(argv[12], nullptr);
        const size_t px_n = (size_t)W * H;
        std::vector<uint8_t> raw, want;
        REQUIRE(read_file(argv[2], raw, 2 * px_n) && read_file(argv[15], want, 2 * px_n), 30);
        mvsv::Mat Lm = mvsv::Mat::wrap(raw.data(), H, W, mvsv::MAT_8UC1, W);
        mvsv::Mat Rm = mvsv::Mat::wrap(raw.data() + px_n, H, W, mvsv::MAT_8UC1, W);
        Stereopair s(Lm, Rm);
        int64_t got_l = 0, got_r = 0, got_whole = 0;
        const double sharpL = mvsv::Utility::checkSharpness(s.mLeft, viewArea, &got_l);
        const double sharpR = mvsv::Utility::checkSharpness(s.mRight, viewArea, &got_r);
        std::printf("%.17g %.17g\n", sharpL, sharpR);
        REQUIRE(got_l == want_l && got_r == want_r, 31);
        REQUIRE(sharpL == want_vl && sharpR == want_vr, 32);
        const double whole = mvsv::Utility::checkSharpness(s.mLeft);
        mvsv::Utility::checkSharpness(s.mLeft, mvsv::Rect{0, 0, W, H}, &got_whole);
        REQUIRE(got_whole == want_whole && whole == ((double)want_whole / 4.0) * (1.0 / ((double)W * H)), 33);
        REQUIRE(throws_invalid([&] { mvsv::Utility::checkSharpness(s.mLeft, mvsv::Rect{W - 3, 0, 4, 4}); }), 34);

        // the same values with every frame of a stream
        {
            auto sgbm = mvsv::StereoSGBM::create(0, 64, 9, 8 * 81, 32 * 81);
            mvsv::DisparityStream st(*sgbm, W, H, 2);
            REQUIRE(throws_invalid([&] { st.enableSharpness(&viewArea, &viewArea); st.push(s); st.enableSharpness(); }), 40);
            mvsv::Sharpness f = st.frontSharpness();
            REQUIRE(st.pending() == 1, 41);
            REQUIRE(f.left == want_vl && f.right == want_vr && f.sum4_left == want_l && f.sum4_right == want_r, 42);
            mvsv::Mat map;
            st.pop(map);
            st.disableSharpness();
            st.push(s);
            REQUIRE(throws_invalid([&] { st.frontSharpness(); }), 43);
            st.pop(map);
        }

        // ---- trgt/liveUndistortion.cpp: the undistorted pair, written back into the pair ------
        mvsv::Stereosystem sys(W, H);
        REQUIRE(sys.loadIntrinsic(argv[14]), 50);
        for (int round = 0; round < 2; round++) {  // the second round finds the maps on the device
            mvsv::Mat l(H, W, mvsv::MAT_8UC1), r(H, W, mvsv::MAT_8UC1);
            for (int y = 0; y < H; y++) {
                std::memcpy(l.ptr<uint8_t>(y), raw.data() + (size_t)y * W, W);
                std::memcpy(r.ptr<uint8_t>(y), raw.data() + px_n + (size_t)y * W, W);
            }
            Stereopair p(l, r);
            REQUIRE(sys.getUndistortedImagepair(p), 51);
            REQUIRE(p.mLeft.cols == W && p.mLeft.rows == H, 52);
            REQUIRE(same_image(p.mLeft, want.data()) && same_image(p.mRight, want.data() + px_n), 53);
        }
        mvsv::Mat small(4, 8, mvsv::MAT_8UC1);
        Stereopair wrong_size(small, small);
        REQUIRE(!sys.getUndistortedImagepair(wrong_size), 54);
        std::printf("gpu ok\n");
    } catch (const mvsv::Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
