// C++ RawDisparityStream check (include/mvsv_stereosystem.hpp), linked to libmvsv.so.
//   raw_stream_check cpu <calib dir> <tmp dir>   what needs no GPU: the wrapper refuses a
//                                                Stereosystem without initRectification()
//   raw_stream_check gpu <calib dir> <tmp dir>   Stereosystem -> RawDisparityStream, three
//                                                frames: writes the raw pairs, the rectified
//                                                pairs and the maps for the Python side to
//                                                compare with the oracle
#include <cstdio>
#include <cstring>
#include <string>

#include "mvsv_stereosystem.hpp"

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

static const int W = 376, H = 240;  // trgt/obstacle.cpp:342-345: baseline_small with binning

static bool dump(const std::string& path, const mvsv::Mat& m)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "%d %d\n", m.rows, m.cols);
    const size_t row = (size_t)m.cols * mvsv::Mat::elem(m.type);
    for (int y = 0; y < m.rows; y++) std::fwrite(m.ptr<uint8_t>(y), 1, row, f);
    std::fclose(f);
    return true;
}

// A raw pair that rectifies to a matchable one: both cameras see windows (views with
// step > cols) of one synthetic texture.  The fixture's left and right maps differ by
// about (0.65, -10.7) px over the frame, so the right window lies (13, -11) from the
// left one: the rectified right image is the left one about 12 px further on.
static void raw_pair(uint32_t seed, mvsv::Mat& big, mvsv::Mat& L, mvsv::Mat& R)
{
    big.create(H + 64, W + 128, mvsv::MAT_8UC1);
    mvsv::Mat other(H + 64, W + 128, mvsv::MAT_8UC1);
    mvsv::check(mvsv_synth_pair(seed, W + 128, H + 64, 0, 64, big.data, other.data), nullptr);
    L = big(mvsv::Rect{64, 32, W, H});
    R = big(mvsv::Rect{64 + 13, 32 - 11, W, H});
}

static mvsv::Ptr<mvsv::StereoSGBM> matcher() { return mvsv::StereoSGBM::create(0, 64, 5, 200, 800, 1, 31, 10, 50, 2); }

static int cpu_checks(const std::string& cal)
{
    mvsv::Stereosystem s(W, H, true);
    REQUIRE(s.loadIntrinsic(cal + "/baseline_small/intrinsic.yml"));
    REQUIRE(s.loadExtrinisic(cal + "/baseline_small/extrinsic.yml"));
    REQUIRE(!s.isInit() && s.width() == W && s.height() == H);
    int code = 0;
    try {
        mvsv::RawDisparityStream st(s, *matcher());
    } catch (const mvsv::Error& e) {
        code = e.code();
    }
    REQUIRE(code == MVSV_E_INVALID_ARG);
    REQUIRE(s.initRectification() && s.isInit());
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_run(const std::string& cal, const std::string& tmp)
{
    mvsv::Stereosystem s(W, H, true);
    REQUIRE(s.loadIntrinsic(cal + "/baseline_small/intrinsic.yml"));
    REQUIRE(s.loadExtrinisic(cal + "/baseline_small/extrinsic.yml"));
    REQUIRE(s.initRectification());
    const mvsv_rect roi = s.displayROI();
    auto m = matcher();
    {
        mvsv::RawDisparityStream st(s, *m, 0.f, 2, nullptr, true);
        REQUIRE(st.width() == roi.x1 - roi.x0 && st.height() == roi.y1 - roi.y0);
        mvsv::Mat big[3], L[3], R[3];
        int popped = 0;
        auto pop = [&]() {
            mvsv::Mat d;
            Stereopair rect;
            st.pop(d, nullptr, &rect);
            const std::string k = std::to_string(popped++);
            return dump(tmp + "/disp_" + k + ".bin", d) && dump(tmp + "/rect_l_" + k + ".bin", rect.mLeft) &&
                   dump(tmp + "/rect_r_" + k + ".bin", rect.mRight);
        };
        for (int i = 0; i < 3; i++) {
            raw_pair(0x5EED0000u + 40 + i, big[i], L[i], R[i]);
            const std::string k = std::to_string(i);
            REQUIRE(dump(tmp + "/raw_l_" + k + ".bin", L[i]) && dump(tmp + "/raw_r_" + k + ".bin", R[i]));
            if (st.pending() == 2) REQUIRE(pop());  // depth 2: the ring wraps
            st.push_raw(L[i], R[i]);
        }
        while (st.pending()) REQUIRE(pop());
        REQUIRE(popped == 3);
        // misuse comes back as mvsv::Error and leaves the stream usable
        int code = 0;
        try {
            mvsv::Mat small(H / 2, W / 2, mvsv::MAT_8UC1);
            st.push_raw(small, small);
        } catch (const mvsv::Error& e) {
            code = e.code();
        }
        REQUIRE(code == MVSV_E_INVALID_ARG && st.pending() == 0);
    }
    {
        // the factor overload's loop: every frame resized; no rectified pair kept
        mvsv::RawDisparityStream st(s, *m, 0.5f);
        int dw = 0, dh = 0;
        REQUIRE(mvsv_resize_size(roi.x1 - roi.x0, roi.y1 - roi.y0, 0.5, 0.5, &dw, &dh) == MVSV_OK);
        REQUIRE(st.width() == dw && st.height() == dh);
        mvsv::Mat big, L, R, d;
        raw_pair(0x5EED0000u + 40, big, L, R);
        st.push_raw(L, R);
        int code = 0;
        try {
            Stereopair rect;
            st.pop(d, nullptr, &rect);
        } catch (const mvsv::Error& e) {
            code = e.code();
        }
        REQUIRE(code == MVSV_E_INVALID_ARG && st.pending() == 1);
        st.pop(d);
        REQUIRE(dump(tmp + "/half_0.bin", d));
    }
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s cpu|gpu <calib dir> <tmp dir>\n", argv[0]);
        return 2;
    }
    if (!std::strcmp(argv[1], "cpu")) return cpu_checks(argv[2]);
    return gpu_run(argv[2], argv[3]);
}
