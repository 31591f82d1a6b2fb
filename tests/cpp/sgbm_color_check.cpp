// trgt/disparityTest.cpp:201-232 without its two cvtColor lines: the colour pair goes to
// Disparity::sgbm as it is, and cv::StereoSGBM::compute matches in colour.
//   sgbm_color_check cpu           the type rules of the mirror, without a device
//   sgbm_color_check gpu <file>    + the loop itself on a CV_8UC3 Stereopair (ROI views with
//                                    step > 3 * cols); writes the pair and its map to <file> for
//                                    the Python restatement (tests/test_cpp_sgbm_color.py)
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mvsv_disparity.hpp"

#define REQUIRE(cond, code)                                  \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("failed: %s (%d)\n", #cond, code);   \
            return code;                                     \
        }                                                    \
    } while (0)

template <class Matcher>
static std::string thrown(Matcher& m, const mvsv::Mat& l, const mvsv::Mat& r)
{
    try {
        mvsv::Mat out;
        m->compute(l, r, out);
    } catch (const mvsv::Error& e) {
        return e.code() == MVSV_E_INVALID_ARG ? e.what() : "other code";
    }
    return "";
}

static bool same(const mvsv::Mat& a, const mvsv::Mat& b)
{
    if (a.type != mvsv::MAT_16SC1 || b.type != a.type || a.rows != b.rows || a.cols != b.cols) return false;
    for (int y = 0; y < a.rows; y++)
        if (std::memcmp(a.ptr<int16_t>(y), b.ptr<int16_t>(y), (size_t)a.cols * 2) != 0) return false;
    return true;
}

// channel c of every pixel of a colour image from a grey one
static void put_channel(mvsv::Mat& bgr, const mvsv::Mat& grey, int c)
{
    for (int y = 0; y < grey.rows; y++)
        for (int x = 0; x < grey.cols; x++) bgr.ptr<uint8_t>(y)[3 * x + c] = grey.ptr<uint8_t>(y)[x];
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        auto sgbm = mvsv::StereoSGBM::create(0, 32, 5, 200, 800, 0, 31, 10, 20, 2);
        auto bm = mvsv::StereoBM::create(32, 9);
        mvsv::Mat g(20, 90, mvsv::MAT_8UC1), c(20, 90, mvsv::MAT_8UC3), c2(20, 91, mvsv::MAT_8UC3), none;
        mvsv::Mat s16(20, 90, mvsv::MAT_16SC1);
        // mixed types, sizes and other depths throw cv::StereoSGBM::compute's assert
        const std::string want = "left.size() == right.size() && left.type() == right.type() && left.depth() == CV_8U";
        REQUIRE(thrown(sgbm, g, c).find(want) != std::string::npos, 10);
        REQUIRE(thrown(sgbm, c, g).find(want) != std::string::npos, 11);
        REQUIRE(thrown(sgbm, c, c2).find(want) != std::string::npos, 12);
        REQUIRE(thrown(sgbm, s16, s16).find(want) != std::string::npos, 13);
        REQUIRE(thrown(sgbm, none, none).find(want) != std::string::npos, 14);
        // StereoBM stays CV_8UC1 only
        REQUIRE(thrown(bm, c, c).find("CV_8UC1") != std::string::npos, 15);
        uint8_t px[12] = {0};
        int16_t o[4];
        REQUIRE(mvsv_sgbm_bgr(nullptr, px, 6, px, 6, 2, 2, &sgbm->p, o, 2) == MVSV_E_INVALID_ARG, 16);
        REQUIRE(mvsv_sgbm_bgr_device(nullptr, 1, px, 6, 12, px, 6, 12, 2, 2, &sgbm->p, o, 2, 4) == MVSV_E_INVALID_ARG, 17);
        std::printf("cpu ok\n");
        if (!gpu) return 0;
        if (argc < 3) return 2;

        // the "loaded" colour images: three synthetic rectified pairs as B, G and R, inside
        // larger images so that the pair handed on is a ROI view (step > 3 * cols)
        const int W = 150, H = 37, PADX = 7, PADY = 3;
        mvsv::Mat bigL(H + 2 * PADY, W + 2 * PADX, mvsv::MAT_8UC3), bigR(H + 2 * PADY, W + 2 * PADX, mvsv::MAT_8UC3);
        std::memset(bigL.data, 0x4d, (size_t)bigL.rows * bigL.step);
        std::memset(bigR.data, 0xb2, (size_t)bigR.rows * bigR.step);
        mvsv::Mat lv = bigL(mvsv::Rect{PADX, PADY, W, H}), rv = bigR(mvsv::Rect{PADX, PADY, W, H});
        REQUIRE(lv.step > (size_t)3 * lv.cols, 30);
        mvsv::Mat gl[3], gr[3];
        for (int ch = 0; ch < 3; ch++) {
            gl[ch].create(H, W, mvsv::MAT_8UC1);
            gr[ch].create(H, W, mvsv::MAT_8UC1);
            REQUIRE(mvsv_synth_pair(0x5EED0000u + 17 * ch, W, H, 0, 32, gl[ch].data, gr[ch].data) == MVSV_OK, 31);
            put_channel(lv, gl[ch], ch);
            put_channel(rv, gr[ch], ch);
        }
        Stereopair s(lv, rv);
        mvsv::Mat dMapSGBM;
        Disparity::sgbm(s, dMapSGBM, sgbm);  // trgt/disparityTest.cpp:232, on the colour pair
        REQUIRE(dMapSGBM.type == mvsv::MAT_16SC1 && dMapSGBM.rows == H && dMapSGBM.cols == W, 32);
        // the same pixels as whole images give the same map
        mvsv::Mat cl(H, W, mvsv::MAT_8UC3), crr(H, W, mvsv::MAT_8UC3), again;
        for (int y = 0; y < H; y++) {
            std::memcpy(cl.ptr<uint8_t>(y), lv.ptr<uint8_t>(y), (size_t)3 * W);
            std::memcpy(crr.ptr<uint8_t>(y), rv.ptr<uint8_t>(y), (size_t)3 * W);
        }
        Stereopair whole(cl, crr);
        Disparity::sgbm(whole, again, sgbm);
        REQUIRE(same(dMapSGBM, again), 33);
        // colour is matched: the map is not that of any single channel
        mvsv::Mat grey;
        for (int ch = 0; ch < 3; ch++) {
            Stereopair sg(gl[ch], gr[ch]);
            Disparity::sgbm(sg, grey, sgbm);
            REQUIRE(!same(dMapSGBM, grey), 34);
        }
        // one live channel among constant ftzero channels is exactly the grey pair (ftzero = 31)
        for (int ch = 0; ch < 3; ch++) {
            mvsv::Mat ol(H, W, mvsv::MAT_8UC3), orr(H, W, mvsv::MAT_8UC3), one;
            std::memset(ol.data, 31, (size_t)H * ol.step);
            std::memset(orr.data, 31, (size_t)H * orr.step);
            put_channel(ol, gl[1], ch);
            put_channel(orr, gr[1], ch);
            Stereopair so(ol, orr);
            Disparity::sgbm(so, one, sgbm);
            Stereopair sg(gl[1], gr[1]);
            Disparity::sgbm(sg, grey, sgbm);
            REQUIRE(same(one, grey), 35);
        }
        // the BM half of the loop still needs the grey pair
        REQUIRE(thrown(bm, lv, rv).find("CV_8UC1") != std::string::npos, 36);

        std::FILE* f = std::fopen(argv[2], "wb");
        REQUIRE(f != nullptr, 40);
        const int hdr[2] = {H, W};
        std::fwrite(hdr, sizeof(int), 2, f);
        std::fwrite(cl.data, 1, (size_t)H * W * 3, f);
        std::fwrite(crr.data, 1, (size_t)H * W * 3, f);
        for (int y = 0; y < H; y++) std::fwrite(dMapSGBM.ptr<int16_t>(y), 2, W, f);
        std::fclose(f);
        std::printf("gpu ok\n");
    } catch (const mvsv::Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
