// trgt/disparityTest.cpp's loop -- cv::resize(.., 0.5, 0.5, INTER_AREA), cv::cvtColor(
// BGR2GRAY) (:201-211), then Disparity::sgbm and Disparity::bm on every pair (:267-268)
// -- on include/mvsv_detection.hpp and include/mvsv_stereosystem.hpp.
//   prepare_check cpu      the arithmetic restated here, argument checks without a device
//   prepare_check gpu      + Utility::prepareGray on the device, StereoBM and colour
//                            frames on a stream
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mvsv_stereosystem.hpp"  // also compiles RawDisparityStream's StereoBM constructor

#define REQUIRE(cond, code)                                  \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("failed: %s (%d)\n", #cond, code);   \
            return code;                                     \
        }                                                    \
    } while (0)

static int gray_of(int b, int g, int r, int variant)
{
    return variant == MVSV_GRAY_Q15 ? (b * 3735 + g * 19235 + r * 9798 + 16384) >> 15
                                    : (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14;
}

// one channel of one halved pixel: whole blocks (a+b+c+d+2) >> 2, clipped ones the
// float mean rounded half to even
static int halve_of(const mvsv::Mat& s, int dx, int dy, int c)
{
    int sum = 0, cnt = 0;
    for (int yy = 0; yy < 2 && 2 * dy + yy < s.rows; yy++)
        for (int xx = 0; xx < 2 && 2 * dx + xx < s.cols; xx++) {
            sum += s.ptr<uint8_t>(2 * dy + yy)[3 * (2 * dx + xx) + c];
            cnt++;
        }
    if (cnt == 4) return (sum + 2) >> 2;
    volatile float mean = (float)sum / (float)cnt;
    return (int)std::lrint((double)mean);
}

static void restate(const mvsv::Mat& bgr, bool halve, int variant, std::vector<uint8_t>& out, int& w, int& h)
{
    w = halve ? (int)std::nearbyint(bgr.cols * 0.5) : bgr.cols;
    h = halve ? (int)std::nearbyint(bgr.rows * 0.5) : bgr.rows;
    out.resize((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int ch[3];
            for (int c = 0; c < 3; c++) ch[c] = halve ? halve_of(bgr, x, y, c) : bgr.ptr<uint8_t>(y)[3 * x + c];
            out[(size_t)y * w + x] = (uint8_t)gray_of(ch[0], ch[1], ch[2], variant);
        }
}

static bool same(const mvsv::Mat& got, const std::vector<uint8_t>& want, int w, int h)
{
    if (got.type != mvsv::MAT_8UC1 || got.cols != w || got.rows != h) return false;
    for (int y = 0; y < h; y++)
        if (std::memcmp(got.ptr<uint8_t>(y), want.data() + (size_t)y * w, w) != 0) return false;
    return true;
}

static bool same_map(const mvsv::Mat& a, const mvsv::Mat& b)
{
    if (a.rows != b.rows || a.cols != b.cols) return false;
    for (int y = 0; y < a.rows; y++)
        if (std::memcmp(a.ptr<int16_t>(y), b.ptr<int16_t>(y), (size_t)a.cols * 2) != 0) return false;
    return true;
}

// a colour image around a grey one: every channel the grey value plus a little of its own
static mvsv::Mat colour(const std::vector<uint8_t>& g, int w, int h, unsigned salt)
{
    mvsv::Mat m(h, w, mvsv::MAT_8UC3);
    unsigned s = salt * 2654435761u + 1u;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) {
                s = s * 1664525u + 1013904223u;
                const int v = (int)g[(size_t)y * w + x] + (int)((s >> 24) % 7u) - 3;
                m.ptr<uint8_t>(y)[3 * x + c] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
            }
    return m;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        // spot values and sizes
        REQUIRE(gray_of(255, 255, 255, MVSV_GRAY_Q14) == 255 && gray_of(255, 255, 255, MVSV_GRAY_Q15) == 255, 10);
        REQUIRE(gray_of(255, 0, 0, MVSV_GRAY_Q14) == 29, 11);
        int w = 0, h = 0;
        REQUIRE(mvsv_prepare_size(5, 7, 1, &w, &h) == MVSV_OK && w == 2 && h == 4, 12);
        REQUIRE(mvsv_prepare_size(7, 5, 1, &w, &h) == MVSV_OK && w == 4 && h == 2, 13);
        REQUIRE(mvsv_prepare_size(7, 5, 0, &w, &h) == MVSV_OK && w == 7 && h == 5, 14);
        REQUIRE(mvsv_prepare_size(1, 1, 1, &w, &h) == MVSV_E_INVALID_ARG, 15);
        REQUIRE(mvsv_prepare_size(8, 8, 2, &w, &h) == MVSV_E_INVALID_ARG, 16);
        // argument checks that need no device
        uint8_t px[3] = {0, 0, 0}, byte = 0;
        REQUIRE(mvsv_prepare_gray(nullptr, px, 3, 1, 1, 0, 0, &byte, 1) == MVSV_E_INVALID_ARG, 17);
        REQUIRE(mvsv_stream_enable_bgr(nullptr, 2, 2, 1, 0) == MVSV_E_INVALID_ARG, 18);
        REQUIRE(mvsv_stream_push_bgr(nullptr, px, 3, px, 3) == MVSV_E_INVALID_ARG, 19);
        REQUIRE(mvsv_stream_set_bm_params(nullptr, nullptr) == MVSV_E_INVALID_ARG && mvsv_stream_matcher(nullptr) == -1, 20);
        bool threw = false;
        try {
            mvsv::Mat grey(4, 4, mvsv::MAT_8UC1), out;
            mvsv::Utility::prepareGray(grey, out);  // not CV_8UC3
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw, 21);
        std::printf("cpu ok\n");
        if (!gpu) return 0;

        // the two images of a 203 x 135 colour pair (clipped last column and row)
        const int SW = 203, SH = 135;
        std::vector<uint8_t> gl((size_t)SW * SH), gr((size_t)SW * SH);
        REQUIRE(mvsv_synth_pair(0x5EED0000u + 77, SW, SH, 0, 64, gl.data(), gr.data()) == MVSV_OK, 30);
        mvsv::Mat cl = colour(gl, SW, SH, 1), cr = colour(gr, SW, SH, 2);
        std::vector<uint8_t> wl, wr, wq;
        mvsv::Mat pl, pr, pq;
        restate(cl, true, MVSV_GRAY_Q14, wl, w, h);
        restate(cr, true, MVSV_GRAY_Q14, wr, w, h);
        REQUIRE(w == 102 && h == 68, 31);
        mvsv::Utility::prepareGray(cl, pl);
        mvsv::Utility::prepareGray(cr, pr);
        REQUIRE(same(pl, wl, w, h) && same(pr, wr, w, h), 32);
        int qw = 0, qh = 0;
        restate(cl, false, MVSV_GRAY_Q15, wq, qw, qh);
        mvsv::Utility::prepareGray(cl, pq, false, MVSV_GRAY_Q15);
        REQUIRE(same(pq, wq, SW, SH), 33);
        // a BGR view entered one pixel in
        mvsv::Mat part = cl(mvsv::Rect{1, 1, 101, 67});
        restate(part, true, MVSV_GRAY_Q14, wq, qw, qh);
        mvsv::Utility::prepareGray(part, pq);
        REQUIRE(same(pq, wq, qw, qh), 34);

        // disparityTest's loop: both matchers on the prepared pair, one-shot ...
        auto sgbm = mvsv::StereoSGBM::create(0, 32, 5, 200, 800, 1, 31, 10, 50, 2);
        auto bm = mvsv::StereoBM::create(32, 9);
        mvsv::Mat ds, db;
        sgbm->compute(pl, pr, ds);
        bm->compute(pl, pr, db);
        REQUIRE(!same_map(ds, db), 40);
        // ... and as a StereoBM stream that takes the colour pair
        mvsv::DisparityStream st(*bm, w, h, 3);
        REQUIRE(st.matcher() == MVSV_MATCHER_BM, 41);
        threw = false;
        try {
            st.pushBgr(cl, cr);  // not enabled
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw && st.pending() == 0, 42);
        threw = false;
        try {
            st.enableBgr(SW - 3, SH);  // halves to another size
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw, 43);
        st.enableBgr(SW, SH);
        st.setBatch(3);
        Stereopair grey(pl, pr);
        st.pushBgr(cl, cr);
        st.push(grey);
        st.setParams(*sgbm);  // the two BM frames are launched; SGBM from here on
        REQUIRE(st.matcher() == MVSV_MATCHER_SGBM && st.pending() == 2, 44);
        st.pushBgr(cl, cr);
        mvsv::Mat m0, m1, m2;
        st.pop(m0);
        st.pop(m1);
        st.pop(m2);
        REQUIRE(same_map(m0, db) && same_map(m1, db) && same_map(m2, ds), 45);
        st.setParams(*bm);
        st.disableBgr();
        st.push(grey);
        st.pop(m0);
        REQUIRE(same_map(m0, db) && st.matcher() == MVSV_MATCHER_BM, 46);
        std::printf("gpu ok\n");
    } catch (const mvsv::Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
