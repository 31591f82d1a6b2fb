// trgt/disparityTest.cpp:269 -- Disparity::tm(s, dispMapTM, 5) -- on include/mvsv_disparity.hpp.
//   tm_check cpu      the accepted kernel sizes, argument checks without a device
//   tm_check gpu      + the call itself against the loops of src/disparity.cpp:39-56 restated
//                       here with exact 128-bit score comparisons, whole images and ROI views
#include <cstdio>
#include <cstring>
#include <vector>

#include "mvsv_disparity.hpp"

#define REQUIRE(cond, code)                                  \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("failed: %s (%d)\n", #cond, code);   \
            return code;                                     \
        }                                                    \
    } while (0)

// the reference's loops; score_x > score_b iff N_x^2 * SS_b > N_b^2 * SS_x, a window of
// zeros (or a zero template, where every N is 0) scoring 0
static void restate(const mvsv::Mat& L, const mvsv::Mat& R, unsigned k, std::vector<uint8_t>& out)
{
    const unsigned rows = (unsigned)L.rows, cols = (unsigned)L.cols;
    out.assign((size_t)rows * cols, 0);
    for (unsigned i = 0; i < rows - k; ++i)
        for (unsigned j = 0; j < cols - k; ++j) {
            const int destWidth = (int)cols - (int)j - 1;
            unsigned long long bn = 0, bs = 1;
            int loc = 0;
            for (int x = 0; x + (int)k <= destWidth; ++x) {
                unsigned long long n = 0, s = 0;
                for (unsigned y = 0; y < k; ++y)
                    for (unsigned c = 0; c < k; ++c) {
                        const unsigned long long t = L.ptr<uint8_t>(i + y)[j + c], v = R.ptr<uint8_t>(i + y)[j + x + c];
                        n += t * v;
                        s += v * v;
                    }
                if (s == 0) s = 1;
                if ((unsigned __int128)(n * n) * bs > (unsigned __int128)(bn * bn) * s) {
                    bn = n;
                    bs = s;
                    loc = x;
                }
            }
            out[(size_t)i * cols + j] = (uint8_t)loc;
        }
}

static bool same(const mvsv::Mat& got, const std::vector<uint8_t>& want, int w, int h)
{
    if (got.type != mvsv::MAT_8UC1 || got.cols != w || got.rows != h) return false;
    for (int y = 0; y < h; y++)
        if (std::memcmp(got.ptr<uint8_t>(y), want.data() + (size_t)y * w, w) != 0) return false;
    return true;
}

static bool throws_invalid(const Stereopair& s, unsigned k)
{
    try {
        mvsv::Mat out;
        Disparity::tm(s, out, k);
    } catch (const mvsv::Error& e) {
        return e.code() == MVSV_E_INVALID_ARG;
    }
    return false;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        REQUIRE(mvsv_tm_validate(5, 640, 480) == MVSV_OK && mvsv_tm_validate(31, 640, 480) == MVSV_OK, 10);
        REQUIRE(mvsv_tm_validate(0, 640, 480) == MVSV_E_INVALID_ARG, 11);
        REQUIRE(mvsv_tm_validate(32, 640, 480) == MVSV_E_INVALID_ARG, 12);
        REQUIRE(mvsv_tm_validate(12, 40, 12) == MVSV_E_INVALID_ARG && mvsv_tm_validate(11, 40, 12) == MVSV_OK, 13);
        uint8_t px[4] = {0, 0, 0, 0};
        REQUIRE(mvsv_tm(nullptr, px, 2, px, 2, 2, 2, 1, px, 2) == MVSV_E_INVALID_ARG, 14);
        REQUIRE(mvsv_tm_device(nullptr, 1, px, 2, 4, px, 2, 4, 2, 2, 1, px, 2, 4, 1) == MVSV_E_INVALID_ARG, 15);
        mvsv::Mat a(12, 40, mvsv::MAT_8UC1), b(12, 40, mvsv::MAT_8UC1), narrow(12, 39, mvsv::MAT_8UC1);
        Stereopair flat(a, b), uneven(a, narrow);
        REQUIRE(throws_invalid(flat, 0) && throws_invalid(flat, 12) && throws_invalid(flat, 32), 16);
        REQUIRE(throws_invalid(flat, 0xffffffffu) && throws_invalid(uneven, 5), 17);
        std::printf("cpu ok\n");
        if (!gpu) return 0;

        // disparityTest's pair: a synthetic rectified pair, 331 wide so that shifts pass 255
        const int W = 331, H = 20;
        mvsv::Mat l(H, W, mvsv::MAT_8UC1), r(H, W, mvsv::MAT_8UC1);
        REQUIRE(mvsv_synth_pair(0x5EED0000u + 5, W, H, 0, 64, l.data, r.data) == MVSV_OK, 30);
        for (int y = 0; y < H; y++) {  // a zero band in each image and a far match
            std::memset(r.ptr<uint8_t>(y) + 100, 0, 12);
            std::memset(l.ptr<uint8_t>(y) + 200, 0, 9);
            std::memcpy(l.ptr<uint8_t>(y), r.ptr<uint8_t>(y) + 290, 30);
        }
        Stereopair s(l, r);
        mvsv::Mat dispMapTM;
        Disparity::tm(s, dispMapTM, 5);  // trgt/disparityTest.cpp:269
        std::vector<uint8_t> want;
        restate(l, r, 5, want);
        REQUIRE(same(dispMapTM, want, W, H), 31);
        REQUIRE(dispMapTM.ptr<uint8_t>(0)[0] == (uint8_t)290 && dispMapTM.ptr<uint8_t>(H - 5)[0] == 0, 32);
        for (unsigned k : {1u, 8u, 19u}) {
            Disparity::tm(s, dispMapTM, k);
            restate(l, r, k, want);
            REQUIRE(same(dispMapTM, want, W, H), 33);
        }
        // ROI views: step > cols, entered a few bytes in
        mvsv::Mat lv = l(mvsv::Rect{3, 2, 130, 15}), rv = r(mvsv::Rect{3, 2, 130, 15});
        Stereopair sv(lv, rv);
        Disparity::tm(sv, dispMapTM, 5);
        restate(lv, rv, 5, want);
        REQUIRE(same(dispMapTM, want, 130, 15), 34);
        std::printf("gpu ok\n");
    } catch (const mvsv::Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
