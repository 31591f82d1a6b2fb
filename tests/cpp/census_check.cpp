// Disparity::binary_sgbm (inc/disparity.h:30, src/disparity.cpp:12-15, commented out in the
// reference) through include/mvsv_disparity.hpp against the C ABI call.
//   census_check cpu           the rules of the mirror and of mvsv_sgbm_census_validate, no device
//   census_check gpu <file>    + binary_sgbm on a Stereopair of ROI views (step > cols) against
//                                mvsv_sgbm_census on the same pixels; writes the pair and its map
//                                to <file> for the Python restatement (tests/test_cpp_census.py)
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

static std::string thrown(mvsv::Ptr<mvsv::StereoSGBM> m, const mvsv::Mat& l, const mvsv::Mat& r, int cw, int ch)
{
    try {
        mvsv::Mat out;
        Stereopair s;
        s.mLeft = l;
        s.mRight = r;
        Disparity::binary_sgbm(s, out, m, cw, ch);
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

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        auto sgbm = mvsv::StereoSGBM::create(0, 32, 5, 10, 120, 0, 0, 10, 20, 2);
        auto bin = mvsv::stereo::StereoBinarySGBM::create(0, 32, 5, 10, 120, 0, 0, 10, 20, 2);
        REQUIRE(bin->getCensusWidth() == 9 && bin->getCensusHeight() == 7, 10);
        REQUIRE(bin->validate(640, 480), 11);
        bin->setCensusWindow(9, 9);
        REQUIRE(!bin->validate(640, 480), 12);
        bin->setCensusWindow(5, 5);
        REQUIRE(bin->validate(640, 480), 13);
        // the validation entry: window rule, int16 bound on both sides, MODE_SGBM_3WAY
        REQUIRE(mvsv_sgbm_census_validate(&sgbm->p, 640, 480, 9, 7) == MVSV_OK, 14);
        REQUIRE(mvsv_sgbm_census_validate(&sgbm->p, 640, 480, 8, 7) == MVSV_E_INVALID_ARG, 15);
        REQUIRE(mvsv_sgbm_census_validate(&sgbm->p, 640, 480, 1, 1) == MVSV_E_INVALID_ARG, 16);
        REQUIRE(mvsv_sgbm_census_validate(&sgbm->p, 640, 480, 13, 5) == MVSV_OK, 17);
        auto edge = mvsv::StereoSGBM::create(0, 16, 21, 10, 5425);
        REQUIRE(mvsv_sgbm_census_validate(&edge->p, 640, 480, 9, 7) == MVSV_OK, 18);
        edge->setP2(5426);
        REQUIRE(mvsv_sgbm_census_validate(&edge->p, 640, 480, 9, 7) == MVSV_E_INVALID_ARG, 19);
        auto way3 = mvsv::StereoSGBM::create(0, 16, 3, 0, 0, 0, 0, 0, 0, 0, MVSV_MODE_SGBM_3WAY);
        REQUIRE(mvsv_sgbm_census_validate(&way3->p, 640, 480, 9, 7) == MVSV_E_INVALID_ARG, 20);
        REQUIRE(mvsv_sgbm_workspace_bytes_census(1, 640, 480, &sgbm->p, 9, 7) > 0, 21);
        REQUIRE(mvsv_sgbm_workspace_bytes_census(1, 640, 480, &sgbm->p, 9, 8) == 0, 22);
        // the mirror's type rules need no device: grey pairs of one size only
        mvsv::Mat g(20, 90, mvsv::MAT_8UC1), g2(20, 91, mvsv::MAT_8UC1), c(20, 90, mvsv::MAT_8UC3), none;
        REQUIRE(thrown(sgbm, g, g2, 9, 7).find("CV_8UC1") != std::string::npos, 23);
        REQUIRE(thrown(sgbm, c, c, 9, 7).find("CV_8UC1") != std::string::npos, 24);
        REQUIRE(thrown(sgbm, none, none, 9, 7).find("CV_8UC1") != std::string::npos, 25);
        uint8_t px[4] = {0};
        int16_t o[4];
        uint64_t t[4];
        REQUIRE(mvsv_sgbm_census(nullptr, px, 2, px, 2, 2, 2, &sgbm->p, o, 2, 9, 7) == MVSV_E_INVALID_ARG, 26);
        REQUIRE(mvsv_sgbm_census_device(nullptr, 1, px, 2, 4, px, 2, 4, 2, 2, &sgbm->p, o, 2, 4, 9, 7) ==
                    MVSV_E_INVALID_ARG, 27);
        REQUIRE(mvsv_census(nullptr, px, 2, 2, 2, 3, 3, t, 2) == MVSV_E_INVALID_ARG, 28);
        REQUIRE(mvsv_stream_set_census(nullptr, 9, 7) == MVSV_E_INVALID_ARG, 29);
        std::printf("cpu ok\n");
        if (!gpu) return 0;
        if (argc < 3) return 2;

        // a rectified pair inside larger images: the Stereopair holds ROI views
        const int W = 150, H = 37, PADX = 7, PADY = 3;
        mvsv::Mat bigL(H + 2 * PADY, W + 2 * PADX, mvsv::MAT_8UC1), bigR(H + 2 * PADY, W + 2 * PADX, mvsv::MAT_8UC1);
        std::memset(bigL.data, 0x4d, (size_t)bigL.rows * bigL.step);
        std::memset(bigR.data, 0xb2, (size_t)bigR.rows * bigR.step);
        mvsv::Mat lv = bigL(mvsv::Rect{PADX, PADY, W, H}), rv = bigR(mvsv::Rect{PADX, PADY, W, H});
        REQUIRE(lv.step > (size_t)lv.cols, 30);
        mvsv::Mat wl(H, W, mvsv::MAT_8UC1), wr(H, W, mvsv::MAT_8UC1);
        REQUIRE(mvsv_synth_pair(0x5EED0C00u, W, H, 0, 32, wl.data, wr.data) == MVSV_OK, 31);
        for (int y = 0; y < H; y++) {
            std::memcpy(lv.ptr<uint8_t>(y), wl.ptr<uint8_t>(y), W);
            std::memcpy(rv.ptr<uint8_t>(y), wr.ptr<uint8_t>(y), W);
        }
        Stereopair s(lv, rv);
        mvsv::Mat dMap;
        Disparity::binary_sgbm(s, dMap, sgbm);  // the default window, (9, 7)
        REQUIRE(dMap.type == mvsv::MAT_16SC1 && dMap.rows == H && dMap.cols == W, 32);
        // the C ABI call on the same pixels as whole images
        mvsv::Mat abi(H, W, mvsv::MAT_16SC1);
        mvsv_ctx* ctx = mvsv::thread_context();
        REQUIRE(mvsv_sgbm_census(ctx, wl.data, wl.step, wr.data, wr.step, W, H, &sgbm->p, abi.ptr<int16_t>(0),
                                 abi.step / 2, 9, 7) == MVSV_OK, 33);
        REQUIRE(same(dMap, abi), 34);
        // the matcher that carries its window: the reference's signature
        mvsv::Mat viaBin, abi55(H, W, mvsv::MAT_16SC1);
        Disparity::binary_sgbm(s, viaBin, bin);  // (5, 5)
        REQUIRE(mvsv_sgbm_census(ctx, wl.data, wl.step, wr.data, wr.step, W, H, &bin->p, abi55.ptr<int16_t>(0),
                                 abi55.step / 2, 5, 5) == MVSV_OK, 35);
        REQUIRE(same(viaBin, abi55), 36);
        REQUIRE(!same(viaBin, dMap), 37);
        mvsv::Mat explicit55;
        Disparity::binary_sgbm(s, explicit55, sgbm, 5, 5);
        REQUIRE(same(explicit55, abi55), 38);
        // it is not the BT map, and Disparity::sgbm on the same matcher afterwards still is
        mvsv::Mat bt, bt2(H, W, mvsv::MAT_16SC1);
        Disparity::sgbm(s, bt, sgbm);
        REQUIRE(mvsv_sgbm(ctx, wl.data, wl.step, wr.data, wr.step, W, H, &sgbm->p, bt2.ptr<int16_t>(0), bt2.step / 2) ==
                    MVSV_OK, 39);
        REQUIRE(same(bt, bt2) && !same(bt, dMap), 40);
        // a refused window throws with the rule's name
        REQUIRE(thrown(sgbm, lv, rv, 9, 9).find("census window") != std::string::npos, 41);
        // the descriptors alone, on the ROI view
        std::vector<uint64_t> T((size_t)W * H);
        REQUIRE(mvsv_census(ctx, lv.data, lv.step, W, H, 3, 3, T.data(), W) == MVSV_OK, 42);
        for (int y = 1; y < H - 1; y++)
            for (int x = 1; x < W - 1; x++) {
                uint64_t want = 0;
                int k = 0;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        if (!dy && !dx) continue;
                        want |= (uint64_t)(wl.ptr<uint8_t>(y + dy)[x + dx] < wl.ptr<uint8_t>(y)[x]) << k++;
                    }
                REQUIRE(T[(size_t)y * W + x] == want, 43);
            }

        std::FILE* f = std::fopen(argv[2], "wb");
        REQUIRE(f != nullptr, 50);
        const int hdr[2] = {H, W};
        std::fwrite(hdr, sizeof(int), 2, f);
        std::fwrite(wl.data, 1, (size_t)H * W, f);
        std::fwrite(wr.data, 1, (size_t)H * W, f);
        for (int y = 0; y < H; y++) std::fwrite(dMap.ptr<int16_t>(y), 2, W, f);
        std::fclose(f);
        std::printf("gpu ok\n");
    } catch (const mvsv::Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
