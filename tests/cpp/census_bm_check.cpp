// Disparity::binary_bm through include/mvsv_disparity.hpp against the C ABI call.
//   census_bm_check cpu                the rules of the mirror and of mvsv_bm_census_validate, no device
//   census_bm_check gpu <in> <out>     + binary_bm on a Stereopair of ROI views (step > cols) holding the
//                                        pair of <in> (int32 H, W, then the left and the right bytes)
//                                        against mvsv_bm_census on the same pixels; writes the map to <out>
//                                        for the fixture and the restatement (tests/test_cpp_census_bm.py)
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

static std::string thrown(mvsv::Ptr<mvsv::StereoBM> m, const mvsv::Mat& l, const mvsv::Mat& r, int cw, int ch)
{
    try {
        mvsv::Mat out;
        Stereopair s;
        s.mLeft = l;
        s.mRight = r;
        Disparity::binary_bm(s, out, m, cw, ch);
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
        auto bm = mvsv::StereoBM::create(16, 5);
        auto bin = mvsv::stereo::StereoBinaryBM::create(16, 5);
        REQUIRE(bin->getCensusWidth() == 9 && bin->getCensusHeight() == 7, 10);
        REQUIRE(bin->getNumDisparities() == 16 && bin->getBlockSize() == 5, 11);
        REQUIRE(bin->validate(640, 480), 12);
        bin->setCensusWindow(9, 9);
        REQUIRE(!bin->validate(640, 480), 13);
        bin->setCensusWindow(5, 5);
        REQUIRE(bin->validate(640, 480), 14);
        // the validation entry: the window rule and mvsv_bm_validate's own
        REQUIRE(mvsv_bm_census_validate(&bm->p, 640, 480, 9, 7) == MVSV_OK, 15);
        REQUIRE(mvsv_bm_census_validate(&bm->p, 640, 480, 8, 7) == MVSV_E_INVALID_ARG, 16);
        REQUIRE(mvsv_bm_census_validate(&bm->p, 640, 480, 1, 1) == MVSV_E_INVALID_ARG, 17);
        REQUIRE(mvsv_bm_census_validate(&bm->p, 640, 480, 13, 5) == MVSV_OK, 18);
        auto odd = mvsv::StereoBM::create(24, 5);
        REQUIRE(mvsv_bm_census_validate(&odd->p, 640, 480, 9, 7) == MVSV_E_INVALID_ARG, 19);
        auto even = mvsv::StereoBM::create(16, 6);
        REQUIRE(mvsv_bm_census_validate(&even->p, 640, 480, 9, 7) == MVSV_E_INVALID_ARG, 20);
        REQUIRE(mvsv_bm_census_validate(&bm->p, 640, 5, 9, 7) == MVSV_E_INVALID_ARG, 21);
        // the mirror's type rules need no device: grey pairs of one size only
        mvsv::Mat g(20, 90, mvsv::MAT_8UC1), g2(20, 91, mvsv::MAT_8UC1), c(20, 90, mvsv::MAT_8UC3), none;
        REQUIRE(!thrown(bm, g, g2, 9, 7).empty(), 23);
        REQUIRE(!thrown(bm, c, c, 9, 7).empty(), 24);
        REQUIRE(!thrown(bm, none, none, 9, 7).empty(), 25);
        uint8_t px[4] = {0};
        int16_t o[4];
        REQUIRE(mvsv_bm_census(nullptr, px, 2, px, 2, 2, 2, &bm->p, o, 2, 9, 7) == MVSV_E_INVALID_ARG, 26);
        REQUIRE(mvsv_bm_census_device(nullptr, 1, px, 2, 4, px, 2, 4, 2, 2, &bm->p, o, 2, 4, 9, 7) ==
                    MVSV_E_INVALID_ARG, 27);
        REQUIRE(mvsv_stream_set_bm_census(nullptr, 9, 7) == MVSV_E_INVALID_ARG, 28);
        std::printf("cpu ok\n");
        if (!gpu) return 0;
        if (argc < 4) return 2;

        std::FILE* in = std::fopen(argv[2], "rb");
        REQUIRE(in != nullptr, 29);
        int hdr[2];
        REQUIRE(std::fread(hdr, sizeof(int), 2, in) == 2, 29);
        const int H = hdr[0], W = hdr[1], PADX = 7, PADY = 3;
        mvsv::Mat wl(H, W, mvsv::MAT_8UC1), wr(H, W, mvsv::MAT_8UC1);
        REQUIRE(std::fread(wl.data, 1, (size_t)H * W, in) == (size_t)H * W, 29);
        REQUIRE(std::fread(wr.data, 1, (size_t)H * W, in) == (size_t)H * W, 29);
        std::fclose(in);
        // the pair inside larger images: the Stereopair holds ROI views
        mvsv::Mat bigL(H + 2 * PADY, W + 2 * PADX, mvsv::MAT_8UC1), bigR(H + 2 * PADY, W + 2 * PADX, mvsv::MAT_8UC1);
        std::memset(bigL.data, 0x4d, (size_t)bigL.rows * bigL.step);
        std::memset(bigR.data, 0xb2, (size_t)bigR.rows * bigR.step);
        mvsv::Mat lv = bigL(mvsv::Rect{PADX, PADY, W, H}), rv = bigR(mvsv::Rect{PADX, PADY, W, H});
        REQUIRE(lv.step > (size_t)lv.cols, 30);
        for (int y = 0; y < H; y++) {
            std::memcpy(lv.ptr<uint8_t>(y), wl.ptr<uint8_t>(y), W);
            std::memcpy(rv.ptr<uint8_t>(y), wr.ptr<uint8_t>(y), W);
        }
        Stereopair s(lv, rv);
        mvsv::Mat dMap;
        Disparity::binary_bm(s, dMap, bm);  // the default window, (9, 7)
        REQUIRE(dMap.type == mvsv::MAT_16SC1 && dMap.rows == H && dMap.cols == W, 32);
        // the C ABI call on the same pixels as whole images
        mvsv::Mat abi(H, W, mvsv::MAT_16SC1);
        mvsv_ctx* ctx = mvsv::thread_context();
        REQUIRE(mvsv_bm_census(ctx, wl.data, wl.step, wr.data, wr.step, W, H, &bm->p, abi.ptr<int16_t>(0),
                               abi.step / 2, 9, 7) == MVSV_OK, 33);
        REQUIRE(same(dMap, abi), 34);
        // the matcher that carries its window
        mvsv::Mat viaBin, abi55(H, W, mvsv::MAT_16SC1);
        Disparity::binary_bm(s, viaBin, bin);  // (5, 5)
        REQUIRE(mvsv_bm_census(ctx, wl.data, wl.step, wr.data, wr.step, W, H, &bin->p, abi55.ptr<int16_t>(0),
                               abi55.step / 2, 5, 5) == MVSV_OK, 35);
        REQUIRE(same(viaBin, abi55), 36);
        REQUIRE(!same(viaBin, dMap), 37);
        mvsv::Mat explicit55;
        Disparity::binary_bm(s, explicit55, bm, 5, 5);
        REQUIRE(same(explicit55, abi55), 38);
        // it is not the SAD map, and Disparity::bm on the same matcher afterwards still is
        mvsv::Mat sad, sad2(H, W, mvsv::MAT_16SC1);
        Disparity::bm(s, sad, bm);
        REQUIRE(mvsv_bm(ctx, wl.data, wl.step, wr.data, wr.step, W, H, &bm->p, sad2.ptr<int16_t>(0), sad2.step / 2) ==
                    MVSV_OK, 39);
        REQUIRE(same(sad, sad2) && !same(sad, dMap), 40);
        // a refused window throws with the rule's name
        REQUIRE(thrown(bm, lv, rv, 9, 9).find("census window") != std::string::npos, 41);

        std::FILE* f = std::fopen(argv[3], "wb");
        REQUIRE(f != nullptr, 50);
        for (int y = 0; y < H; y++) std::fwrite(dMap.ptr<int16_t>(y), 2, W, f);
        std::fclose(f);
        std::printf("gpu ok\n");
    } catch (const mvsv::Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
