// mvsv_convert_maps under AddressSanitizer + UBSan (built with mvsv_io.cpp by
// tests/test_raw_stream_host.py): exact-size heap buffers, so a read or write past a
// row or past the last row is reported; results against the definition in integers.
#include <cmath>
#include <cstdio>
#include <vector>

#include "mvsv.h"

static int check(int W, int H, size_t ms, size_t xs, size_t fs, float scale)
{
    // exact sizes: the last row holds W entries only
    std::vector<float> mx((size_t)(H - 1) * ms + W), my(mx.size());
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            // multiples of 1/64: every other one is a tie of the rounding to 1/32
            mx[(size_t)y * ms + x] = scale * (float)(((x * 37 + y * 11) % 4001) - 2000) / 64.0f;
            my[(size_t)y * ms + x] = scale * (float)(((x * 13 + y * 29) % 3001) - 1500) / 64.0f;
        }
    std::vector<int16_t> xy(((size_t)(H - 1) * xs + W) * 2, 7);
    std::vector<uint16_t> frac((size_t)(H - 1) * fs + W, 9);
    if (mvsv_convert_maps(mx.data(), my.data(), ms, W, H, xy.data(), xs, frac.data(), fs) != MVSV_OK) return 1;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const long X = std::lrintf(mx[(size_t)y * ms + x] * 32.0f), Y = std::lrintf(my[(size_t)y * ms + x] * 32.0f);
            // floor division and non-negative remainder, without shifts of negatives
            const long qx = (X - ((X % 32 + 32) % 32)) / 32, qy = (Y - ((Y % 32 + 32) % 32)) / 32;
            const long sx = qx < -32768 ? -32768 : qx > 32767 ? 32767 : qx;
            const long sy = qy < -32768 ? -32768 : qy > 32767 ? 32767 : qy;
            const long fr = ((Y % 32 + 32) % 32) * 32 + (X % 32 + 32) % 32;
            if (xy[((size_t)y * xs + x) * 2] != sx || xy[((size_t)y * xs + x) * 2 + 1] != sy ||
                frac[(size_t)y * fs + x] != fr) {
                std::fprintf(stderr, "mismatch at (%d, %d) of %d x %d\n", x, y, W, H);
                return 1;
            }
        }
    // padding between rows stays untouched
    for (int y = 0; y + 1 < H; y++) {
        for (size_t x = W; x < xs; x++)
            if (xy[((size_t)y * xs + x) * 2] != 7 || xy[((size_t)y * xs + x) * 2 + 1] != 7) return 1;
        for (size_t x = W; x < fs; x++)
            if (frac[(size_t)y * fs + x] != 9) return 1;
    }
    return 0;
}

int main()
{
    int failures = 0;
    failures += check(1, 1, 1, 1, 1, 1.0f);
    failures += check(203, 125, 203, 203, 203, 1.0f);
    failures += check(181, 108, 203, 184, 184, 1.0f);  // a ROI of wider maps into padded rows
    failures += check(13, 7, 17, 16, 21, 1.0f);
    failures += check(64, 5, 64, 64, 64, 1500.0f);     // far past the short's range: saturation
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
