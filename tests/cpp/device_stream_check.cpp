// C++ check of the stream's device ends (include/mvsv_detection.hpp: pushDevice,
// popDevice, frontMapDevice, hostOutputs, fence), linked to libmvsv.so.
//   device_stream_check cpu             what needs no GPU: the bits and the null-handle answers
//   device_stream_check gpu <tmp dir>   seven frames through a ring of three from device
//                                       memory (single pushes and a batch over the ring's
//                                       end), compared with the same frames pushed from the
//                                       host; writes the frames and maps for the Python side
// The HIP runtime is the one libmvsv.so brought in: its allocation calls are looked up by name.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mvsv_detection.hpp"

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

static const int W = 101, H = 67, FRAMES = 7, DEPTH = 3;

using malloc_fn = int (*)(void**, size_t);
using memcpy_fn = int (*)(void*, const void*, size_t, int);
using free_fn = int (*)(void*);
using sync_fn = int (*)();

static bool dump(const std::string& path, const void* data, int rows, int cols, size_t elem)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "%d %d\n", rows, cols);
    std::fwrite(data, elem, (size_t)rows * cols, f);
    std::fclose(f);
    return true;
}

static int cpu_checks()
{
    REQUIRE((MVSV_HOST_MAP | MVSV_HOST_RECTIFIED | MVSV_HOST_DISPLAY | MVSV_HOST_VIEW) == MVSV_HOST_ALL);
    uint8_t px = 0;
    const int16_t* map = nullptr;
    const uint8_t* bytes = nullptr;
    REQUIRE(mvsv_stream_push_device(nullptr, 1, &px, 1, 1, &px, 1, 1, nullptr) == MVSV_E_INVALID_ARG);
    REQUIRE(mvsv_stream_push_raw_device(nullptr, 1, &px, 1, 1, &px, 1, 1, nullptr) == MVSV_E_INVALID_ARG);
    REQUIRE(mvsv_stream_push_bgr_device(nullptr, 1, &px, 3, 3, &px, 3, 3, nullptr) == MVSV_E_INVALID_ARG);
    REQUIRE(mvsv_stream_set_host_outputs(nullptr, MVSV_HOST_ALL) == MVSV_E_INVALID_ARG);
    REQUIRE(mvsv_stream_pop_device(nullptr, nullptr, 0, nullptr, nullptr) == MVSV_E_INVALID_ARG);
    REQUIRE(mvsv_stream_front_map_device(nullptr, &map, nullptr) == MVSV_E_INVALID_ARG);
    REQUIRE(mvsv_stream_front_rectified_device(nullptr, &bytes, &bytes) == MVSV_E_INVALID_ARG);
    REQUIRE(mvsv_stream_front_display_device(nullptr, &bytes, nullptr) == MVSV_E_INVALID_ARG);
    REQUIRE(mvsv_stream_front_view_device(nullptr, &bytes, nullptr) == MVSV_E_INVALID_ARG);
    REQUIRE(mvsv_stream_fence(nullptr, nullptr) == MVSV_E_INVALID_ARG);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_run(const std::string& tmp)
{
    auto m = mvsv::StereoSGBM::create(0, 32, 5, 200, 800, 1, 31, 10, 50, 2);
    const size_t px = (size_t)W * H;
    std::vector<uint8_t> L(px * FRAMES), R(px * FRAMES);
    for (int i = 0; i < FRAMES; i++)
        mvsv::check(mvsv_synth_pair(0xD0000u + i, W, H, 0, 32, L.data() + i * px, R.data() + i * px), nullptr);
    // host pushes: the maps to compare with
    std::vector<int16_t> want(px * FRAMES), got(px * FRAMES, 0), front(px, 0);
    mvsv::DisparityStream host(*m, W, H, DEPTH);
    for (int i = 0; i < FRAMES; i++) {
        mvsv::Mat l(H, W, mvsv::MAT_8UC1), r(H, W, mvsv::MAT_8UC1), d;
        for (int y = 0; y < H; y++) {
            std::memcpy(l.ptr<uint8_t>(y), L.data() + i * px + (size_t)y * W, W);
            std::memcpy(r.ptr<uint8_t>(y), R.data() + i * px + (size_t)y * W, W);
        }
        Stereopair pair(l, r);
        host.push(pair);
        host.pop(d);
        for (int y = 0; y < H; y++) std::memcpy(want.data() + i * px + (size_t)y * W, d.ptr<int16_t>(y), W * 2);
    }
    auto dmalloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
    auto dcopy = (memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    auto dfree = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
    auto dsync = (sync_fn)dlsym(RTLD_DEFAULT, "hipDeviceSynchronize");
    REQUIRE(dmalloc && dcopy && dfree && dsync);
    const int kH2D = 1, kD2H = 2;  // hipMemcpyHostToDevice, hipMemcpyDeviceToHost
    uint8_t *dL = nullptr, *dR = nullptr;
    int16_t* dOut = nullptr;
    REQUIRE(dmalloc((void**)&dL, L.size()) == 0 && dmalloc((void**)&dR, R.size()) == 0);
    REQUIRE(dmalloc((void**)&dOut, px * 2) == 0);
    REQUIRE(dcopy(dL, L.data(), L.size(), kH2D) == 0 && dcopy(dR, R.data(), R.size(), kH2D) == 0);
    {
        mvsv::DisparityStream st(*m, W, H, DEPTH);
        st.setBatch(2);
        st.hostOutputs(MVSV_HOST_ALL & ~MVSV_HOST_MAP);
        int popped = 0;
        // frames 0, 1 one by one; 2 .. 4 as a batch from slot 2 over the ring's end; 5, 6 as a batch
        auto pop_front = [&]() {  // zero copy, then pop without a map
            const int16_t* map = st.frontMapDevice();
            if (!map || dcopy(front.data(), map, px * 2, kD2H) != 0) return false;
            mvsv::Mat none;
            int code = 0;
            try {
                st.pop(none);  // the host map is switched off
            } catch (const mvsv::Error& e) {
                code = e.code();
            }
            if (code != MVSV_E_INVALID_ARG) return false;
            st.fence();
            return true;
        };
        auto pop_copy = [&]() {
            st.popDevice(dOut, W);
            const bool ok = dsync() == 0 && dcopy(got.data() + popped * px, dOut, px * 2, kD2H) == 0;
            popped++;
            return ok;
        };
        st.pushDevice(1, dL, W, 0, dR, W, 0);
        st.pushDevice(1, dL + px, W, 0, dR + px, W, 0);
        REQUIRE(st.pending() == 2);
        REQUIRE(pop_front());  // frame 0 read in place ...
        REQUIRE(st.pending() == 2);
        REQUIRE(pop_copy());   // ... and popped through popDevice
        REQUIRE(pop_copy());
        REQUIRE(st.pending() == 0 && popped == 2);
        st.pushDevice(3, dL + 2 * px, W, px, dR + 2 * px, W, px);
        REQUIRE(st.pending() == 3);
        int code = 0;
        try {
            st.pushDevice(1, dL, W, 0, dR, W, 0);  // full
        } catch (const mvsv::Error& e) {
            code = e.code();
        }
        REQUIRE(code == MVSV_E_INVALID_ARG && st.pending() == 3);
        REQUIRE(pop_copy() && pop_copy());
        st.pushDevice(2, dL + 5 * px, W, px, dR + 5 * px, W, px);
        while (st.pending()) REQUIRE(pop_copy());
        REQUIRE(popped == FRAMES);
        code = 0;
        try {
            st.pushDevice(DEPTH + 1, dL, W, px, dR, W, px);  // more than the ring holds
        } catch (const mvsv::Error& e) {
            code = e.code();
        }
        REQUIRE(code == MVSV_E_INVALID_ARG && st.pending() == 0);
    }
    REQUIRE(dfree(dL) == 0 && dfree(dR) == 0 && dfree(dOut) == 0);
    for (int i = 0; i < FRAMES; i++)
        if (std::memcmp(got.data() + i * px, want.data() + i * px, px * 2) != 0) {
            std::fprintf(stderr, "frame %d: the map from device pushes differs from the host pushes' map\n", i);
            return 1;
        }
    REQUIRE(std::memcmp(front.data(), want.data(), px * 2) == 0);  // frontMapDevice saw frame 0
    REQUIRE(std::memcmp(want.data(), want.data() + px, px * 2) != 0);  // an order mix-up would show
    REQUIRE(dump(tmp + "/left.bin", L.data(), FRAMES * H, W, 1) && dump(tmp + "/right.bin", R.data(), FRAMES * H, W, 1) &&
            dump(tmp + "/disp.bin", got.data(), FRAMES * H, W, 2));
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s cpu | gpu <tmp dir>\n", argv[0]);
        return 2;
    }
    if (!std::strcmp(argv[1], "cpu")) return cpu_checks();
    if (argc < 3) return 2;
    try {
        return gpu_run(argv[2]);
    } catch (const mvsv::Error& e) {
        std::fprintf(stderr, "mvsv::Error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
