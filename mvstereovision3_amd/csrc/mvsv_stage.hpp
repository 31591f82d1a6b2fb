// mvsv_stage.hpp — staging of the host-pointer calls: one frame goes up into the
// context's arena, the _device call runs on it with n = 1, the result comes down.
// The layout part is free of HIP, so the CPU suite checks every call's reservation
// under ASan + UBSan: a StageLayout hands out slices, one struct per call shape names
// them.  The device part (HIP builds only): the one grow-only buffer, the copies on
// the context stream, the wait, and the last-use event.
#pragma once

#include <cassert>
#include <cstddef>

namespace mvsv {

constexpr size_t kStageAlign = 256;  // every slice starts on such a boundary
constexpr int kStageMaxSlices = 5;
// row alignments (bytes) the kernels' packed paths ask for
constexpr size_t kRowTight = 1;
constexpr size_t kRow4 = 4;        // u8 rows read as 32-bit words: sharpness, BGR prepare
constexpr size_t kRow8xI16 = 16;   // int16 rows 8 elements apart: display, view, cloud maps
constexpr size_t kRow8xU8 = 8;     // u8 rows as many bytes apart as such a map's rows have elements

struct StageSlice {
    size_t off = 0, bytes = 0;            // where in the arena
    size_t pitch = 0;                     // bytes from one row to the next
    size_t row_bytes = 0, row_align = 1;  // what the pitch was made from
};

struct StageLayout {
    StageSlice slice[kStageMaxSlices];
    int count = 0;
    size_t total = 0;  // bytes of arena the slices need

    StageSlice image(size_t rows, size_t row_bytes, size_t row_align = kRowTight)
    {
        assert(count < kStageMaxSlices && row_align > 0);
        const size_t pitch = (row_bytes + row_align - 1) / row_align * row_align;
        const StageSlice s{total, rows * pitch, pitch, row_bytes, row_align};
        total = (s.off + s.bytes + kStageAlign - 1) / kStageAlign * kStageAlign;
        return slice[count++] = s;
    }
    StageSlice linear(size_t bytes) { return image(1, bytes); }
};

// One struct per call shape: its slices, reserved in this order.
// mvsv_sgbm / mvsv_sgbm_bgr / mvsv_bm (cn bytes per input pixel, int16 map: out_elem 2)
// and mvsv_tm (cn 1, u8 map: out_elem 1)
struct PairStage : StageLayout {
    StageSlice left, right, out;
    PairStage(size_t W, size_t H, size_t cn, size_t out_elem)
        : left(image(H, W * cn)), right(image(H, W * cn)), out(image(H, W * out_elem)) {}
};
// mvsv_mean_disparity_grid (81 means) and mvsv_samplepoint_values (nx * ny values)
struct MapFloatsStage : StageLayout {
    StageSlice map, floats;
    MapFloatsStage(size_t W, size_t H, size_t n) : map(image(H, W * 2)), floats(linear(n * 4)) {}
};
// mvsv_normalize_minmax
struct NormalizeStage : StageLayout {
    StageSlice map, out, minmax;
    NormalizeStage(size_t W, size_t H) : map(image(H, W * 2, kRow8xI16)), out(image(H, W, kRow8xU8)), minmax(linear(4)) {}
};
// mvsv_view: 81 tile means, npts sample values (0 without FOUND_POINTS)
struct ViewStage : StageLayout {
    StageSlice map, out, minmax, means, values;
    ViewStage(size_t W, size_t H, size_t npts)
        : map(image(H, W * 2, kRow8xI16)), out(image(H, 3 * W)), minmax(linear(4)),
          means(linear(81 * 4)), values(linear(npts * 4)) {}
};
// mvsv_point_cloud / mvsv_dmap2pcl: a (count, min, max) header, then 16-byte records: as
// many as the caller has room for, and no more than the map has pixels
struct CloudStage : StageLayout {
    StageSlice map, header, records;
    CloudStage(size_t W, size_t H, size_t capacity)
        : map(image(H, W * 2, kRow8xI16)), header(linear(12)),
          records(linear((capacity < W * H ? capacity : W * H) * 16)) {}
};
// mvsv_resize (rows of sw bytes, tight) and mvsv_prepare_gray (3 sw bytes, kRow4): u8 dw x dh out
struct ImageStage : StageLayout {
    StageSlice in, out;
    ImageStage(size_t sh, size_t row, size_t align, size_t dw, size_t dh)
        : in(image(sh, row, align)), out(image(dh, dw)) {}
};
// mvsv_rectify_pair (nmap = 4 W H map floats) and mvsv_undistort_pair (0: its maps are cached apart):
// [2][H][W] inputs, and [2][H][W] outputs of their own, so in-place calls are safe
struct RemapStage : StageLayout {
    StageSlice src, dst, maps;
    RemapStage(size_t W, size_t H, size_t nmap) : src(image(2 * H, W)), dst(image(2 * H, W)), maps(linear(nmap * 4)) {}
};
// mvsv_sharpness: the 64-bit sum behind the image
struct SharpnessStage : StageLayout {
    StageSlice img, sum;
    SharpnessStage(size_t W, size_t H) : img(image(H, W, kRow4)), sum(linear(8)) {}
};

}  // namespace mvsv

#ifdef __HIPCC__
#include "mvsv_internal.hpp"

namespace mvsv {

// The arena of one host-pointer call, ctx->stage: nothing is kept from call to call
// but the buffer, and every copy runs on ctx->stream.
struct Staging {
    mvsv_ctx* ctx;

    template <typename T>
    T* at(const StageSlice& s) const
    {
        assert(s.off + s.bytes <= ctx->stage.bytes);
        return (T*)((char*)ctx->stage.ptr + s.off);
    }
    // rows of row_bytes bytes, pitches in bytes
    int up(void* dev, size_t dpitch, const void* host, size_t hpitch, size_t row_bytes, size_t rows, const char* what)
    {
        return check_hip(ctx, hipMemcpy2DAsync(dev, dpitch, host, hpitch, row_bytes, rows, hipMemcpyHostToDevice,
                                               ctx->stream), what);
    }
    int up(void* dev, const void* host, size_t bytes, const char* what)
    {
        return check_hip(ctx, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream), what);
    }
    int down(void* host, size_t hpitch, const void* dev, size_t dpitch, size_t row_bytes, size_t rows, const char* what)
    {
        return check_hip(ctx, hipMemcpy2DAsync(host, hpitch, dev, dpitch, row_bytes, rows, hipMemcpyDeviceToHost,
                                               ctx->stream), what);
    }
    int down(void* host, const void* dev, size_t bytes, const char* what)
    {
        return check_hip(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream), what);
    }
    // the host may read what came down; a call may finish more than once
    int finish() { return check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"); }
};

// One host-pointer call: grows the arena to lay through ensure() (`what` names it in an
// allocation error), runs body(staging), and on every exit records the context's
// last-use event behind what was enqueued, so that a later stream switch waits for it.
template <typename Body>
int staged_call(mvsv_ctx* ctx, const StageLayout& lay, const char* what, Body&& body)
{
    Staging sg{ctx};
    int rc = ensure(ctx, ctx->stage, lay.total, what);
    if (!rc) rc = body(sg);
    return mark_last_use(ctx, rc);
}

}  // namespace mvsv
#endif  // __HIPCC__
