// mvsv_prepare.hip — grey pair preparation on MI355X: what trgt/disparityTest.cpp
// does to an image between cv::imread and the matchers (:201-211):
//   cv::resize(img, img, Size(), 0.5, 0.5, INTER_AREA);  cv::cvtColor(img, img, BGR2GRAY);
// on interleaved 8-bit BGR, in one pass.  Per channel the halving is the rule of
// resize_linear_kernel's area2 branch (mvsv_post.hip, oracle: orc_resize_linear):
// (a+b+c+d+2) >> 2 on whole 2 x 2 blocks, the float mean rounded half to even on
// blocks clipped by an odd width or height.  Each channel is rounded to 8 bits
// before the grey conversion, as the two OpenCV calls do; the grey value is
// (B*1868 + G*9617 + R*4899 + 8192) >> 14 (MVSV_GRAY_Q14) or
// (B*3735 + G*19235 + R*9798 + 16384) >> 15 (MVSV_GRAY_Q15).  DESIGN.md §4l.
//
// Memory-bound (12 B read, 1 B written per output pixel when halving): a lane
// makes four output pixels from 24 (halving) or 12 (conversion alone) contiguous
// source bytes of a row, read as dwords where the source's base and strides are
// multiples of 4 and the four pixels are whole; bytes otherwise.  No LDS.
//
// Also here: stream_copy_kernel, which puts the frames of a device push
// (mvsv_stream_push_device) into the stream's slots, with the same dword / byte
// split by alignment.  DESIGN.md §4m.
#include "mvsv_device.hpp"
#include "mvsv_internal.hpp"

namespace mvsv {
namespace {

using namespace dev;

__device__ __forceinline__ int gray_of(int b, int g, int r, int q15)
{
    return q15 ? (b * 3735 + g * 19235 + r * 9798 + 16384) >> 15 : (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14;
}

// byte i of a row segment held as dwords (i is a constant after unrolling)
template <int N>
__device__ __forceinline__ int byte_of(const uint32_t (&w)[N], int i)
{
    return (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
}

// one channel of one halved pixel from the bytes themselves: the clipped-block
// rule included (sx0 < sw and sy0 < sh)
__device__ __forceinline__ int halve_narrow(const uint8_t* S, size_t ss, int sw, int sh, int sx0, int sy0, int c)
{
    const uint8_t* r = S + (size_t)sy0 * ss + 3 * (size_t)sx0 + c;
    if (sy0 + 2 <= sh && sx0 + 2 <= sw) return (r[0] + r[3] + r[ss] + r[ss + 3] + 2) >> 2;
    int sum = 0, cnt = 0;
    for (int yy = 0; yy < 2 && sy0 + yy < sh; yy++)
        for (int xx = 0; xx < 2 && sx0 + xx < sw; xx++) {
            sum += r[(size_t)yy * ss + 3 * xx];
            cnt++;
        }
    return clampi(__float2int_rn((float)sum / (float)cnt), 0, 255);
}

// wide: src, ss and sfs are multiples of 4 (the same for every lane)
template <bool HALVE>
__global__ __launch_bounds__(256) void bgr_gray_kernel(const uint8_t* __restrict__ src, size_t ss, size_t sfs, int sw,
                                                       int sh, int q15, int wide, uint8_t* __restrict__ dst,
                                                       size_t ds, size_t dfs, int dw, int dh)
{
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.z;
    if (x >= dw || y >= dh) return;
    const uint8_t* S = src + f * sfs;
    int v[4];
    if (HALVE) {
        // the four blocks are whole: both rows exist and source columns 2x .. 2x+7 do
        if (wide && 2 * y + 2 <= sh && 2 * x + 8 <= sw) {
            // 6 * x bytes into the row: a multiple of 8
            const uint32_t* p0 = reinterpret_cast<const uint32_t*>(S + (size_t)(2 * y) * ss + 6 * (size_t)x);
            const uint32_t* p1 = reinterpret_cast<const uint32_t*>(S + (size_t)(2 * y + 1) * ss + 6 * (size_t)x);
            uint32_t a[6], b[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                a[i] = p0[i];
                b[i] = p1[i];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int ch[3];
#pragma unroll
                for (int c = 0; c < 3; c++)
                    ch[c] = (byte_of(a, 6 * j + c) + byte_of(a, 6 * j + 3 + c) + byte_of(b, 6 * j + c) +
                             byte_of(b, 6 * j + 3 + c) + 2) >> 2;
                v[j] = gray_of(ch[0], ch[1], ch[2], q15);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                v[j] = 0;
                if (x + j < dw && 2 * (x + j) < sw && 2 * y < sh)
                    v[j] = gray_of(halve_narrow(S, ss, sw, sh, 2 * (x + j), 2 * y, 0),
                                   halve_narrow(S, ss, sw, sh, 2 * (x + j), 2 * y, 1),
                                   halve_narrow(S, ss, sw, sh, 2 * (x + j), 2 * y, 2), q15);
            }
        }
    } else {
        const uint8_t* r = S + (size_t)y * ss + 3 * (size_t)x;
        if (wide && x + 4 <= sw) {
            // 3 * x bytes into the row: a multiple of 4
            const uint32_t* p = reinterpret_cast<const uint32_t*>(r);
            const uint32_t a[3] = {p[0], p[1], p[2]};
#pragma unroll
            for (int j = 0; j < 4; j++)
                v[j] = gray_of(byte_of(a, 3 * j), byte_of(a, 3 * j + 1), byte_of(a, 3 * j + 2), q15);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = x + j < dw ? gray_of(r[3 * j], r[3 * j + 1], r[3 * j + 2], q15) : 0;
        }
    }
    uint8_t* d = dst + f * dfs + (size_t)y * ds + x;
    if (x + 3 < dw && ((uintptr_t)d & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d) =
            (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    } else {
        d[0] = (uint8_t)v[0];
        if (x + 1 < dw) d[1] = (uint8_t)v[1];
        if (x + 2 < dw) d[2] = (uint8_t)v[2];
        if (x + 3 < dw) d[3] = (uint8_t)v[3];
    }
}

// The halving alone, for the frames a stream matches in colour: a lane per output
// byte (consecutive lanes, consecutive bytes of an interleaved row), each from its
// channel's 2 x 2 block by halve_narrow's rules.
__global__ __launch_bounds__(256) void bgr_halve_kernel(const uint8_t* __restrict__ src, size_t ss, size_t sfs, int sw,
                                                        int sh, uint8_t* __restrict__ dst, size_t ds, size_t dfs,
                                                        int dw, int dh)
{
    const int b = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.z;
    if (b >= 3 * dw || y >= dh) return;
    const int x = b / 3, c = b - 3 * x;
    int v = 0;
    if (2 * x < sw && 2 * y < sh) v = halve_narrow(src + f * sfs, ss, sw, sh, 2 * x, 2 * y, c);
    dst[f * dfs + (size_t)y * ds + b] = (uint8_t)v;
}

// The frame stream's device push (mvsv_stream_push_device): rows of row_bytes bytes
// of both sides of n frames, from the caller's buffers into consecutive slots.
// blockIdx.z = 2 * frame + side; a block is 64 units of 4 rows.  A wide side moves
// a dword per lane (consecutive lanes, consecutive dwords) and the row's last
// row_bytes % 4 bytes one by one; any other side moves a byte per lane.  wide is
// the same for every lane of a block: source and destination base, row stride and
// frame stride are all multiples of 4.  Nothing outside [row, row + row_bytes) is
// read or written.
struct CopySide {
    const uint8_t* src;
    size_t ss, sfs;
    uint8_t* dst;
    int wide;
};

__global__ __launch_bounds__(256) void stream_copy_kernel(CopySide left, CopySide right, size_t ds, size_t dfs,
                                                          int row_bytes, int rows)
{
    const CopySide& s = (blockIdx.z & 1) ? right : left;
    const size_t f = blockIdx.z >> 1;
    const uint8_t* __restrict__ S = s.src + f * s.sfs;
    uint8_t* __restrict__ D = s.dst + f * dfs;
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int x = s.wide ? 4 * u : u;
    if (x >= row_bytes) return;
    for (int y = blockIdx.y * 4 + (threadIdx.x >> 6); y < rows; y += gridDim.y * 4) {
        const uint8_t* p = S + (size_t)y * s.ss + x;
        uint8_t* q = D + (size_t)y * ds + x;
        if (!s.wide) {
            *q = *p;
        } else if (x + 4 <= row_bytes) {
            *reinterpret_cast<uint32_t*>(q) = *reinterpret_cast<const uint32_t*>(p);
        } else {
            for (int k = 0; x + k < row_bytes; k++) q[k] = p[k];
        }
    }
}

}  // namespace

int stream_copy_device(mvsv_ctx* ctx, hipStream_t stream, int n, const uint8_t* L, size_t ls, size_t lfs,
                       const uint8_t* R, size_t rs, size_t rfs, uint8_t* dL, uint8_t* dR, size_t ds, size_t dfs,
                       int row_bytes, int rows)
{
    if (n < 1 || row_bytes < 1 || rows < 1 || ls < (size_t)row_bytes || rs < (size_t)row_bytes ||
        ds < (size_t)row_bytes)
        return set_error(ctx, MVSV_E_INVALID_ARG, "stream copy: empty frame or stride smaller than the row");
    if (n == 1) lfs = rfs = dfs = 0;  // unused, and no reason to leave the dword path
    const size_t dst_bits = ds | dfs;
    CopySide left{L, ls, lfs, dL, (((uintptr_t)L | ls | lfs | (uintptr_t)dL | dst_bits) & 3) == 0};
    CopySide right{R, rs, rfs, dR, (((uintptr_t)R | rs | rfs | (uintptr_t)dR | dst_bits) & 3) == 0};
    const int units = left.wide && right.wide ? (row_bytes + 3) / 4 : row_bytes;
    dim3 grid((units + 63) / 64, std::min((rows + 3) / 4, 65535), 2 * n);
    hipLaunchKernelGGL(stream_copy_kernel, grid, dim3(256), 0, stream, left, right, ds, dfs, row_bytes, rows);
    return check_hip(ctx, hipGetLastError(), "stream copy");
}

int prepare_size(int sw, int sh, int halve, int* dw, int* dh)
{
    if (halve != 0 && halve != 1) return MVSV_E_INVALID_ARG;
    if (halve) return resize_size(sw, sh, 0.5, 0.5, dw, dh);
    if (sw <= 0 || sh <= 0 || sw > 1 << 20 || sh > 1 << 20) return MVSV_E_INVALID_ARG;
    *dw = sw;
    *dh = sh;
    return MVSV_OK;
}

int halve_bgr_device(mvsv_ctx* ctx, int n, const uint8_t* bgr, size_t ss, size_t sfs, int sw, int sh, uint8_t* dst,
                     size_t ds, size_t dfs)
{
    int dw, dh;
    if (n < 1 || prepare_size(sw, sh, 1, &dw, &dh))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad prepare size or factor");
    if (ss < 3 * (size_t)sw || ds < 3 * (size_t)dw)
        return set_error(ctx, MVSV_E_INVALID_ARG, "prepare stride smaller than the row");
    dim3 grid((3 * dw + 63) / 64, (dh + 3) / 4, n);
    hipLaunchKernelGGL(bgr_halve_kernel, grid, dim3(256), 0, ctx->stream, bgr, ss, sfs, sw, sh, dst, ds, dfs, dw, dh);
    return check_hip(ctx, hipGetLastError(), "halve bgr");
}

int prepare_gray_device(mvsv_ctx* ctx, int n, const uint8_t* bgr, size_t ss, size_t sfs, int sw, int sh, int halve,
                        int variant, uint8_t* dst, size_t ds, size_t dfs)
{
    int dw, dh;
    if (prepare_size(sw, sh, halve, &dw, &dh)) return set_error(ctx, MVSV_E_INVALID_ARG, "bad prepare size or factor");
    if (variant != MVSV_GRAY_Q14 && variant != MVSV_GRAY_Q15)
        return set_error(ctx, MVSV_E_INVALID_ARG, "unknown grey variant");
    if (ss < 3 * (size_t)sw || ds < (size_t)dw)
        return set_error(ctx, MVSV_E_INVALID_ARG, "prepare stride smaller than the row");
    if (n == 1) sfs = dfs = 0;  // unused, and no reason to leave the packed path
    const int wide = (((uintptr_t)bgr | ss | sfs) & 3) == 0;
    dim3 grid((dw + 255) / 256, (dh + 3) / 4, n);
    if (halve)
        hipLaunchKernelGGL(bgr_gray_kernel<true>, grid, dim3(256), 0, ctx->stream, bgr, ss, sfs, sw, sh,
                           variant == MVSV_GRAY_Q15, wide, dst, ds, dfs, dw, dh);
    else
        hipLaunchKernelGGL(bgr_gray_kernel<false>, grid, dim3(256), 0, ctx->stream, bgr, ss, sfs, sw, sh,
                           variant == MVSV_GRAY_Q15, wide, dst, ds, dfs, dw, dh);
    return check_hip(ctx, hipGetLastError(), "prepare gray");
}

}  // namespace mvsv
