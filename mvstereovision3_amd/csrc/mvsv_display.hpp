// mvsv_display.hpp — the display byte of cv::normalize(NORM_MINMAX, CV_8U), shared
// by the kernels that write it: normalize_u8_kernel (mvsv_post.hip) and
// view_kernel (mvsv_view.hip).  One definition, so both give the same bytes.
#pragma once

#include <cfloat>

#include "mvsv_device.hpp"

namespace mvsv {
namespace dev {

__device__ __forceinline__ int wave_max_i32(int v)
{
    v = row_max_i32(v);
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return max(max(a, b), max(c, d));
}

// a frame's nblk <= 64 partial pairs folded by one (whole) wave; wave-uniform result
__device__ __forceinline__ void fold_partials(const int2* __restrict__ partials, int f, int nblk, int lane, int& lo,
                                              int& hi)
{
    int2 p = make_int2(32767, -32768);
    if (lane < nblk) p = partials[(size_t)f * nblk + lane];
    lo = wave_min_i32(p.x);
    hi = wave_max_i32(p.y);
}

// OpenCV 3.4's arithmetic (normalize -> Mat::convertTo, CV_16S -> CV_8U, SSE2 /
// scalar form): scale and shift in double, every operation rounded on its own;
// then per pixel a float product and a float sum, each rounded, and a convert
// with round-half-to-even and saturation.  The library is built with the
// compiler's default contraction, which would fuse smin * scale into the
// subtraction and the pixel's product into its sum (the rounding intrinsics
// are plain operators once inlined): contraction is off in these two functions.
__device__ __forceinline__ void display_scale(int smin, int smax, double dmin, double dmax, float& sf, float& hf)
{
#pragma clang fp contract(off)
    const double range = (double)smax - (double)smin;
    const double recip = range > DBL_EPSILON ? 1.0 / range : 0.0;
    const double scale = (dmax - dmin) * recip;
    const double prod = (double)smin * scale;
    const double shift = dmin - prod;
    sf = (float)scale;
    hf = (float)shift;
}

__device__ __forceinline__ uint32_t display_u8(int v, float sf, float hf)
{
#pragma clang fp contract(off)
    const float p = (float)v * sf;
    const float t = p + hf;
    return (uint32_t)clampi(__float2int_rn(t), 0, 255);
}

}  // namespace dev
}  // namespace mvsv
