// mvsv_census.hip — the census transform on MI355X (gfx950).
//
// The descriptor of mvsv_sgbm_census: for an 8-bit image I and an
// odd cw x ch window (3 <= cw * ch <= 65), the window offsets run dy = -ch/2 .. ch/2
// outside and dx = -cw/2 .. cw/2 inside, the centre is skipped, and bit k of T(y, x)
// is 1 iff the k-th offset's pixel, clamped into the image, is darker than I(y, x).
// One u64 per pixel, the bits above cw * ch - 1 zero: exactly the word the LDS-ring
// cost kernel stages per pixel, so the SGBM pipeline writes the descriptors of both
// views into its `pre` planes [frame][2][H][W] and nothing after the pixel cost
// changes (mvsv_cost.hip sgbm_cost_census_kernel).
#include "mvsv_device.hpp"
#include "mvsv_internal.hpp"

namespace mvsv {
namespace {

using namespace dev;

// Block = 256 threads owns kCensusTW x kCensusTH descriptors of one view of one
// frame.  The (TH + ch - 1) x (TW + cw - 1) source bytes around them, clamped
// into the image, go into LDS with byte loads that are contiguous along a row
// (row-strided sources, any base address); thread (ty, tx) then produces the
// run of kCensusRun columns tx * 4 .. tx * 4 + 3 of tile row ty: it walks the
// ch x (cw + 3) bytes its four windows cover once, and every byte feeds the
// up-to-four windows it lies in: the first and last three bytes of a row and
// the centres' row test which (wave-uniform, so scalar branches), the bytes in
// between lie in all four.  A window sees its offsets in the contract's order,
// so each descriptor is shifted in from the bottom (first offset ends highest)
// and bit-reversed once at the end.
constexpr int kCensusTW = 128, kCensusTH = 8, kCensusRun = 4;
static_assert(kCensusTW / kCensusRun * kCensusTH == 256, "one run per thread");

__global__ __launch_bounds__(256) void census_kernel(const uint8_t* __restrict__ L, size_t ls, size_t lfs,
                                                     const uint8_t* __restrict__ R, size_t rs, size_t rfs,
                                                     int nimg, int W, int H, int cw, int ch,
                                                     uint64_t* __restrict__ out, size_t ors, size_t ois, size_t ofs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int hx = cw >> 1, hy = ch >> 1;
    const int pitch = kCensusTW + cw - 1, rows = kCensusTH + ch - 1;
    const int x0 = blockIdx.x * kCensusTW, y0 = blockIdx.y * kCensusTH;
    const int f = blockIdx.z / nimg, img = blockIdx.z - f * nimg;  // 0 = left, 1 = right
    const uint8_t* base = img == 0 ? L + f * lfs : R + f * rfs;
    const size_t st = img == 0 ? ls : rs;
    const int tid = threadIdx.x;
    for (int i = tid; i < rows * pitch; i += 256) {
        const int r = i / pitch, c = i - r * pitch;
        const int sy = clampi(y0 - hy + r, 0, H - 1), sx = clampi(x0 - hx + c, 0, W - 1);
        smem[i] = base[(size_t)sy * st + sx];
    }
    __syncthreads();
    const int ty = tid >> 5, tx = (tid & 31) * kCensusRun;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
    // window row 0, window column 0 of the run's first pixel
    const unsigned char* win = smem + ty * pitch + tx;
    uint32_t cen[kCensusRun];
    uint64_t t[kCensusRun];
#pragma unroll
    for (int i = 0; i < kCensusRun; i++) {
        cen[i] = win[hy * pitch + hx + i];
        t[i] = 0;
    }
    for (int r = 0; r < ch; r++) {
        const unsigned char* wr = win + r * pitch;
        const bool crow = r == hy;  // the row that holds the centres
        // byte c of the row, fed to the windows it lies in (all wave-uniform tests)
        auto some = [&](int c) {
            const uint32_t b = wr[c];
#pragma unroll
            for (int i = 0; i < kCensusRun; i++) {
                const int dx = c - i;  // window column of byte c in pixel i's window
                if (dx >= 0 && dx < cw && !(crow && dx == hx)) t[i] = (t[i] << 1) | (uint64_t)(b < cen[i]);
            }
        };
        if (crow || cw < kCensusRun) {
            for (int c = 0; c < cw + kCensusRun - 1; c++) some(c);
            continue;
        }
        // bytes kCensusRun - 1 .. cw - 1 lie in all four windows, and none is a centre
#pragma unroll
        for (int c = 0; c < kCensusRun - 1; c++) some(c);
        for (int c = kCensusRun - 1; c < cw; c++) {
            const uint32_t b = wr[c];
#pragma unroll
            for (int i = 0; i < kCensusRun; i++) t[i] = (t[i] << 1) | (uint64_t)(b < cen[i]);
        }
#pragma unroll
        for (int c = 0; c < kCensusRun - 1; c++) some(cw + c);
    }
    const int bits = cw * ch - 1;  // 2 .. 64
    uint64_t* o = out + f * ofs + img * ois + (size_t)y * ors + x;
#pragma unroll
    for (int i = 0; i < kCensusRun; i++)
        if (x + i < W) o[i] = __brevll(t[i]) >> (64 - bits);
}

}  // namespace

const char* census_window_check(int cw, int ch)
{
    if (cw <= 0 || ch <= 0 || cw % 2 == 0 || ch % 2 == 0)
        return "census window: width and height must be odd and positive";
    if ((long)cw * ch < 3 || (long)cw * ch > 65)
        return "census window: 3 <= width * height <= 65 (a descriptor of at most 64 bits)";
    return nullptr;
}

int census_device(mvsv_ctx* ctx, int n, int nimg, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                  size_t rs, size_t rfs, int W, int H, int cw, int ch, uint64_t* out, size_t ors, size_t ois,
                  size_t ofs)
{
    if (const char* why = census_window_check(cw, ch)) return set_error(ctx, MVSV_E_INVALID_ARG, why);
    if ((long)n * nimg > 65535) return set_error(ctx, MVSV_E_INVALID_ARG, "census: too many frames in one launch");
    const size_t lds = (size_t)(kCensusTH + ch - 1) * (kCensusTW + cw - 1);  // <= 72 * 128 bytes
    const dim3 grid((W + kCensusTW - 1) / kCensusTW, (H + kCensusTH - 1) / kCensusTH, n * nimg);
    if (grid.y > 65535) return set_error(ctx, MVSV_E_INVALID_ARG, "census: image too tall");
    StageTimer tm(ctx, kStagePre);
    hipLaunchKernelGGL(census_kernel, grid, dim3(256), lds, ctx->stream, L, ls, lfs, R, rs, rfs, nimg, W, H, cw, ch,
                       out, ors, ois, ofs);
    return check_hip(ctx, hipGetLastError(), "census transform");
}

}  // namespace mvsv
