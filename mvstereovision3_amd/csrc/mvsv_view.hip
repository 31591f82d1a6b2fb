// mvsv_view.hip — the detection view on MI355X: the annotated BGR frame the
// reference's detection programs show (trgt/demo.cpp:280-298 and the other loops):
//   cv::normalize(dMap, norm, 0, 255, NORM_MINMAX, CV_8U); cv::cvtColor(GRAY2BGR);
//   View::drawSubimageGrid / drawObstacleGrid (src/view.cpp); drawFoundObstacles
//   (filled red tiles of MeanDisparityDetection, filled red circles of
//   SamplepointDetection).
// One pass from the int16 row to the BGR row, written as a gather: every pixel
// derives its display byte and then asks which layers cover it, so every output
// byte is written exactly once and the layer order is arithmetic.  The drawing
// rules are stated in include/mvsv.h and DESIGN.md §4k.
#include <algorithm>
#include <cmath>

#include "mvsv_device.hpp"
#include "mvsv_display.hpp"
#include "mvsv_internal.hpp"

namespace mvsv {
namespace {

using namespace dev;

constexpr int kViewRows = 8;         // rows per block (two per wave), as normalize_u8_kernel
constexpr uint32_t kSubMask = 0x1B6; // k in {1, 2, 4, 5, 7, 8} of drawSubimageGrid
constexpr uint32_t kRed = 0xFF0000u, kGridBlue = 100u;  // B | G << 8 | R << 16

// What a launch draws, the same for every wave.  A layer that is off has values
// that never match (line positions -1, masks 0, no lattice rows).
struct ViewGeom {
    int dx, dy;              // tile size W / 9, H / 9 (also the subimage grid's step)
    uint32_t sub_mask;       // kSubMask, or 0
    int ox1, ox2, oy1, oy2;  // obstacle grid lines, or -1
    int tiles;               // FOUND_TILES
    float tile_first, tile_second;
    int sx, sy, nx, ny;      // lattice (ny = 0: FOUND_POINTS off or no point)
    int pwords;              // 32-bit words of one lattice row's found bits in LDS (even)
    int radius;
    uint32_t half_widths;    // cv::circle's half-width per row offset 0..3, 4 bits each
    float point_first, point_second;
};

// Where pixel x stands among the columns: its tile and lattice cell.
struct ColPos {
    int c, rem;  // x = c * dx + rem
    int pc, q;   // x + 3 = pc * sx + q: q - 3 is the offset from centre pc * sx
    __device__ __forceinline__ void at(int x, const ViewGeom& g)
    {
        c = x / g.dx;
        rem = x - c * g.dx;
        pc = (x + 3) / g.sx;
        q = x + 3 - pc * g.sx;
    }
    __device__ __forceinline__ void next(const ViewGeom& g)
    {
        if (++rem == g.dx) {
            rem = 0;
            c++;
        }
        if (++q == g.sx) {
            q = 0;
            pc++;
        }
    }
};

// What row y contributes, wave-uniform.
struct RowState {
    bool red;            // an obstacle grid row
    bool blue;           // a subimage grid row
    uint32_t tile_cols;  // tile columns found in the (at most two) tile rows that cover y
    int prow;            // lattice row 1..ny whose circles reach y, or 0
    int half;            // their half-width in this row
    const uint32_t* pts; // that lattice row's found bits (LDS), bit c - 1 for lattice column c
};

// is lattice column pc (1..nx) of the row found
__device__ __forceinline__ bool point_found(const RowState& r, int pc, int nx)
{
    const int c = pc - 1;
    return c >= 0 && c < nx && ((r.pts[c >> 5] >> (c & 31)) & 1u) != 0;
}

// B | G << 8 | R << 16 of pixel x, display byte b.  Layers in order, each over
// the ones before: grey, subimage grid, then red for the obstacle grid, a found
// tile or a found point -- the three red layers cannot be told apart.
// point: the lattice column p.pc of r.prow is found.
__device__ __forceinline__ uint32_t view_pixel(int x, uint32_t b, const ColPos& p, const RowState& r,
                                               const ViewGeom& g, bool point)
{
    const int c = min(p.c, 31);
    bool red = r.red | (x == g.ox1) | (x == g.ox2);
    // tile c covers x; tile c - 1 too where x is its inclusive right edge
    red |= ((r.tile_cols >> c) & 1u) != 0;
    red |= p.rem == 0 && c >= 1 && ((r.tile_cols >> (c - 1)) & 1u) != 0;
    red |= point && abs(p.q - 3) <= r.half;
    const bool blue = r.blue | (p.rem == 0 && ((g.sub_mask >> c) & 1u) != 0);
    return red ? kRed : blue ? kGridBlue : b * 0x010101u;
}

__device__ __forceinline__ void store_bgr(uint8_t* o, uint32_t p)
{
    o[0] = (uint8_t)p;
    o[1] = (uint8_t)(p >> 8);
    o[2] = (uint8_t)(p >> 16);
}

// The 24 output bytes of the 8 pixels of one 16-byte load, x0 the first pixel, as 6
// little-endian dwords.
__device__ __forceinline__ void view_group(const uint4 q, int x0, const RowState& r, const ViewGeom& g, float sf,
                                           float hf, uint32_t d[6])
{
    const int v[8] = {lo16(q.x), hi16(q.x), lo16(q.y), hi16(q.y), lo16(q.z), hi16(q.z), lo16(q.w), hi16(q.w)};
    uint32_t c[8];
    ColPos p;
    p.at(x0, g);
    // 8 pixels meet at most two lattice columns (sx >= 8): the first pixel's and the next
    const int pc0 = p.pc;
    const bool pt0 = r.prow && point_found(r, pc0, g.nx), pt1 = r.prow && point_found(r, pc0 + 1, g.nx);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        c[k] = view_pixel(x0 + k, display_u8(v[k], sf, hf), p, r, g, p.pc == pc0 ? pt0 : pt1);
        p.next(g);
    }
    d[0] = c[0] | c[1] << 24;
    d[1] = c[1] >> 8 | c[2] << 16;
    d[2] = c[2] >> 16 | c[3] << 8;
    d[3] = c[4] | c[5] << 24;
    d[4] = c[5] >> 8 | c[6] << 16;
    d[5] = c[6] >> 16 | c[7] << 8;
}

// ... stored straight from the lane that made them, in pieces of w = 8, 4, 2 or 1 bytes
__device__ __forceinline__ void store_group(uint8_t* t, const uint32_t d[6], int w)
{
    if (w == 8) {
        ((uint2*)t)[0] = make_uint2(d[0], d[1]);
        ((uint2*)t)[1] = make_uint2(d[2], d[3]);
        ((uint2*)t)[2] = make_uint2(d[4], d[5]);
    } else if (w == 4) {
#pragma unroll
        for (int k = 0; k < 6; k++) ((uint32_t*)t)[k] = d[k];
    } else if (w == 2) {
#pragma unroll
        for (int k = 0; k < 6; k++) {
            ((uint16_t*)t)[2 * k] = (uint16_t)d[k];
            ((uint16_t*)t)[2 * k + 1] = (uint16_t)(d[k] >> 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 24; k++) t[k] = (uint8_t)(d[k >> 2] >> (8 * (k & 3)));
    }
}

// LDS written by some lanes of a wave is read by others of the same wave: the
// wave's LDS operations run in order, the compiler must keep them so.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Block (tile, frame): kViewRows rows of a frame.  Wave 0 folds the frame's
// min / max partials and derives (sf, hf); nine lanes of wave 1 turn the frame's
// 81 means into one found mask per tile row; all waves turn the (at most two)
// lattice rows whose circles reach the block's rows into found bits, once, so
// that no pixel reads a value from global memory.  A row is walked like
// normalize_u8_kernel: head pixels, packed groups of 8 pixels from one 16-byte
// load (24 output bytes, stored in pieces of store_w bytes by the alignment of
// out + 3 * head and of the output strides; with 16-byte alignment a wave's pass
// goes through LDS so that neighbouring lanes store neighbouring 16-byte pieces
// instead of 24-byte strides), tail pixels.
__global__ __launch_bounds__(256) void view_kernel(const int16_t* __restrict__ dmap, size_t st, size_t fs, int W, int H,
                                                   int head, int nvec, const int2* __restrict__ partials, int nblk,
                                                   double dmin, double dmax, ViewGeom g,
                                                   const float* __restrict__ means, const float* __restrict__ values,
                                                   uint8_t* __restrict__ out, size_t os, size_t ofs, int store_w,
                                                   int16_t* __restrict__ minmax)
{
    __shared__ float s_sf, s_hf;
    __shared__ uint32_t s_tile[9];
    __shared__ __attribute__((aligned(16))) uint32_t s_out[4][6 * 64];  // a wave's pass of 64 groups x 24 bytes
    extern __shared__ uint32_t s_pts[];  // [2][g.pwords]: lattice rows pr0 and pr0 + 1
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), f = blockIdx.y;
    if (w == 0) {
        int lo, hi;
        fold_partials(partials, f, nblk, lane, lo, hi);
        if (lane == 0) {
            float sf, hf;
            display_scale(lo, hi, dmin, dmax, sf, hf);
            s_sf = sf;
            s_hf = hf;
            if (minmax && blockIdx.x == 0) {
                minmax[2 * f] = (int16_t)lo;
                minmax[2 * f + 1] = (int16_t)hi;
            }
        }
    } else if (w == 1 && lane < 9) {
        uint32_t m = 0;
        if (g.tiles) {
            const float* mf = means + (size_t)f * 81 + lane * 9;
            for (int c = 0; c < 9; c++) m |= (mf[c] < g.tile_first && mf[c] > g.tile_second) ? 1u << c : 0u;
        }
        s_tile[lane] = m;
    }
    // rows y0 .. y0 + 7 reach lattice rows (y + 3) / sy: pr0 or pr0 + 1, as sy >= 8
    const int pr0 = ((int)blockIdx.x * kViewRows + 3) / g.sy;
    if (g.ny > 0) {
        const float* vals = values + (size_t)f * g.nx * g.ny;
        for (int k = 0; k < 2; k++) {
            const int pr = pr0 + k;
            const bool row_ok = pr >= 1 && pr <= g.ny;
            for (int c0 = 0; c0 < g.pwords * 32; c0 += 256) {
                const int c = c0 + (int)threadIdx.x;
                bool found = false;
                if (row_ok && c < g.nx) {
                    const float v = vals[(size_t)c * g.ny + (pr - 1)];
                    found = v < g.point_first && v > g.point_second;
                }
                const unsigned long long m = __ballot(found);
                const int word = (c0 + w * 64) >> 5;
                if (lane == 0 && word < g.pwords) {
                    s_pts[k * g.pwords + word] = (uint32_t)m;
                    s_pts[k * g.pwords + word + 1] = (uint32_t)(m >> 32);
                }
            }
        }
    }
    __syncthreads();
    const float sf = s_sf, hf = s_hf;
    const int tail0 = head + nvec * 8;
    const int y1 = min(H, ((int)blockIdx.x + 1) * kViewRows);
    for (int y = blockIdx.x * kViewRows + w; y < y1; y += 4) {
        RowState r;
        const int ty = y / g.dy, trem = y - ty * g.dy;
        r.red = y == g.oy1 || y == g.oy2;
        r.blue = trem == 0 && ((g.sub_mask >> min(ty, 31)) & 1u) != 0;
        // tile row ty covers y; tile row ty - 1 too where y is its inclusive bottom edge
        r.tile_cols = (ty <= 8 ? s_tile[ty] : 0u) | (trem == 0 && ty >= 1 && ty <= 9 ? s_tile[ty - 1] : 0u);
        r.prow = 0;
        r.half = 0;
        r.pts = s_pts;
        if (g.ny > 0) {
            const int pr = (y + 3) / g.sy, off = abs(y + 3 - pr * g.sy - 3);
            if (pr >= 1 && pr <= g.ny && off <= g.radius) {
                r.prow = pr;
                r.half = (int)((g.half_widths >> (4 * off)) & 15u);
                r.pts = s_pts + (pr - pr0) * g.pwords;
            }
        }
        const int16_t* in = dmap + f * fs + (size_t)y * st;
        uint8_t* o = out + f * ofs + (size_t)y * os;
        ColPos p;
        for (int x = lane; x < head; x += 64) {
            p.at(x, g);
            store_bgr(o + 3 * (size_t)x,
                      view_pixel(x, display_u8(in[x], sf, hf), p, r, g, r.prow && point_found(r, p.pc, g.nx)));
        }
        const uint4* rv = (const uint4*)(in + head);
        for (int j0 = 0; j0 < nvec; j0 += 64) {  // a pass: up to 64 groups, one per lane
            const int j = j0 + lane;
            uint8_t* pass = o + 3 * (size_t)(head + j0 * 8);
            if (j < nvec) {
                uint32_t d[6];
                view_group(rv[j], head + j * 8, r, g, sf, hf, d);
                if (store_w == 16) {  // into the wave's LDS row, stored below
                    uint2* l = (uint2*)(s_out[w] + 6 * lane);
                    l[0] = make_uint2(d[0], d[1]);
                    l[1] = make_uint2(d[2], d[3]);
                    l[2] = make_uint2(d[4], d[5]);
                } else {
                    store_group(pass + 24 * lane, d, store_w);
                }
            }
            if (store_w == 16) {
                // the pass's 24 * cnt bytes are contiguous: lanes store neighbouring 16-byte
                // pieces of them (whole 128-byte lines per instruction); an odd cnt leaves 8 bytes
                const int cnt = min(64, nvec - j0), pieces = cnt * 3 >> 1;
                wave_lds_sync();
                for (int i = lane; i < pieces; i += 64) ((uint4*)pass)[i] = ((const uint4*)s_out[w])[i];
                if ((cnt & 1) && lane == 0) ((uint2*)pass)[2 * pieces] = ((const uint2*)s_out[w])[2 * pieces];
                wave_lds_sync();  // before the next pass overwrites the row
            }
        }
        for (int x = tail0 + lane; x < W; x += 64) {
            p.at(x, g);
            store_bgr(o + 3 * (size_t)x,
                      view_pixel(x, display_u8(in[x], sf, hf), p, r, g, r.prow && point_found(r, p.pc, g.nx)));
        }
    }
}

// OpenCV 3.4's Circle() (imgproc/src/drawing.cpp), the filled non-antialiased
// path, run for a centre far from every border: the half-width of the filled
// span per row offset 0..radius, 4 bits each.  Rows cy -+ dy get cx -+ dx and rows
// cy -+ dx get cx -+ dy; a row filled twice keeps the wider span.
uint32_t circle_half_widths(int radius)
{
    int hw[4] = {0, 0, 0, 0};
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        hw[dy] = std::max(hw[dy], dx);
        hw[dx] = std::max(hw[dx], dy);
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
    return (uint32_t)(hw[0] | hw[1] << 4 | hw[2] << 8 | hw[3] << 12);
}

}  // namespace

const char* view_check(const mvsv_view_spec* spec, int W, int H)
{
    constexpr int all = MVSV_VIEW_SUBIMAGE_GRID | MVSV_VIEW_OBSTACLE_GRID | MVSV_VIEW_FOUND_TILES | MVSV_VIEW_FOUND_POINTS;
    if (!spec) return "null view spec";
    if (W < 9 || H < 9) return "the view needs a map of at least 9 x 9";
    if (spec->layers & ~all) return "unknown view layer bits";
    if (!std::isfinite(spec->alpha) || !std::isfinite(spec->beta)) return "view alpha / beta must be finite";
    if (spec->point_radius < 0 || spec->point_radius > 3) return "view point radius must be 0..3";
    return nullptr;
}

int view_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                const mvsv_view_spec& spec, uint8_t* out, size_t os, size_t ofs, int16_t* minmax)
{
    int rc, nblk, head, nvec;
    if ((rc = minmax_partials(ctx, n, dmap, st, fs, W, H, false, &nblk))) return rc;
    display_split(dmap, st, fs, n, W, &head, &nvec);
    ViewGeom g{};
    g.dx = W / 9;
    g.dy = H / 9;
    g.sub_mask = (spec.layers & MVSV_VIEW_SUBIMAGE_GRID) ? kSubMask : 0u;
    const bool obstacle = (spec.layers & MVSV_VIEW_OBSTACLE_GRID) != 0;
    g.ox1 = obstacle ? W / 3 : -1;
    g.ox2 = obstacle ? 2 * (W / 3) : -1;
    g.oy1 = obstacle ? H / 3 : -1;
    g.oy2 = obstacle ? 2 * (H / 3) : -1;
    g.tiles = (spec.layers & MVSV_VIEW_FOUND_TILES) ? 1 : 0;
    g.tile_first = spec.tile_first;
    g.tile_second = spec.tile_second;
    g.sx = g.sy = 8;  // never a divisor of 0; a launch without lattice keeps ny = 0
    if (spec.layers & MVSV_VIEW_FOUND_POINTS) {
        int sx, sy, nx, ny;
        sample_layout(W, H, &sx, &sy, &nx, &ny);
        if (nx > 0 && ny > 0) {
            g.sx = sx;
            g.sy = sy;
            g.nx = nx;
            g.ny = ny;
            g.pwords = 2 * ((nx + 63) / 64);
        }
    }
    g.radius = spec.point_radius;
    g.half_widths = circle_half_widths(spec.point_radius);
    g.point_first = spec.point_first;
    g.point_second = spec.point_second;
    // the widest store that is aligned at out + 3 * head of every row of every frame
    const uintptr_t a = ((uintptr_t)out + 3 * (size_t)head) | os | (n == 1 ? 0 : ofs);
    const int store_w = a % 16 == 0 ? 16 : a % 8 == 0 ? 8 : a % 4 == 0 ? 4 : a % 2 == 0 ? 2 : 1;
    const size_t lds = 2 * (size_t)g.pwords * sizeof(uint32_t);
    if (lds > 32768) return set_error(ctx, MVSV_E_INVALID_ARG, "map too wide for the view's found points");
    dim3 grid((H + kViewRows - 1) / kViewRows, n);
    hipLaunchKernelGGL(view_kernel, grid, dim3(256), lds, ctx->stream, dmap, st, fs, W, H, head, nvec,
                       (const int2*)ctx->mm_part.ptr, nblk, std::min(spec.alpha, spec.beta),
                       std::max(spec.alpha, spec.beta), g, spec.means, spec.values, out, os, ofs, store_w, minmax);
    return check_hip(ctx, hipGetLastError(), "detection view");
}

// The same layers painted over a host BGR image the way the reference does it:
// one after the other, each over what is there (View::draw*Grid on the host).
void view_draw_host(uint8_t* img, size_t stride, int W, int H, const mvsv_view_spec& spec)
{
    auto fill = [&](int x0, int y0, int x1, int y1, uint32_t bgr) {  // inclusive corners, clipped
        for (int y = std::max(y0, 0); y <= std::min(y1, H - 1); y++)
            for (int x = std::max(x0, 0); x <= std::min(x1, W - 1); x++) {
                uint8_t* p = img + (size_t)y * stride + 3 * (size_t)x;
                p[0] = (uint8_t)bgr;
                p[1] = (uint8_t)(bgr >> 8);
                p[2] = (uint8_t)(bgr >> 16);
            }
    };
    const int dx = W / 9, dy = H / 9;
    if (spec.layers & MVSV_VIEW_SUBIMAGE_GRID)
        for (int k = 1; k <= 8; k++)
            if ((kSubMask >> k) & 1u) {
                fill(dx * k, 0, dx * k, H, kGridBlue);
                fill(0, dy * k, W, dy * k, kGridBlue);
            }
    if (spec.layers & MVSV_VIEW_OBSTACLE_GRID)
        for (int k = 1; k <= 2; k++) {
            fill((W / 3) * k, 0, (W / 3) * k, H, kRed);
            fill(0, (H / 3) * k, W, (H / 3) * k, kRed);
        }
    if (spec.layers & MVSV_VIEW_FOUND_TILES)
        for (int i = 0; i < 81; i++)
            if (spec.means[i] < spec.tile_first && spec.means[i] > spec.tile_second)
                fill((i % 9) * dx, (i / 9) * dy, (i % 9) * dx + dx, (i / 9) * dy + dy, kRed);
    int sx, sy, nx, ny;
    sample_layout(W, H, &sx, &sy, &nx, &ny);
    if ((spec.layers & MVSV_VIEW_FOUND_POINTS) && nx > 0 && ny > 0) {
        const uint32_t hw = circle_half_widths(spec.point_radius);
        for (int c = 1; c <= nx; c++)
            for (int r = 1; r <= ny; r++) {
                const float v = spec.values[(c - 1) * ny + (r - 1)];
                if (!(v < spec.point_first && v > spec.point_second)) continue;
                for (int off = -spec.point_radius; off <= spec.point_radius; off++) {
                    const int h = (int)((hw >> (4 * std::abs(off))) & 15u);
                    fill(c * sx - h, r * sy + off, c * sx + h, r * sy + off, kRed);
                }
            }
    }
}

}  // namespace mvsv
