// mvsv_post.hip — post-filters of the disparity path on MI355X:
//   * 3x3 median, replicate border  ([OpenCV] medianBlur(disp, disp, 3), applied
//     by StereoSGBM::compute after the core)
//   * speckle filter                ([OpenCV] filterSpeckles, CV_16S): 4-connected
//     components of pixels != newVal whose neighbours differ by <= maxDiff;
//     components of size <= maxSpeckleSize become newVal.  Computed with a
//     lock-free union-find (atomicMin linking towards the smaller index), which
//     yields exactly the same components as OpenCV's raster-order flood fill.
//   * MeanDisparityDetection grid   (src/MeanDisparityDetection.cpp:159-206,
//     Utility::calcMeanDisparity src/utility.cpp:265-285)
//   * SamplepointDetection lattice  (src/SamplePointDetection.cpp: values of the
//     5x5 patches, range test + ordered compaction + calcCoordinate of the hits)
//   * display maps                  (cv::normalize(dMap, out, 0, 255, NORM_MINMAX,
//     CV_8U) of the reference's loops; min / max of Utility::calcMinMaxDisparity)
//   * point clouds                  (the loop of Utility::dmap2pcl, src/utility.cpp:248-259,
//     as an ordered compaction: the pixels with v > 0 in raster order, with
//     ply::write's grey)
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "mvsv_device.hpp"
#include "mvsv_display.hpp"
#include "mvsv_internal.hpp"

namespace mvsv {
namespace {

using namespace dev;

__device__ __forceinline__ void sort2(int& a, int& b)
{
    int lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// median of 9 with the 19-exchange network (Paeth / Devillard opt_med9)
__device__ __forceinline__ int med9(int p0, int p1, int p2, int p3, int p4, int p5, int p6, int p7,
                                    int p8)
{
    sort2(p1, p2); sort2(p4, p5); sort2(p7, p8);
    sort2(p0, p1); sort2(p3, p4); sort2(p6, p7);
    sort2(p1, p2); sort2(p4, p5); sort2(p7, p8);
    sort2(p0, p3); sort2(p5, p8); sort2(p4, p7);
    sort2(p3, p6); sort2(p1, p4); sort2(p2, p5);
    sort2(p4, p7); sort2(p4, p2); sort2(p6, p4);
    sort2(p4, p2);
    return p4;
}

__global__ __launch_bounds__(256) void median3x3_kernel(const int16_t* __restrict__ src, size_t ss,
                                                        size_t sfs, int16_t* __restrict__ dst,
                                                        size_t ds, size_t dfs, int W, int H,
                                                        const int* __restrict__ poison,
                                                        unsigned epoch, int invalid)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.z;
    if (x >= W || y >= H) return;
    if (poison && __builtin_expect(*poison == (int)epoch, 0)) {
        dst[f * dfs + (size_t)y * ds + x] = (int16_t)invalid;
        return;
    }
    const int16_t* s = src + f * sfs;
    const int xm = max(x - 1, 0), xp = min(x + 1, W - 1);
    const int16_t* r0 = s + (size_t)max(y - 1, 0) * ss;
    const int16_t* r1 = s + (size_t)y * ss;
    const int16_t* r2 = s + (size_t)min(y + 1, H - 1) * ss;
    int m = med9(r0[xm], r0[x], r0[xp], r1[xm], r1[x], r1[xp], r2[xm], r2[x], r2[xp]);
    dst[f * dfs + (size_t)y * ds + x] = (int16_t)m;
}

// Two horizontally adjacent pixels per thread on packed int16 pairs
// (v_pk_min_i16 / v_pk_max_i16): the three taps of a row are the dwords
// (p[x-1], p[x]), (p[x], p[x+1]), (p[x+1], p[x+2]) made by v_alignbit from the
// aligned words at x - 2, x, x + 2 (replicate border).  Needs an even width,
// even strides and 4-byte-aligned rows (median3x3_device checks).
__device__ __forceinline__ void sort2p(uint32_t& a, uint32_t& b)
{
    const uint32_t lo = pk_min(a, b), hi = as_u(__builtin_elementwise_max(as_s2(a), as_s2(b)));
    a = lo;
    b = hi;
}

__global__ __launch_bounds__(256) void median3x3_pk_kernel(const int16_t* __restrict__ src, size_t ss,
                                                           size_t sfs, int16_t* __restrict__ dst,
                                                           size_t ds, size_t dfs, int W, int H,
                                                           const int* __restrict__ poison,
                                                           unsigned epoch, int invalid)
{
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);  // pixel pair (2i, 2i + 1)
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.z;
    if (2 * i >= W || y >= H) return;
    uint32_t* o = (uint32_t*)(dst + f * dfs + (size_t)y * ds) + i;
    if (poison && __builtin_expect(*poison == (int)epoch, 0)) {
        *o = (uint32_t)(invalid & 0xffff) * 0x10001u;
        return;
    }
    const int16_t* s = src + f * sfs;
    uint32_t t[9];
    const int rows[3] = {max(y - 1, 0), y, min(y + 1, H - 1)};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t* q = (const uint32_t*)(s + (size_t)rows[k] * ss);
        const uint32_t M = q[i];
        const uint32_t P = i > 0 ? q[i - 1] : M << 16;             // hi half = p[x - 1] (p[0] at x = 0)
        const uint32_t N = 2 * i + 2 < W ? q[i + 1] : M >> 16;     // lo half = p[x + 2] (p[W - 1] at the end)
        t[3 * k] = __builtin_amdgcn_alignbit(M, P, 16);
        t[3 * k + 1] = M;
        t[3 * k + 2] = __builtin_amdgcn_alignbit(N, M, 16);
    }
    // the 19-exchange network of med9 on both pixels at once
    sort2p(t[1], t[2]); sort2p(t[4], t[5]); sort2p(t[7], t[8]);
    sort2p(t[0], t[1]); sort2p(t[3], t[4]); sort2p(t[6], t[7]);
    sort2p(t[1], t[2]); sort2p(t[4], t[5]); sort2p(t[7], t[8]);
    sort2p(t[0], t[3]); sort2p(t[5], t[8]); sort2p(t[4], t[7]);
    sort2p(t[3], t[6]); sort2p(t[1], t[4]); sort2p(t[2], t[5]);
    sort2p(t[4], t[7]); sort2p(t[4], t[2]); sort2p(t[6], t[4]);
    sort2p(t[4], t[2]);
    *o = t[4];
}

// ---- speckle filter: union-find ----------------------------------------------
// Stage 1: union-find inside a 32x32 tile in LDS (one 256-thread block per
// tile, 4 pixels per thread).  Outputs: per pixel its tile-local root (u16, lroot; row-major
// local order is monotone in the global index, so a root is the smallest
// global index of its tile component); per tile component (at its root's
// global index gi): parent[gi] = gi, tilew[gi] = the component's pixel count,
// size[gi] = 0, and gi + frame * W * H appended to the compact root list.
constexpr int kSpTile = 32;

__device__ __forceinline__ int lds_load(const int* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int lfind(int* par, int i)
{
    int p = lds_load(par + i);
    while (p != i) {
        int gp = lds_load(par + p);
        if (gp != p) atomicMin(par + i, gp);
        i = p;
        p = gp;
    }
    return i;
}

// the root without path compression: the lanes of a wave mostly walk the same
// chains, and the compressing atomicMin of lfind serialised them on one LDS
// address (0.51 of the kernel's LDS cycles were bank conflicts, round 5)
__device__ __forceinline__ int lroot_ro(const int* par, int i)
{
    int p = lds_load(par + i);
    for (;;) {
        const int q = lds_load(par + p);
        if (q == p) return p;
        p = q;
    }
}

__device__ void lunite(int* par, int a, int b)
{
    for (;;) {
        a = lfind(par, a);
        b = lfind(par, b);
        if (a == b) return;
        if (a > b) {
            int t = a;
            a = b;
            b = t;
        }
        int old = atomicMin(par + b, a);
        if (old == b) return;
        b = old;
    }
}

__global__ __launch_bounds__(256) void speckle_local_kernel(int16_t* __restrict__ img, size_t st, size_t fs,
                                                            int W, int H, int new_val, int max_diff,
                                                            int* __restrict__ parent,
                                                            int* __restrict__ tilew,
                                                            int* __restrict__ size,
                                                            uint16_t* __restrict__ lroot,
                                                            unsigned* __restrict__ list)
{
    __shared__ int lpar[kSpTile * kSpTile];
    __shared__ int lval[kSpTile * kSpTile];
    __shared__ int lcnt[kSpTile * kSpTile];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int lane = threadIdx.x & 63;
    const int x0 = blockIdx.x * kSpTile, y0 = blockIdx.y * kSpTile;
    const int f = blockIdx.z;
    const int kInvalid = 0x7fffffff;
    const int16_t* s = img + f * fs;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = ty + 8 * k, li = ly * kSpTile + tx;
        const int gx = x0 + tx, gy = y0 + ly;
        int v = kInvalid;
        if (gx < W && gy < H) {
            int t = s[(size_t)gy * st + gx];
            if (t != new_val) v = t;
        }
        lval[li] = v;
        lpar[li] = li;
        lcnt[li] = 0;
    }
    __syncthreads();
    // Horizontal runs without atomics: a wave holds two whole tile rows, so the
    // ballot of "connected to the right neighbour" gives each lane its run's
    // first pixel (the smallest index, so roots stay minimal), and every pixel
    // links straight to it.
    __shared__ unsigned hrow[kSpTile];  // bit x: (x, ly) -- (x + 1, ly) connected
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = ty + 8 * k, li = ly * kSpTile + tx;
        const int v = lval[li];
        const int u = tx + 1 < kSpTile ? lval[li + 1] : kInvalid;
        const bool h = v != kInvalid && u != kInvalid && abs(v - u) <= max_diff;
        const unsigned hm = (unsigned)(__ballot(h) >> (lane & 32));
        const unsigned starts = ~(hm << 1) & ((2u << tx) - 1u);  // run starts at or left of tx
        lpar[li] = ly * kSpTile + 31 - __clz(starts);
        if (tx == 0) hrow[ly] = hm;
    }
    __syncthreads();
    // Vertical links join runs; of a stretch of vertical links between the same
    // two runs only the leftmost one unites
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = ty + 8 * k, li = ly * kSpTile + tx;
        if (ly + 1 >= kSpTile) continue;
        const int v = lval[li], u = lval[li + kSpTile];
        if (v == kInvalid || u == kInvalid || abs(v - u) > max_diff) continue;
        if (tx > 0 && ((hrow[ly] & hrow[ly + 1]) >> (tx - 1) & 1u)) {
            const int vl = lval[li - 1], ul = lval[li + kSpTile - 1];
            if (abs(vl - ul) <= max_diff) continue;  // both valid: h bits set
        }
        lunite(lpar, li, li + kSpTile);
    }
    __syncthreads();
    int root[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = ty + 8 * k, li = ly * kSpTile + tx;
        root[k] = lval[li] != kInvalid ? lroot_ro(lpar, li) : -1;
        // component sizes by horizontal runs: a run (one root) adds its length
        // once, from its first pixel -- one LDS atomic per run instead of one
        // per pixel (same-address atomics of a smooth region serialise) or a
        // ballot loop over the wave's distinct roots (many in a noisy region)
        const unsigned hm = hrow[ly];
        const bool start = tx == 0 || !((hm >> (tx - 1)) & 1u);
        if (root[k] >= 0 && start) {
            const unsigned rest = ~(hm >> tx);  // bit j: (tx + j) not joined to its right neighbour
            atomicAdd(lcnt + root[k], __builtin_ctz(rest) + 1);
        }
    }
    __shared__ unsigned s_roots, s_base;
    if (threadIdx.x == 0) s_roots = 0u;
    __syncthreads();
    const size_t npix = (size_t)W * H;
    int* par = parent + f * npix;
    int* tl = tilew + f * npix;
    int* sz = size + f * npix;
    uint16_t* lr = lroot + f * npix;
    // the tile's components go to the compact root list (list[0] = count) with
    // ONE global atomic per block: every block appending per wave and row group
    // put 16 same-address L2 atomics per tile on list[0], serialised across the
    // whole launch (9 600 tiles per 8-frame step)
    unsigned long long rm[4];
    unsigned roff[4];
    int rgi[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = ty + 8 * k, li = ly * kSpTile + tx;
        const int gx = x0 + tx, gy = y0 + ly;
        const bool in = gx < W && gy < H;
        const int gi = gy * W + gx;
        if (in) lr[gi] = (uint16_t)(root[k] >= 0 ? root[k] : 0xffff);
        const int c = lcnt[li];
        const bool isroot = in && c > 0;
        if (isroot) {
            par[gi] = gi;
            tl[gi] = c;
            sz[gi] = 0;
        }
        rgi[k] = isroot ? gi : -1;
        rm[k] = __ballot(isroot);
        roff[k] = 0;
        if (rm[k]) {
            const int leader = __ffsll((long long)rm[k]) - 1;
            unsigned o = 0;
            if (lane == leader) o = atomicAdd(&s_roots, (unsigned)__popcll(rm[k]));  // LDS
            roff[k] = (unsigned)__builtin_amdgcn_readlane((int)o, leader);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_roots ? atomicAdd(list, s_roots) : 0u;
    __syncthreads();
    const unsigned base = s_base;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (rgi[k] >= 0)
            list[1 + base + roff[k] + (unsigned)__popcll(rm[k] & ((1ull << lane) - 1ull))] =
                (unsigned)(f * npix + rgi[k]);
}

// Union-find over tile components (the global parent words of tile roots).
// Parent words are read with agent-scope relaxed atomics (L1-bypassing):
// other workgroups rewrite them inside the same launch.  Roots are linked
// towards the smaller index with atomicMin (ECL-CC style): parents only ever
// decrease and stay inside their component, so concurrent unions never lose a
// link.
__device__ __forceinline__ int uf_load(const int* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int uf_find(int* parent, int i)
{
    int p = uf_load(parent + i);
    while (p != i) {
        int gp = uf_load(parent + p);
        if (gp != p) atomicMin(parent + i, gp);  // path halving, never increases
        i = p;
        p = gp;
    }
    return i;
}

__device__ void uf_unite(int* parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a > b) {
            int t = a;
            a = b;
            b = t;
        }
        int old = atomicMin(parent + b, a);  // link root b under a (a < b)
        if (old == b) return;
        b = old;  // b was re-linked concurrently: continue with its new parent
    }
}

// the tile root (global index) of pixel (x, y) from its local root
__device__ __forceinline__ int tile_root(const uint16_t* lr, int W, int x, int y)
{
    const int l = lr[y * W + x];
    return (y & ~(kSpTile - 1)) * W + (x & ~(kSpTile - 1)) + (l / kSpTile) * W + (l % kSpTile);
}

// Stage 2: unions across tile borders (right and bottom edge of each tile),
// one wave per tile, four tiles per block.  A pair joins the two pixels' tile
// components; lanes whose (component, component) pair repeats a lower lane's
// skip it, so a tile edge inside one smooth region costs one union instead of
// 32.
__global__ __launch_bounds__(256) void speckle_border_kernel(const int16_t* __restrict__ img,
                                                             size_t st, size_t fs, int W, int H,
                                                             int new_val, int max_diff,
                                                             int* __restrict__ parent,
                                                             const uint16_t* __restrict__ lroot,
                                                             int tiles_x)
{
    const int t = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int tyi = tile / tiles_x;
    const int x0 = (tile - tyi * tiles_x) * kSpTile, y0 = tyi * kSpTile;
    const int f = blockIdx.y;
    int x, y, nx, ny;
    if (t < kSpTile) {  // right edge: (x0+31, y0+t) -- (x0+32, y0+t)
        x = x0 + kSpTile - 1;
        y = y0 + t;
        nx = x + 1;
        ny = y;
    } else {  // bottom edge: (x0+t', y0+31) -- (x0+t', y0+32)
        x = x0 + (t - kSpTile);
        y = y0 + kSpTile - 1;
        nx = x;
        ny = y + 1;
    }
    const size_t npix = (size_t)W * H;
    int* par = parent + f * npix;
    const uint16_t* lr = lroot + f * npix;
    int a = -1, b = -1;
    if (y0 < H && x < W && y < H && nx < W && ny < H) {
        const int16_t* s = img + f * fs;
        const int v = s[(size_t)y * st + x], u = s[(size_t)ny * st + nx];
        if (v != new_val && u != new_val && abs(v - u) <= max_diff) {
            a = tile_root(lr, W, x, y);
            b = tile_root(lr, W, nx, ny);
        }
    }
    bool pending = a >= 0;
    for (;;) {
        unsigned long long m = __ballot(pending);
        if (m == 0ull) break;
        const int leader = __ffsll((long long)m) - 1;
        const int a0 = __builtin_amdgcn_readlane(a, leader);
        const int b0 = __builtin_amdgcn_readlane(b, leader);
        if (t == leader) uf_unite(par, a0, b0);
        if (a == a0 && b == b0) pending = false;
    }
}

// Stage 3: per tile component (the compact root list, grid-stride): its
// global root, the component sizes, and the tile word becomes ~root
// (negative: "resolved").
__global__ __launch_bounds__(256) void speckle_count_kernel(int W, int H, int* __restrict__ parent,
                                                            int* __restrict__ tilew,
                                                            int* __restrict__ size,
                                                            const unsigned* __restrict__ list)
{
    const unsigned cnt = list[0];
    const size_t npix = (size_t)W * H;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
        const unsigned e = list[1 + i];
        const size_t f = e / npix;
        const int gi = (int)(e - f * npix);
        int* par = parent + f * npix;
        const int g = uf_find(par, gi);
        atomicAdd(size + f * npix + g, tilew[f * npix + gi]);
        tilew[f * npix + gi] = ~g;
    }
}

// Stage 4: pixel -> tile root -> global root -> size.  Block (0, 0, 0) also
// rewinds the root list for the next call (stage 3 has finished with it).
__global__ __launch_bounds__(256) void speckle_apply_kernel(int16_t* __restrict__ img, size_t st,
                                                            size_t fs, int W, int H, int new_val,
                                                            int max_size,
                                                            const int* __restrict__ tilew,
                                                            const int* __restrict__ size,
                                                            const uint16_t* __restrict__ lroot,
                                                            unsigned* __restrict__ list)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && f == 0 && threadIdx.x == 0) list[0] = 0u;
    if (x >= W || y >= H) return;
    int16_t* p = img + f * fs + (size_t)y * st + x;
    if (*p == new_val) return;
    const size_t base = (size_t)f * W * H;
    const int g = ~tilew[base + tile_root(lroot + base, W, x, y)];
    if (size[base + g] <= max_size) *p = (int16_t)new_val;
}

// ---- MeanDisparityDetection::build(MEAN_VALUE) --------------------------------
__global__ __launch_bounds__(256) void mean_grid_kernel(const int16_t* __restrict__ dmap,
                                                        size_t st, size_t fs, int W, int H,
                                                        float* __restrict__ means)
{
    __shared__ int s_tot[4], s_cnt[4];
    const int tile = blockIdx.x;  // 0..80, row-major 9x9
    const int f = blockIdx.y;
    const int r = tile / 9, c = tile % 9;
    const int dx = W / 9, dy = H / 9;
    const int16_t* m = dmap + f * fs;
    int tot = 0, cnt = 0;
    for (int i = threadIdx.x; i < dx * dy; i += 256) {
        int yy = r * dy + i / dx, xx = c * dx + i % dx;
        int v = m[(size_t)yy * st + xx];
        if (v > 1) {
            tot += v;
            cnt++;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        tot += __shfl_xor(tot, o);
        cnt += __shfl_xor(cnt, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_tot[w] = tot;
        s_cnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int T = s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
        int N = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        means[(size_t)f * 81 + tile] = (T == 0 || N == 0) ? 0.0f : (float)(T / abs(N));
    }
}

// ---- cv::remap(INTER_LINEAR, BORDER_CONSTANT 0), CV_8UC1, CV_32FC1 maps ----------
// The rectification step of Stereosystem::getRectifiedImagepair
// (src/Stereosystem.cpp:243-262).  [OpenCV 3.4 RemapInvoker + remapBilinear]:
// X = cvRound(mapx * 32), Y = cvRound(mapy * 32) (round half to even);
// (sx, sy) = (X >> 5, Y >> 5) saturated to short, (ax, ay) = the low 5 bits;
// weights (32-ay)(32-ax)*32, (32-ay)ax*32, ay(32-ax)*32, ay*ax*32 (sum 2^15,
// exact for bilinear); out = (sum + 2^14) >> 15.  A 2x2 footprint entirely
// outside the source gives 0; partially outside, the outside taps read 0.
__device__ __forceinline__ int remap_tap(const uint8_t* s, size_t ss, int W, int H, int x, int y)
{
    return (x >= 0 && x < W && y >= 0 && y < H) ? (int)s[(size_t)y * ss + x] : 0;
}

__global__ __launch_bounds__(256) void remap_linear_kernel(
    const uint8_t* __restrict__ src, size_t ss, size_t sfs, int sw, int sh,
    const float* __restrict__ mx, const float* __restrict__ my, size_t ms,
    uint8_t* __restrict__ dst, size_t ds, size_t dfs, int dw, int dh)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.z;
    if (x >= dw || y >= dh) return;
    const int X = __float2int_rn(mx[(size_t)y * ms + x] * 32.0f);
    const int Y = __float2int_rn(my[(size_t)y * ms + x] * 32.0f);
    const int sx = clampi(X >> 5, -32768, 32767), sy = clampi(Y >> 5, -32768, 32767);
    const int ax = X & 31, ay = Y & 31;
    const uint8_t* s = src + f * sfs;
    int v;
    if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
        v = 0;
    } else {
        const int w00 = (32 - ay) * (32 - ax) * 32, w01 = (32 - ay) * ax * 32;
        const int w10 = ay * (32 - ax) * 32, w11 = ay * ax * 32;
        const int acc = remap_tap(s, ss, sw, sh, sx, sy) * w00 + remap_tap(s, ss, sw, sh, sx + 1, sy) * w01 +
                        remap_tap(s, ss, sw, sh, sx, sy + 1) * w10 +
                        remap_tap(s, ss, sw, sh, sx + 1, sy + 1) * w11;
        v = clampi((acc + (1 << 14)) >> 15, 0, 255);
    }
    dst[f * dfs + (size_t)y * ds + x] = (uint8_t)v;
}

// ---- the raw frame stream's rectification: both sides of n frames, ROI only -----
// cv::remap as above on maps already in cv::convertMaps' form (mvsv_convert_maps:
// (sx, sy) as a short pair and ay * 32 + ax as a u16 per pixel, cropped to the
// display ROI, rows padded with zero entries to a multiple of 4 pixels, left
// side then right side).  raw is [n][2][sh][sw]; blockIdx.z = 2 * frame + side.
// A thread computes 4 adjacent pixels of a row: one 16-byte and one 8-byte map
// load, the 2x2 taps as bounds-checked gathers, one dword store where the
// destination is 4-byte aligned (the row stride may be odd) and byte stores
// otherwise and in the row's tail.
__device__ __forceinline__ int rectify_px(const uint8_t* s, size_t ss, int sw, int sh, int sxy, int fr)
{
    const int sx = (int)(short)(sxy & 0xffff), sy = sxy >> 16;
    const int ax = fr & 31, ay = fr >> 5;
    if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) return 0;
    const int w00 = (32 - ay) * (32 - ax) * 32, w01 = (32 - ay) * ax * 32;
    const int w10 = ay * (32 - ax) * 32, w11 = ay * ax * 32;
    const int acc = remap_tap(s, ss, sw, sh, sx, sy) * w00 + remap_tap(s, ss, sw, sh, sx + 1, sy) * w01 +
                    remap_tap(s, ss, sw, sh, sx, sy + 1) * w10 + remap_tap(s, ss, sw, sh, sx + 1, sy + 1) * w11;
    return clampi((acc + (1 << 14)) >> 15, 0, 255);
}

// cv::remap with CV_16SC2 + CV_16UC1 maps (mvsv_remap_fixed_device): rectify_px on
// strided views, one pixel per thread; xs in int16 pairs, fs in elements, any
// 2-byte-aligned maps.  frac's bits above the 10 used ones are ignored, as
// cv::remap masks them (INTER_TAB_SIZE2 - 1).
__global__ __launch_bounds__(256) void remap_fixed_kernel(
    const uint8_t* __restrict__ src, size_t ss, size_t sfs, int sw, int sh, const int16_t* __restrict__ xy, size_t xs,
    const uint16_t* __restrict__ frac, size_t fs, uint8_t* __restrict__ dst, size_t ds, size_t dfs, int dw, int dh)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.z;
    if (x >= dw || y >= dh) return;
    const int16_t* p = xy + 2 * ((size_t)y * xs + x);
    const int sxy = (int)(uint16_t)p[0] | (int)p[1] << 16;
    dst[f * dfs + (size_t)y * ds + x] =
        (uint8_t)rectify_px(src + f * sfs, ss, sw, sh, sxy, (int)(frac[(size_t)y * fs + x] & 1023u));
}

__global__ __launch_bounds__(256) void rectify_pair_kernel(
    const uint8_t* __restrict__ raw, int sw, int sh, const int16_t* __restrict__ xy,
    const uint16_t* __restrict__ frac, size_t ms, uint8_t* __restrict__ dL, uint8_t* __restrict__ dR,
    size_t ds, size_t dfs, int dw, int dh)
{
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int side = blockIdx.z & 1, f = blockIdx.z >> 1;
    if (x >= dw || y >= dh) return;
    const uint8_t* s = raw + (size_t)blockIdx.z * sw * sh;
    // ms and x are multiples of 4: 16- / 8-byte aligned, and inside the padded row
    const size_t m = ((size_t)side * dh + y) * ms + x;
    const int4 q = *reinterpret_cast<const int4*>(xy + 2 * m);
    const uint2 a = *reinterpret_cast<const uint2*>(frac + m);
    const int v0 = rectify_px(s, sw, sw, sh, q.x, (int)(a.x & 0xffffu));
    const int v1 = rectify_px(s, sw, sw, sh, q.y, (int)(a.x >> 16));
    const int v2 = rectify_px(s, sw, sw, sh, q.z, (int)(a.y & 0xffffu));
    const int v3 = rectify_px(s, sw, sw, sh, q.w, (int)(a.y >> 16));
    uint8_t* d = (side ? dR : dL) + f * dfs + (size_t)y * ds + x;
    if (x + 3 < dw && ((uintptr_t)d & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d) = (uint32_t)v0 | (uint32_t)v1 << 8 | (uint32_t)v2 << 16 | (uint32_t)v3 << 24;
    } else {
        d[0] = (uint8_t)v0;
        if (x + 1 < dw) d[1] = (uint8_t)v1;
        if (x + 2 < dw) d[2] = (uint8_t)v2;
        if (x + 3 < dw) d[3] = (uint8_t)v3;
    }
}

// ---- cv::resize(src, dst, Size(0, 0), fx, fy, INTER_LINEAR), CV_8UC1 ----------
// The resize of Stereosystem::getRectifiedImagepair(Stereopair&, float)
// (src/Stereosystem.cpp:279-315).  [OpenCV 3.4 resize.cpp, x86 build] (oracle:
// orc_resize_linear): x / y source taps and 11-bit coefficients per output
// column / row in float (fx = (float)((dx + 0.5) * scale - 0.5), sx = floor,
// coefficients cvRound((1 - f) * 2048), cvRound(f * 2048); x clamped with
// f = 0, rows clamped); horizontal taps exact in int32; vertical combine as
// the SIMD op for columns x < simd_end ((S >> 4) x beta >> 16 per row, int16
// saturating add, (+2) >> 2) and (sum + 2^21) >> 22 past it.  A 2 x 2
// reduction (scale exactly 2) is INTER_AREA's fast path: (a+b+c+d+2) >> 2 on
// whole blocks, a float mean rounded half to even on clipped edge blocks.
__device__ __forceinline__ int sat16(int v) { return clampi(v, -32768, 32767); }

__global__ __launch_bounds__(256) void resize_linear_kernel(const uint8_t* __restrict__ src, size_t ss,
                                                            size_t sfs, int sw, int sh, double scale_x,
                                                            double scale_y, int area2, int simd_end,
                                                            uint8_t* __restrict__ dst, size_t ds, size_t dfs,
                                                            int dw, int dh)
{
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.z;
    if (dx >= dw || dy >= dh) return;
    const uint8_t* S = src + f * sfs;
    int v;
    if (area2) {
        const int sy0 = 2 * dy, sx0 = 2 * dx;
        const int w1 = sw / 2;
        const int w = sy0 + 2 <= sh ? w1 : 0;
        if (sy0 >= sh || sx0 >= sw) {
            v = 0;
        } else if (dx < w) {
            const uint8_t* r = S + (size_t)sy0 * ss + sx0;
            v = (r[0] + r[1] + r[ss] + r[ss + 1] + 2) >> 2;
        } else {
            int sum = 0, cnt = 0;
            for (int yy = 0; yy < 2 && sy0 + yy < sh; yy++)
                for (int xx = 0; xx < 2 && sx0 + xx < sw; xx++) {
                    sum += S[(size_t)(sy0 + yy) * ss + sx0 + xx];
                    cnt++;
                }
            v = clampi(__float2int_rn((float)sum / (float)cnt), 0, 255);
        }
    } else {
        float fxv = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fxv);
        fxv -= (float)sx;
        if (sx < 0) fxv = 0.f, sx = 0;
        if (sx >= sw - 1) fxv = 0.f, sx = sw - 1;
        const int a0 = __float2int_rn((1.f - fxv) * 2048.f), a1 = __float2int_rn(fxv * 2048.f);
        float fyv = (float)((dy + 0.5) * scale_y - 0.5);
        const int sy = (int)floorf(fyv);
        fyv -= (float)sy;
        const int b0 = (int)(short)__float2int_rn((1.f - fyv) * 2048.f);
        const int b1 = (int)(short)__float2int_rn(fyv * 2048.f);
        const int r0 = clampi(sy, 0, sh - 1), r1 = clampi(sy + 1, 0, sh - 1);
        const uint8_t* p0 = S + (size_t)r0 * ss + sx;
        const uint8_t* p1 = S + (size_t)r1 * ss + sx;
        const int s0 = p0[0] * a0 + (a1 ? p0[1] * a1 : 0);
        const int s1 = p1[0] * a0 + (a1 ? p1[1] * a1 : 0);
        if (dx < simd_end) {
            const int h0 = sat16(s0 >> 4), h1 = sat16(s1 >> 4);
            const int r = sat16(((h0 * b0) >> 16) + ((h1 * b1) >> 16));
            v = sat16(r + 2) >> 2;
        } else {
            v = (s0 * b0 + s1 * b1 + (1 << 21)) >> 22;
        }
        v = clampi(v, 0, 255);
    }
    dst[f * dfs + (size_t)dy * ds + dx] = (uint8_t)v;
}

// ---- Utility::calcCoordinate per pixel (src/utility.cpp:176-198) -------------
// (X, Y, Z, W) = Q * (x, y, v / 16, 1) with OpenCV's float GEMM (products and
// sums in double, one rounding to float per element), then Mat /= W as
// convertTo(alpha = (float)(1 / W)) (float multiply); Z = 0 when Z / 1000 is
// infinite.  The 4th output is 1 for v > 0 (the pixels Utility::dmap2pcl keeps).
struct QMat {
    float q[16];
};

// one point: (X, Y, Z) of (x, y, v) -- shared by the per-pixel kernel and the
// lattice detector, so both round exactly as mvsv_calc_coordinate does
__device__ __forceinline__ void calc_coordinate_dev(const QMat& Q, float x, float y, float v, float& X, float& Y,
                                                    float& Z)
{
    const float c[4] = {x, y, v / 16.0f, 1.0f};
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) acc = __dadd_rn(acc, __dmul_rn((double)Q.q[4 * i + k], (double)c[k]));
        r[i] = (float)acc;
    }
    const float alpha = (float)(1.0 / (double)r[3]);
    X = __fmul_rn(r[0], alpha);
    Y = __fmul_rn(r[1], alpha);
    Z = __fmul_rn(r[2], alpha);
    if (isinf(__fdiv_rn(Z, 1000.0f))) Z = 0.0f;
}

__global__ __launch_bounds__(256) void reproject_kernel(const int16_t* __restrict__ dmap, size_t st,
                                                        size_t fs, int W, int H, QMat Q,
                                                        float4* __restrict__ out, size_t os,
                                                        size_t ofs)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int f = blockIdx.z;
    if (x >= W || y >= H) return;
    const float v = (float)dmap[f * fs + (size_t)y * st + x];
    float X, Y, Z;
    calc_coordinate_dev(Q, (float)x, (float)y, v, X, Y, Z);
    out[f * ofs + (size_t)y * os + x] = make_float4(X, Y, Z, v > 0.0f ? 1.0f : 0.0f);
}

// ---- SamplepointDetection (src/SamplePointDetection.cpp:29-75,117-178) -------------
// The lattice: dX = W / 8, dY = H / 8, steps W / dX, H / dY (8..15), centres
// ((c + 1) * step_x, (r + 1) * step_y) for c < nx = dX - 1, r < ny = dY - 1, point
// index c * ny + r (the reference's loops: columns outside, rows inside).
//
// Values (Samplepoint::calculateSamplepointValue, inc/Samplepoint.h:32-40): a
// block takes up to kSpPts neighbouring points of one lattice row.  Its threads
// walk the map columns of that stretch -- lane j reads column x0 + j of each of
// the 2r + 1 map rows, so a wave reads contiguous row segments -- and leave each
// column's filtered sum and count in LDS; columns between two patches are
// skipped.  Then one lane per point adds its patch's 2r + 1 columns.  Radius 0
// is the raw centre value (no > 1 filter).  The host checks radius <
// min(step_x, step_y), which keeps every patch inside the map.
constexpr int kSpPts = 32;
constexpr int kSpSpan = 512;  // >= (kSpPts - 1) * 15 + 2 * 14 + 1 columns

__global__ __launch_bounds__(256) void sample_grid_kernel(const int16_t* __restrict__ dmap, size_t st,
                                                          size_t fs, int step_x, int step_y, int nx, int ny,
                                                          int radius, float* __restrict__ values)
{
    __shared__ int s_tot[kSpSpan], s_cnt[kSpSpan];
    const int c0 = blockIdx.x * kSpPts;
    const int r = blockIdx.y, f = blockIdx.z;
    const int pts = min(kSpPts, nx - c0);
    const int rows = 2 * radius + 1;
    const int span = (pts - 1) * step_x + rows;
    const int16_t* m = dmap + f * fs + (size_t)((r + 1) * step_y - radius) * st + ((c0 + 1) * step_x - radius);
    for (int j = threadIdx.x; j < span; j += 256) {
        if (j % step_x >= rows) continue;  // between two patches
        int tot = 0, cnt = 0;
        if (radius == 0) {
            tot = m[j];
        } else {
            for (int k = 0; k < rows; k++) {
                const int v = m[(size_t)k * st + j];
                if (v > 1) {
                    tot += v;
                    cnt++;
                }
            }
        }
        s_tot[j] = tot;
        s_cnt[j] = cnt;
    }
    __syncthreads();
    if ((int)threadIdx.x < pts) {
        const int b = threadIdx.x * step_x;
        int T = 0, N = 0;
        for (int k = 0; k < rows; k++) {
            T += s_tot[b + k];
            N += s_cnt[b + k];
        }
        const float v = radius == 0 ? (float)T : ((T == 0 || N == 0) ? 0.0f : (float)(T / N));
        values[(size_t)f * nx * ny + (size_t)(c0 + threadIdx.x) * ny + r] = v;
    }
}

// Detection (SamplepointDetection::detectObstacles, :134-178): value < first &&
// value > second, hits in index order with their calcCoordinate.  One block per
// frame walks the points in chunks of its 1024 threads; a hit's output position
// is the hits of earlier chunks + of earlier waves of the chunk (LDS) + of lower
// lanes of its wave (ballot), so the order never depends on timing.  count is
// the total; records beyond max_hits are dropped.
__global__ __launch_bounds__(1024) void sample_detect_kernel(const float* __restrict__ values, int npts, int ny,
                                                             int step_x, int step_y, QMat Q, float first,
                                                             float second, int max_hits, int* __restrict__ counts,
                                                             mvsv_sample_hit* __restrict__ hits)
{
    __shared__ int s_wave[16];
    const int f = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* v = values + (size_t)f * npts;
    mvsv_sample_hit* out = hits + (size_t)f * max_hits;
    int base = 0;
    for (int i0 = 0; i0 < npts; i0 += 1024) {
        const int i = i0 + threadIdx.x;
        const float val = i < npts ? v[i] : 0.0f;
        const bool hit = i < npts && val < first && val > second;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_wave[w] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int c = s_wave[k];
            before += k < w ? c : 0;
            total += c;
        }
        const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (hit && pos < max_hits) {
            const int c = i / ny, r = i - c * ny;
            float X, Y, Z;
            calc_coordinate_dev(Q, (float)((c + 1) * step_x), (float)((r + 1) * step_y), val, X, Y, Z);
            out[pos].index = i;
            out[pos].x = X;
            out[pos].y = Y;
            out[pos].z = Z;
        }
        base += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (threadIdx.x == 0) counts[f] = base;
}

// ---- display maps: cv::normalize(dMap, out, alpha, beta, NORM_MINMAX, CV_8U) ---------
// (trgt/liveDisparity.cpp:92 and every other loop of the reference), and the
// min / max of Utility::calcMinMaxDisparity (src/utility.cpp:287-304).
//
// A row of a view is walked as head | nvec packed 16-byte groups | tail: the
// host picks `head` so that row + head is 16-byte aligned in every row of every
// frame (display_split), or head = W (nvec = 0) where the strides do not allow
// that.  Head and tail elements are 2-byte loads, so no access leaves
// [row, row + W).  A wave takes a row, its lanes neighbouring elements / groups.
constexpr int kMmBlocks = 64;  // partial pairs per frame at most: one wave folds them
constexpr int kNormRows = 8;   // rows per block of normalize_u8_kernel (two per wave)

// Min and max of the part of a frame its block's waves walk: one (min, max)
// pair per block, written unconditionally -- no atomics, no init pass, the same
// partials on every run.  kPositive: only values > 0 count (calcMinMaxDisparity's
// rule); a block that saw none leaves the identities (32767, -32768).
template <bool kPositive>
__global__ __launch_bounds__(256) void minmax_kernel(const int16_t* __restrict__ dmap, size_t st, size_t fs, int W,
                                                     int H, int head, int nvec, int2* __restrict__ partials)
{
    __shared__ int s_lo[4], s_hi[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, f = blockIdx.y;
    const int16_t* m = dmap + f * fs;
    int lo = 32767, hi = -32768;
    auto take = [&](int v) {
        if (!kPositive || v > 0) {
            lo = min(lo, v);
            hi = max(hi, v);
        }
    };
    const int tail0 = head + nvec * 8;
    for (int y = blockIdx.x * 4 + w; y < H; y += gridDim.x * 4) {
        const int16_t* r = m + (size_t)y * st;
        for (int x = lane; x < head; x += 64) take(r[x]);
        const uint4* rv = (const uint4*)(r + head);
        for (int j = lane; j < nvec; j += 64) {
            const uint4 q = rv[j];
            take(lo16(q.x)); take(hi16(q.x)); take(lo16(q.y)); take(hi16(q.y));
            take(lo16(q.z)); take(hi16(q.z)); take(lo16(q.w)); take(hi16(q.w));
        }
        for (int x = tail0 + lane; x < W; x += 64) take(r[x]);
    }
    lo = wave_min_i32(lo);
    hi = wave_max_i32(hi);
    if (lane == 0) {
        s_lo[w] = lo;
        s_hi[w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        partials[(size_t)f * gridDim.x + blockIdx.x] = make_int2(min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3])),
                                                                 max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3])));
}

__global__ __launch_bounds__(64) void minmax_final_kernel(const int2* __restrict__ partials, int nblk,
                                                          int16_t* __restrict__ minmax)
{
    int lo, hi;
    fold_partials(partials, blockIdx.x, nblk, threadIdx.x, lo, hi);
    if (threadIdx.x == 0) {
        minmax[2 * blockIdx.x] = (int16_t)lo;
        minmax[2 * blockIdx.x + 1] = (int16_t)hi;
    }
}

// ---- focus measure: Utility::checkSharpness (src/utility.cpp:163-174) -----------------
// S4 = sum over the ROI of |KX (*) s| + |KY (*) s| on the BORDER_REFLECT_101
// extension s of the parent image, KX = (1,2,1)^T (-1,2,-1) = 4 Lx and
// KY = (-1,2,-1)^T (1,2,1) = 4 Ly of the two cv::sepFilter2D calls: an exact
// integer, at most 4080 a pixel (include/mvsv.h).
//
// A wave takes a work item: a strip of 256 columns (4 adjacent ones per lane) by
// a band of kShBand ROI rows; it requests all kShBand + 2 rows at once and then
// walks them with a three-row register window of the horizontal passes
// m = (-1,2,-1) and g = (1,2,1).  Strips start
// at xs <= roi x0 with row + xs 4-byte aligned in every row of every frame where
// the strides allow (packed: one dword load per lane and row); lanes that cross
// the image's border, and every lane otherwise, assemble their columns from byte
// loads at reflected indices.  The two halo columns come from the neighbouring
// lanes, for lanes 0 / 63 from one more byte load.  Only columns roi x0 - 1 ..
// x1 and rows y0 - 1 .. y1 (reflected into the parent) are needed; nothing
// outside [row, row + W) of a parent row is read.
constexpr int kShBand = 8;       // ROI rows per work item (2 halo rows on top: 1/4 more row reads, mostly L2 hits)
constexpr int kShBlocks = 1024;  // partial sums per frame at most

__device__ __forceinline__ int reflect101(int i, int n) { return n == 1 ? 0 : i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

struct ShRaw {  // a lane's part of one parent row: 4 columns packed, the halo columns beside them
    uint32_t w;
    int left, right;
};

__device__ __forceinline__ ShRaw sharp_load(const uint8_t* __restrict__ r, int W, int c0, int lo, int hi, bool packed,
                                            int lane)
{
    ShRaw q;
    if (packed && c0 >= 0 && c0 + 3 < W) {
        q.w = *reinterpret_cast<const uint32_t*>(r + c0);
    } else {
        q.w = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = c0 + k;
            if (c >= lo && c <= hi) q.w |= (uint32_t)r[reflect101(c, W)] << (8 * k);
        }
    }
    q.left = q.right = 0;
    if (lane == 0 && c0 - 1 >= lo && c0 - 1 <= hi) q.left = r[reflect101(c0 - 1, W)];
    if (lane == 63 && c0 + 4 >= lo && c0 + 4 <= hi) q.right = r[reflect101(c0 + 4, W)];
    return q;
}

// the horizontal passes of a lane's 4 columns: m = 2 p - l - r, g = 2 p + l + r
__device__ __forceinline__ void sharp_hpass(const ShRaw& q, int lane, int* m, int* g)
{
    const int up = __shfl_up((int)(q.w >> 24), 1), dn = __shfl_down((int)(q.w & 0xffu), 1);
    int p[6];
    p[0] = lane == 0 ? q.left : up;
    p[1] = (int)(q.w & 0xffu);
    p[2] = (int)((q.w >> 8) & 0xffu);
    p[3] = (int)((q.w >> 16) & 0xffu);
    p[4] = (int)(q.w >> 24);
    p[5] = lane == 63 ? q.right : dn;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        m[k] = 2 * p[k + 1] - p[k] - p[k + 2];
        g[k] = 2 * p[k + 1] + p[k] + p[k + 2];
    }
}

// One 64-bit partial per block, written unconditionally: no atomics, no init
// pass, the same partials on every run (integer sums do not depend on order).
__global__ __launch_bounds__(256) void sharpness_kernel(const uint8_t* __restrict__ img, size_t st, size_t fs, int W,
                                                        int H, int x0, int y0, int x1, int y1, int xs, int packed,
                                                        int nstrips, int nbands,
                                                        unsigned long long* __restrict__ partials)
{
    __shared__ unsigned long long s_sum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, f = blockIdx.y;
    const uint8_t* im = img + f * fs;
    const int lo = x0 - 1, hi = x1;
    unsigned long long total = 0;
    for (int it = blockIdx.x * 4 + w; it < nstrips * nbands; it += gridDim.x * 4) {
        const int strip = it % nstrips, band = it / nstrips;
        const int c0 = xs + strip * 256 + lane * 4;
        const int yb = y0 + band * kShBand, ye = min(yb + kShBand, y1);
        bool own[4];
#pragma unroll
        for (int k = 0; k < 4; k++) own[k] = c0 + k >= x0 && c0 + k < x1;
        // every row of the band is requested before the first is summed; rows past a short
        // band's end repeat its last halo row and are not summed
        ShRaw raw[kShBand + 2];
#pragma unroll
        for (int i = 0; i < kShBand + 2; i++)
            raw[i] = sharp_load(im + (size_t)reflect101(min(yb - 1 + i, ye), H) * st, W, c0, lo, hi, packed, lane);
        int am[4], ag[4], bm[4], bg[4], cm[4], cg[4];
        sharp_hpass(raw[0], lane, am, ag);
        sharp_hpass(raw[1], lane, bm, bg);
        uint32_t acc = 0;  // at most 4 * kShBand * 4080
#pragma unroll
        for (int i = 0; i < kShBand; i++) {
            sharp_hpass(raw[i + 2], lane, cm, cg);
            const bool row = yb + i < ye;  // wave-uniform
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int v = abs(am[k] + 2 * bm[k] + cm[k]) + abs(2 * bg[k] - ag[k] - cg[k]);
                acc += row && own[k] ? (uint32_t)v : 0u;
                am[k] = bm[k];
                ag[k] = bg[k];
                bm[k] = cm[k];
                bg[k] = cg[k];
            }
        }
        total += acc;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) total += __shfl_down(total, o);
    if (lane == 0) s_sum[w] = total;
    __syncthreads();
    if (threadIdx.x == 0)
        partials[(size_t)f * gridDim.x + blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// a frame's nblk partials folded by one wave into sums[f * ss]
__global__ __launch_bounds__(64) void sharpness_fold_kernel(const unsigned long long* __restrict__ partials, int nblk,
                                                            int64_t* __restrict__ sums, size_t ss)
{
    unsigned long long t = 0;
    for (int i = threadIdx.x; i < nblk; i += 64) t += partials[(size_t)blockIdx.x * nblk + i];
#pragma unroll
    for (int o = 32; o; o >>= 1) t += __shfl_down(t, o);
    if (threadIdx.x == 0) sums[(size_t)blockIdx.x * ss] = (int64_t)t;
}

// The display byte itself (display_scale, display_u8: OpenCV 3.4's arithmetic
// with contraction off) is in mvsv_display.hpp, shared with the detection view.
//
// Block (tile, frame): kNormRows rows of a frame to 8 bit.  Wave 0 folds the
// frame's partials and lane 0 derives (sf, hf) once for the block.  A packed group
// is 8 pixels = 8 output bytes, stored as one, two, four or eight stores by the
// alignment of out + head (store_w, chosen by the host for the whole launch).
__global__ __launch_bounds__(256) void normalize_u8_kernel(const int16_t* __restrict__ dmap, size_t st, size_t fs,
                                                           int W, int H, int head, int nvec,
                                                           const int2* __restrict__ partials, int nblk, double dmin,
                                                           double dmax, uint8_t* __restrict__ out, size_t os,
                                                           size_t ofs, int store_w, int16_t* __restrict__ minmax)
{
    __shared__ float s_sf, s_hf;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, f = blockIdx.y;
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
    }
    __syncthreads();
    const float sf = s_sf, hf = s_hf;
    const int tail0 = head + nvec * 8;
    const int y1 = min(H, ((int)blockIdx.x + 1) * kNormRows);
    for (int y = blockIdx.x * kNormRows + w; y < y1; y += 4) {
        const int16_t* r = dmap + f * fs + (size_t)y * st;
        uint8_t* o = out + f * ofs + (size_t)y * os;
        for (int x = lane; x < head; x += 64) o[x] = (uint8_t)display_u8(r[x], sf, hf);
        const uint4* rv = (const uint4*)(r + head);
        for (int j = lane; j < nvec; j += 64) {
            const uint4 q = rv[j];
            const uint32_t b0 = display_u8(lo16(q.x), sf, hf), b1 = display_u8(hi16(q.x), sf, hf);
            const uint32_t b2 = display_u8(lo16(q.y), sf, hf), b3 = display_u8(hi16(q.y), sf, hf);
            const uint32_t b4 = display_u8(lo16(q.z), sf, hf), b5 = display_u8(hi16(q.z), sf, hf);
            const uint32_t b6 = display_u8(lo16(q.w), sf, hf), b7 = display_u8(hi16(q.w), sf, hf);
            uint8_t* p = o + head + (size_t)j * 8;
            if (store_w == 8) {
                *(uint2*)p = make_uint2(b0 | b1 << 8 | b2 << 16 | b3 << 24, b4 | b5 << 8 | b6 << 16 | b7 << 24);
            } else if (store_w == 4) {
                ((uint32_t*)p)[0] = b0 | b1 << 8 | b2 << 16 | b3 << 24;
                ((uint32_t*)p)[1] = b4 | b5 << 8 | b6 << 16 | b7 << 24;
            } else if (store_w == 2) {
                ((uint16_t*)p)[0] = (uint16_t)(b0 | b1 << 8);
                ((uint16_t*)p)[1] = (uint16_t)(b2 | b3 << 8);
                ((uint16_t*)p)[2] = (uint16_t)(b4 | b5 << 8);
                ((uint16_t*)p)[3] = (uint16_t)(b6 | b7 << 8);
            } else {
                p[0] = (uint8_t)b0; p[1] = (uint8_t)b1; p[2] = (uint8_t)b2; p[3] = (uint8_t)b3;
                p[4] = (uint8_t)b4; p[5] = (uint8_t)b5; p[6] = (uint8_t)b6; p[7] = (uint8_t)b7;
            }
        }
        for (int x = tail0 + lane; x < W; x += 64) o[x] = (uint8_t)display_u8(r[x], sf, hf);
    }
}

// ---- point clouds: Utility::dmap2pcl's loop (src/utility.cpp:248-259) as an ordered compaction ----
// The records of a frame are its pixels with v > 0 in raster order: (x, y, z) of
// calc_coordinate_dev and the grey ply::write prints in WITH_COLOR mode
// (src/ply.cpp:90).  Three launches, no block waits on another and no atomics, so
// a record's position never depends on timing:
//   cloud_rows_kernel     a wave per row: (count, min, max over v > 0) of the row,
//                         written unconditionally
//   cloud_scan_kernel     a block per frame: the counts become the rows' first
//                         record positions (exclusive scan, in chunks of the block's
//                         width), min / max are folded, the frame's count is written
//   cloud_scatter_kernel  a wave per row again: a pixel's position is its row's
//                         first + the valid pixels of earlier steps of the walk +
//                         those of lower lanes / elements of this step (ballots)
// Rows are walked head | packed 16-byte groups | tail as in minmax_kernel; every
// loop bound is wave-uniform, so every ballot sees the whole wave.
constexpr int kCloudScan = 256;                      // rows per step of cloud_scan_kernel
constexpr int kCloudNone = (int)0x80007fffu;         // packed (min, max) identities (32767, -32768)

__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

__global__ __launch_bounds__(256) void cloud_rows_kernel(const int16_t* __restrict__ dmap, size_t st, size_t fs, int W,
                                                         int H, int head, int nvec, int2* __restrict__ rows)
{
    const int lane = threadIdx.x & 63, f = blockIdx.y;
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= H) return;  // whole waves
    const int16_t* r = dmap + f * fs + (size_t)y * st;
    int cnt = 0, lo = 32767, hi = -32768;
    auto take = [&](int v) {
        const bool ok = v > 0;
        cnt += __popcll(__ballot(ok));
        if (ok) {
            lo = min(lo, v);
            hi = max(hi, v);
        }
    };
    for (int x0 = 0; x0 < head; x0 += 64) take(x0 + lane < head ? r[x0 + lane] : 0);
    const uint4* rv = (const uint4*)(r + head);
    for (int j0 = 0; j0 < nvec; j0 += 64) {
        const uint4 q = j0 + lane < nvec ? rv[j0 + lane] : make_uint4(0u, 0u, 0u, 0u);
        take(lo16(q.x)); take(hi16(q.x)); take(lo16(q.y)); take(hi16(q.y));
        take(lo16(q.z)); take(hi16(q.z)); take(lo16(q.w)); take(hi16(q.w));
    }
    for (int x0 = head + nvec * 8; x0 < W; x0 += 64) take(x0 + lane < W ? r[x0 + lane] : 0);
    lo = wave_min_i32(lo);
    hi = wave_max_i32(hi);
    if (lane == 0) rows[(size_t)f * H + y] = make_int2(cnt, (int)((uint32_t)(lo & 0xffff) | (uint32_t)hi << 16));
}

// frames[f] = (min, max); counts / minmax are the caller's (element strides cs, ms; minmax may be null)
__global__ __launch_bounds__(kCloudScan) void cloud_scan_kernel(int2* __restrict__ rows, int H, int2* __restrict__ frames,
                                                                int* __restrict__ counts, size_t cs,
                                                                int* __restrict__ minmax, size_t ms)
{
    constexpr int kWaves = kCloudScan / 64;
    __shared__ int s_cnt[kWaves], s_lo[kWaves], s_hi[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, f = blockIdx.x;
    int2* r = rows + (size_t)f * H;
    int base = 0, lo = 32767, hi = -32768;
    for (int i0 = 0; i0 < H; i0 += kCloudScan) {
        const int i = i0 + threadIdx.x;
        const int2 t = i < H ? r[i] : make_int2(0, kCloudNone);
        lo = min(lo, lo16((uint32_t)t.y));
        hi = max(hi, hi16((uint32_t)t.y));
        int inc = t.x;  // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) s_cnt[w] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) {
            const int c = s_cnt[k];
            before += k < w ? c : 0;
            total += c;
        }
        if (i < H) r[i].x = base + before + inc - t.x;
        base += total;
        __syncthreads();  // s_cnt is rewritten by the next chunk
    }
    lo = wave_min_i32(lo);
    hi = wave_max_i32(hi);
    if (lane == 0) {
        s_lo[w] = lo;
        s_hi[w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kWaves; k++) {
            lo = min(lo, s_lo[k]);
            hi = max(hi, s_hi[k]);
        }
        frames[f] = make_int2(lo, hi);
        counts[(size_t)f * cs] = base;
        if (minmax) {
            minmax[(size_t)f * ms] = lo;
            minmax[(size_t)f * ms + 1] = hi;
        }
    }
}

// int((z - mn) / (mx - mn) * 255.0) as the host writer computes it: a float
// difference and a correctly rounded float quotient, a double product, truncation;
// INT32_MIN where the double is NaN or outside int32 (what the x86-64 conversion
// yields; mx == mn divides by zero).  No contraction: nothing here may fuse.
__device__ __forceinline__ int cloud_grey(float z, float mn, float range)
{
#pragma clang fp contract(off)
    const float num = z - mn;
    const float q = __fdiv_rn(num, range);
    const double d = (double)q * 255.0;
    return (d > -2147483649.0 && d < 2147483648.0) ? (int)d : (int)0x80000000u;
}

__global__ __launch_bounds__(256) void cloud_scatter_kernel(const int16_t* __restrict__ dmap, size_t st, size_t fs,
                                                            int W, int H, int head, int nvec, QMat Q,
                                                            const int2* __restrict__ rows,
                                                            const int2* __restrict__ frames,
                                                            float4* __restrict__ records, int capacity)
{
    const int lane = threadIdx.x & 63, f = blockIdx.y;
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= H) return;  // whole waves
    int base = rows[(size_t)f * H + y].x;  // wave-uniform: the records of earlier rows
    if (base >= capacity) return;
    const int2 mm = frames[f];
    const float mn = (float)mm.x, range = (float)(mm.y - mm.x);
    const int16_t* r = dmap + f * fs + (size_t)y * st;
    float4* out = records + (size_t)f * capacity;
    auto emit = [&](int x, int v, int pos) {
        if (v > 0 && pos < capacity) {
            float X, Y, Z;
            calc_coordinate_dev(Q, (float)x, (float)y, (float)v, X, Y, Z);
            out[pos] = make_float4(X, Y, Z, __int_as_float(cloud_grey(Z, mn, range)));
        }
    };
    auto narrow = [&](int x0, int x1) {
        for (; x0 < x1; x0 += 64) {
            const int x = x0 + lane;
            const int v = x < x1 ? r[x] : 0;
            const unsigned long long m = __ballot(v > 0);
            emit(x, v, base + lanes_below(m, lane));
            base += __popcll(m);
        }
    };
    narrow(0, head);
    const uint4* rv = (const uint4*)(r + head);
    for (int j0 = 0; j0 < nvec; j0 += 64) {
        const int j = j0 + lane;
        const uint4 q = j < nvec ? rv[j] : make_uint4(0u, 0u, 0u, 0u);
        // a lane holds 8 neighbouring pixels: the records of lower lanes come first
        int below = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t d = k < 2 ? q.x : k < 4 ? q.y : k < 6 ? q.z : q.w;
            const unsigned long long m = __ballot(((k & 1) ? hi16(d) : lo16(d)) > 0);
            below += lanes_below(m, lane);
            total += __popcll(m);
        }
        int pos = base + below;
#pragma unroll 1
        for (int k = 0; k < 8; k++) {
            const uint32_t d = k < 2 ? q.x : k < 4 ? q.y : k < 6 ? q.z : q.w;
            const int v = (k & 1) ? hi16(d) : lo16(d);
            emit(head + j * 8 + k, v, pos);
            pos += v > 0 ? 1 : 0;
        }
        base += total;
    }
    narrow(head + nvec * 8, W);
}

}  // namespace

int median3x3_device(mvsv_ctx* ctx, int n, const int16_t* src, size_t ss, size_t sfs, int16_t* dst,
                     size_t ds, size_t dfs, int W, int H, const int* poison, unsigned epoch,
                     int invalid)
{
    const bool packed = (W % 2) == 0 && (ss % 2) == 0 && (sfs % 2) == 0 && (ds % 2) == 0 && (dfs % 2) == 0 &&
                        ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0;
    if (packed) {
        dim3 grid((W / 2 + 63) / 64, (H + 3) / 4, n);
        hipLaunchKernelGGL(median3x3_pk_kernel, grid, dim3(256), 0, ctx->stream, src, ss, sfs, dst, ds, dfs, W, H,
                           poison, epoch, invalid);
    } else {
        dim3 grid((W + 63) / 64, (H + 3) / 4, n);
        hipLaunchKernelGGL(median3x3_kernel, grid, dim3(256), 0, ctx->stream, src, ss, sfs, dst, ds, dfs, W, H,
                           poison, epoch, invalid);
    }
    return check_hip(ctx, hipGetLastError(), "median3x3");
}

// The speckle filter's buffers: parent / tile words / sizes (int per pixel,
// only tile-component roots used), the tile-local root of every pixel (u16)
// and the compact root list (count + entries).
static int speckle_buffers(mvsv_ctx* ctx, int n, int W, int H, int** parent, int** tilew, int** size,
                           uint16_t** lroot, unsigned** list)
{
    int rc;
    const SpeckleBytes sb = speckle_bytes(n, W, H);  // (mvsv_sgbm_plan.hpp: also the workspace estimate's)
    // the list count is rewound by the apply kernel of every run; a fresh
    // (re)allocation, or a run that did not reach its apply launch, rewinds here
    const bool fresh_list = ctx->uf_list.bytes < sb.list || ctx->uf_list_dirty;
    if ((rc = ensure(ctx, ctx->uf_parent, sb.parent, "speckle labels"))) return rc;
    if ((rc = ensure(ctx, ctx->uf_size, sb.size, "speckle sizes"))) return rc;
    if ((rc = ensure(ctx, ctx->uf_tile, sb.tile, "speckle tile components"))) return rc;
    if ((rc = ensure(ctx, ctx->uf_lroot, sb.lroot, "speckle local roots"))) return rc;
    if ((rc = ensure(ctx, ctx->uf_list, sb.list, "speckle root list"))) return rc;
    if (fresh_list && (rc = check_hip(ctx, hipMemsetAsync(ctx->uf_list.ptr, 0, 4, ctx->stream), "root list reset")))
        return rc;
    ctx->uf_list_dirty = true;  // until this run's apply kernel is launched
    *parent = (int*)ctx->uf_parent.ptr;
    *size = (int*)ctx->uf_size.ptr;
    *tilew = (int*)ctx->uf_tile.ptr;
    *lroot = (uint16_t*)ctx->uf_lroot.ptr;
    *list = (unsigned*)ctx->uf_list.ptr;
    return MVSV_OK;
}

// stages 2-4 (stage 1 launched by the caller)
static int speckle_tail(mvsv_ctx* ctx, int n, int16_t* img, size_t st, size_t fs, int W, int H, int new_val,
                        int max_size, int max_diff, int* parent, int* tilew, int* size, uint16_t* lroot,
                        unsigned* list)
{
    hipStream_t s = ctx->stream;
    const int tx = (W + kSpTile - 1) / kSpTile, tyn = (H + kSpTile - 1) / kSpTile;
    hipLaunchKernelGGL(speckle_border_kernel, dim3((unsigned)((tx * tyn + 3) / 4), n), dim3(256), 0, s, img, st, fs,
                       W, H, new_val, max_diff, parent, lroot, tx);
    hipLaunchKernelGGL(speckle_count_kernel, dim3((unsigned)std::max(1, ctx->cus * 4)), dim3(256), 0, s, W, H, parent,
                       tilew, size, list);
    dim3 grid((W + 63) / 64, (H + 3) / 4, n);
    hipLaunchKernelGGL(speckle_apply_kernel, grid, dim3(256), 0, s, img, st, fs, W, H, new_val, max_size, tilew,
                       size, lroot, list);
    const int rc = check_hip(ctx, hipGetLastError(), "speckle filter");
    if (rc == MVSV_OK) ctx->uf_list_dirty = false;
    return rc;
}

int speckle_device(mvsv_ctx* ctx, int n, int16_t* img, size_t st, size_t fs, int W, int H,
                   int new_val, int max_size, int max_diff)
{
    int rc, *parent, *tilew, *size;
    uint16_t* lroot;
    unsigned* list;
    if ((rc = speckle_buffers(ctx, n, W, H, &parent, &tilew, &size, &lroot, &list))) return rc;
    dim3 tiles((W + kSpTile - 1) / kSpTile, (H + kSpTile - 1) / kSpTile, n);
    hipLaunchKernelGGL(speckle_local_kernel, tiles, dim3(256), 0, ctx->stream, img, st, fs, W, H, new_val, max_diff,
                       parent, tilew, size, lroot, list);
    return speckle_tail(ctx, n, img, st, fs, W, H, new_val, max_size, max_diff, parent, tilew, size, lroot, list);
}

int mean_grid_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                     float* means)
{
    hipLaunchKernelGGL(mean_grid_kernel, dim3(81, n), dim3(256), 0, ctx->stream, dmap, st, fs, W,
                       H, means);
    return check_hip(ctx, hipGetLastError(), "mean disparity grid");
}

int sample_layout(int W, int H, int* step_x, int* step_y, int* nx, int* ny)
{
    if (W <= 0 || H <= 0) return MVSV_E_INVALID_ARG;
    const int dX = W / 8, dY = H / 8;
    *step_x = dX ? W / dX : 0;
    *step_y = dY ? H / dY : 0;
    *nx = std::max(dX - 1, 0);
    *ny = std::max(dY - 1, 0);
    return MVSV_OK;
}

int sample_grid_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H, int radius,
                       float* values)
{
    int sx, sy, nx, ny;
    if (sample_layout(W, H, &sx, &sy, &nx, &ny)) return set_error(ctx, MVSV_E_INVALID_ARG, "empty map");
    if (nx == 0 || ny == 0) return MVSV_OK;  // narrower or lower than 16: no lattice point
    if (radius < 0 || radius >= std::min(sx, sy))
        return set_error(ctx, MVSV_E_INVALID_ARG, "sample point radius must be 0 .. min(step_x, step_y) - 1");
    dim3 grid((nx + kSpPts - 1) / kSpPts, ny, n);
    hipLaunchKernelGGL(sample_grid_kernel, grid, dim3(256), 0, ctx->stream, dmap, st, fs, sx, sy, nx, ny, radius,
                       values);
    return check_hip(ctx, hipGetLastError(), "sample point values");
}

int sample_detect_device(mvsv_ctx* ctx, int n, const float* values, int W, int H, const float* Q, float first,
                         float second, int max_hits, int* counts, mvsv_sample_hit* hits)
{
    int sx, sy, nx, ny;
    if (sample_layout(W, H, &sx, &sy, &nx, &ny)) return set_error(ctx, MVSV_E_INVALID_ARG, "empty map");
    if (nx == 0 || ny == 0) return MVSV_OK;
    QMat q;
    for (int i = 0; i < 16; i++) q.q[i] = Q[i];
    hipLaunchKernelGGL(sample_detect_kernel, dim3(n), dim3(1024), 0, ctx->stream, values, nx * ny, ny, sx, sy, q,
                       first, second, max_hits, counts, hits);
    return check_hip(ctx, hipGetLastError(), "sample point detection");
}

// The packed path needs row + head 16-byte aligned in every row of every frame:
// row and frame strides that are multiples of 8 elements (16 bytes), any
// 2-byte-aligned base -- head = the 0..7 elements up to the next 16-byte
// boundary.  Other strides take the narrow path (head = W: 2-byte loads only).
void display_split(const int16_t* dmap, size_t st, size_t fs, int n, int W, int* head, int* nvec)
{
    const bool packed = st % 8 == 0 && (n == 1 || fs % 8 == 0) && ((uintptr_t)dmap & 1) == 0;
    *head = packed ? std::min(W, (int)(((16 - ((uintptr_t)dmap & 15)) & 15) / 2)) : W;
    *nvec = (W - *head) / 8;
}

int minmax_partials(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H, bool positive_only,
                    int* nblk)
{
    int rc, head, nvec;
    // room for 16 frames at least: the usual batches never grow (and so never synchronise) it
    if ((rc = ensure(ctx, ctx->mm_part, (size_t)std::max(n, 16) * kMmBlocks * sizeof(int2), "min / max partials")))
        return rc;
    display_split(dmap, st, fs, n, W, &head, &nvec);
    *nblk = std::min(kMmBlocks, (H + 3) / 4);
    dim3 grid(*nblk, n);
    if (positive_only)
        hipLaunchKernelGGL(minmax_kernel<true>, grid, dim3(256), 0, ctx->stream, dmap, st, fs, W, H, head, nvec,
                           (int2*)ctx->mm_part.ptr);
    else
        hipLaunchKernelGGL(minmax_kernel<false>, grid, dim3(256), 0, ctx->stream, dmap, st, fs, W, H, head, nvec,
                           (int2*)ctx->mm_part.ptr);
    return check_hip(ctx, hipGetLastError(), "min / max");
}

int minmax_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H, bool positive_only,
                  int16_t* minmax)
{
    int rc, nblk;
    if ((rc = minmax_partials(ctx, n, dmap, st, fs, W, H, positive_only, &nblk))) return rc;
    hipLaunchKernelGGL(minmax_final_kernel, dim3(n), dim3(64), 0, ctx->stream, (const int2*)ctx->mm_part.ptr, nblk,
                       minmax);
    return check_hip(ctx, hipGetLastError(), "min / max");
}

int normalize_minmax_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                            double alpha, double beta, uint8_t* out, size_t os, size_t ofs, int16_t* minmax)
{
    int rc, nblk, head, nvec;
    if ((rc = minmax_partials(ctx, n, dmap, st, fs, W, H, false, &nblk))) return rc;
    display_split(dmap, st, fs, n, W, &head, &nvec);
    // the widest store that is aligned at out + head of every row of every frame
    const uintptr_t a = ((uintptr_t)out + head) | os | (n == 1 ? 0 : ofs);
    const int store_w = a % 8 == 0 ? 8 : a % 4 == 0 ? 4 : a % 2 == 0 ? 2 : 1;
    dim3 grid((H + kNormRows - 1) / kNormRows, n);
    hipLaunchKernelGGL(normalize_u8_kernel, grid, dim3(256), 0, ctx->stream, dmap, st, fs, W, H, head, nvec,
                       (const int2*)ctx->mm_part.ptr, nblk, std::min(alpha, beta), std::max(alpha, beta), out, os,
                       ofs, store_w, minmax);
    return check_hip(ctx, hipGetLastError(), "normalize");
}

int sharpness_device(mvsv_ctx* ctx, int n, const uint8_t* img, size_t st, size_t fs, int W, int H, const mvsv_rect& q,
                     int64_t* sums, size_t ss)
{
    // strips start where a row is 4-byte aligned: row strides and frame stride multiples of 4
    const bool packed = st % 4 == 0 && (n == 1 || fs % 4 == 0);
    const int xs = packed ? q.x0 - (int)(((uintptr_t)img + q.x0) & 3) : q.x0;
    const int nstrips = (q.x1 - xs + 255) / 256, nbands = (q.y1 - q.y0 + kShBand - 1) / kShBand;
    const int nblk = (int)std::min<long>(kShBlocks, ((long)nstrips * nbands + 3) / 4);
    int rc;
    // room for 16 frames at least: the usual batches never grow (and so never synchronise) it
    if ((rc = ensure(ctx, ctx->sh_part, (size_t)std::max(n, 16) * kShBlocks * sizeof(unsigned long long),
                     "sharpness partials")))
        return rc;
    unsigned long long* part = (unsigned long long*)ctx->sh_part.ptr;
    hipLaunchKernelGGL(sharpness_kernel, dim3(nblk, n), dim3(256), 0, ctx->stream, img, st, fs, W, H, q.x0, q.y0, q.x1,
                       q.y1, xs, packed ? 1 : 0, nstrips, nbands, part);
    hipLaunchKernelGGL(sharpness_fold_kernel, dim3(n), dim3(64), 0, ctx->stream, (const unsigned long long*)part, nblk,
                       sums, ss);
    return check_hip(ctx, hipGetLastError(), "sharpness");
}

int remap_fixed_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t ss, size_t sfs, int sw, int sh,
                       const int16_t* xy, size_t xs, const uint16_t* frac, size_t fs, uint8_t* dst, size_t ds,
                       size_t dfs, int dw, int dh)
{
    dim3 grid((dw + 63) / 64, (dh + 3) / 4, n);
    hipLaunchKernelGGL(remap_fixed_kernel, grid, dim3(256), 0, ctx->stream, src, ss, sfs, sw, sh, xy, xs, frac, fs,
                       dst, ds, dfs, dw, dh);
    return check_hip(ctx, hipGetLastError(), "remap fixed");
}

int remap_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t ss, size_t sfs, int sw, int sh,
                 const float* mx, const float* my, size_t ms, uint8_t* dst, size_t ds, size_t dfs,
                 int dw, int dh)
{
    dim3 grid((dw + 63) / 64, (dh + 3) / 4, n);
    hipLaunchKernelGGL(remap_linear_kernel, grid, dim3(256), 0, ctx->stream, src, ss, sfs, sw, sh,
                       mx, my, ms, dst, ds, dfs, dw, dh);
    return check_hip(ctx, hipGetLastError(), "remap");
}

int rectify_pair_device(mvsv_ctx* ctx, int n, const uint8_t* raw, int sw, int sh, const int16_t* xy,
                        const uint16_t* frac, size_t ms, int dw, int dh, uint8_t* dL, uint8_t* dR, size_t ds,
                        size_t dfs)
{
    dim3 grid((dw + 255) / 256, (dh + 3) / 4, 2 * n);
    hipLaunchKernelGGL(rectify_pair_kernel, grid, dim3(256), 0, ctx->stream, raw, sw, sh, xy, frac, ms, dL, dR, ds,
                       dfs, dw, dh);
    return check_hip(ctx, hipGetLastError(), "rectify pair");
}

int resize_size(int sw, int sh, double fx, double fy, int* dw, int* dh)
{
    if (sw <= 0 || sh <= 0 || !(fx > 0) || !(fy > 0)) return MVSV_E_INVALID_ARG;
    const double w = std::nearbyint(sw * fx), h = std::nearbyint(sh * fy);  // cvRound (half to even)
    if (!(w >= 1 && h >= 1 && w <= 1 << 20 && h <= 1 << 20)) return MVSV_E_INVALID_ARG;
    *dw = (int)w;
    *dh = (int)h;
    return MVSV_OK;
}

int resize_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t ss, size_t sfs, int sw, int sh, double fx,
                  double fy, uint8_t* dst, size_t ds, size_t dfs)
{
    int dw, dh;
    if (resize_size(sw, sh, fx, fy, &dw, &dh)) return set_error(ctx, MVSV_E_INVALID_ARG, "bad resize factors");
    if (ds < (size_t)dw) return set_error(ctx, MVSV_E_INVALID_ARG, "resize destination stride smaller than width");
    if (dw == sw && dh == sh) {
        // [OpenCV 3.4 resize] dsize == ssize: src.copyTo(dst), whatever fx, fy
        for (int f = 0; f < n; f++) {
            const int rc = check_hip(ctx, hipMemcpy2DAsync(dst + (size_t)f * dfs, ds, src + (size_t)f * sfs, ss, sw, sh,
                                                           hipMemcpyDeviceToDevice, ctx->stream),
                                     "resize copy");
            if (rc) return rc;
        }
        return MVSV_OK;
    }
    const double scale_x = 1.0 / fx, scale_y = 1.0 / fy;
    const double isx = std::nearbyint(scale_x), isy = std::nearbyint(scale_y);
    const bool area2 = std::fabs(scale_x - isx) < DBL_EPSILON && std::fabs(scale_y - isy) < DBL_EPSILON &&
                       isx == 2.0 && isy == 2.0;
    // columns the SIMD vertical op covers: its 16-wide loop, then its 8-wide one
    int simd_end = 0;
    while (simd_end <= dw - 16) simd_end += 16;
    while (simd_end < dw - 8) simd_end += 8;
    dim3 grid((dw + 63) / 64, (dh + 3) / 4, n);
    hipLaunchKernelGGL(resize_linear_kernel, grid, dim3(256), 0, ctx->stream, src, ss, sfs, sw, sh, scale_x,
                       scale_y, area2 ? 1 : 0, simd_end, dst, ds, dfs, dw, dh);
    return check_hip(ctx, hipGetLastError(), "resize");
}

int reproject_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                     const float* Q, float* out, size_t os, size_t ofs)
{
    QMat q;
    for (int i = 0; i < 16; i++) q.q[i] = Q[i];
    dim3 grid((W + 63) / 64, (H + 3) / 4, n);
    hipLaunchKernelGGL(reproject_kernel, grid, dim3(256), 0, ctx->stream, dmap, st, fs, W, H, q,
                       (float4*)out, os, ofs);
    return check_hip(ctx, hipGetLastError(), "reprojection");
}

int point_cloud_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H, const float* Q,
                       mvsv_cloud_point* records, int capacity, int* counts, size_t cs, int* minmax, size_t ms)
{
    int rc, head, nvec;
    // (min, max) per frame, then (first record, min | max) per row; room for 16
    // frames of 1024 rows at least, so the usual streams never grow (and so never
    // synchronise) it
    const size_t need = (size_t)n * ((size_t)H + 1);
    if ((rc = ensure(ctx, ctx->cl_rows, std::max(need, (size_t)16 * 1025) * sizeof(int2), "point cloud row counts")))
        return rc;
    int2* frames = (int2*)ctx->cl_rows.ptr;
    int2* rows = frames + n;
    QMat q;
    for (int i = 0; i < 16; i++) q.q[i] = Q[i];
    display_split(dmap, st, fs, n, W, &head, &nvec);
    dim3 grid((H + 3) / 4, n);
    hipLaunchKernelGGL(cloud_rows_kernel, grid, dim3(256), 0, ctx->stream, dmap, st, fs, W, H, head, nvec, rows);
    hipLaunchKernelGGL(cloud_scan_kernel, dim3(n), dim3(kCloudScan), 0, ctx->stream, rows, H, frames, counts, cs,
                       minmax, ms);
    hipLaunchKernelGGL(cloud_scatter_kernel, grid, dim3(256), 0, ctx->stream, dmap, st, fs, W, H, head, nvec, q,
                       (const int2*)rows, (const int2*)frames, (float4*)records, capacity);
    return check_hip(ctx, hipGetLastError(), "point cloud");
}

}  // namespace mvsv
