// mvsv_sgbm_lines.hpp — SGBM path aggregation along scanlines, 16 (or 8) lanes
// per line: one direction per launch (sgbm_path16_kernel) or all directions of
// a small launch side by side (sgbm_pathdirs16_kernel).
#pragma once

#include "mvsv_sgbm_common.hpp"

namespace mvsv {
namespace {

// ---------------------------------------------------------------------------
// 4b. path aggregation, 16 lanes per scanline (D = 32 * NP, NP in {1,2,4,8}).
// A wave walks four scanlines at once, one per 16-lane DPP row: every lane
// owns 2*NP consecutive disparities (16 B of C per lane for D = 128), the d+-1
// neighbours cross lanes with row_shr/row_shl, the per-step min over d is a
// four-step DPP butterfly inside the row (no readlane / SGPR round trip).
// Rows whose scanline is shorter than the wave's longest one keep running on
// clamped loads and store into a private dummy slot (branch-free memory).
// ---------------------------------------------------------------------------
constexpr int kPath16PF = 12;

// LPC lanes per line (2*NP disparities each, D = 2*NP*LPC): 16 (a DPP row),
// or 8 for D = 16 (captureDisparity's create(0, 16, 5, 200, 800)), eight lines
// per wave
template <int LPC>
constexpr int path16_lines_per_block() { return 4 * (64 / LPC); }

template <int NP, bool FIRST, typename AccT, bool NW = false, bool RES = false, int LPC = 16>
__device__ __forceinline__ void path16_lines(const void* __restrict__ C, AccT* __restrict__ A,
                                             AccT* __restrict__ dummy, int H, int W1, int D, int dx,
                                             int dy, int P1, int P2, int bx, int f)
{
    static_assert(LPC == 8 || LPC == 16, "row-DPP segments of 8 or 16 lanes");
    using AV = AccVec<NP, AccT>;
    using CI = CostIn<NP, RES>;
    constexpr int PF = kPath16PF;
    constexpr int LPW = 64 / LPC;  // lines per wave
    const int lane = threadIdx.x & 63;
    const int row = lane / LPC, rl = lane % LPC;
    const int nl = num_lines(dx, dy, W1, H);
    const int line0 = __builtin_amdgcn_readfirstlane((bx * 4 + (int)(threadIdx.x >> 6)) * LPW);
    if (line0 >= nl) return;
    const int line = min(line0 + row, nl - 1);
    const Line g = line_geometry(line, dx, dy, W1, H);
    const int len = line0 + row < nl ? g.len : 0;
    int maxlen = __builtin_amdgcn_readlane(len, 0);
#pragma unroll
    for (int r = 1; r < LPW; r++) maxlen = max(maxlen, __builtin_amdgcn_readlane(len, r * LPC));
    const size_t frame = (size_t)H * W1 * D;
    const ptrdiff_t step = ((ptrdiff_t)dy * W1 + dx) * D;
    const int d0 = rl * 2 * NP;
    const size_t off = f * frame + ((size_t)g.ys * W1 + g.xs) * D + d0;
    const void* cp = CI::at(C, (ptrdiff_t)off);
    AccT* ap = acc_add(A, (ptrdiff_t)off);
    AccT* dp = acc_add(dummy, (ptrdiff_t)threadIdx.x * 2 * NP);
    const int last = max(len - 1, 0);
    uint32_t lp[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) lp[p] = 0u;
    const uint32_t p1x2 = (uint32_t)(P1 & 0xffff) * 0x10001u;
    const uint32_t p2x2 = (uint32_t)(P2 & 0xffff) * 0x10001u;
    int minp = 0;

    CI cb[PF];
    uint32_t ab[PF][NP];
#pragma unroll
    for (int j = 0; j < PF; j++) {
        const ptrdiff_t t = min(j, last);
        cb[j].load(CI::at(cp, t * step));
        if constexpr (!FIRST) AV::load(acc_add(ap, t * step), ab[j]);
    }
    auto body = [&](int s, int j) {
        const uint32_t delta2 = sgm_delta2<NW>(minp, P2);
        uint32_t c[NP], ln[NP], o[NP], tt[NP];
        cb[j].get(c);
        sgm_step_row_t<NP, NW, LPC>(lp, delta2, p1x2, c, ln, tt);
        minp = seg_lane_min<LPC>(lane_min_row<NP>(ln));
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const uint32_t dv = sgm_delta<NW>(tt[p], p2x2);  // delta = t + P2 = P2 - u
            if constexpr (FIRST)
                o[p] = dv;
            else
                o[p] = AV::add(ab[j][p], dv);
            lp[p] = ln[p];
        }
        AccT* dst = s < len ? acc_add(ap, (ptrdiff_t)s * step) : dp;
        AV::store(dst, o);
    };
    int s = 0;
    for (; s + PF <= maxlen; s += PF) {
#pragma unroll
        for (int j = 0; j < PF; j++) {
            body(s + j, j);
            const ptrdiff_t t = min(s + j + PF, last);
            cb[j].load(CI::at(cp, t * step));
            if constexpr (!FIRST) AV::load(acc_add(ap, t * step), ab[j]);
        }
    }
    const int rem = maxlen - s;
#pragma unroll
    for (int j = 0; j < PF; j++)
        if (j < rem) body(s + j, j);
}


template <int NP, bool FIRST, typename AccT, bool NW = false, bool RES = false>
__global__ __launch_bounds__(256) void sgbm_path16_kernel(const void* __restrict__ C,
                                                          AccT* __restrict__ A,
                                                          AccT* __restrict__ dummy, int H, int W1,
                                                          int D, int dx, int dy, int P1, int P2)
{
    path16_lines<NP, FIRST, AccT, NW, RES>(C, A, dummy, H, W1, D, dx, dy, P1, P2, blockIdx.x, blockIdx.y);
}

// All directions of a small launch at once (blockIdx.z = direction k, its
// deltas into plane k): one frame's 4 or 7 line directions run side by side
// instead of as sheared strips, whose 480-step chain is the single-frame
// critical path.
struct PathDirs {
    int dx[8], dy[8];
};
template <int NP, typename AccT, bool NW, bool RES = false, int LPC = 16>
__global__ __launch_bounds__(256) void sgbm_pathdirs16_kernel(const void* __restrict__ C,
                                                              AccT* __restrict__ A, size_t plane,
                                                              AccT* __restrict__ dummy, int H, int W1,
                                                              int D, PathDirs dirs, int P1, int P2)
{
    const int k = blockIdx.z;
    path16_lines<NP, true, AccT, NW, RES, LPC>(C, acc_add(A, (ptrdiff_t)k * (ptrdiff_t)plane), dummy, H, W1, D,
                                          dirs.dx[k], dirs.dy[k], P1, P2, blockIdx.x, blockIdx.y);
}

// the line directions: the first four are MODE_SGBM's, the first seven
// MODE_HH's, MODE_HH4's are L->R, down and up (sgbm_pass_dir picks a mode's
// k-th); the last is R->L as a chain set of its own (the split WTA form)
constexpr int kPathDirs[8][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {1, -1}, {0, -1}, {-1, -1}, {-1, 0}};

}  // namespace
}  // namespace mvsv
