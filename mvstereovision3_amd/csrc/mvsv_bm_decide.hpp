// mvsv_bm_decide.hpp — the per-row decision phase of the disparities-on-the-lanes
// StereoBM kernels, from the [column][disparity] slab of window sums on: argmin
// (ties -> smallest index), uniqueness test, parabola neighbours, texture verdict,
// the per-wave output records and their flush.  The slab layout, the lane roles
// and the record format are bm_match2_kernel's (mvsv_bm.hip); the census kernel
// (mvsv_bm_census.hip) fills the same slab from popcounts and has no texture sums.
#pragma once

#include "mvsv_device.hpp"
#include "mvsv_internal.hpp"

namespace mvsv {
namespace bm2 {

constexpr int kCols = 16;              // output columns per column group
constexpr int kWaves = 4;              // waves per block
constexpr uint32_t kPad = 0x10000u;    // per-column offset of the unused disparity lanes

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the NR waves of a column group meet (NR == 2: both groups, the whole block)
template <int NR>
__device__ __forceinline__ void group_sync()
{
    if constexpr (NR == 1)
        wave_sync();
    else
        __syncthreads();
}

// what a block knows about its place in the launch
struct Where {
    int f, xl0, c0, yr0, W, H, keep_border;
    int16_t* out;
    size_t os, ofs;
    int* cost;
};

// output records: rows t0 .. t0 + cnt - 1 of the wave's CPW columns; lane
// (slot, column) = (lane / CPW, lane % CPW)
template <int NR>
__device__ __forceinline__ void flush(const uint2* recs, int lane, int g, int t0, int cnt, const BmEff& e,
                                      const Where& w)
{
    constexpr int CPW = kCols / NR;
    wave_sync();  // the h == 0 lanes' records
    const int slot = lane / CPW, qf = g * CPW + lane % CPW;
    const int xf = w.xl0 + w.c0 + qf, xi = e.lofs + xf;
    if (slot < cnt && xf < e.ncol) {
        const uint2 r = recs[lane];
        const int y = w.yr0 + t0 + slot;
        const int nd = e.ndisp;
        const int mind = (int)(r.x & 0xffu);
        const int minsad = (int)((r.x & 0x3fffffffu) >> 8);
        int16_t res = (int16_t)e.filtered;
        const bool fail = (!w.keep_border && (xi < e.xmin || xi >= e.xmax)) || (r.x >> 30) != 0;
        if (!fail) {
            const int pp = (int)(r.y & 0xffffu), nn = (int)(r.y >> 16);
            const int v1 = nd - mind - 1 + e.mindisp;
            int val;
            if (0 < mind && mind < nd - 1) {
                const int d = pp + nn - 2 * minsad + abs(pp - nn);
                val = (v1 * 256 + (d != 0 ? (pp - nn) * 256 / d : 0) + 15) >> 4;
            } else {
                val = (v1 * 256 + 15) >> 4;
            }
            res = (int16_t)val;
            if (w.cost) w.cost[((size_t)w.f * w.H + y) * w.W + xi] = minsad;
        }
        w.out[w.f * w.ofs + (size_t)y * w.os + xi] = res;
    }
}

// One row of a column group after its slab sadx[column][NR * 64 + 4] is written:
// 4 NR lanes per output column (each wave of the group takes 16 / NR of the
// columns), each lane scanning 16 disparity indices; keys (sad << 8 | index),
// DPP reductions; the uniqueness test masks the winner and its two neighbours in
// the slab and takes a second minimum.  TEX: tcb holds the texture column sums of
// the wave's virtual columns and the window's sum is tested against e.tex.
template <int NR, int WIN, bool TEX>
__device__ __forceinline__ void decide_row(uint32_t* sadx, const int* tcb, uint2* recs, int lane, int g, int t,
                                           int rows, const BmEff& e, const Where& w)
{
    constexpr int SS = NR * 64 + 4;
    constexpr int LPC = 4 * NR, CPW = kCols / NR, RB = LPC;
    const int qx = g * CPW + lane / LPC, h = lane % LPC;
    group_sync<NR>();
    uint32_t* srow = sadx + qx * SS;
    const int k0 = h * 16;
    // argmin over this lane's 16 slab entries, keys (sad << 8) | index
    uint32_t best;
    {
        uint32_t key[16];
#pragma unroll
        for (int i = 0; i < 16; i += 4) {
            const uint4 q = *(const uint4*)(srow + k0 + i);
            key[i] = (q.x << 8) | (uint32_t)i;
            key[i + 1] = (q.y << 8) | (uint32_t)(i + 1);
            key[i + 2] = (q.z << 8) | (uint32_t)(i + 2);
            key[i + 3] = (q.w << 8) | (uint32_t)(i + 3);
        }
        best = min(key[0], key[1]);
#pragma unroll
        for (int i = 2; i < 16; i += 2) best = min(min(best, key[i]), key[i + 1]);
        best |= (uint32_t)k0;
    }
    best = min(best, (uint32_t)__builtin_amdgcn_mov_dpp((int)best, 0xB1, 0xf, 0xf, false));
    best = min(best, (uint32_t)__builtin_amdgcn_mov_dpp((int)best, 0x4E, 0xf, 0xf, false));
    if constexpr (NR == 2)  // row_half_mirror: quad 0 <-> quad 1 of each 8 lanes
        best = min(best, (uint32_t)__builtin_amdgcn_mov_dpp((int)best, 0x141, 0xf, 0xf, false));
    const int mind = (int)(best & 0xff);
    const uint32_t minsad = best >> 8;
    // parabola neighbours (read before the uniqueness pass masks them)
    const int pp = (int)srow[min(mind + 1, 64 * NR - 1)];
    const int nn = (int)srow[max(mind - 1, 0)];
    bool bad = false;
    if (e.uniq > 0) {
        const uint32_t ms = minsad;
        const uint32_t thresh = ms + (uint32_t)((int)ms * e.uniq / 100);
        wave_sync();  // every lane of the column has read the slab row
        if (h == 0) {
            srow[mind] = 0xffffffffu;
            if (mind > 0) srow[mind - 1] = 0xffffffffu;
            if (mind + 1 < 64 * NR) srow[mind + 1] = 0xffffffffu;
        }
        wave_sync();
        uint32_t m2 = 0xffffffffu;
#pragma unroll
        for (int i = 0; i < 16; i += 4) {
            const uint4 q = *(const uint4*)(srow + k0 + i);
            m2 = min(min(m2, q.x), q.y);
            m2 = min(min(m2, q.z), q.w);
        }
        m2 = min(m2, (uint32_t)__builtin_amdgcn_mov_dpp((int)m2, 0xB1, 0xf, 0xf, false));
        m2 = min(m2, (uint32_t)__builtin_amdgcn_mov_dpp((int)m2, 0x4E, 0xf, 0xf, false));
        if constexpr (NR == 2)
            m2 = min(m2, (uint32_t)__builtin_amdgcn_mov_dpp((int)m2, 0x141, 0xf, 0xf, false));
        bad = m2 <= thresh;
    }
    bool flat = false;
    if constexpr (TEX) {
        int tsum = 0;
#pragma unroll
        for (int qq = 0; qq < WIN; qq++) tsum += tcb[qx + qq];
        flat = tsum < e.tex;
    }
    // park the column's verdict; every RB rows the wave's 64 lanes finish
    // RB x CPW pixels at once (division, stores) instead of 16 / NR lanes per row
    if (h == 0)
        recs[(t & (RB - 1)) * CPW + lane / LPC] =
            make_uint2(best | (bad ? 1u << 31 : 0u) | (flat ? 1u << 30 : 0u),
                       ((uint32_t)pp & 0xffffu) | ((uint32_t)nn << 16));
    if ((t & (RB - 1)) == RB - 1 || t == rows - 1) flush<NR>(recs, lane, g, t & ~(RB - 1), (t & (RB - 1)) + 1, e, w);
    group_sync<NR>();
}

}  // namespace bm2
}  // namespace mvsv
