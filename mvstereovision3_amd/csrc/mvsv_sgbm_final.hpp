// mvsv_sgbm_final.hpp — the last SGBM stage on packed planes: the R->L
// direction fused with WTA, uniqueness, sub-pixel fit, right-view keys and the
// left-right check (sgbm_final16_kernel, launch_final16), and the WTA of the
// split side-by-side form (sgbm_wta_planes_kernel).
#pragma once

#include "mvsv_sgbm_common.hpp"

namespace mvsv {
namespace {

// ---------------------------------------------------------------------------
// 5b. last direction (R->L) + WTA + uniqueness + sub-pixel + LR check with 16
// lanes per image row (4 rows per wave).  The right-view map is built with
// order-independent atomicMin on keys (minS << 16 | 0xFFFF - x): smallest cost,
// then the largest x -- exactly OpenCV's descending scan with a strict '>'.
// ---------------------------------------------------------------------------

#ifndef MVSV_FINAL32_PF
#define MVSV_FINAL32_PF 8  // steps of prefetch in the 32-lanes-per-row final kernel
#endif
#ifndef MVSV_FINAL_LPR
#define MVSV_FINAL_LPR 32  // lanes per row of the final kernel for D >= 128 (16: A/B)
#endif

// Raw accumulator words of one lane (2*NP disparities): the NACC planes are
// summed in storage format -- u8 bytes never carry because the total over all
// directions is <= ndir*P2 <= 255 (acc_is_u8) -- and unpacked to u16 pairs once.
template <int NP, typename AccT>
struct AccRaw;
template <int NP>
struct AccRaw<NP, uint8_t> {
    static constexpr int NW = NP >= 2 ? NP / 2 : 1;
    static __device__ __forceinline__ void load(const uint8_t* p, uint32_t (&w)[NW])
    {
        if constexpr (NP == 1) {
            w[0] = *(const uint16_t*)p;
        } else if constexpr (NP == 2) {
            w[0] = *(const uint32_t*)p;
        } else if constexpr (NP == 4) {
            const uint2 t = *(const uint2*)p;
            w[0] = t.x;
            w[1] = t.y;
        } else {
            const uint4 t = *(const uint4*)p;
            w[0] = t.x;
            w[1] = t.y;
            w[2] = t.z;
            w[3] = t.w;
        }
    }
    static __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) { return a + b; }
    static __device__ __forceinline__ void unpack(const uint32_t (&w)[NW], uint32_t (&v)[NP])
    {
#pragma unroll
        for (int p = 0; p < NP; p++) v[p] = u8x2_to_u16x2(w[p >> 1], p & 1);
    }
    template <int NACC>
    static __device__ __forceinline__ void combine(const uint32_t (&w)[NACC][NW], uint32_t (&v)[NP])
    {
        uint32_t s[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) {
            s[k] = w[0][k];
#pragma unroll
            for (int i = 1; i < NACC; i++) s[k] = add(s[k], w[i][k]);
        }
        unpack(s, v);
    }
};
template <int NP>
struct AccRaw<NP, uint16_t> {
    static constexpr int NW = NP;
    static __device__ __forceinline__ void load(const uint16_t* p, uint32_t (&w)[NW])
    {
        AccVec<NP, uint16_t>::load(p, w);
    }
    static __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b)
    {
        return AccVec<NP, uint16_t>::add(a, b);
    }
    static __device__ __forceinline__ void unpack(const uint32_t (&w)[NW], uint32_t (&v)[NP])
    {
#pragma unroll
        for (int p = 0; p < NP; p++) v[p] = w[p];
    }
    template <int NACC>
    static __device__ __forceinline__ void combine(const uint32_t (&w)[NACC][NW], uint32_t (&v)[NP])
    {
        uint32_t s[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) {
            s[k] = w[0][k];
#pragma unroll
            for (int i = 1; i < NACC; i++) s[k] = add(s[k], w[i][k]);
        }
        unpack(s, v);
    }
};
// Nibble planes (AccVec<NP, nib2_t> layout): the planes' sums exceed a
// nibble, so each word is split into its even and odd nibbles as bytes
// (E, O), the planes are added bytewise (<= NACC * 15), then spread to pairs.
template <int NP>
struct AccRaw<NP, nib2_t> {
    static constexpr int NW = NP >= 4 ? NP / 4 : 1;
    static __device__ __forceinline__ void load(const nib2_t* p, uint32_t (&w)[NW])
    {
        if constexpr (NP == 1) {
            w[0] = *(const uint8_t*)p;
        } else if constexpr (NP == 2) {
            w[0] = *(const uint16_t*)p;
        } else if constexpr (NP == 4) {
            w[0] = *(const uint32_t*)p;
        } else {
            const uint2 t = *(const uint2*)p;
            w[0] = t.x;
            w[1] = t.y;
        }
    }
    template <int NACC>
    static __device__ __forceinline__ void combine(const uint32_t (&w)[NACC][NW], uint32_t (&v)[NP])
    {
        constexpr uint32_t M = 0x0f0f0f0fu;
#pragma unroll
        for (int k = 0; k < NW; k++) {
            uint32_t E = w[0][k] & M, O = (w[0][k] >> 4) & M;
#pragma unroll
            for (int i = 1; i < NACC; i++) {
                E += w[i][k] & M;
                O += (w[i][k] >> 4) & M;
            }
            if constexpr (NP >= 4) {
                // E bytes: d0 d1 d4 d5, O bytes: d2 d3 d6 d7
                v[4 * k + 0] = __builtin_amdgcn_perm(0u, E, 0x0c010c00u);
                v[4 * k + 1] = __builtin_amdgcn_perm(0u, O, 0x0c010c00u);
                v[4 * k + 2] = __builtin_amdgcn_perm(0u, E, 0x0c030c02u);
                v[4 * k + 3] = __builtin_amdgcn_perm(0u, O, 0x0c030c02u);
            } else if constexpr (NP == 2) {
                // E bytes: lo0 hi0, O bytes: lo1 hi1
                v[0] = __builtin_amdgcn_perm(0u, E, 0x0c010c00u);
                v[1] = __builtin_amdgcn_perm(0u, O, 0x0c010c00u);
            } else {
                v[0] = (E & 0xffu) | ((O & 0xffu) << 16);
            }
        }
    }
};

// Steps of C / accumulator prefetch: as deep as ~160 VGPRs of buffers allow
// (a power of two dividing the 16-step flush period).  The kernel is bound by
// load latency at ~2 waves per SIMD, so depth is what buys bandwidth.
template <int NP, int NACC, typename AccT, bool UQ>
constexpr int final16_pf()
{
    constexpr int words = NP + NACC * AccRaw<NP, AccT>::NW;  // VGPRs per step
    // three or more planes (MODE_HH, side by side) unpack more per step: at
    // 160 buffer VGPRs those instances spilled 36-105 VGPRs (round 6 audit)
    constexpr int budget = UQ ? 96 : (NACC >= 3 ? 80 : 160);
    return budget / words >= 16 ? 16 : (budget / words >= 8 ? 8 : 4);
}

// raw buffer loads of BYTES bytes into little-endian words (zero-extended)
constexpr int kBufWord3 = 0x00020000;  // buffer descriptor word 3: 32-bit data format
template <int BYTES, int NWD>
__device__ __forceinline__ void buf_words(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff,
                                          uint32_t (&w)[NWD])
{
    if constexpr (BYTES == 1) {
        w[0] = __builtin_amdgcn_raw_buffer_load_b8(r, voff, soff, 0);
    } else if constexpr (BYTES == 2) {
        w[0] = __builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0);
    } else if constexpr (BYTES == 4) {
        w[0] = __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
    } else if constexpr (BYTES == 8) {
        const auto t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
        w[0] = t[0];
        w[1] = t[1];
    } else {
        static_assert(BYTES % 16 == 0 && NWD == BYTES / 4, "buffer load size");
#pragma unroll
        for (int q = 0; q < BYTES / 16; q++) {
            const auto t = __builtin_amdgcn_raw_buffer_load_b128(r, voff + 16 * q, soff, 0);
#pragma unroll
            for (int k = 0; k < 4; k++) w[4 * q + k] = t[k];
        }
    }
}

// a * b + c per u16 half, saturated at 0xffff (VOP3P clamp)
__device__ __forceinline__ uint32_t pk_mad_u16_clamp(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_pk_mad_u16 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// NACC accumulator planes (A + i * plane) hold the summed deltas of disjoint
// direction groups written by concurrent passes; their sum is the S input.
// UQ: uniquenessRatio > 0.
// RESF (round 4; uniquenessRatio == 0 only, no-wrap regime): the recurrence
// and the WTA run on the residual plane R instead of C.  With C' = C - m
// (m = the pixel's minimum cost, Mv) and C'' = min(C', 2 P2) = R - P2, the
// step computes S'' = n C'' + sum of deltas (n = 8 or 5 directions);
// S = min(n (m - P2) + S', MAX_COST) has the same argmin and ties as S'' (the
// minimum of S' is <= n P2 < 2 n P2 <= S'' of any clamped d), and with
// uniquenessRatio 0 no d is ever rejected.  Only the sub-pixel fit needs
// exact S(best -+ 1): where S'' >= 2 n P2 the residual
// may be clamped and the flush loads C(best -+ 1) from the cost volume (one
// 2-byte gather per pixel, issued one flush ahead of its use so the prefetch
// loads are never waited for).
template <int NP, int NACC, typename AccT, bool UQ, int LPR, bool NOWRAP = false, bool RESF = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NP >= 8 ? 1 : 2))) void sgbm_final16_kernel(const int16_t* __restrict__ C,
                                                         const AccT* __restrict__ A, size_t plane,
                                                         int H, int W, SgbmEff e,
                                                         int16_t* __restrict__ raw,
                                                         uint32_t* __restrict__ keys,
                                                         int16_t* __restrict__ dummy,
                                                         const uint8_t* __restrict__ Rv,
                                                         const uint16_t* __restrict__ Mv)
{
    static_assert(!(RESF && UQ), "the residual final kernel needs uniquenessRatio 0");
    using AR = AccRaw<NP, AccT>;
    constexpr int NW = AR::NW;
    // 32 lanes per row: twice the waves, so a shallower prefetch keeps the
    // kernel at <= 128 VGPRs (4 waves per SIMD); wide slots (u16 planes of D =
    // 256, config 5: 12 words per step) take 4 steps -- 8 spilled 14 VGPRs
    // into scratch (round 6 dispatch census, tests/test_kernel_scratch.py).
    // The step loop is unrolled by LPR, so PF must divide it.
    constexpr int kF32Words = (RESF ? 1 : NP) + NACC * AccRaw<NP, AccT>::NW;
    constexpr int PF = LPR == 32 ? (kF32Words > 24 ? 2 : kF32Words > 10 ? 4 : MVSV_FINAL32_PF)
                                 : (final16_pf<NP, NACC, AccT, UQ>() < LPR ? final16_pf<NP, NACC, AccT, UQ>() : LPR);
    static_assert(LPR % PF == 0, "prefetch slots must divide the unrolled step loop");
    constexpr int RPW = 64 / LPR;     // image rows per wave
    constexpr int DR = 2 * NP * LPR;  // disparities of a row (D)
    // S of the current step, one D-vector per row: S[best -+ 1] come back
    // through LDS instead of lane shuffles.
    __shared__ __attribute__((aligned(16))) uint16_t srow[RPW * DR];
    const int lane = threadIdx.x;
    const int row = lane / LPR, rl = lane % LPR;
    const bool seg_first = rl == 0, seg_last = rl == LPR - 1;
    const int yr = blockIdx.x * RPW + row;
    const bool exists = yr < H;
    const int y = min(yr, H - 1);
    const int f = blockIdx.y;
    const int D = e.D, W1 = e.W1, minD = e.minD, minX1 = e.minX1;
    const int INV = e.invalid;
    int16_t* orow = raw + ((size_t)f * H + y) * W;
    uint32_t* krow = keys + ((size_t)f * H + y) * W;
    if (exists)
        for (int x = rl; x < W; x += LPR) {
            orow[x] = (int16_t)INV;
            krow[x] = 0xffffffffu;
        }
    __threadfence_block();
    __syncthreads();

    const bool lane_rule = !e.fullDP && !(e.variant & MVSV_VARIANT_WTA_MIN_D);
    const size_t frame = (size_t)H * W1 * D;
    const int d0 = rl * 2 * NP;
    uint16_t* ms = srow + row * DR;
    uint32_t lp[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) lp[p] = 0u;
    const uint32_t p1x2 = (uint32_t)(e.P1 & 0xffff) * 0x10001u;
    const uint32_t p2x2 = (uint32_t)(e.P2 & 0xffff) * 0x10001u;
    // S = min(ndir*(C - P2) + sum of deltas, MAX_COST) = min((ndir-1)*cb + L + acc, MAX_COST)
    // with cb = C - P2, L = cb + delta of the R->L direction computed here
    const uint32_t ndm1 = (uint32_t)(sgbm_ndir(e) - 1) * 0x10001u;
    // The general form (NOWRAP false) where a cost may pass 32767: C is a signed int16 as in
    // OpenCV, S = clamp(ndir*(C - P2) + sum of deltas, -32768, MAX_COST) in int32 per half.
    // (Every L of a pixel and disparity has C's sign -- L = C + t, t in [-P2, 0], C >= P2 or
    // C < 0 -- so OpenCV's chain of saturating adds is this two-sided clamp of the sum.)  The
    // general form carries S as a signed half everywhere: the key's high half, the records,
    // the LDS row; the uniqueness minimum and the right-view keys take it biased by 32768.
    const bool sgn = !NOWRAP && sgbm_signed_costs(e);
    const int ndS = sgbm_ndir(e);
    const int uq = e.uniq;
    // tie order of the WTA key: d, or OpenCV's SIMD lane order for MODE_SGBM
    uint32_t subk[2 * NP];
#pragma unroll
    for (int i = 0; i < 2 * NP; i++) {
        const int d = d0 + i;
        subk[i] = lane_rule ? (uint32_t)(((d & 7) << 12) | (d >> 3)) : (uint32_t)d;
    }
    uint32_t dpair[NP];  // (d, d + 1) of each packed pair
#pragma unroll
    for (int p = 0; p < NP; p++) dpair[p] = (uint32_t)(d0 + 2 * p) | ((uint32_t)(d0 + 2 * p + 1) << 16);
    int minp = 0;

    // cost words per prefetch slot: NP packed pairs of C, or the lane's 2 NP
    // residual nibbles (NP bytes, one word)
    constexpr int NCW = RESF ? 1 : NP;
    uint32_t cw[PF][NCW];
    uint32_t ab[PF][NACC][NW];
    // Buffer loads: one descriptor per volume over the wave's RPW rows, the
    // lane's row/disparity offset in a VGPR and the column (x = W1 - 1 - t)
    // in the scalar offset, so the per-step address update is SALU work.
    const int ybase = (int)blockIdx.x * RPW;  // <= y
    const size_t rbase = f * frame + (size_t)ybase * W1 * D;
    const uint32_t loff = (uint32_t)((y - ybase) * W1 * D + d0);  // elements, even
    constexpr uint32_t kAccNum = (uint32_t)sizeof(AccT), kAccDen = AccEpu<AccT>::v;  // bytes per element
    constexpr uint32_t kCNum = RESF ? 1u : 4u, kCDen = 2u;  // cost input bytes per element: 1/2 or 2
    const int nrec_c = (int)((uint32_t)(RPW * W1 * D) * kCNum / kCDen);
    const int nrec_a = (int)((uint32_t)(RPW * W1 * D) * kAccNum / kAccDen);
    const void* cbase = RESF ? (const void*)(Rv + rbase / 2) : (const void*)(C + rbase);
    const __amdgpu_buffer_rsrc_t rc_c =
        __builtin_amdgcn_make_buffer_rsrc((void*)cbase, (short)0, nrec_c, kBufWord3);
    __amdgpu_buffer_rsrc_t rc_a[NACC];
#pragma unroll
    for (int i = 0; i < NACC; i++)
        rc_a[i] = __builtin_amdgcn_make_buffer_rsrc(
            (void*)acc_add(A, (ptrdiff_t)(rbase + (size_t)i * plane)), (short)0, nrec_a, kBufWord3);
    const uint32_t vo_c = loff * kCNum / kCDen, vo_a = loff * kAccNum / kAccDen;
    auto prefetch = [&](int j, ptrdiff_t t) {
        const uint32_t xd = (uint32_t)((W1 - 1 - (int)t) * D);
        buf_words<(int)(2 * NP * kCNum / kCDen)>(rc_c, vo_c, xd * kCNum / kCDen, cw[j]);
#pragma unroll
        for (int i = 0; i < NACC; i++)
            buf_words<2 * NP * kAccNum / kAccDen>(rc_a[i], vo_a, xd * kAccNum / kAccDen, ab[j][i]);
    };
#pragma unroll
    for (int j = 0; j < PF; j++) prefetch(j, min(j, W1 - 1));
    // Per step the row's 16 lanes agree on K = (minS << 16 | tie-order sub),
    // S[best-1], S[best+1] and the uniqueness verdict; they park that record in
    // LDS slot (s & 15) of the row, and every 16 steps lane rl picks up record
    // rl and the 16 lanes finish 16 columns at once (sub-pixel division, raw
    // store, right-view atomicMin) -- the per-step path stays branch-free so
    // consecutive steps overlap.
    __shared__ uint2 srec[RPW * LPR];
    uint2* recs = srec + row * LPR;
    auto body = [&](int s, int j) {
        const uint32_t delta2 = sgm_delta2<NOWRAP>(minp, e.P2);
        uint32_t c[NP], ln[NP], st[NP], acc[NP], tt[NP];
        if constexpr (RESF) {
            CostIn<NP, true> ci;
            ci.w[0] = cw[j][0];
            ci.get(c);
        } else {
#pragma unroll
            for (int p = 0; p < NP; p++) c[p] = cw[j][p];
        }
        sgm_step_seg_t<NP, LPR, NOWRAP>(lp, delta2, p1x2, c, ln, tt, seg_first, seg_last);
        minp = seg_min_i32<LPR>(lane_min_row<NP>(ln));
        AR::template combine<NACC>(ab[j], acc);
        typename std::conditional<NOWRAP, uint32_t, int>::type key = 0x7fffffff;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            if (sgn) {
                auto one = [&](uint32_t cw, uint32_t tw, uint32_t aw) -> uint32_t {
                    const int S32 = ndS * ((int)(int16_t)cw - e.P2) + (int)(aw & 0xffffu) + (int)(int16_t)tw + e.P2;
                    return (uint32_t)max(min(S32, kMaxCost), -32768) & 0xffffu;
                };
                st[p] = one(c[p] & 0xffffu, tt[p] & 0xffffu, acc[p]) | (one(c[p] >> 16, tt[p] >> 16, acc[p] >> 16) << 16);
            } else {
                // residual form (RESF): R >= P2, L + deltas <= 4 P2 + 7 P2 -- the
                // full-rate 32-bit sub / add never borrow or carry
                const uint32_t cbv = RESF ? sub2_nb(c[p], p2x2) : pk_sub_u16(c[p], p2x2);
                const uint32_t sv = pk_mad_u16_clamp(cbv, ndm1, RESF ? add2_nc(ln[p], acc[p]) : pk_add_u16(ln[p], acc[p]));
                st[p] = pk_min_u16(sv, 0x7fff7fffu);
            }
            lp[p] = ln[p];
            const uint32_t klo = (st[p] << 16) | subk[2 * p];
            const uint32_t khi = (st[p] & 0xffff0000u) | subk[2 * p + 1];
            if constexpr (NOWRAP)
                key = min(key, min(klo, khi));
            else
                key = min(key, min((int)klo, (int)khi));  // a signed S in the high half
        }
        const int K = seg_min_i32<LPR>((int)key);
        const int minS = K >> 16;
        const int sub = K & 0xffff;
        const int best = lane_rule ? (((sub & 0xfff) << 3) | (sub >> 12)) : sub;
        // S[best -+ 1] (clamped into [0, D)) through the row's LDS vector
        {
            Vec<NP> o;
#pragma unroll
            for (int p = 0; p < NP; p++) o.v[p] = st[p];
            o.store((int16_t*)(ms + d0));
        }
        // the wave barriers order the lanes' LDS hand-over for the compiler
        // (without them it moved accesses across lanes' writes: wrong maps)
        __builtin_amdgcn_wave_barrier();
        const int bm = max(best - 1, 0), bp = min(best + 1, DR - 1);
        const int Sm = ms[bm], Sp = ms[bp];  // (16 bits go into the record; the flush sign-extends them)
        int rej = 0;
        if constexpr (UQ) {
            // min of S outside [best-1, best+1]: y = best + 1 - d is <= 2
            // (unsigned) exactly there; those cells are lifted to >= 0xfffd
            const uint32_t b2 = (uint32_t)(best + 1) * 0x10001u;
            uint32_t m2 = 0xffffffffu;
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const uint32_t yv = pk_sub_u16(b2, dpair[p]);
                const uint32_t lift = pk_sub_u16(pk_min_u16(yv, 0x00030003u), 0x00030003u);
                if constexpr (NOWRAP)
                    m2 = pk_min_u16(m2, pk_max_u16(st[p], lift));
                else  // S biased by 32768 (order-preserving for a signed half); lifted cells to 0xffff
                    m2 = pk_min_u16(m2, pk_max_u16(st[p] ^ 0x80008000u, lift | ((lift >> 1) & 0x7fff7fffu)));
            }
            const int m2r = seg_min_i32<LPR>((int)min(m2 & 0xffffu, m2 >> 16));
            if constexpr (NOWRAP)
                rej = m2r < 0xfffd && m2r * (100 - uq) < minS * 100;
            else  // (D >= 16: a cell outside [best-1, best+1] always exists)
                rej = (m2r - 32768) * (100 - uq) < minS * 100;
        }
        if constexpr (NOWRAP)
            recs[s & (LPR - 1)] = make_uint2((uint32_t)K | ((uint32_t)rej << 31),
                                      ((uint32_t)Sp << 16) | ((uint32_t)Sm & 0xffffu));
        else  // bit 31 is S's sign: the verdict goes into bit 15 (sub has 15 bits)
            recs[s & (LPR - 1)] = make_uint2(((uint32_t)K & 0xffff7fffu) | ((uint32_t)rej << 15),
                                      ((uint32_t)Sp << 16) | ((uint32_t)Sm & 0xffffu));
        __builtin_amdgcn_wave_barrier();
    };
    // lane rl finishes column s0 + rl of the sweep (x = W1 - 1 - s)
    // Branch-free around memory (so the prefetch loads keep their exact
    // vmcnt accounting across the flush): a lane without a column stores to
    // its dummy slot, a rejected column rewrites INVALID, and an atomicMin
    // that must not count carries the all-ones key (a no-op).
    int16_t* dslot = dummy + (blockIdx.x & 63) * 64 + lane;
    // store + right-view key of one finished column (x, exact minS, Sm, Sp)
    auto finish = [&](bool own, int x, int best, int minS, int Sm, int Sp, int kRej) {
        if (minS >= kMaxCost) best = -1;  // no strict minimum below MAX_COST
        const int den = max(Sm + Sp - 2 * minS, 1);
        const int frac = ((Sm - Sp) * kDispScale + den) / (den * 2);
        // arithmetic mask, not a select: the division stays unconditional (no
        // branch inside the loop body)
        const int d16 = best * kDispScale + (frac & -(int)(0 < best && best < D - 1));
        const int16_t v = kRej ? (int16_t)INV : (int16_t)(d16 + minD * kDispScale);
        *(own ? orow + x + minX1 : dslot) = v;
        const int x2 = x + minX1 - best - minD;
        const bool hit = own && !kRej && minS < kMaxCost && x2 >= 0 && x2 < W;
        constexpr int kKeyBias = NOWRAP ? 0 : 32768;  // a signed minS orders as unsigned
        atomicMin(krow + clampi(x2, 0, W - 1),
                  hit ? (((uint32_t)(minS + kKeyBias) << 16) | (uint32_t)(0xffff - x)) : 0xffffffffu);
    };
    auto flush = [&](int s0, int cnt) {
        const int s = s0 + rl;
        const bool own = exists && rl < cnt;
        const uint2 rec = recs[rl];
        const uint32_t kK = rec.x & 0x7fffffffu, kS = rec.y;
        const int kRej = NOWRAP ? (int)(rec.x >> 31) : (int)((rec.x >> 15) & 1u);
        const int minS = NOWRAP ? (int)(kK >> 16) : ((int)rec.x >> 16);
        const int sub = NOWRAP ? (int)(kK & 0xffffu) : (int)(rec.x & 0x7fffu);
        const int best = lane_rule ? (((sub & 0xfff) << 3) | (sub >> 12)) : sub;
        const int Sm = (int)(int16_t)(kS & 0xffffu), Sp = (int)(int16_t)(kS >> 16);
        finish(own, W1 - 1 - s, best, minS, Sm, Sp, kRej);
    };
    // RESF: a flush reads its columns' records and issues their loads (the
    // pixel minimum, C(best -+ 1) where the residual may be clamped); the next
    // flush (or the row end) finishes them.  Pending state per lane: the
    // record and three loaded values (the column and ownership follow from
    // the pending flush's first step and count, wave-uniform).
    struct Pend {
        uint2 rec;
        int mC;
        uint2 cw;  // C[base .. base + 3] of the column, base = min((best - 1) & ~1, D - 4)
    } pend{};
    int pend_s0 = 0, pend_cnt = 0;
    const int16_t* crow = C + f * frame + (size_t)y * W1 * D;
    const uint16_t* mrowp = RESF ? Mv + ((size_t)f * H + y) * W1 : nullptr;
    const int ndir = sgbm_ndir(e);
    const int clampS = ndir * 2 * e.P2;  // S'' >= this: C'' may be the clamp value
    auto rec_best = [&](uint32_t kK) {
        const int sub = (int)(kK & 0xffffu);
        return lane_rule ? (((sub & 0xfff) << 3) | (sub >> 12)) : sub;
    };
    auto finish_res = [&](const Pend& q, int s0, int cnt) {
        const uint32_t kK = q.rec.x & 0x7fffffffu;
        const int base = ndir * (q.mC - e.P2);  // S = min(base + S', MAX_COST)
        auto exact = [&](int Spp, int cv) -> int {
            // S'' = ndir C'' + deltas; where the flush loaded C(d) (S'' >=
            // clampS: cv is exact, else a placeholder) replace C'' = min(C', 2 P2)
            // by C'
            const int c1 = Spp >= clampS ? cv - q.mC : 0;
            return min(base + Spp + ndir * (c1 - min(c1, 2 * e.P2)), kMaxCost);
        };
        const int best = rec_best(kK);
        const int bm = max(best - 1, 0), bp = min(best + 1, D - 1);
        const int cb0 = min(bm & ~1, D - 4);
        auto cword = [&](int d) -> int {  // C(d) out of the loaded 4-element window
            const int i = d - cb0;
            const uint32_t w = (i & 2) ? q.cw.y : q.cw.x;
            return (int)((i & 1) ? (w >> 16) : (w & 0xffffu));
        };
        const int Sm = exact((int)(q.rec.y & 0xffffu), cword(bm)), Sp = exact((int)(q.rec.y >> 16), cword(bp));
        finish(exists && rl < cnt, W1 - 1 - (s0 + rl), best, min(base + (int)(kK >> 16), kMaxCost), Sm, Sp, 0);
    };
    auto flush_res = [&](int s0, int cnt) {
        Pend q;
        const bool own = exists && rl < cnt;
        q.rec = recs[rl];
        const int best = rec_best(q.rec.x & 0x7fffffffu);
        const int xc = own ? W1 - 1 - (s0 + rl) : 0;
        q.mC = mrowp[xc];
        // C(best - 1) and C(best + 1) in one 8-byte load (4-byte aligned, inside
        // the pixel's D costs); one shared address for the lanes that need no
        // exact cost
        const int cb0 = min(max(best - 1, 0) & ~1, D - 4);
        const bool need = own && ((int)(q.rec.y & 0xffffu) >= clampS || (int)(q.rec.y >> 16) >= clampS);
        q.cw = *(const uint2*)(crow + (need ? (size_t)xc * D + cb0 : 0));
        finish_res(pend, pend_s0, pend_cnt);  // the previous flush's columns (none the first time)
        pend = q;
        pend_s0 = s0;
        pend_cnt = cnt;
    };
    int s = 0;
    for (; s + LPR <= W1; s += LPR) {
#pragma unroll
        for (int j = 0; j < LPR; j++) {
            body(s + j, j % PF);
            prefetch(j % PF, min(s + j + PF, W1 - 1));
        }
        if constexpr (RESF)
            flush_res(s, LPR);
        else
            flush(s, LPR);
    }
    const int rem = W1 - s;
#pragma unroll
    for (int j = 0; j < LPR; j++) {
        if (j < rem) {
            body(s + j, j % PF);
            prefetch(j % PF, min(s + j + PF, W1 - 1));
        }
    }
    if constexpr (RESF) {
        if (rem > 0) flush_res(s, rem);
        finish_res(pend, pend_s0, pend_cnt);
    } else {
        if (rem > 0) flush(s, rem);
    }
    __threadfence_block();
    __syncthreads();
    if (!exists) return;
    // left-right check (src: OpenCV 3.4 final loop) -- reads the finished row
    for (int x = minX1 + rl; x < e.maxX1; x += LPR) {
        const int v = orow[x];
        if (v == INV) continue;
        const int dlo = v >> kDispShift, dhi = (v + kDispScale - 1) >> kDispShift;
        const int xl = x - dlo, xh = x - dhi;
        auto d2at = [&](int xx) -> int {
            const uint32_t k = __hip_atomic_load(krow + xx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // untouched entries keep OpenCV's INVALID_DISP_SCALED (compared as a disparity)
            if (k == 0xffffffffu) return INV;
            const int xc = 0xffff - (int)(k & 0xffffu);
            return xc + minX1 - xx;  // best + minD of the winning cost column
        };
        if (0 <= xl && xl < W && 0 <= xh && xh < W) {
            const int a = d2at(xl), b = d2at(xh);
            if (a >= minD && abs(a - dlo) > e.disp12 && b >= minD && abs(b - dhi) > e.disp12)
                orow[x] = (int16_t)INV;
        }
    }
}

// ---------------------------------------------------------------------------
// 5b. WTA of the split side-by-side form (round 6): the R->L direction ran as
// one more side-by-side chain set, so every pixel's S is a sum of planes --
// S = min(ndir (C - P2) + sum of the ndir deltas, MAX_COST), exact in int32 --
// and the WTA, uniqueness ratio, sub-pixel fit and right-view keys run on a
// thread per pixel with no chain along the row; a row's block then runs the
// left-right check (as sgbm_final16_kernel).  Byte / u16 planes, element order
// d within a pixel.
// ---------------------------------------------------------------------------
constexpr int kWtaThreads = 256;

template <typename AccT>
__device__ __forceinline__ void load8_planes(const AccT* p, uint32_t (&v)[8])
{
    if constexpr (sizeof(AccT) == 2) {
        const uint4 t = *(const uint4*)p;
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[2 * i] = w[i] & 0xffffu;
            v[2 * i + 1] = w[i] >> 16;
        }
    } else {
        const uint2 t = *(const uint2*)p;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[i] = (t.x >> (8 * i)) & 0xffu;
            v[4 + i] = (t.y >> (8 * i)) & 0xffu;
        }
    }
}

// LPP = D / 8 lanes per pixel, 8 disparities per lane (coalesced 16-byte
// loads of C and of every plane); the lanes of a pixel reduce the key, the
// uniqueness minimum and S(best -+ 1) with lane shuffles, and the pixel's first
// lane finishes it.
template <typename AccT, bool UQ, int LPP>
__global__ __launch_bounds__(kWtaThreads) void sgbm_wta_planes_kernel(const int16_t* __restrict__ C,
                                                                     const AccT* __restrict__ A, size_t plane,
                                                                     int nplanes, int H, int W, SgbmEff e,
                                                                     int16_t* __restrict__ raw,
                                                                     uint32_t* __restrict__ keys)
{
    static_assert(LPP >= 2 && LPP <= 32 && (LPP & (LPP - 1)) == 0, "8 disparities per lane, D = 16 .. 256");
    constexpr int PPB = kWtaThreads / LPP;  // pixels per block iteration
    const int y = blockIdx.x, f = blockIdx.y;
    const int D = 8 * LPP, W1 = e.W1, INV = e.invalid, minD = e.minD, minX1 = e.minX1;
    int16_t* orow = raw + ((size_t)f * H + y) * W;
    uint32_t* krow = keys + ((size_t)f * H + y) * W;
    for (int x = threadIdx.x; x < W; x += kWtaThreads) {
        orow[x] = (int16_t)INV;
        krow[x] = 0xffffffffu;
    }
    __threadfence_block();
    __syncthreads();
    const bool lane_rule = !e.fullDP && !(e.variant & MVSV_VARIANT_WTA_MIN_D);
    const int ndir = sgbm_ndir(e);
    // costs past 32767 are negative int16 as in OpenCV (sgbm_signed_costs): S is then signed,
    // saturated on both sides, and the keys carry it biased by 32768
    const bool sgn = sgbm_signed_costs(e);
    const int bias = sgn ? 32768 : 0;
    const size_t row0 = ((size_t)f * H + y) * W1;
    const int sl = threadIdx.x % LPP, gbase = (int)(threadIdx.x & 63) - sl;  // lane in the pixel, its first lane
    const int d0 = 8 * sl;
    for (int xb = 0; xb < W1; xb += PPB) {
        const int xr = xb + (int)threadIdx.x / LPP;
        const int x = min(xr, W1 - 1);
        const size_t off = (row0 + x) * D + d0;
        int S[8];
        {
            const uint4 cw = *(const uint4*)(C + off);
            const uint32_t cv[4] = {cw.x, cw.y, cw.z, cw.w};
            int acc[8];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int clo = (int)(cv[i] & 0xffffu), chi = (int)(cv[i] >> 16);
                acc[2 * i] = ndir * ((sgn ? (int)(int16_t)clo : clo) - e.P2);
                acc[2 * i + 1] = ndir * ((sgn ? (int)(int16_t)chi : chi) - e.P2);
            }
            for (int k = 0; k < nplanes; k++) {
                uint32_t dv[8];
                load8_planes<AccT>(A + (size_t)k * plane + off, dv);
#pragma unroll
                for (int i = 0; i < 8; i++) acc[i] += (int)dv[i];
            }
#pragma unroll
            for (int i = 0; i < 8; i++) S[i] = max(min(acc[i], kMaxCost), -bias);
        }
        // argmin, ties in OpenCV's order (d, or MODE_SGBM's SIMD lane d mod 8 first)
        uint32_t key = 0xffffffffu;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int d = d0 + i;
            const uint32_t sub = lane_rule ? (uint32_t)((i << 12) | (d >> 3)) : (uint32_t)d;
            key = min(key, ((uint32_t)(S[i] + bias) << 16) | sub);
        }
#pragma unroll
        for (int m = 1; m < LPP; m <<= 1) key = min(key, (uint32_t)__shfl_xor((int)key, m, 64));
        const int minS = (int)(key >> 16) - bias, sub = (int)(key & 0xffffu);
        const int best = lane_rule ? (((sub & 0xfff) << 3) | (sub >> 12)) : sub;
        const int bm = max(best - 1, 0), bp = min(best + 1, D - 1);
        auto elem = [&](int d) -> int {  // S[d & 7] of this lane
            int v = S[0];
#pragma unroll
            for (int i = 1; i < 8; i++) v = (d & 7) == i ? S[i] : v;
            return v;
        };
        const int Sm = __shfl(elem(bm), gbase + (bm >> 3), 64);
        const int Sp = __shfl(elem(bp), gbase + (bp >> 3), 64);
        bool rej = false;
        if constexpr (UQ) {
            int m2 = 0x7fffffff;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int d = d0 + i;
                if (d < best - 1 || d > best + 1) m2 = min(m2, S[i]);
            }
#pragma unroll
            for (int m = 1; m < LPP; m <<= 1) m2 = min(m2, __shfl_xor(m2, m, 64));
            rej = m2 != 0x7fffffff && m2 * (100 - e.uniq) < minS * 100;
        }
        if (sl == 0 && xr < W1) {
            const int bst = minS >= kMaxCost ? -1 : best;  // no strict minimum below MAX_COST
            const int den = max(Sm + Sp - 2 * minS, 1);
            const int frac = ((Sm - Sp) * kDispScale + den) / (den * 2);
            const int d16 = bst * kDispScale + (frac & -(int)(0 < bst && bst < D - 1));
            orow[x + minX1] = rej ? (int16_t)INV : (int16_t)(d16 + minD * kDispScale);
            const int x2 = x + minX1 - bst - minD;
            if (!rej && minS < kMaxCost && x2 >= 0 && x2 < W)
                atomicMin(krow + x2, ((uint32_t)(minS + bias) << 16) | (uint32_t)(0xffff - x));
        }
    }
    __threadfence_block();
    __syncthreads();
    // left-right check (src: OpenCV 3.4 final loop) -- reads the finished row
    for (int x = minX1 + threadIdx.x; x < e.maxX1; x += kWtaThreads) {
        const int v = orow[x];
        if (v == INV) continue;
        const int dlo = v >> kDispShift, dhi = (v + kDispScale - 1) >> kDispShift;
        const int xl = x - dlo, xh = x - dhi;
        auto d2at = [&](int xx) -> int {
            const uint32_t k = __hip_atomic_load(krow + xx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == 0xffffffffu) return INV;  // untouched: OpenCV's INVALID_DISP_SCALED
            return 0xffff - (int)(k & 0xffffu) + minX1 - xx;
        };
        if (0 <= xl && xl < W && 0 <= xh && xh < W) {
            const int a = d2at(xl), b = d2at(xh);
            if (a >= minD && abs(a - dlo) > e.disp12 && b >= minD && abs(b - dhi) > e.disp12)
                orow[x] = (int16_t)INV;
        }
    }
}

template <int NP, int NACC, typename AccT, bool NW = false, bool RES = false, int LPC = 16>
void launch_final16(mvsv_ctx* ctx, int n, int H, int W, const SgbmEff& e, const int16_t* Cv,
                    const AccT* Av, size_t plane, int16_t* raw, const void* Rv = nullptr,
                    const uint16_t* Mv = nullptr)
{
    // NP: disparity pairs per lane at LPC lanes per row (LPC = 8: D = 16, eight
    // rows per wave).  D >= 128: 32 lanes per row (half the pairs per lane,
    // twice the rows in flight per SIMD); a lane keeps >= 2 pairs, so it reads
    // whole 4-disparity nibble groups.
    constexpr int LPR = LPC == 8 ? 8 : (NP >= 4 ? MVSV_FINAL_LPR : 16);
    constexpr int NPL = LPC == 8 ? NP : NP * 16 / LPR;
    constexpr int RPW = 64 / LPR;
    const dim3 grid((H + RPW - 1) / RPW, n);
    uint32_t* keys = (uint32_t*)ctx->keys.ptr;
    int16_t* dummy = (int16_t*)ctx->dummy.ptr;
    if constexpr (RES) {
        // residual plane: WTA on R, exact costs gathered for the sub-pixel fit
        // (uniquenessRatio 0 only: a ratio test needs every exact cost)
        if (e.uniq == 0) {
            hipLaunchKernelGGL((sgbm_final16_kernel<NPL, NACC, AccT, false, LPR, NW, true>), grid, dim3(64), 0,
                               ctx->stream, Cv, Av, plane, H, W, e, raw, keys, dummy, (const uint8_t*)Rv, Mv);
            return;
        }
    }
    if (e.uniq > 0)
        hipLaunchKernelGGL((sgbm_final16_kernel<NPL, NACC, AccT, true, LPR, NW>), grid, dim3(64), 0,
                           ctx->stream, Cv, Av, plane, H, W, e, raw, keys, dummy, nullptr, nullptr);
    else
        hipLaunchKernelGGL((sgbm_final16_kernel<NPL, NACC, AccT, false, LPR, NW>), grid, dim3(64), 0,
                           ctx->stream, Cv, Av, plane, H, W, e, raw, keys, dummy, nullptr, nullptr);
}

}  // namespace
}  // namespace mvsv
