// mvsv_sgbm_common.hpp — what every packed-int16 SGBM kernel shares: scanline
// geometry, the accumulator planes' storage forms (u16, u8, nibble), the cost
// input (cost volume or residual plane), the SGM recurrences on packed pairs
// and the lane / segment minima.  Device code of the SGBM units only
// (mvsv_sgbm.hip, mvsv_sgbm_packed.hip); the stage headers build on it:
//   mvsv_sgbm_lines.hpp   16 / 8 lanes per scanline, one or all directions
//   mvsv_sgbm_strips.hpp  three vertical-ish directions over sheared strips
//   mvsv_sgbm_final.hpp   R->L + WTA, and the split WTA over planes
//   mvsv_sgbm_launch.hpp  the schedules' launchers
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "mvsv_device.hpp"
#include "mvsv_internal.hpp"

namespace mvsv {
namespace {

using namespace dev;

struct Line {
    int xs, ys, len;
};

// 4-bit accumulator planes: the sheared-strip schedule writes one plane per
// group of at most three directions (3 strip directions, or the L->R line),
// so each plane holds sums <= 3 * P2; with P2 <= 5 they fit a nibble
// (acc_is_nib, mvsv_sgbm_plan.hpp).
// Element offsets stay in disparity units; a byte holds two of them.
struct nib2_t {
    uint8_t v;
};
template <typename T>
struct AccEpu {
    static constexpr int v = 1;  // accumulator elements per storage unit
};
template <>
struct AccEpu<nib2_t> {
    static constexpr int v = 2;
};
template <>
struct AccEpu<const nib2_t> {
    static constexpr int v = 2;
};
template <typename T>
__host__ __device__ __forceinline__ T* acc_add(T* p, ptrdiff_t e)
{
    return p + e / AccEpu<T>::v;  // e is even for nib2_t (d0 and D are even)
}
static_assert(AccEpu<const nib2_t>::v == 2 && AccEpu<const uint8_t>::v == 1, "accumulator units");
// non-negative 32-bit offsets: the unit division is a shift and the 64-bit
// address add needs no sign extension
template <typename T>
__device__ __forceinline__ T* acc_addu(T* p, uint32_t e)
{
    return p + e / (uint32_t)AccEpu<T>::v;
}

__device__ __forceinline__ Line line_geometry(int line, int dx, int dy, int W1, int H)
{
    Line g;
    if (dy == 0) {
        g.ys = line;
        g.xs = dx > 0 ? 0 : W1 - 1;
        g.len = W1;
    } else if (dx == 0) {
        g.xs = line;
        g.ys = dy > 0 ? 0 : H - 1;
        g.len = H;
    } else {
        const int ye = dy > 0 ? 0 : H - 1, xe = dx > 0 ? 0 : W1 - 1;
        if (line < W1) {
            g.xs = line;
            g.ys = ye;
        } else {
            g.xs = xe;
            g.ys = ye + dy * (line - W1 + 1);
        }
        int nx = dx > 0 ? W1 - g.xs : g.xs + 1;
        int ny = dy > 0 ? H - g.ys : g.ys + 1;
        g.len = min(nx, ny);
    }
    return g;
}

__host__ __device__ inline int num_lines(int dx, int dy, int W1, int H)
{
    return dy == 0 ? H : (dx == 0 ? W1 : W1 + H - 1);
}

template <int NP>
struct Vec;
template <>
struct Vec<1> {
    uint32_t v[1];
    __device__ __forceinline__ void load(const int16_t* p) { v[0] = *(const uint32_t*)p; }
    __device__ __forceinline__ void store(int16_t* p) const { *(uint32_t*)p = v[0]; }
};
template <>
struct Vec<2> {
    uint32_t v[2];
    __device__ __forceinline__ void load(const int16_t* p)
    {
        uint2 t = *(const uint2*)p;
        v[0] = t.x;
        v[1] = t.y;
    }
    __device__ __forceinline__ void store(int16_t* p) const { *(uint2*)p = make_uint2(v[0], v[1]); }
};
template <>
struct Vec<4> {
    uint32_t v[4];
    __device__ __forceinline__ void load(const int16_t* p)
    {
        uint4 t = *(const uint4*)p;
        v[0] = t.x;
        v[1] = t.y;
        v[2] = t.z;
        v[3] = t.w;
    }
    __device__ __forceinline__ void store(int16_t* p) const
    {
        *(uint4*)p = make_uint4(v[0], v[1], v[2], v[3]);
    }
};

template <>
struct Vec<8> {
    uint32_t v[8];
    __device__ __forceinline__ void load(const int16_t* p)
    {
        uint4 a = *(const uint4*)p, b = *(const uint4*)(p + 8);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    __device__ __forceinline__ void store(int16_t* p) const
    {
        *(uint4*)p = make_uint4(v[0], v[1], v[2], v[3]);
        *(uint4*)(p + 8) = make_uint4(v[4], v[5], v[6], v[7]);
    }
};

// Cost input of the direction passes: the int16 cost volume C (RES = false)
// or the residual plane R (RES = true, two nibbles per byte, see above).
// Offsets are in cost elements (disparity units) either way; get() returns the
// lane's NP packed (d, d+1) u16 pairs.
template <int NP, bool RES>
struct CostIn;
template <int NP>
struct CostIn<NP, false> {
    Vec<NP> b;
    static __device__ __forceinline__ const void* at(const void* base, ptrdiff_t e)
    {
        return (const int16_t*)base + e;
    }
    __device__ __forceinline__ void load(const void* p) { b.load((const int16_t*)p); }
    __device__ __forceinline__ void get(uint32_t (&c)[NP]) const
    {
#pragma unroll
        for (int i = 0; i < NP; i++) c[i] = b.v[i];
    }
};
template <int NP>
struct CostIn<NP, true> {
    static constexpr int NWD = NP >= 8 ? 2 : 1;
    uint32_t w[NWD];
    static __device__ __forceinline__ const void* at(const void* base, ptrdiff_t e)
    {
        return (const uint8_t*)base + e / 2;  // e is even (D and the lane offsets are)
    }
    __device__ __forceinline__ void load(const void* p)
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
    // byte k = (R(2k), R(2k+1)) nibbles -> pair k = R(2k) | R(2k+1) << 16:
    // low nibbles E and high nibbles O as bytes, then one v_perm_b32 per pair
    __device__ __forceinline__ void get(uint32_t (&c)[NP]) const
    {
#pragma unroll
        for (int q = 0; q < NWD; q++) {
            const uint32_t E = w[q] & 0x0f0f0f0fu, O = (w[q] >> 4) & 0x0f0f0f0fu;
#pragma unroll
            for (int k = 0; k < (NP < 4 ? NP : 4); k++)
                c[4 * q + k] = __builtin_amdgcn_perm(O, E, 0x0c000c00u | (uint32_t)k | ((uint32_t)(4 + k) << 16));
        }
    }
};

// One SGM step for the NP packed pairs a lane owns.  lp: previous L (MAX in
// padded slots), delta = (int16)(minLp + P2) packed twice, c: cost C.
template <int NP>
__device__ __forceinline__ void sgm_step(const uint32_t (&lp)[NP], uint32_t delta2, uint32_t p1x2,
                                         const uint32_t (&c)[NP], const bool (&valid)[NP],
                                         uint32_t (&ln)[NP])
{
    const uint32_t MAXP = 0x7fff7fffu;
    const uint32_t prev_hi = wave_shr1(lp[NP - 1], MAXP);  // lane-1's last pair
    const uint32_t next_lo = wave_shl1(lp[0], MAXP);       // lane+1's first pair
#pragma unroll
    for (int p = 0; p < NP; p++) {
        uint32_t ph = p == 0 ? prev_hi : lp[p - 1];
        uint32_t nl = p == NP - 1 ? next_lo : lp[p + 1];
        uint32_t lm = __builtin_amdgcn_alignbit(lp[p], ph, 16);  // (L[d-1], L[d])
        uint32_t lq = __builtin_amdgcn_alignbit(nl, lp[p], 16);  // (L[d+1], L[d+2])
        uint32_t m = pk_min(lp[p], pk_add_sat(lm, p1x2));
        m = pk_min(m, pk_add_sat(lq, p1x2));
        m = pk_min(m, delta2);
        uint32_t r = pk_add_sat(pk_sub_sat(m, delta2), c[p]);
        ln[p] = valid[p] ? r : MAXP;
    }
}

template <int NP>
__device__ __forceinline__ int lane_min(const uint32_t (&ln)[NP])
{
    int m = 32767;
#pragma unroll
    for (int p = 0; p < NP; p++) m = min(m, min(lo16(ln[p]), hi16(ln[p])));
    return m;
}


// Cross-direction accumulator.  With cb = C - P2 (the unbiased box cost) every
// path cost is L_r = cb + delta_r with delta_r in [0, P2] (the min() term of
// the recurrence minus min_k L_r(p-r,k) lies in [0, P2]); hence
//     S = min(sum_r L_r, MAX_COST) = min(ndir*cb + sum_r delta_r, MAX_COST)
// and only sum_r delta_r has to travel between the direction kernels: one byte
// per (pixel, disparity) when ndir*P2 <= 255 (sgbm.yml: P2 = 5), else a
// saturating u16 (saturation above MAX_COST cannot change the min()).
template <int NP, typename AccT>
struct AccVec;

template <int NP>
struct AccVec<NP, uint16_t> {  // packed u16 pairs, one dword per pair
    static __device__ __forceinline__ void load(const uint16_t* p, uint32_t (&v)[NP])
    {
        Vec<NP> t;
        t.load((const int16_t*)p);
#pragma unroll
        for (int i = 0; i < NP; i++) v[i] = t.v[i];
    }
    static __device__ __forceinline__ void store(uint16_t* p, const uint32_t (&v)[NP])
    {
        Vec<NP> t;
#pragma unroll
        for (int i = 0; i < NP; i++) t.v[i] = v[i];
        t.store((int16_t*)p);
    }
    static __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b)
    {
        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_elementwise_add_sat(
                                                __builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
    }
};

// u8 storage: byte pair <-> u16 pair with v_perm_b32
__device__ __forceinline__ uint32_t u8x2_to_u16x2(uint32_t w, int half)
{
    return __builtin_amdgcn_perm(0u, w, half ? 0x0c030c02u : 0x0c010c00u);
}

template <>
struct AccVec<1, uint8_t> {
    static __device__ __forceinline__ void load(const uint8_t* p, uint32_t (&v)[1])
    {
        v[0] = u8x2_to_u16x2(*(const uint16_t*)p, 0);
    }
    static __device__ __forceinline__ void store(uint8_t* p, const uint32_t (&v)[1])
    {
        *(uint16_t*)p = (uint16_t)__builtin_amdgcn_perm(0u, v[0], 0x0c0c0200u);
    }
    static __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) { return a + b; }
};
template <>
struct AccVec<2, uint8_t> {
    static __device__ __forceinline__ void load(const uint8_t* p, uint32_t (&v)[2])
    {
        uint32_t w = *(const uint32_t*)p;
        v[0] = u8x2_to_u16x2(w, 0);
        v[1] = u8x2_to_u16x2(w, 1);
    }
    static __device__ __forceinline__ void store(uint8_t* p, const uint32_t (&v)[2])
    {
        *(uint32_t*)p = __builtin_amdgcn_perm(v[1], v[0], 0x06040200u);
    }
    static __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) { return a + b; }
};
template <>
struct AccVec<4, uint8_t> {
    static __device__ __forceinline__ void load(const uint8_t* p, uint32_t (&v)[4])
    {
        uint2 w = *(const uint2*)p;
        v[0] = u8x2_to_u16x2(w.x, 0);
        v[1] = u8x2_to_u16x2(w.x, 1);
        v[2] = u8x2_to_u16x2(w.y, 0);
        v[3] = u8x2_to_u16x2(w.y, 1);
    }
    static __device__ __forceinline__ void store(uint8_t* p, const uint32_t (&v)[4])
    {
        *(uint2*)p = make_uint2(__builtin_amdgcn_perm(v[1], v[0], 0x06040200u),
                                __builtin_amdgcn_perm(v[3], v[2], 0x06040200u));
    }
    static __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) { return a + b; }
};

template <>
struct AccVec<8, uint8_t> {
    static __device__ __forceinline__ void load(const uint8_t* p, uint32_t (&v)[8])
    {
        uint4 w = *(const uint4*)p;
        v[0] = u8x2_to_u16x2(w.x, 0);
        v[1] = u8x2_to_u16x2(w.x, 1);
        v[2] = u8x2_to_u16x2(w.y, 0);
        v[3] = u8x2_to_u16x2(w.y, 1);
        v[4] = u8x2_to_u16x2(w.z, 0);
        v[5] = u8x2_to_u16x2(w.z, 1);
        v[6] = u8x2_to_u16x2(w.w, 0);
        v[7] = u8x2_to_u16x2(w.w, 1);
    }
    static __device__ __forceinline__ void store(uint8_t* p, const uint32_t (&v)[8])
    {
        *(uint4*)p = make_uint4(__builtin_amdgcn_perm(v[1], v[0], 0x06040200u),
                                __builtin_amdgcn_perm(v[3], v[2], 0x06040200u),
                                __builtin_amdgcn_perm(v[5], v[4], 0x06040200u),
                                __builtin_amdgcn_perm(v[7], v[6], 0x06040200u));
    }
    static __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) { return a + b; }
};

// nibble storage of the sums (each <= 15): every 4 consecutive disparities
// d..d+3 = pairs (d, d+1), (d+2, d+3) form one u16 with d, d+2, d+1, d+3 in
// nibbles 0..3 -- independent of how many pairs a lane holds, so writers with
// 16 lanes per row and the final kernel's 32 lanes per row agree.  (One pair
// per lane, D = 32 only: nibbles 0, 1 of a byte.)
template <int NP>
struct AccVec<NP, nib2_t> {
    static __device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
    {
        const uint32_t h0 = a | (b << 4), h1 = c | (d << 4);  // bytes 0 and 2 carry the groups
        return __builtin_amdgcn_perm(h1, h0, 0x06040200u);
    }
    static __device__ __forceinline__ void store(nib2_t* p, const uint32_t (&v)[NP])
    {
        if constexpr (NP == 1) {
            *(uint8_t*)p = (uint8_t)(v[0] | (v[0] >> 12));
        } else if constexpr (NP == 2) {
            const uint32_t w = v[0] | (v[1] << 4);
            *(uint16_t*)p = (uint16_t)(w | (w >> 8));
        } else if constexpr (NP == 4) {
            *(uint32_t*)p = pack4(v[0], v[1], v[2], v[3]);
        } else {
            *(uint2*)p = make_uint2(pack4(v[0], v[1], v[2], v[3]), pack4(v[4], v[5], v[6], v[7]));
        }
    }
};

// delta = L - C + P2 (exact, in [0, P2]) for a packed pair
__device__ __forceinline__ uint32_t path_delta(uint32_t ln, uint32_t c, uint32_t p2x2)
{
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    u16x2 r = __builtin_bit_cast(u16x2, ln) - __builtin_bit_cast(u16x2, c) + __builtin_bit_cast(u16x2, p2x2);
    return __builtin_bit_cast(uint32_t, r);
}

template <int NP>
__device__ __forceinline__ void sgm_step_row(const uint32_t (&lp)[NP], uint32_t delta2,
                                             uint32_t p1x2, const uint32_t (&c)[NP],
                                             uint32_t (&ln)[NP])
{
    const uint32_t MAXP = 0x7fff7fffu;
    const uint32_t prev_hi = row_shr1(lp[NP - 1], MAXP);
    const uint32_t next_lo = row_shl1(lp[0], MAXP);
#pragma unroll
    for (int p = 0; p < NP; p++) {
        uint32_t ph = p == 0 ? prev_hi : lp[p - 1];
        uint32_t nl = p == NP - 1 ? next_lo : lp[p + 1];
        uint32_t lm = __builtin_amdgcn_alignbit(lp[p], ph, 16);
        uint32_t lq = __builtin_amdgcn_alignbit(nl, lp[p], 16);
        // min(L[d-1] + P1, L[d+1] + P1) == min(L[d-1], L[d+1]) + P1 (saturating add is monotone)
        uint32_t m = pk_min(lp[p], pk_add_sat(pk_min(lm, lq), p1x2));
        m = pk_min(m, delta2);
        ln[p] = pk_add_sat(pk_sub_sat(m, delta2), c[p]);
    }
}

// sgm_step_row that also returns t = sat(m - delta) = delta_r - P2 in [-P2, 0]
// (delta_r = the path's increment over cb, exact: every candidate of m lies
// in [minLp, minLp + P2]).  The neighbour minima min(L[d-1], L[d+1]) of the
// NP pairs come from NP + 1 pairwise minima X_q = min(pair q, pair q + 1):
// pair p's is (X_{p-1}.hi, X_p.lo) -- one v_pk_min + one v_alignbit per pair.
//
// NW ("no wrap", chosen by the host when P2 + blockSize^2 * (2*ftzero + 63) +
// P2 <= 32767, sgbm_no_wrap): every C, L and delta = minLp + P2 is then a
// non-negative int16, so with u = delta - min(m, delta) = max(delta - m, 0)
// (one unsigned saturating subtract) L = C - u, and the path's increment over
// cb is P2 - u: five VALU per pair instead of six.  tu[] returns u (NW) or the
// signed t = -u (the general form: signed saturating int16 as OpenCV's SIMD
// recurrence, so it stays exact on a wrapped -- negative -- cost; the final
// kernels carry a signed S there, DESIGN.md 4b-wrap, tests/test_gpu_sgbm_wrap.py).
template <bool NW>
__device__ __forceinline__ void sgm_pair(uint32_t lp, uint32_t nb, uint32_t delta2, uint32_t p1x2,
                                         uint32_t c, uint32_t& ln, uint32_t& tu)
{
    if constexpr (NW) {
        // full-rate 32-bit forms, exact here: nb <= 0x7fff and P1 < 0x8000, so
        // nb + P1 never carries out of its half (the unsigned min then equals
        // min(L, sat(nb + P1)) because L <= 0x7fff); u <= P2 <= C (every cost
        // of the no-wrap regime is P2 + a window sum, every residual is in
        // [P2, 3 P2]), so C - u never borrows
        const uint32_t m = pk_min_u16(lp, add2_nc(nb, p1x2));
        tu = pk_subsat_u16(delta2, m);
        ln = sub2_nb(c, tu);
    } else {
        const uint32_t m = pk_min(lp, pk_add_sat(nb, p1x2));
        tu = pk_sub_sat(pk_min(m, delta2), delta2);
        ln = pk_add_sat(tu, c);
    }
}
// delta = t + P2 (general) = P2 - u (NW, u <= P2: no borrow), in [0, P2]
template <bool NW>
__device__ __forceinline__ uint32_t sgm_delta(uint32_t tu, uint32_t p2x2)
{
    return NW ? sub2_nb(p2x2, tu) : pk_add_u16(tu, p2x2);
}
// the packed delta = (short)(minLp + P2) of the next step
template <bool NW>
__device__ __forceinline__ uint32_t sgm_delta2(int minp, int P2)
{
    return NW ? (uint32_t)(minp + P2) * 0x10001u : (uint32_t)((minp + P2) & 0xffff) * 0x10001u;
}
template <int NP, bool NW = false, int LPC = 16>
__device__ __forceinline__ void sgm_step_row_t(const uint32_t (&lp)[NP], uint32_t delta2,
                                               uint32_t p1x2, const uint32_t (&c)[NP],
                                               uint32_t (&ln)[NP], uint32_t (&t)[NP])
{
    static_assert(LPC == 8 || LPC == 16, "row-DPP segments of 8 or 16 lanes");
    const uint32_t MAXP = 0x7fff7fffu;
    // d-1 / d+1 neighbours across the lane boundary: zero-filled DPP shifts
    // (bound_ctrl) OR'ed with MAX at the segment ends fold into v_or_b32_dpp
    // (an 8-lane segment's first lane receives the previous segment's last
    // lane; the OR with MAX discards it: L values are in [0, 0x7fff] -- in the
    // no-wrap form.  In the general form an L may be negative (a wrapped cost)
    // and x | MAX would be -1, so the 8-lane segment ends select MAX instead.)
    const uint32_t rls = __lane_id() % LPC;
    uint32_t prev_hi, next_lo;
    if constexpr (NW || LPC == 16) {
        prev_hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)lp[NP - 1], 0x111, 0xf, 0xf, true) |
                  (rls == 0 ? MAXP : 0u);
        next_lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)lp[0], 0x101, 0xf, 0xf, true) |
                  (rls == LPC - 1 ? MAXP : 0u);
    } else {
        const uint32_t sh_hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)lp[NP - 1], 0x111, 0xf, 0xf, true);
        prev_hi = rls == 0 ? MAXP : sh_hi;
        const uint32_t sh_lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)lp[0], 0x101, 0xf, 0xf, true);
        next_lo = rls == LPC - 1 ? MAXP : sh_lo;
    }
    uint32_t X[NP + 1];  // X[q + 1] = X_q, X[0] = X_{-1}
    X[0] = pk_min(prev_hi, lp[0]);
#pragma unroll
    for (int q = 0; q + 1 < NP; q++) X[q + 1] = pk_min(lp[q], lp[q + 1]);
    X[NP] = pk_min(lp[NP - 1], next_lo);
#pragma unroll
    for (int p = 0; p < NP; p++)
        sgm_pair<NW>(lp[p], __builtin_amdgcn_alignbit(X[p + 1], X[p], 16), delta2, p1x2, c[p], ln[p], t[p]);
}

// Minimum over an LPC-lane segment (8: one half of a DPP row, 16: a row);
// every lane of the segment gets it.
template <int LPC>
__device__ __forceinline__ int seg_lane_min(int v)
{
    static_assert(LPC == 8 || LPC == 16, "row-DPP segments of 8 or 16 lanes");
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true));  // row_half_mirror
    if constexpr (LPC == 16) v = min(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xf, 0xf, true));  // row_mirror
    return v;
}

// Lane segments of the final kernel: LPR lanes own one image row (16: a DPP
// row; 32: two DPP rows joined by v_permlane16_swap).
template <int LPR>
__device__ __forceinline__ int seg_min_i32(int v)
{
    if constexpr (LPR == 8) return seg_lane_min<8>(v);
    v = row_min_i32(v);
    if constexpr (LPR == 32) {
        const auto sw = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
        v = min((int)sw[0], (int)sw[1]);
    }
    return v;
}
// sgm_step_row_t over an LPR-lane segment: the d-1 / d+1 neighbours of a lane's
// first / last pair come from the adjacent lane of the segment (MAX at the
// segment ends).
template <int NP, int LPR, bool NW>
__device__ __forceinline__ void sgm_step_seg_t(const uint32_t (&lp)[NP], uint32_t delta2,
                                               uint32_t p1x2, const uint32_t (&c)[NP],
                                               uint32_t (&ln)[NP], uint32_t (&t)[NP], bool seg_first,
                                               bool seg_last)
{
    if constexpr (LPR <= 16) {
        sgm_step_row_t<NP, NW, LPR>(lp, delta2, p1x2, c, ln, t);
    } else {
        const uint32_t MAXP = 0x7fff7fffu;
        // zero-filled wave shifts (bound_ctrl) OR'ed with MAX at the segment
        // ends (no-wrap form: L values are in [0, 0x7fff], so x | MAXP == MAXP): one
        // v_or_b32_dpp per neighbour
        // (general form: an L of the other row's end lane may be negative, so select)
        const uint32_t sh_hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)lp[NP - 1], 0x138, 0xf, 0xf, true);
        const uint32_t sh_lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)lp[0], 0x130, 0xf, 0xf, true);
        const uint32_t prev_hi = NW ? (sh_hi | (seg_first ? MAXP : 0u)) : (seg_first ? MAXP : sh_hi);
        const uint32_t next_lo = NW ? (sh_lo | (seg_last ? MAXP : 0u)) : (seg_last ? MAXP : sh_lo);
        uint32_t X[NP + 1];  // X[q + 1] = X_q, X[0] = X_{-1}
        X[0] = pk_min(prev_hi, lp[0]);
#pragma unroll
        for (int q = 0; q + 1 < NP; q++) X[q + 1] = pk_min(lp[q], lp[q + 1]);
        X[NP] = pk_min(lp[NP - 1], next_lo);
#pragma unroll
        for (int p = 0; p < NP; p++)
            sgm_pair<NW>(lp[p], __builtin_amdgcn_alignbit(X[p + 1], X[p], 16), delta2, p1x2, c[p], ln[p],
                         t[p]);
    }
}

// The lane's minimum over its NP pairs in BOTH halves (the swap is a VOP3P
// op_sel, no extra instruction): for L in [0, 0x7fff] the packed (m, m) orders
// like m as an int32, so the segment butterfly runs on it unchanged and the
// next step's packed delta = (minLp + P2) x 2 is one v_add_u32 (no-wrap form).
template <int NP>
__device__ __forceinline__ uint32_t lane_min_pk(const uint32_t (&ln)[NP])
{
    uint32_t m = ln[0];
#pragma unroll
    for (int p = 1; p < NP; p++) m = pk_min(m, ln[p]);
    const s16x2 v = as_s2(m);
    return as_u(__builtin_elementwise_min(v, __builtin_shufflevector(v, v, 1, 0)));
}

template <int NP>
__device__ __forceinline__ int lane_min_row(const uint32_t (&ln)[NP])
{
    uint32_t m = ln[0];
#pragma unroll
    for (int p = 1; p < NP; p++) m = pk_min(m, ln[p]);
    return min(lo16(m), hi16(m));
}

__device__ __forceinline__ uint32_t pk_mad_u16(uint32_t a, uint32_t b, uint32_t c)
{
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) * __builtin_bit_cast(u16x2, b) +
                                            __builtin_bit_cast(u16x2, c));
}

}  // namespace
}  // namespace mvsv
