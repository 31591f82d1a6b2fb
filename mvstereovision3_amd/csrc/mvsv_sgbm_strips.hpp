// mvsv_sgbm_strips.hpp — the sheared-strip schedule of the SGBM path
// aggregation: sgbm_tri_kernel, its LDS / granule layouts and its launchers
// (launch_tri_wv with the strip statistics, launch_strips).
#pragma once

#include <algorithm>
#include <cstdio>
#include <vector>

#include "mvsv_sgbm_common.hpp"

namespace mvsv {
namespace {

// ---------------------------------------------------------------------------
// 4c. three vertical-ish directions in one sweep over sheared strips.
// With U = x - t + (H - 1) for step t (row y = t top-down, y = H-1-t
// bottom-up), the cell (x, y) at step t has its predecessors at step t-1 in
// U-column U (dir (1, sy)), U+1 (dir (0, sy)) and U+2 (dir (-1, sy)), sy = +1
// (down) or -1 (up).  So one block owning U-columns [U0, U0+SW) walks its
// strip one step per row -- every step is SW contiguous x-columns of C and of
// the accumulator -- and needs only the two U-columns right of it from the
// previous step: the strip to its right (lower block index) publishes them as
// tagged 8-byte granules with write-through stores, this strip polls them
// (bounded spin).  C is read once for three directions instead of three
// times.  Cells outside the image carry L = 0, min 0: exactly the zero start
// state of every path at the image border.
// Lanes: 16 per U-column (2*NP disparities each), 4 columns per compute wave;
// one extra wave per block does all strip-to-strip traffic, so the compute
// waves' memory counters only ever wait for their own C loads.
// ---------------------------------------------------------------------------
// compute waves per block (WV): wide strips, 15 (+ the exchange wave = 1024
// threads, <= 128 VGPRs) for up to 8 disparities per lane, 7 for D = 256 (16
// per lane, ~200 VGPRs) -- the throughput shape for frame batches; narrow
// strips, 8 (4 for D = 256) compute waves -- the latency shape for one or two
// frames, where wide strips leave most CUs idle and each step of a strip is
// the serial work of its CU (the strip shape is chosen by sgbm_make_plan)
// LPC = lanes per U-column (2*NP disparities each, D = 2*NP*LPC): 16 (one DPP
// row per column) or 8 (half a DPP row, twice the disparities per lane: the
// per-column minimum is a 3-step butterfly, and the lane-boundary neighbours,
// the step's row minima and its bookkeeping are shared by twice the work --
// the throughput shape for D = 128 batches, two 512-thread blocks per CU).
// LPC = 32 (round 6, D = 256 launches too small for wide strips: config 5's
// one or two frames): two DPP rows per U-column, 4 disparity pairs per lane --
// half the per-wave work of a strip step at the same strip width (8 compute
// waves x 2 columns); the three boundary items then need 96 exchange lanes,
// so such a block has two exchange waves.
// (the wave counts per (NP, LPC): tri_wide_waves / tri_narrow_waves, mvsv_sgbm_plan.hpp)
template <int NP, int WV, int LPC = 16>
struct TriCfg {
    static constexpr int kWaves = WV;
    static constexpr int kCPW = 64 / LPC;   // U-columns per compute wave
    static constexpr int kSW = tri_strip_cols(WV, LPC);  // U-columns per strip
    static constexpr int kComm = LPC == 32 ? 2 : 1;  // exchange waves: 3 items x LPC lanes
    static constexpr int kThreads = 64 * (kWaves + kComm);
    // blocks per CU the register budget aims at: one 1024-thread block, or two
    // 512-thread ones (4 waves per SIMD either way); D = 256 on 16 lanes: 2.
    // (Narrow strips reading the cost residual aim at 5: two 9-wave blocks
    // per CU, each filling the other's step-barrier and hand-off waits.)
    static constexpr int kWavesPerEU = (NP >= 8 && LPC == 16) ? 2 : 4;
};
#ifndef MVSV_TRI_PF
#define MVSV_TRI_PF 4
#endif
#ifndef MVSV_TRI_STEP_SEQ
#define MVSV_TRI_STEP_SEQ 0  // 1: the three recurrences of a step one after the other (A/B)
#endif
constexpr int kTriPF = MVSV_TRI_PF;     // steps of C prefetch (compute waves)
constexpr int kTriBF = 4;               // steps of boundary prefetch (comm wave)
constexpr int kTriUnroll = 4;           // lcm(kTriPF, kTriBF, 2)

template <int NP, int WV, int LPC = 16>
struct TriLayout {
    static constexpr int kCols = TriCfg<NP, WV, LPC>::kSW + 2;  // + two columns of the right strip
    // Element-major columns: lane (column c, rl) keeps element p of its 2*NP
    // disparities at c*kColDw + p*LPC + rl.  A b32 access (ds_read2_b32 /
    // ds_write2_b32) is served per 32-lane half-wave on 32 banks ((a/4) mod 32,
    // MI355X_MICROARCH.md §LDS); the half-wave holds 32/LPC columns, and with
    // kColDw = LPC (mod 32) they land on disjoint bank ranges: conflict-free.
    // (The former lane-major layout, c*kColDw + rl*NP + p with an odd stride,
    // mapped lanes rl and rl + 32/NP of a column onto one bank: 2-way
    // conflicts, SQ_LDS_BANK_CONFLICT 44 % of the LDS cycles.)
    static constexpr int kColDw = ((NP * LPC + 31) / 32) * 32 + LPC % 32;
    static constexpr int kBufDw = 2 * kCols * kColDw;   // dirs b and c
    static constexpr int kLDw = 2 * kBufDw;             // double-buffered
    static constexpr int kMinInts = 2 * 2 * kCols;      // [buf][dir][col]
    static constexpr size_t kBytes = (size_t)(kLDw + kMinInts) * 4;
};

// Boundary granules of one strip and step: [NG][4 item rows][LPC lanes] u64
// (the 4th item row is never written: the comm wave's spare lanes repeat
// item 2).  Item 0 = L of dir
// (0, sy) at the strip's first column, 1 = dir (-1, sy) at the first column,
// 2 = dir (-1, sy) at the second column.  A lane's item is its 2*NP int16
// costs + the column min, three int16 per granule under a 16-bit launch tag
// (bits 48-63): the tag is the data-ready flag.
template <int NP>
struct TriGran {
    static constexpr int NG = tri_granules(NP);
    static __device__ __forceinline__ void pack(const uint32_t (&v)[NP], int mn, unsigned long long tag,
                                                unsigned long long (&g)[NG])
    {
        uint32_t s[3 * NG];
#pragma unroll
        for (int i = 0; i < 3 * NG; i++) s[i] = 0u;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            s[2 * p] = v[p] & 0xffffu;
            s[2 * p + 1] = v[p] >> 16;
        }
        s[2 * NP] = (uint32_t)mn & 0xffffu;
#pragma unroll
        for (int i = 0; i < NG; i++)
            g[i] = tag | ((unsigned long long)s[3 * i + 2] << 32) | (s[3 * i + 1] << 16) | s[3 * i];
    }
    static __device__ __forceinline__ void unpack(const unsigned long long (&g)[NG], uint32_t (&v)[NP],
                                                  int& mn)
    {
        uint32_t s[3 * NG];
#pragma unroll
        for (int i = 0; i < NG; i++) {
            s[3 * i] = (uint32_t)g[i] & 0xffffu;
            s[3 * i + 1] = (uint32_t)g[i] >> 16;
            s[3 * i + 2] = (uint32_t)(g[i] >> 32) & 0xffffu;
        }
#pragma unroll
        for (int p = 0; p < NP; p++) v[p] = s[2 * p] | (s[2 * p + 1] << 16);
        mn = (int)(int16_t)s[2 * NP];
    }
};

template <int NP, int LPC = 16>
__device__ __forceinline__ size_t tri_slot(int chain, int k, int t, int nchains, int H)
{
    return ((((size_t)k * nchains + chain) * H + t) * 4) * LPC * TriGran<NP>::NG;
}

template <int NP, int WV, int LPC, typename AccT, bool NW = false, bool RES = false>
__global__ __launch_bounds__((TriCfg<NP, WV, LPC>::kThreads))
__attribute__((amdgpu_waves_per_eu(TriCfg<NP, WV, LPC>::kWavesPerEU + (RES && WV <= 8 && NP <= 4 ? 1 : 0)))) void sgbm_tri_kernel(
    const void* __restrict__ C, AccT* __restrict__ A, size_t plane, AccT* __restrict__ dummy,
    int H, int W1, int D, int npass, int P1, int P2, unsigned long long* __restrict__ bnd,
    unsigned epoch, int nframes, int nstrips, int* __restrict__ status, unsigned spin_limit,
    int* __restrict__ report, unsigned long long* __restrict__ stats, int trace_h, long long ticket0)
{
    using AV = AccVec<NP, AccT>;
    using CI = CostIn<NP, RES>;
    using TL = TriLayout<NP, WV, LPC>;
    using TG = TriGran<NP>;
    constexpr int NG = TG::NG;
    constexpr int kTriWaves = TriCfg<NP, WV, LPC>::kWaves;
    constexpr int kTriSW = TriCfg<NP, WV, LPC>::kSW;
    constexpr int kCPW = TriCfg<NP, WV, LPC>::kCPW;
    constexpr int PF = NP >= 8 ? 2 : kTriPF;  // 16 disparities per lane: registers
    constexpr int BF = kTriBF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* lds = (uint32_t*)smem;
    int* lmin = (int*)(lds + TL::kLDw);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool comm = w >= kTriWaves;
    const int cw = comm ? w - kTriWaves : 0;  // exchange wave rank (LPC = 32: 0 or 1)
    const bool comm0 = comm && cw == 0;     // the one that records statistics / traces
    const int r = lane / LPC, rl = lane % LPC;
    // strips counted from the right; pass 0 sweeps down (sy = +1), pass 1 up
    // (sy = -1), each into its own accumulator plane; every strip's producer
    // is strip k - 1 of its chain (same pass and frame).  Which strip a block
    // runs is the ticket it draws on arrival (status[2] counts the context's
    // strip blocks, ticket0 = this launch's first), not its blockIdx: a strip
    // only ever waits on a strip whose block arrived before it and is running
    // or done, so the chain progresses whatever order and placement the
    // dispatcher picks (ticket0 < 0: blockIdx order, which relies on in-order
    // dispatch -- measured on gfx950, tools/ubench/xcc_map.hip -- and keeps a
    // chain on one XCD under round-robin placement: strips 1.60 vs 1.68 ms).
    __shared__ int s_ticket;
    if (threadIdx.x == 0)
        s_ticket = ticket0 < 0 ? (int)blockIdx.x
                               : (int)(__hip_atomic_fetch_add((unsigned*)status + 2, 1u, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT) - (unsigned)ticket0);
    __syncthreads();
    const int bx = s_ticket;
    if ((unsigned)bx >= gridDim.x) {  // ticket count out of step with the host: drain, report
        if (threadIdx.x == 0) {
            __hip_atomic_store(status, (int)epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(report, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    const int nchains = npass * nframes;
    const int k = bx / nchains;
    const int chain = bx - k * nchains;
    const int pass = chain / nframes;
    const int f = chain - pass * nframes;
    const int sy = pass == 0 ? 1 : -1;
    A = acc_add(A, (ptrdiff_t)pass * (ptrdiff_t)plane);
    const int Utot = W1 + H - 1;
    const int U0 = Utot - kTriSW * (k + 1);
    const int col = kCPW * w + r;  // compute waves
    const int U = U0 + col;
    // active steps: some column of the strip has 0 <= x = U - (H-1) + t < W1
    const int tb = max(0, (H - 1) - (U0 + kTriSW - 1));
    const int te = min(H, W1 + (H - 1) - U0);
    if (tb >= te) return;
    unsigned long long st_t0 = stats ? __builtin_amdgcn_s_memtime() : 0ull, st_spin = 0, st_n = 0;
    const int d0 = rl * 2 * NP;
    const size_t frame = (size_t)H * W1 * D;
    const void* Cf = CI::at(C, (ptrdiff_t)(f * frame + d0));
    AccT* Af = acc_add(A, (ptrdiff_t)(f * frame + d0));
    AccT* dp = acc_add(dummy, (ptrdiff_t)threadIdx.x * 2 * NP);
    const uint32_t p1x2 = (uint32_t)(P1 & 0xffff) * 0x10001u;
    const uint32_t p2x3 = (uint32_t)((3 * P2) & 0xffff) * 0x10001u;
    const unsigned tag16 = epoch & 0xffffu;
    const unsigned long long tag = (unsigned long long)tag16 << 48;

    auto lcol = [&](int buf, int dir, int c) -> uint32_t* {
        return lds + (size_t)((buf * 2 + dir) * TL::kCols + c) * TL::kColDw + rl;  // element p at [p * LPC]
    };
    auto mcol = [&](int buf, int dir, int c) -> int* { return lmin + (buf * 2 + dir) * TL::kCols + c; };

    // zero both LDS rows (cells outside the image / before the first step)
    for (int i = threadIdx.x; i < TL::kLDw + TL::kMinInts; i += TriCfg<NP, WV, LPC>::kThreads) lds[i] = 0u;

    // ---- comm wave: lanes (item j = min(r, 2), rl); row 3 repeats item 2's
    // loads and stores at item 2's own addresses (same values: the duplicate
    // lanes cost no extra traffic), so every comm-wave memory instruction is
    // unpredicated and its wait counts are exact.  A step's granules are laid
    // out [granule i][item row][lane]: each of the NG store / load
    // instructions covers 512 contiguous bytes.
    const int ir = cw * (64 / LPC) + r;  // item row of this exchange lane
    const int jj = min(ir, 2);
    const bool jlive = ir < 3;
    const int bcol = kTriSW + (jj == 2 ? 1 : 0);  // LDS column the consumed item lands in
    const int bdir = jj == 0 ? 0 : 1;
    const int pcol = jj == 2 ? 1 : 0;              // own column published as item jj
    const size_t bstep = (size_t)4 * LPC * NG;
    const unsigned long long* bsrc =
        bnd + tri_slot<NP, LPC>(chain, k > 0 ? k - 1 : k, 0, nchains, H) + (size_t)jj * LPC + rl;
    unsigned long long* pdst = bnd + tri_slot<NP, LPC>(chain, k, 0, nchains, H) + (size_t)jj * LPC + rl;
    auto bvalid = [&](int t) {
        const int xx = U0 + bcol - (H - 1) + t;
        return k > 0 && t >= 0 && xx >= 0 && xx < W1;
    };
    auto bload = [&](int t, unsigned long long (&g)[NG]) {
        const unsigned long long* q = bsrc + (size_t)clampi(t, 0, H - 1) * bstep;
#pragma unroll
        for (int i = 0; i < NG; i++) g[i] = __hip_atomic_load(q + 4 * LPC * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // item t into LDS row buf, spinning until the producer's tag shows
    auto bconsume = [&](int t, int buf, unsigned long long (&g)[NG]) {
        const bool need = jlive && bvalid(t);
        bool ok = true;
#pragma unroll
        for (int i = 0; i < NG; i++) ok &= !need || (unsigned)(g[i] >> 48) == tag16;
        if (!__all(ok)) {
            const unsigned long long sp0 = stats ? __builtin_amdgcn_s_memtime() : 0ull;
            unsigned spins = 0;
            while (!__all(ok)) {
                // give up after spin_limit polls, or soon after any block of
                // this launch gave up (status = this launch's epoch): the
                // launch then drains, the median kernel writes its maps as
                // INVALID and the host reports MVSV_E_TIMEOUT
                if (++spins > spin_limit) {
                    if (lane == 0) {
                        __hip_atomic_store(status, (int)epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(report, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    break;
                }
                if ((spins & 63) == 0 &&
                    __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)epoch)
                    break;
                __builtin_amdgcn_s_sleep(1);
                const unsigned long long* q = bsrc + (size_t)clampi(t, 0, H - 1) * bstep;
                ok = true;
#pragma unroll
                for (int i = 0; i < NG; i++) {
                    g[i] = __hip_atomic_load(q + 4 * LPC * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok &= !need || (unsigned)(g[i] >> 48) == tag16;
                }
            }
            if (stats) {
                st_spin += __builtin_amdgcn_s_memtime() - sp0;
                st_n += spins;
            }
        }
        uint32_t v[NP];
        int mn;
        TG::unpack(g, v, mn);
        if (jlive) {
            uint32_t* dst = lcol(buf, bdir, bcol);
#pragma unroll
            for (int i = 0; i < NP; i++) dst[i * LPC] = need ? v[i] : 0u;
            // the compute waves keep column minima packed (m, m) in the no-wrap form
            if (rl == 0) *mcol(buf, bdir, bcol) = need ? (NW ? (int)((uint32_t)mn * 0x10001u) : mn) : 0;
        }
    };
    // publish step t of this strip's columns 0 and 1 (LDS row buf) for the left
    // strip; unconditional stores (idle lanes and unused steps hit unread slots)
    auto publish = [&](int t, int buf) {
        uint32_t v[NP];
        const uint32_t* src = lcol(buf, bdir, pcol);
#pragma unroll
        for (int i = 0; i < NP; i++) v[i] = src[i * LPC];
        const int mn = *mcol(buf, bdir, pcol);
        unsigned long long g[NG];
        TG::pack(v, mn, tag, g);
        unsigned long long* q = pdst + (size_t)clampi(t, 0, H - 1) * bstep;
#pragma unroll
        for (int i = 0; i < NG; i++) __hip_atomic_store(q + 4 * LPC * i, g[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (trace_h && comm0 && lane == 0)  // MVSV_TRI_TRACE: when step t went out (100 MHz clock)
            stats[(size_t)bx * (8 + 2 * trace_h) + 8 + t] = __builtin_amdgcn_s_memrealtime();
    };

    // ---- compute waves ----
    // cell (x, y) of step t: y*W1 + x = c0 + t*(sy*W1 + 1), element offsets in
    // int32 (the launcher checks H*W1*D < 2^31); cells outside the image read
    // the frame's first cell and store into the lane's dummy slot
    auto cell_x = [&](int t) { return U - (H - 1) + t; };
    const int c0D = ((sy > 0 ? 0 : (H - 1) * W1) + U - (H - 1)) * D;
    const int cstepD = (sy * W1 + 1) * D;
    auto cell_off = [&](int t) -> uint32_t {  // >= 0: in-image cells only
        return (unsigned)cell_x(t) < (unsigned)W1 ? (uint32_t)(c0D + t * cstepD) : 0u;
    };
    uint32_t la[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) la[p] = 0u;
    int ma = 0;
    CI cb[PF];
    unsigned long long bg[BF][NG];

    __syncthreads();  // LDS zeroed
    if (comm) __builtin_amdgcn_s_setprio(1);  // the exchange wave gates every step's barrier
    if (comm) {
        bload(tb - 1, bg[0]);
        bconsume(tb - 1, 1, bg[0]);  // the right strip's cells the first step reads
#pragma unroll
        for (int j = 0; j < BF; j++) bload(tb + j, bg[j]);
    } else {
#pragma unroll
        for (int j = 0; j < PF; j++) cb[j].load(CI::at(Cf, cell_off(min(tb + j, te - 1))));
    }
    __syncthreads();

    // The exchange wave and the compute waves run separate loops with the same
    // number of block barriers (one per step): the register allocator then
    // gives each path its own registers (the exchange wave's granule prefetch
    // no longer competes with the compute waves' C prefetch).
    auto comm_step = [&](int i, int j) {
        const int t = tb + i;
        const int cur = i & 1, prv = cur ^ 1;
        if (i > 0) publish(t - 1, prv);
        bconsume(t, cur, bg[j % BF]);
        if (trace_h && comm0 && lane == 0)  // when the producer's step t was in
            stats[(size_t)bx * (8 + 2 * trace_h) + 8 + trace_h + t] = __builtin_amdgcn_s_memrealtime();
        bload(t + BF, bg[j % BF]);
        __syncthreads();
    };
    // One step: the three recurrences one after the other (each direction's
    // neighbours, update, column minimum and LDS hand-over before the next
    // starts, so only one direction's temporaries are live); the output word
    // accumulates the deltas as they come.
    const uint32_t p2x2 = (uint32_t)(P2 & 0xffff) * 0x10001u;
    auto step = [&](int i, int j) {
        const int t = tb + i;
        const int cur = i & 1, prv = cur ^ 1;
        const int x = cell_x(t);
        const bool valid = x >= 0 && x < W1;
        const bool allv = __all(valid);
        uint32_t c[NP];
        cb[j % PF].get(c);
        cb[j % PF].load(CI::at(Cf, cell_off(min(t + PF, te - 1))));
        // the column minimum of one direction (packed (m, m) in the no-wrap
        // form) and the next step's delta from it
        auto dmin = [&](const uint32_t (&n)[NP]) -> int {
            if constexpr (LPC == 32)
                return seg_min_i32<32>(NW ? (int)lane_min_pk<NP>(n) : lane_min_row<NP>(n));
            else if constexpr (NW)
                return seg_lane_min<LPC>((int)lane_min_pk<NP>(n));
            else
                return seg_lane_min<LPC>(lane_min_row<NP>(n));
        };
        // one recurrence step over the column's LPC lanes
        auto rstep = [&](const uint32_t (&lp)[NP], uint32_t delta2, uint32_t (&n)[NP], uint32_t (&u)[NP]) {
            if constexpr (LPC == 32)
                sgm_step_seg_t<NP, 32, NW>(lp, delta2, p1x2, c, n, u, rl == 0, rl == LPC - 1);
            else
                sgm_step_row_t<NP, NW, LPC>(lp, delta2, p1x2, c, n, u);
        };
        auto dl2 = [&](int m) -> uint32_t {
            if constexpr (NW)
                return (uint32_t)m + p2x2;  // (minLp + P2) x 2, no carry between halves
            else
                return sgm_delta2<false>(m, P2);
        };
        // sum of the three deltas t_r + P2 = 3 P2 - (u_a + u_b + u_c) (no-wrap)
        // or t_a + t_b + t_c + 3 P2, exact in u16 wrap arithmetic
        // (no-wrap: 3 P2 minus three u <= P2 each never borrows -> one full-rate v_sub_u32)
        auto acc = [&](uint32_t o, uint32_t u) -> uint32_t { return NW ? sub2_nb(o, u) : pk_add_u16(o, u); };
        uint32_t o[NP];
#if MVSV_TRI_STEP_SEQ
        {  // (1, sy): the strip's own column, state in registers
            uint32_t n[NP], u[NP];
            rstep(la, dl2(ma), n, u);
#pragma unroll
            for (int p = 0; p < NP; p++) o[p] = acc(p2x3, u[p]);
            const int mn = dmin(n);
            if (__builtin_expect(!allv, 0)) {
#pragma unroll
                for (int p = 0; p < NP; p++) n[p] = valid ? n[p] : 0u;
            }
#pragma unroll
            for (int p = 0; p < NP; p++) la[p] = n[p];
            ma = valid ? mn : 0;
        }
#pragma unroll
        for (int dir = 0; dir < 2; dir++) {  // (0, sy) from column col + 1, (-1, sy) from col + 2
            uint32_t pv[NP];
            const uint32_t* src = lcol(prv, dir, col + 1 + dir);
#pragma unroll
            for (int p = 0; p < NP; p++) pv[p] = src[p * LPC];
            const int mp = *mcol(prv, dir, col + 1 + dir);
            uint32_t n[NP], u[NP];
            rstep(pv, dl2(mp), n, u);
#pragma unroll
            for (int p = 0; p < NP; p++) o[p] = acc(o[p], u[p]);
            const int mn = dmin(n);
            if (__builtin_expect(!allv, 0)) {
#pragma unroll
                for (int p = 0; p < NP; p++) n[p] = valid ? n[p] : 0u;
            }
            uint32_t* dst = lcol(cur, dir, col);
#pragma unroll
            for (int p = 0; p < NP; p++) dst[p * LPC] = n[p];
            if (rl == 0) *mcol(cur, dir, col) = valid ? mn : 0;
        }
#else
        // the three recurrences side by side (the compiler interleaves their
        // independent chains; measured faster than one after the other)
        uint32_t pb[NP], pc[NP];
        {
            const uint32_t* sb = lcol(prv, 0, col + 1);
            const uint32_t* sc = lcol(prv, 1, col + 2);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                pb[p] = sb[p * LPC];
                pc[p] = sc[p * LPC];
            }
        }
        const int mb = *mcol(prv, 0, col + 1), mc = *mcol(prv, 1, col + 2);
        uint32_t na[NP], nb[NP], nc[NP], ta[NP], tb_[NP], tc[NP];
        rstep(la, dl2(ma), na, ta);
        rstep(pb, dl2(mb), nb, tb_);
        rstep(pc, dl2(mc), nc, tc);
        const int mna = dmin(na), mnb = dmin(nb), mnc = dmin(nc);
#pragma unroll
        for (int p = 0; p < NP; p++) o[p] = acc(acc(acc(p2x3, ta[p]), tb_[p]), tc[p]);
        if (__builtin_expect(!allv, 0)) {
#pragma unroll
            for (int p = 0; p < NP; p++) {
                na[p] = valid ? na[p] : 0u;
                nb[p] = valid ? nb[p] : 0u;
                nc[p] = valid ? nc[p] : 0u;
            }
        }
#pragma unroll
        for (int p = 0; p < NP; p++) la[p] = na[p];
        ma = valid ? mna : 0;
        {
            uint32_t* db = lcol(cur, 0, col);
            uint32_t* dc = lcol(cur, 1, col);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                db[p * LPC] = nb[p];
                dc[p * LPC] = nc[p];
            }
            if (rl == 0) {
                *mcol(cur, 0, col) = valid ? mnb : 0;
                *mcol(cur, 1, col) = valid ? mnc : 0;
            }
        }
#endif
        AV::store(valid ? acc_addu(Af, cell_off(t)) : dp, o);
        __syncthreads();
    };
    const int len = te - tb;
    int i = 0;
    if (comm) {
        for (; i + kTriUnroll <= len; i += kTriUnroll) {
#pragma unroll
            for (int j = 0; j < kTriUnroll; j++) comm_step(i + j, j);
        }
#pragma unroll
        for (int j = 0; j < kTriUnroll; j++)
            if (i + j < len) comm_step(i + j, j);
    } else {
        for (; i + kTriUnroll <= len; i += kTriUnroll) {
#pragma unroll
            for (int j = 0; j < kTriUnroll; j++) step(i + j, j);
        }
#pragma unroll
        for (int j = 0; j < kTriUnroll; j++)
            if (i + j < len) step(i + j, j);
    }
    if (comm) {
        publish(te - 1, (len - 1) & 1);
        if (stats && comm0 && lane == 0) {
            unsigned long long* q = stats + (size_t)bx * (8 + 2 * trace_h);
            q[0] = st_t0;
            q[1] = __builtin_amdgcn_s_memtime();
            q[2] = st_spin;
            q[3] = st_n;
            q[4] = (unsigned long long)len;
            q[5] = (unsigned long long)k;
            q[6] = (unsigned long long)pass;
            q[7] = (unsigned long long)tb;
        }
    }
}

template <int NP, int WV, int LPC, typename AccT, bool NW, bool RES>
int launch_tri_wv(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, const SgbmEff& e, const void* Cv, AccT* Av,
                  size_t plane)
{
    using TL = TriLayout<NP, WV, LPC>;
    constexpr int kTriSW = TriCfg<NP, WV, LPC>::kSW;
    const int nstrips = plan.nstrips, npass = plan.passes;
    int rc;
    unsigned epoch;
    long long ticket0;
    if ((rc = strip_begin(ctx, ctx->tri_bnd, 16, &epoch, &ticket0))) return rc;
    dim3 grid((unsigned)plan.blocks);
    // tri_stats: per-strip summary on stderr; tri_trace: also every step's
    // publish / consume time (100 MHz) of every strip, to a file
    const bool trace = !ctx->opt.tri_trace.empty();
    const size_t sb = 8 + (trace ? 2 * (size_t)H : 0);  // u64 per block
    unsigned long long* stats = (ctx->opt.tri_stats || trace) ? strip_stats_alloc(ctx, (size_t)grid.x * sb * 8) : nullptr;
    const int trace_h = stats && trace ? H : 0;
    if (TL::kBytes > 65536 &&
        (rc = check_hip(ctx, hipFuncSetAttribute((const void*)sgbm_tri_kernel<NP, WV, LPC, AccT, NW, RES>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)TL::kBytes),
                        "sgbm strip LDS attribute")))
        return rc;
    hipLaunchKernelGGL((sgbm_tri_kernel<NP, WV, LPC, AccT, NW, RES>), grid, dim3(TriCfg<NP, WV, LPC>::kThreads), TL::kBytes,
                       ctx->stream, Cv, Av, plane, (AccT*)ctx->dummy.ptr, H, e.W1, e.D, npass, e.P1,
                       e.P2, (unsigned long long*)ctx->tri_bnd.ptr, epoch, n, nstrips,
                       (int*)ctx->status.ptr, ctx->opt.spin_limit, ctx->report_target, stats, trace_h, ticket0);
    rc = check_hip(ctx, hipGetLastError(), "sgbm sheared-strip path kernel");
    if (rc == MVSV_OK && ticket0 >= 0) ctx->tri_tickets += grid.x;  // one ticket per block (u32 wrap is harmless)
    std::vector<unsigned long long> h;
    if (stats && strip_stats_read(ctx, stats, (size_t)grid.x * sb, &h)) {
        if (trace_h) {
            if (FILE* fp = std::fopen(ctx->opt.tri_trace.c_str(), "wb")) {
                const unsigned long long hdr[8] = {grid.x, sb, (unsigned long long)H, (unsigned long long)nstrips,
                                                   (unsigned long long)npass, (unsigned long long)n,
                                                   (unsigned long long)kTriSW, (unsigned long long)e.W1};
                std::fwrite(hdr, 8, 8, fp);
                std::fwrite(h.data(), 8, h.size(), fp);
                std::fclose(fp);
            }
        }
        unsigned long long t0 = ~0ull, t1 = 0, spin = 0, busy = 0, steps = 0, longest = 0, lst = 0;
        for (size_t b = 0; b < grid.x; b++) {
            const unsigned long long* q = &h[b * sb];
            if (!q[1]) continue;
            t0 = std::min(t0, q[0]);
            t1 = std::max(t1, q[1]);
            spin += q[2];
            busy += q[1] - q[0];
            steps += q[4];
            if (q[4] > longest) { longest = q[4]; lst = q[1] - q[0]; }
        }
        std::fprintf(stderr, "[tri] span %llu ticks, blocks %u, block-ticks %llu, spin-ticks %llu (%.1f%%), "
                     "ticks/step %.1f, longest strip %llu steps in %llu ticks\n",
                     t1 - t0, grid.x, busy, spin, 100.0 * spin / std::max(busy, 1ull),
                     (double)busy / std::max(steps, 1ull), longest, lst);
        for (size_t b = 0; b < grid.x; b += grid.x / 24 + 1) {
            const unsigned long long* q = &h[b * sb];
            std::fprintf(stderr, "[tri]  blk %zu k %llu pass %llu tb %llu len %llu start %llu dur %llu spin %llu n %llu\n",
                         b, q[5], q[6], q[7], q[4], q[0] - t0, q[1] - q[0], q[2], q[3]);
        }
    }
    return rc;
}

// The strip kernel of the plan's shape: 32 lanes per column (D = 256 launches
// too small for wide strips), else wide or narrow strips on 16 lanes.
// (Round 3's 8-lanes-per-column variant, LPC = 8, measured slower and is no
// longer instantiated; the kernel keeps the LPC parameter.)
template <int NP, typename AccT, bool NW, bool RES>
int launch_strips(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, const SgbmEff& e, const void* Cv, AccT* Av,
                  size_t plane)
{
    if constexpr (NP == 8 && !RES) {
        if (plan.lpc == 32)
            return launch_tri_wv<NP / 2, tri_narrow_waves(NP / 2, 32), 32, AccT, NW, RES>(ctx, plan, n, H, e, Cv, Av,
                                                                                         plane);
    }
    constexpr int wide = tri_wide_waves(NP, 16), narrow = tri_narrow_waves(NP, 16);
    if (plan.lpc != 16 || (plan.waves != wide && plan.waves != narrow))
        return set_error(ctx, MVSV_E_HIP, "internal: no strip kernel of the SGBM plan's shape");
    if (plan.waves == narrow) return launch_tri_wv<NP, narrow, 16, AccT, NW, RES>(ctx, plan, n, H, e, Cv, Av, plane);
    return launch_tri_wv<NP, wide, 16, AccT, NW, RES>(ctx, plan, n, H, e, Cv, Av, plane);
}

}  // namespace
}  // namespace mvsv
