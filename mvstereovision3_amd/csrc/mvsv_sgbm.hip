// mvsv_sgbm.hip — StereoSGBM on MI355X (gfx950).
//
// Replaces Disparity::sgbm (src/disparity.cpp:6-10) -> cv::StereoSGBM::compute.
// Pipeline per batch of frames (all launches on the context stream):
//   1. sgbm_prefilter_kernel   clipped x-Sobel + raw channel per row    (u8 planes)
//      (a census call: census_kernel, mvsv_census.hip, and the census form of 2)
//      (stages 1-3 live in mvsv_cost.hip)
//   2. sgbm_cost_kernel        Birchfield-Tomasi pixel cost + bs x bs box
//                              sum -> C[y][x][d] int16 (+P2 bias), LDS-staged
//                              rows, running vertical sums in registers
//   3. sgbm_cost_fixup_*_kernel OpenCV 3.4's cost-row quirks (column x=0 and
//                              the bottom SH2 rows are not refreshed)
//   4. sgbm_path_kernel        one wave per scanline of one direction: the
//                              SGM recurrence on packed int16 pairs
//                              (v_pk_*_i16), d+-1 neighbours via DPP
//                              wave_shr/shl, per-step min over d via a DPP
//                              butterfly; S += L with int16 saturation
//   5. sgbm_final_kernel       the last direction (R->L) fused with WTA,
//                              uniqueness, sub-pixel fit, right-view map and
//                              the left-right check (one wave per row)
//   6. median 3x3 + optional speckle filter (mvsv_post.hip)
// Data layout in HBM: C and S are [frame][y][x][d] int16 with d contiguous,
// so one cost column (D = 128 -> 256 B) is one coalesced wave access.
//
// This unit holds sgbm_device and its host helpers, the generic kernels of
// stages 4 and 5 (any other D: one wave per scanline) and the D = 16 launcher.
// The packed kernels (D = 32, 64, 128, 256) are device code in the stage
// headers mvsv_sgbm_{common,lines,strips,final,launch}.hpp; each D's instances
// compile in an object of their own (mvsv_sgbm_packed.hip), reached through
// launch_packed16<NP> (declared in mvsv_internal.hpp).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "mvsv_cost_layout.hpp"
#include "mvsv_device.hpp"
#include "mvsv_bitslice.hpp"
#include "mvsv_internal.hpp"
#include "mvsv_sgbm_launch.hpp"


namespace mvsv {
namespace {

using namespace dev;

// ---------------------------------------------------------------------------
// 4. path aggregation along one direction (predecessor (x-dx, y-dy)).
// ---------------------------------------------------------------------------
// One wave per scanline.  The loop is branch-free around memory: every
// prefetch address is clamped into the line (duplicates are never consumed),
// so the compiler can count outstanding loads exactly and keep kPathPF steps
// of C / accumulator loads in flight.  FULL = every lane owns real
// disparities (D == 128 * NP); otherwise stores are lane-predicated.
constexpr int kPathPF = 8;

template <int NP, bool FIRST, bool FULL, typename AccT>
__global__ __launch_bounds__(256) void sgbm_path_kernel(const int16_t* __restrict__ C,
                                                        AccT* __restrict__ A, int H, int W1,
                                                        int D, int dx, int dy, int P1, int P2)
{
    using AV = AccVec<NP, AccT>;
    constexpr int PF = kPathPF;
    const int lane = threadIdx.x & 63;
    // wave-uniform by construction; readfirstlane keeps the line walk scalar
    const int line = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int f = blockIdx.y;
    if (line >= num_lines(dx, dy, W1, H)) return;
    const Line g = line_geometry(line, dx, dy, W1, H);
    const size_t frame = (size_t)H * W1 * D;
    const ptrdiff_t step = ((ptrdiff_t)dy * W1 + dx) * D;
    const int d0 = lane * 2 * NP;
    const bool lane_on = FULL || d0 < D;
    const size_t off = f * frame + ((size_t)g.ys * W1 + g.xs) * D + (lane_on ? d0 : 0);
    const int16_t* cp = C + off;
    AccT* ap = A + off;
    bool valid[NP];
    uint32_t lp[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        valid[p] = FULL || d0 + 2 * p < D;
        lp[p] = valid[p] ? 0u : 0x7fff7fffu;
    }
    const uint32_t p1x2 = (uint32_t)(P1 & 0xffff) * 0x10001u;
    const uint32_t p2x2 = (uint32_t)(P2 & 0xffff) * 0x10001u;
    int minp = 0;
    const int len = g.len;

    Vec<NP> cb[PF];
    uint32_t ab[PF][NP];
#pragma unroll
    for (int j = 0; j < PF; j++) {
        const ptrdiff_t t = min(j, len - 1);
        cb[j].load(cp + t * step);
        if (!FIRST) AV::load(ap + t * step, ab[j]);
    }
    auto body = [&](int s, int j) {
        const int dl = (int16_t)(minp + P2);
        const uint32_t delta2 = (uint32_t)(dl & 0xffff) * 0x10001u;
        uint32_t c[NP], ln[NP], o[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = cb[j].v[p];
        sgm_step<NP>(lp, delta2, p1x2, c, valid, ln);
        minp = wave_min_i32(lane_min<NP>(ln));
#pragma unroll
        for (int p = 0; p < NP; p++) {
            uint32_t dv = path_delta(ln[p], c[p], p2x2);
            o[p] = FIRST ? dv : AV::add(ab[j][p], dv);
            lp[p] = ln[p];
        }
        if (FULL || lane_on) AV::store(ap + (ptrdiff_t)s * step, o);
    };
    int s = 0;
    for (; s + PF <= len; s += PF) {
#pragma unroll
        for (int j = 0; j < PF; j++) {
            body(s + j, j);
            const ptrdiff_t t = min(s + j + PF, len - 1);
            cb[j].load(cp + t * step);
            if (!FIRST) AV::load(ap + t * step, ab[j]);
        }
    }
    const int rem = len - s;
#pragma unroll
    for (int j = 0; j < PF; j++)
        if (j < rem) body(s + j, j);
}

// ---------------------------------------------------------------------------
// 5. last direction (R->L) + WTA + uniqueness + sub-pixel + LR check.
// ---------------------------------------------------------------------------
constexpr int kFinalPF = 4;

template <int NP, bool FULL, typename AccT>
__global__ __launch_bounds__(64) void sgbm_final_kernel(const int16_t* __restrict__ C,
                                                       const AccT* __restrict__ A, int H,
                                                       int W, SgbmEff e,
                                                       int16_t* __restrict__ raw)
{
    using AV = AccVec<NP, AccT>;
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    constexpr int PF = kFinalPF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int16_t* disp1 = (int16_t*)smem;
    int16_t* d2 = disp1 + W;
    int16_t* d2c = d2 + W;
    const int lane = threadIdx.x;
    const int y = blockIdx.x;
    const int f = blockIdx.y;
    const int D = e.D, W1 = e.W1, minD = e.minD, minX1 = e.minX1;
    const int INV = e.invalid;
    for (int x = lane; x < W; x += 64) {
        disp1[x] = (int16_t)INV;
        d2[x] = (int16_t)INV;
        d2c[x] = (int16_t)kMaxCost;
    }
    __syncthreads();

    const bool lane_rule = !e.fullDP && !(e.variant & MVSV_VARIANT_WTA_MIN_D);
    const size_t frame = (size_t)H * W1 * D;
    const int d0 = lane * 2 * NP;
    const bool lane_on = FULL || d0 < D;
    const size_t off = f * frame + ((size_t)y * W1 + (W1 - 1)) * D + (lane_on ? d0 : 0);
    const int16_t* cp = C + off;
    const AccT* sp = A + off;
    bool valid[NP];
    uint32_t lp[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        valid[p] = FULL || d0 + 2 * p < D;
        lp[p] = valid[p] ? 0u : 0x7fff7fffu;
    }
    const uint32_t p1x2 = (uint32_t)(e.P1 & 0xffff) * 0x10001u;
    const uint32_t p2x2 = (uint32_t)(e.P2 & 0xffff) * 0x10001u;
    const int ndir = sgbm_ndir(e);  // 8, 5 or 4
    // a cost may pass 32767: C read as signed, S saturated on both sides
    const bool sgn = sgbm_signed_costs(e);
    int minp = 0;
    const int uq = e.uniq;

    Vec<NP> cb[PF];
    uint32_t sb[PF][NP];
#pragma unroll
    for (int j = 0; j < PF; j++) {
        const ptrdiff_t t = min(j, W1 - 1);
        cb[j].load(cp - t * D);
        AV::load(sp - t * D, sb[j]);
    }
    // phase A of one step: recurrence, total cost, WTA reductions (no LDS, no
    // branches); results per step: minS, best, rejected, Sm, Sp (wave-uniform)
    int rMin[PF], rBest[PF], rRej[PF], rSm[PF], rSp[PF];
    auto phaseA = [&](int j) {
        const int dl = (int16_t)(minp + e.P2);
        const uint32_t delta2 = (uint32_t)(dl & 0xffff) * 0x10001u;
        uint32_t c[NP], ln[NP], st[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = cb[j].v[p];
        sgm_step<NP>(lp, delta2, p1x2, c, valid, ln);
        minp = wave_min_i32(lane_min<NP>(ln));
        int key = 0x7fffffff;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            // S = min(ndir*(C - P2) + sum of deltas, MAX_COST), saturating u16
            u16x2 cbv = __builtin_bit_cast(u16x2, c[p]) - __builtin_bit_cast(u16x2, p2x2);
            u16x2 x2 = __builtin_elementwise_add_sat(cbv, cbv);
            u16x2 x4 = __builtin_elementwise_add_sat(x2, x2);
            u16x2 t = ndir == 8   ? __builtin_elementwise_add_sat(x4, x4)
                      : ndir == 5 ? __builtin_elementwise_add_sat(x4, cbv)
                                  : x4;
            u16x2 acc = __builtin_elementwise_add_sat(
                __builtin_bit_cast(u16x2, sb[j][p]),
                __builtin_bit_cast(u16x2, path_delta(ln[p], c[p], p2x2)));
            u16x2 sv = __builtin_elementwise_min(__builtin_elementwise_add_sat(t, acc),
                                                 (u16x2){32767, 32767});
            st[p] = valid[p] ? __builtin_bit_cast(uint32_t, sv) : 0x7fff7fffu;
            if (sgn && valid[p]) {
                // S = clamp(ndir*(C - P2) + sum of deltas, -32768, MAX_COST) on the signed cost, in int32
                const uint32_t dl2 = path_delta(ln[p], c[p], p2x2);
                auto one = [&](int cs, uint32_t a, uint32_t dlt) -> int {
                    return max(min(ndir * (cs - e.P2) + (int)(a & 0xffffu) + (int)(dlt & 0xffffu), kMaxCost), -32768);
                };
                st[p] = pk2(one(lo16(c[p]), sb[j][p], dl2), one(hi16(c[p]), sb[j][p] >> 16, dl2 >> 16));
            }
            lp[p] = ln[p];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                int d = d0 + 2 * p + h;
                int v = h ? hi16(st[p]) : lo16(st[p]);
                int sub = lane_rule ? (((d & 7) << 12) | (d >> 3)) : d;
                key = min(key, valid[p] ? ((v << 16) | sub) : 0x7fffffff);
            }
        }
        const int K = wave_min_i32(key);
        const int minS = K >> 16;
        const int sub = K & 0xffff;
        int best = lane_rule ? (((sub & 0xfff) << 3) | (sub >> 12)) : sub;
        if (minS >= kMaxCost) best = -1;  // no strict minimum below MAX_COST
        bool rej = false;
#pragma unroll
        for (int p = 0; p < NP; p++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                int d = d0 + 2 * p + h;
                int v = h ? hi16(st[p]) : lo16(st[p]);
                rej |= valid[p] && (v * (100 - uq) < minS * 100) && (abs(best - d) > 1);
            }
        }
        auto fetch = [&](int d) -> int {
            d = clampi(d, 0, D - 1);
            int ln_ = d / (2 * NP), el = d - ln_ * 2 * NP;
            uint32_t v = st[0];
#pragma unroll
            for (int p = 1; p < NP; p++) v = ((el >> 1) == p) ? st[p] : v;
            uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)v, ln_);
            return (el & 1) ? hi16(w) : lo16(w);
        };
        rMin[j] = minS;
        rBest[j] = best;
        rRej[j] = __ballot(rej) != 0ull;
        rSm[j] = fetch(best - 1);
        rSp[j] = fetch(best + 1);
    };
    // phase B of one step (x descending, sequential semantics of the scan)
    auto phaseB = [&](int s, int j) {
        if (rRej[j]) return;
        const int x = W1 - 1 - s;
        const int minS = rMin[j], best = rBest[j];
        const int x2 = x + minX1 - best - minD;
        if (lane == 0 && x2 >= 0 && x2 < W && d2c[x2] > minS) {
            d2c[x2] = (int16_t)minS;
            d2[x2] = (int16_t)(best + minD);
        }
        int d16;
        if (0 < best && best < D - 1) {
            const int Sm = rSm[j], Sp = rSp[j];
            const int den = max(Sm + Sp - 2 * minS, 1);
            d16 = best * kDispScale + ((Sm - Sp) * kDispScale + den) / (den * 2);
        } else {
            d16 = best * kDispScale;
        }
        if (lane == 0) disp1[x + minX1] = (int16_t)(d16 + minD * kDispScale);
    };
    int s = 0;
    for (; s + PF <= W1; s += PF) {
#pragma unroll
        for (int j = 0; j < PF; j++) {
            phaseA(j);
            const ptrdiff_t t = min(s + j + PF, W1 - 1);
            cb[j].load(cp - t * D);
            AV::load(sp - t * D, sb[j]);
        }
#pragma unroll
        for (int j = 0; j < PF; j++) phaseB(s + j, j);
    }
    const int rem = W1 - s;
#pragma unroll
    for (int j = 0; j < PF; j++)
        if (j < rem) phaseA(j);
#pragma unroll
    for (int j = 0; j < PF; j++)
        if (j < rem) phaseB(s + j, j);
    __syncthreads();
    int16_t* out = raw + ((size_t)f * H + y) * W;
    for (int x = lane; x < W; x += 64) {
        int v = disp1[x];
        if (x >= minX1 && x < e.maxX1 && v != INV) {
            int dl = v >> kDispShift, dh = (v + kDispScale - 1) >> kDispShift;
            int xl = x - dl, xh = x - dh;
            if (0 <= xl && xl < W && d2[xl] >= minD && abs(d2[xl] - dl) > e.disp12 && 0 <= xh &&
                xh < W && d2[xh] >= minD && abs(d2[xh] - dh) > e.disp12)
                v = INV;
        }
        out[x] = (int16_t)v;
    }
}

__global__ void fill_s16_kernel(int16_t* __restrict__ out, size_t os, size_t ofs, int W, int H,
                                int16_t v)
{
    const int y = blockIdx.x, f = blockIdx.y;
    int16_t* o = out + f * ofs + (size_t)y * os;
    for (int x = threadIdx.x; x < W; x += blockDim.x) o[x] = v;
}

// the generic kernels: one wave per scanline, NP = ceil(D / 128) pairs per lane
template <int NP, typename AccT>
int launch_paths(mvsv_ctx* ctx, int n, int H, int W, const SgbmEff& e, int16_t* Cv, AccT* Av,
                 int16_t* raw)
{
    hipStream_t s = ctx->stream;
    const int ndir = sgbm_ndir(e) - 1;
    for (int k = 0; k < ndir; k++) {
        const int* dir = kPathDirs[sgbm_pass_dir(e, k)];
        const int dx = dir[0], dy = dir[1];
        int nl = num_lines(dx, dy, e.W1, H);
        dim3 grid((nl + 3) / 4, n);
        StageTimer tm(ctx, kStagePath);
        const bool full = e.D == 128 * NP;
        if (k == 0 && full)
            hipLaunchKernelGGL((sgbm_path_kernel<NP, true, true, AccT>), grid, dim3(256), 0, s,
                               Cv, Av, H, e.W1, e.D, dx, dy, e.P1, e.P2);
        else if (k == 0)
            hipLaunchKernelGGL((sgbm_path_kernel<NP, true, false, AccT>), grid, dim3(256), 0, s,
                               Cv, Av, H, e.W1, e.D, dx, dy, e.P1, e.P2);
        else if (full)
            hipLaunchKernelGGL((sgbm_path_kernel<NP, false, true, AccT>), grid, dim3(256), 0, s,
                               Cv, Av, H, e.W1, e.D, dx, dy, e.P1, e.P2);
        else
            hipLaunchKernelGGL((sgbm_path_kernel<NP, false, false, AccT>), grid, dim3(256), 0, s,
                               Cv, Av, H, e.W1, e.D, dx, dy, e.P1, e.P2);
    }
    size_t lds = (size_t)W * 3 * sizeof(int16_t);
    StageTimer tm(ctx, kStageFinal);
    if (e.D == 128 * NP)
        hipLaunchKernelGGL((sgbm_final_kernel<NP, true, AccT>), dim3(H, n), dim3(64), lds, s, Cv,
                           Av, H, W, e, raw);
    else
        hipLaunchKernelGGL((sgbm_final_kernel<NP, false, AccT>), dim3(H, n), dim3(64), lds, s, Cv,
                           Av, H, W, e, raw);
    return check_hip(ctx, hipGetLastError(), "sgbm path kernels");
}

// D = 16: the directions side by side at 8 lanes per line / row (one disparity
// pair per lane)
int launch_packed8(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, int W, const SgbmEff& e, int16_t* Cv, void* Av,
                   int16_t* raw)
{
    if (plan.acc == kAccU8)
        return launch_paths_dirs<1, uint8_t, false, false, 8>(ctx, plan, n, H, W, e, Cv, Cv, (uint8_t*)Av, raw);
    if (plan.acc == kAccU16)
        return launch_paths_dirs<1, uint16_t, false, false, 8>(ctx, plan, n, H, W, e, Cv, Cv, (uint16_t*)Av, raw);
    if (plan.nw) return launch_paths_dirs<1, nib2_t, true, false, 8>(ctx, plan, n, H, W, e, Cv, Cv, (nib2_t*)Av, raw);
    return launch_paths_dirs<1, nib2_t, false, false, 8>(ctx, plan, n, H, W, e, Cv, Cv, (nib2_t*)Av, raw);
}

template <int NP>
int launch_generic(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, int W, const SgbmEff& e, int16_t* Cv, void* Av,
                   int16_t* raw)
{
    if (plan.acc == kAccU8) return launch_paths<NP, uint8_t>(ctx, n, H, W, e, Cv, (uint8_t*)Av, raw);
    return launch_paths<NP, uint16_t>(ctx, n, H, W, e, Cv, (uint16_t*)Av, raw);
}

// every cached buffer of the call, at the plan's size (0: the call does not touch it)
int ensure_plan_buffers(mvsv_ctx* ctx, const SgbmPlan& plan)
{
    int rc;
    auto need = [&](DevBuf& b, size_t bytes, const char* what) { return bytes ? ensure(ctx, b, bytes, what) : MVSV_OK; };
    // boundary granules and status words start zeroed: fresh granules carry
    // tag 0, which no launch uses; status [0] give-up epoch, [2] strip tickets drawn
    auto need_zeroed = [&](DevBuf& b, size_t bytes, const char* what) {
        if (b.bytes >= bytes) return (int)MVSV_OK;
        if (int r = ensure(ctx, b, bytes, what)) return r;
        return check_hip(ctx, hipMemsetAsync(b.ptr, 0, b.bytes, ctx->stream), what);
    };
    if ((rc = need(ctx->pre, plan.pre, "sgbm BT interval planes")) ||
        (rc = need(ctx->cost, plan.cost, "sgbm cost volume")) ||
        (rc = need(ctx->cres, plan.cres, plan.residual ? "sgbm cost residual plane" : "sgbm bit-sliced cost planes")) ||
        (rc = need(ctx->agg, plan.agg, plan.family == kFamBitslice ? "bit-sliced delta planes"
                                                                   : "sgbm path-delta accumulator")) ||
        (rc = need(ctx->raw, plan.raw, "sgbm raw disparity")) ||
        (rc = need(ctx->keys, plan.keys, "sgbm right-view keys")) ||
        (rc = need(ctx->dummy, plan.dummy, "sgbm dummy slots")) ||
        (rc = need_zeroed(ctx->tri_bnd, plan.tri_bnd, "sgbm strip boundary granules")) ||
        (rc = need_zeroed(ctx->bs_bnd, plan.bs_bnd, "bit-sliced strip boundary granules")))
        return rc;
    if (plan.status && !ctx->status.ptr) {
        if ((rc = need_zeroed(ctx->status, plan.status, "device status words"))) return rc;
        ctx->tri_tickets = 0;
    }
    return MVSV_OK;
}

}  // namespace

int ensure_aux(mvsv_ctx* ctx)
{
    if (ctx->aux) return MVSV_OK;
    int rc;
    if ((rc = check_hip(ctx, hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking), "aux stream")) ||
        (rc = check_hip(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming), "event")) ||
        (rc = check_hip(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming), "event")))
        return rc;
    return MVSV_OK;
}

int strip_begin(mvsv_ctx* ctx, DevBuf& bnd, int tag_bits, unsigned* epoch, long long* ticket0)
{
    if ((++ctx->tri_epoch & 0xffffu) == 0) {
        ++ctx->tri_epoch;
        if (tag_bits == 16)
            if (int rc = check_hip(ctx, hipMemsetAsync(bnd.ptr, 0, bnd.bytes, ctx->stream), "strip boundary reset"))
                return rc;
    }
    *epoch = ctx->tri_epoch;
    *ticket0 = ctx->opt.strip_tickets ? (long long)ctx->tri_tickets : -1ll;
    return MVSV_OK;
}

unsigned long long* strip_stats_alloc(mvsv_ctx* ctx, size_t bytes)
{
    unsigned long long* stats = nullptr;
    if (hipMalloc(&stats, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (hipMemsetAsync(stats, 0, bytes, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(stats);
        return nullptr;
    }
    return stats;
}

bool strip_stats_read(mvsv_ctx* ctx, unsigned long long* stats, size_t words, std::vector<unsigned long long>* h)
{
    h->resize(words);
    const bool ok = hipStreamSynchronize(ctx->stream) == hipSuccess &&
                    hipMemcpy(h->data(), stats, words * 8, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(stats);
    if (!ok) (void)hipGetLastError();
    return ok;
}

// The pipeline: make the plan, ensure every buffer from it, then prefilter,
// cost, fix-up, one dispatch on the plan's fields to the path kernels' template
// instance, post filters.
int sgbm_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                size_t rs, size_t rfs, int W, int H, const SgbmEff& e, int16_t* out, size_t os,
                size_t ofs)
{
    hipStream_t s = ctx->stream;
    int rc;
    if (e.minX1 >= e.maxX1) {
        hipLaunchKernelGGL(fill_s16_kernel, dim3(H, n), dim3(256), 0, s, out, os, ofs, W, H,
                           (int16_t)e.invalid);
        return check_hip(ctx, hipGetLastError(), "sgbm fill");
    }
    if (e.D > 512) return set_error(ctx, MVSV_E_INVALID_ARG, "numDisparities > 512 not supported");
    const SgbmPlan plan = sgbm_make_plan(ctx, e, n, W, H);
    if ((rc = ensure_plan_buffers(ctx, plan))) return rc;
    uint64_t* pre = (uint64_t*)ctx->pre.ptr;
    int16_t* Cv = (int16_t*)ctx->cost.ptr;
    void* Sv = ctx->agg.ptr;
    int16_t* raw = (int16_t*)ctx->raw.ptr;
    // the residual plane (0.5 byte per cost) or the bit-sliced C' planes, and
    // the per-pixel cost minimum (u16 per cost column) behind either
    const bool bits = plan.family == kFamBitslice;
    uint32_t* Bv = bits ? (uint32_t*)ctx->cres.ptr : nullptr;
    uint8_t* Rv = plan.residual ? (uint8_t*)ctx->cres.ptr : nullptr;
    uint16_t* Mv = plan.cres ? (uint16_t*)((uint8_t*)ctx->cres.ptr + plan.cres_min) : nullptr;

    if (sgbm_census(e)) {
        // the descriptors of both views in place of the BT interval planes
        if (e.cn != 1) return set_error(ctx, MVSV_E_INVALID_ARG, "census window: 3-channel pairs are not supported");
        if ((rc = census_device(ctx, n, 2, L, ls, lfs, R, rs, rfs, W, H, e.cw, e.ch, pre, (size_t)W, (size_t)W * H,
                                (size_t)2 * W * H)))
            return rc;
    } else if ((rc = launch_prefilter(ctx, n, L, ls, lfs, R, rs, rfs, W, H, e.ftzero, e.cn, pre))) {
        return rc;
    }
    if ((rc = launch_cost(ctx, plan, n, W, H, e, pre, Cv, Rv, Mv, Bv))) return rc;
    if (bits) {
        // bit-sliced layouts (MODE_SGBM: copied rows / column 0; MODE_HH: pinned
        // by the cost kernel)
        if ((rc = bsgm_cost_fixup(ctx, n, H, e, Cv, Bv, Mv))) return rc;
    } else if (H > 1 && !e.hh4 && !(plan.cost2 && e.fullDP)) {
        // OpenCV 3.4's never-recomputed rows and column 0 (mvsv_cost.hip; the
        // register-ring kernel pins MODE_HH's itself).  MODE_HH4 keeps the clean
        // volume both cost kernels compute.
        if ((rc = launch_cost_fixup(ctx, n, H, e, Cv, Rv, Mv))) return rc;
    }

    switch (plan.family) {
    case kFamBitslice: rc = bsgm_paths(ctx, plan, n, H, W, e, Cv, Bv, Mv, raw); break;
    case kFamPacked8: rc = launch_packed8(ctx, plan, n, H, W, e, Cv, Sv, raw); break;
    case kFamPacked16:
        switch (e.D) {
        case 32: rc = launch_packed16<1>(ctx, plan, n, H, W, e, Cv, Rv, Mv, Sv, raw); break;
        case 64: rc = launch_packed16<2>(ctx, plan, n, H, W, e, Cv, Rv, Mv, Sv, raw); break;
        case 128: rc = launch_packed16<4>(ctx, plan, n, H, W, e, Cv, Rv, Mv, Sv, raw); break;
        default: rc = launch_packed16<8>(ctx, plan, n, H, W, e, Cv, nullptr, nullptr, Sv, raw); break;
        }
        break;
    default:
        rc = e.D <= 128   ? launch_generic<1>(ctx, plan, n, H, W, e, Cv, Sv, raw)
             : e.D <= 256 ? launch_generic<2>(ctx, plan, n, H, W, e, Cv, Sv, raw)
                          : launch_generic<4>(ctx, plan, n, H, W, e, Cv, Sv, raw);
    }
    if (rc) return rc;

    // a strip launch of this call that gave up a wait poisons the median's output
    StageTimer tm(ctx, kStagePost);
    const int* poison = plan.sched == 1 ? (const int*)ctx->status.ptr : nullptr;
    if ((rc = median3x3_device(ctx, n, raw, W, (size_t)W * H, out, os, ofs, W, H, poison, ctx->tri_epoch, e.invalid)))
        return rc;
    if (e.speckle_window > 0)
        return speckle_device(ctx, n, out, os, ofs, W, H, e.invalid, e.speckle_window, e.speckle_diff);
    return MVSV_OK;
}

}  // namespace mvsv
