// mvsv_sgbm_launch.hpp — the schedules of the packed SGBM kernels: sheared
// strips + L->R lines, one line launch per direction, directions side by side.
#pragma once

#include <algorithm>
#include <type_traits>

#include "mvsv_sgbm_final.hpp"
#include "mvsv_sgbm_lines.hpp"
#include "mvsv_sgbm_strips.hpp"

namespace mvsv {
namespace {

// ---------------------------------------------------------------------------
// host side: launchers.  They launch what the SgbmPlan (mvsv_sgbm_plan.hpp)
// names on the buffers sgbm_device ensured from it; none of them decides a
// schedule, a kernel shape or a buffer size.
// ---------------------------------------------------------------------------
// Sheared-strip schedule: the down pass ((1,1) (0,1) (-1,1)), the up pass
// ((1,-1) (0,-1) (-1,-1), MODE_HH) and the L->R lines each write their own
// accumulator plane; the L->R lines run where plan.lines_aux says (0 = after
// the strip kernel on the same stream, 1 = on the second stream launched
// before it, 2 = on the second stream after it), and the final kernel (R->L +
// WTA) sums the planes.  The direction passes read Cin -- the cost volume, or
// (RES) its residual plane -- and the final kernel the cost volume Cv.
template <int NP, typename AccT, bool NW, bool RES = false>
int launch_paths_tri(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, int W, const SgbmEff& e, int16_t* Cv,
                     const void* Cin, AccT* Av, int16_t* raw, const uint16_t* Mv = nullptr)
{
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = ensure_aux(ctx))) return rc;
    const int npass = plan.passes;
    const size_t plane = (size_t)n * H * e.W1 * e.D;
    {
        StageTimer tm(ctx, kStagePath);
        if ((rc = check_hip(ctx, hipEventRecord(ctx->ev_fork, s), "fork")) ||
            (rc = check_hip(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0), "fork wait")))
            return rc;
        hipStream_t ls = plan.lines_aux ? ctx->aux : s;
        auto lines = [&]() {
            StageTimer tl(ctx, kStageLines, ls);
            dim3 grid((num_lines(1, 0, e.W1, H) + 15) / 16, n);
            hipLaunchKernelGGL((sgbm_path16_kernel<NP, true, AccT, NW, RES>), grid, dim3(256), 0, ls, Cin,
                               acc_add(Av, (ptrdiff_t)npass * (ptrdiff_t)plane), (AccT*)ctx->dummy.ptr, H, e.W1,
                               e.D, 1, 0, e.P1, e.P2);
        };
        if (plan.lines_aux == 1) lines();
        if ((rc = check_hip(ctx, hipGetLastError(), "sgbm L->R lines"))) return rc;
        {
            StageTimer ts(ctx, kStageStrips);
            if ((rc = launch_strips<NP, AccT, NW, RES>(ctx, plan, n, H, e, Cin, Av, plane))) return rc;
        }
        if (plan.lines_aux != 1) lines();
        if ((rc = check_hip(ctx, hipEventRecord(ctx->ev_join, ctx->aux), "join")) ||
            (rc = check_hip(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0), "join wait")))
            return rc;
    }
    StageTimer tm(ctx, kStageFinal);
    if (npass == 2)
        launch_final16<NP, 3, AccT, NW, RES>(ctx, n, H, W, e, Cv, Av, plane, raw, Cin, Mv);
    else
        launch_final16<NP, 2, AccT, NW, RES>(ctx, n, H, W, e, Cv, Av, plane, raw, Cin, Mv);
    return check_hip(ctx, hipGetLastError(), "sgbm path kernels (sheared strips)");
}

// schedule 0 on 16 lanes: one launch per direction into one plane
template <int NP, typename AccT>
int launch_paths_lines16(mvsv_ctx* ctx, int n, int H, int W, const SgbmEff& e, int16_t* Cv, AccT* Av, int16_t* raw)
{
    hipStream_t s = ctx->stream;
    AccT* dummy = (AccT*)ctx->dummy.ptr;
    const int ndir = sgbm_ndir(e) - 1;
    for (int k = 0; k < ndir; k++) {
        const int* dir = kPathDirs[sgbm_pass_dir(e, k)];
        const int dx = dir[0], dy = dir[1];
        dim3 grid((num_lines(dx, dy, e.W1, H) + 15) / 16, n);
        StageTimer tm(ctx, kStagePath);
        if (k == 0)
            hipLaunchKernelGGL((sgbm_path16_kernel<NP, true, AccT>), grid, dim3(256), 0, s, Cv, Av,
                               dummy, H, e.W1, e.D, dx, dy, e.P1, e.P2);
        else
            hipLaunchKernelGGL((sgbm_path16_kernel<NP, false, AccT>), grid, dim3(256), 0, s, Cv,
                               Av, dummy, H, e.W1, e.D, dx, dy, e.P1, e.P2);
    }
    StageTimer tm(ctx, kStageFinal);
    launch_final16<NP, 1, AccT>(ctx, n, H, W, e, Cv, Av, (size_t)n * H * e.W1 * e.D, raw);
    return check_hip(ctx, hipGetLastError(), "sgbm path kernels (16-lane)");
}

// Directions side by side: one plane per direction (plan.nplanes of them; the
// split form has the R->L direction as one more chain set and the WTA on its
// own), then the final kernel over the planes.
template <int NP, typename AccT, bool NW, bool RES = false, int LPC = 16>
int launch_paths_dirs(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, int W, const SgbmEff& e, int16_t* Cv,
                      const void* Cin, AccT* Av, int16_t* raw, const uint16_t* Mv = nullptr)
{
    constexpr bool kPlainPlanes = std::is_same<AccT, uint16_t>::value || std::is_same<AccT, uint8_t>::value;
    const int ndir = plan.nplanes;
    if (plan.split && (RES || !kPlainPlanes))
        return set_error(ctx, MVSV_E_HIP, "internal: the SGBM plan splits the WTA on packed planes");
    PathDirs pd{};
    int maxnl = 0;
    for (int k = 0; k < ndir; k++) {
        const int* d = kPathDirs[plan.split && k == ndir - 1 ? kPathDirRL : sgbm_pass_dir(e, k)];
        pd.dx[k] = d[0];
        pd.dy[k] = d[1];
        maxnl = std::max(maxnl, num_lines(pd.dx[k], pd.dy[k], e.W1, H));
    }
    const size_t plane = (size_t)n * H * e.W1 * e.D;
    {
        StageTimer tm(ctx, kStagePath);
        constexpr int lpb = path16_lines_per_block<LPC>();
        hipLaunchKernelGGL((sgbm_pathdirs16_kernel<NP, AccT, NW, RES, LPC>), dim3((maxnl + lpb - 1) / lpb, n, ndir),
                           dim3(256), 0, ctx->stream, Cin, Av, plane, (AccT*)ctx->dummy.ptr, H, e.W1, e.D, pd,
                           e.P1, e.P2);
    }
    StageTimer tm(ctx, kStageFinal);
    if constexpr (kPlainPlanes) {
        if (plan.split) {
            constexpr int LPP = 2 * NP * LPC / 8;  // D / 8
            if (e.uniq > 0)
                hipLaunchKernelGGL((sgbm_wta_planes_kernel<AccT, true, LPP>), dim3(H, n), dim3(kWtaThreads), 0,
                                   ctx->stream, Cv, Av, plane, ndir, H, W, e, raw, (uint32_t*)ctx->keys.ptr);
            else
                hipLaunchKernelGGL((sgbm_wta_planes_kernel<AccT, false, LPP>), dim3(H, n), dim3(kWtaThreads), 0,
                                   ctx->stream, Cv, Av, plane, ndir, H, W, e, raw, (uint32_t*)ctx->keys.ptr);
            return check_hip(ctx, hipGetLastError(), "sgbm path kernels (directions side by side, split WTA)");
        }
    }
    if (ndir == 7)
        launch_final16<NP, 7, AccT, NW, RES, LPC>(ctx, n, H, W, e, Cv, Av, plane, raw, Cin, Mv);
    else if (ndir == 3)
        launch_final16<NP, 3, AccT, NW, RES, LPC>(ctx, n, H, W, e, Cv, Av, plane, raw, Cin, Mv);
    else
        launch_final16<NP, 4, AccT, NW, RES, LPC>(ctx, n, H, W, e, Cv, Av, plane, raw, Cin, Mv);
    return check_hip(ctx, hipGetLastError(), "sgbm path kernels (directions side by side)");
}

// 16 lanes on byte / u16 planes.  The final kernel sums the planes in the
// plane's element type; the strips run the no-wrap recurrence at D = 256 only
// (plan.nw; other D keep the general form: compile time).
template <int NP, typename AccT>
int launch_plain16(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, int W, const SgbmEff& e, int16_t* Cv, AccT* Av,
                   int16_t* raw)
{
    if (plan.sched == 2) return launch_paths_dirs<NP, AccT, false>(ctx, plan, n, H, W, e, Cv, Cv, Av, raw);
    if (plan.sched == 0) return launch_paths_lines16<NP, AccT>(ctx, n, H, W, e, Cv, Av, raw);
    if constexpr (NP == 8)
        if (plan.nw) return launch_paths_tri<NP, AccT, true>(ctx, plan, n, H, W, e, Cv, Cv, Av, raw);
    return launch_paths_tri<NP, AccT, false>(ctx, plan, n, H, W, e, Cv, Cv, Av, raw);
}

}  // namespace
}  // namespace mvsv
