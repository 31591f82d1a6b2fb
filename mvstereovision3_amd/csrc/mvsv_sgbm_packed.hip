// mvsv_sgbm_packed.hip — the packed-int16 SGBM kernels of one disparity count:
// D = 32 * MVSV_SGBM_NP (NP disparity pairs per lane at 16 lanes per line).
// The Makefile compiles this source once per NP in {1, 2, 4, 8}; every kernel
// instance launch_packed16<NP> can reach lives in that NP's object, and
// sgbm_device (mvsv_sgbm.hip) sees only the declaration in mvsv_internal.hpp.
#include "mvsv_sgbm_launch.hpp"

#ifndef MVSV_SGBM_NP
#error "compile with -DMVSV_SGBM_NP=1, 2, 4 or 8"
#endif

namespace mvsv {

// The 16-lane kernels (D = 32 NP): the template instance for the plan's
// schedule, plane element, recurrence and cost input (Rv: the residual plane)
template <int NP>
int launch_packed16(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, int W, const SgbmEff& e, int16_t* Cv,
                    const uint8_t* Rv, const uint16_t* Mv, void* Av, int16_t* raw)
{
    if (plan.acc == kAccU8) return launch_plain16<NP, uint8_t>(ctx, plan, n, H, W, e, Cv, (uint8_t*)Av, raw);
    if (plan.acc == kAccU16) return launch_plain16<NP, uint16_t>(ctx, plan, n, H, W, e, Cv, (uint16_t*)Av, raw);
    nib2_t* A = (nib2_t*)Av;
    const bool side = plan.sched == 2;
    if constexpr (NP <= 4)
        if (plan.residual)
            return side ? launch_paths_dirs<NP, nib2_t, true, true>(ctx, plan, n, H, W, e, Cv, Rv, A, raw, Mv)
                        : launch_paths_tri<NP, nib2_t, true, true>(ctx, plan, n, H, W, e, Cv, Rv, A, raw, Mv);
    if (plan.nw)
        return side ? launch_paths_dirs<NP, nib2_t, true>(ctx, plan, n, H, W, e, Cv, Cv, A, raw)
                    : launch_paths_tri<NP, nib2_t, true>(ctx, plan, n, H, W, e, Cv, Cv, A, raw);
    return side ? launch_paths_dirs<NP, nib2_t, false>(ctx, plan, n, H, W, e, Cv, Cv, A, raw)
                : launch_paths_tri<NP, nib2_t, false>(ctx, plan, n, H, W, e, Cv, Cv, A, raw);
}

template int launch_packed16<MVSV_SGBM_NP>(mvsv_ctx*, const SgbmPlan&, int, int, int, const SgbmEff&, int16_t*,
                                           const uint8_t*, const uint16_t*, void*, int16_t*);

}  // namespace mvsv
