// kernel_forms_check.cpp — host-only: the SGBM launch plan of every case of
// tests/kernel_form_cases.py.  Reads one case per line from stdin,
//   cost2 path16 tri cost_fixed_pp cost_ty path_sched lines_aux cost_xcd bitslice
//   minD D blockSize P1 P2 preFilterCap uniquenessRatio mode channels   n W H cus
// (KernelOptions fields, StereoSGBM parameters, launch shape) and prints, per line,
//   family sched cost2 cost_ty residual acc nplanes split nw lpc waves lines_aux bits stg ppc GX GYn
// of sgbm_make_plan: stg / ppc (staged items per thread, compile-time pair count) and the
// cost grid (tile columns, row bands x frames) of the register-ring cost kernel, -1 where the
// LDS-ring kernel runs.  tests/test_kernel_forms.py compares them with the form each case
// states.  With the argument "wide" every line carries three more KernelOptions fields at its
// end,
//   tri32 final_split strip_waves
// and every printed line one more column, no_wrap (tests/sgbm_wrap_cases.py: the forms of the
// general recurrence).  Plain g++, no library, no GPU.
#include <cstdio>
#include <cstring>

#include "../../mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp"
#include "sgbm_eff.hpp"

using namespace mvsv;

int main(int argc, char** argv)
{
    const bool wide = argc > 1 && !std::strcmp(argv[1], "wide");
    KernelOptions o;
    int minD, D, bs, P1, P2, cap, uniq, mode, cn, n, W, H, cus;
    int lines = 0;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &o.cost2, &o.path16, &o.tri,
                      &o.cost_fixed_pp, &o.cost_ty, &o.path_sched, &o.lines_aux, &o.cost_xcd, &o.bitslice, &minD, &D, &bs,
                      &P1, &P2, &cap, &uniq, &mode, &cn, &n, &W, &H, &cus) == 22) {
        if (wide && std::scanf("%d %d %d", &o.tri32, &o.final_split, &o.strip_waves) != 3) return 2;
        SgbmEff e;
        if (!eff(W, minD, D, bs, P1, P2, cap, uniq, mode, cn, &e)) {
            std::printf("rejected\n");
            return 2;
        }
        const SgbmPlan p = sgbm_make_plan(o, cus, e, n, W, H);
        if (p.empty) {
            std::printf("empty\n");
            return 2;
        }
        int stg = -1, ppc = -1, gx = -1, gyn = -1;
        if (p.cost2) {
            const Cost2Launch c = cost2_launch(e, o.cost_fixed_pp, p.cost_ty);
            stg = c.stg, ppc = c.ppc;
            gx = ceil_div(e.W1, c.l.TX), gyn = ceil_div(H, p.cost_ty) * n;
        }
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", p.family, p.sched, (int)p.cost2, p.cost_ty,
                    (int)p.residual, p.acc, p.nplanes, (int)p.split, (int)p.nw, p.lpc, p.waves, p.lines_aux, p.bits(), stg,
                    ppc, gx, gyn);
        std::printf(wide ? " %d\n" : "\n", (int)p.no_wrap);
        lines++;
    }
    return lines ? 0 : 2;
}
