// sgbm_eff.hpp — resolve_sgbm's rules (mvsv_host.cpp), written out again for the
// host-only checks of the SGBM launch plan (sgbm_plan_check.cpp, kernel_forms_check.cpp).
#pragma once

#include <cstring>

#include "../../mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp"

// false: the parameters are rejected (a cost space no wider than the window's half)
static bool eff(int W, int minD, int D, int bs, int P1, int P2, int cap, int uniq, int mode, int cn, mvsv::SgbmEff* e)
{
    std::memset(e, 0, sizeof *e);
    bs = bs > 0 ? bs : 5;
    e->minD = minD;
    e->D = D;
    e->maxD = minD + D;
    e->SW2 = e->SH2 = bs / 2;
    e->ftzero = (cap > 15 ? cap : 15) | 1;
    e->uniq = uniq >= 0 ? uniq : 10;
    e->disp12 = 1;
    e->P1 = P1 > 0 ? P1 : 2;
    e->P2 = P2 > 0 ? P2 : 5;
    if (e->P2 < e->P1 + 1) e->P2 = e->P1 + 1;
    e->minX1 = e->maxD > 0 ? e->maxD : 0;
    e->maxX1 = W + (minD < 0 ? minD : 0);
    e->W1 = e->maxX1 - e->minX1;
    e->invalid = (minD - 1) * 16;
    e->fullDP = mode;
    e->cn = cn;
    return !(e->W1 > 0 && e->W1 <= e->SW2);
}
