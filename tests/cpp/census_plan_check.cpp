// census_plan_check.cpp — host-only check of the launch plan of a census call
// (mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp, SgbmEff::cw / ch), over the shape grid of
// sgbm_plan_check.cpp: a census plan never orders the register-ring cost kernel, the
// residual plane or the bit planes; every later choice is the one the existing rules make
// for a Birchfield-Tomasi launch that has those three switched off; total_bytes() is the
// sum of the allocations.  Plain g++, no library, no GPU.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp"
#include "sgbm_eff.hpp"  // eff(): resolve_sgbm's rules (memsets the struct: cw = ch = 0, the BT cost)

using namespace mvsv;

static long g_fail = 0, g_plans = 0, g_skipped = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_fail++ < 40) {                          \
                std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static const char* tag(const SgbmEff& e, int n, int W, int H)
{
    static char b[220];
    std::snprintf(b, sizeof b, "n=%d %dx%d D=%d bs=%d P1=%d P2=%d hh=%d hh4=%d uniq=%d minD=%d window %dx%d", n, W, H,
                  e.D, 2 * e.SW2 + 1, e.P1, e.P2, e.fullDP, e.hh4, e.uniq, e.minD, e.cw, e.ch);
    return b;
}

static const int kWindows[][2] = {{9, 7}, {5, 5}, {7, 9}, {3, 3}, {13, 5}, {1, 3}, {3, 1}, {65, 1}};

// mvsv_sgbm_census_validate's bound: no cost leaves int16
static bool census_valid(const SgbmEff& e)
{
    const long bs = 2L * e.SW2 + 1;
    return (long)e.P2 + bs * bs * (e.cw * e.ch - 1) <= 32767;
}

static void check_census_plan(const KernelOptions& o, int cus, const SgbmEff& bt, int wi, int n, int W, int H)
{
    SgbmEff e = bt;
    e.cw = kWindows[wi][0];
    e.ch = kWindows[wi][1];
    if (!census_valid(e)) {
        g_skipped++;
        return;
    }
    const char* t = tag(e, n, W, H);
    g_plans++;
    CHECK(sgbm_census(e) && !sgbm_census(bt) && sgbm_bt_grey(bt) && !sgbm_bt_grey(e), "%s", t);
    CHECK(sgbm_max_pixel_cost(e) == e.cw * e.ch - 1 && sgbm_max_pixel_cost(bt) == 2 * bt.ftzero + 63, "%s", t);
    const SgbmPlan p = sgbm_make_plan(o, cus, e, n, W, H);
    CHECK(p.total_bytes() == p.pre + p.cost + p.cres + p.agg + p.raw + p.keys + p.dummy + p.tri_bnd + p.bs_bnd + p.status,
          "%s", t);
    const bool nonempty = e.minX1 < e.maxX1 && e.D <= 512;
    CHECK(p.empty == !nonempty, "%s", t);
    if (p.empty) {
        CHECK(p.total_bytes() == 0 && p.bits() == 0, "%s", t);
        return;
    }
    // never the register-ring kernel, a residual plane or bit planes
    CHECK(!p.cost2, "%s: register-ring cost kernel", t);
    CHECK(!p.residual && p.cres == 0 && p.cres_min == 0, "%s: residual plane", t);
    CHECK(p.family != kFamBitslice && p.bs_bnd == 0 && p.bs_groups == 0 && p.bs_aplane == 0 && p.bs_dplane == 0,
          "%s: bit planes", t);
    CHECK((p.bits() & (kPlanBitslice | kPlanResidual)) == 0, "%s bits %d", t, p.bits());
    CHECK(!cost2_runs(o, e) && !bsgm_eligible(o, e, n, H) && !use_residual(o, e, 1) && !use_residual(o, e, 2), "%s", t);
    // one u64 descriptor per pixel and view: the BT planes' size for a grey pair
    CHECK(p.pre == (size_t)n * 2 * W * H * 8, "%s", t);
    const long bs = 2L * e.SW2 + 1;
    CHECK(p.no_wrap == (2L * e.P2 + bs * bs * (e.cw * e.ch - 1) <= 32767), "%s", t);
    CHECK(!p.nw || p.no_wrap, "%s", t);
    // everything else: the existing rules, as they decide for a BT launch without those three
    KernelOptions ob = o;
    ob.cost2 = 0;
    ob.cost_res = 0;
    ob.bitslice = 0;
    const SgbmPlan q = sgbm_make_plan(ob, cus, bt, n, W, H);
    CHECK(p.sched == q.sched && p.family == q.family && p.cost_ty == q.cost_ty && p.acc == q.acc && p.nplanes == q.nplanes &&
              p.split == q.split && p.passes == q.passes && p.lpc == q.lpc && p.waves == q.waves &&
              p.strip_cols == q.strip_cols && p.nstrips == q.nstrips && p.blocks == q.blocks && p.lines_aux == q.lines_aux,
          "%s: sched %d/%d family %d/%d acc %d/%d planes %d/%d aux %d/%d", t, p.sched, q.sched, p.family, q.family, p.acc,
          q.acc, p.nplanes, q.nplanes, p.lines_aux, q.lines_aux);
    CHECK(p.pre == q.pre && p.cost == q.cost && p.agg == q.agg && p.raw == q.raw && p.keys == q.keys && p.dummy == q.dummy &&
              p.tri_bnd == q.tri_bnd && p.status == q.status && p.total_bytes() == q.total_bytes(),
          "%s: bytes %zu / %zu", t, p.total_bytes(), q.total_bytes());
    // the no-wrap recurrence follows the census bound, by the same rule
    if (p.no_wrap == q.no_wrap) CHECK(p.nw == q.nw, "%s", t);
}

static KernelOptions option_combo(int k)
{
    static const int waves[] = {0, 8, 15, 4, 7};
    KernelOptions o;
    o.path_sched = k % 3, k /= 3;
    o.bitslice = k & 1, k >>= 1;
    o.cost_res = k & 1, k >>= 1;
    o.tri = k & 1, k >>= 1;
    o.path16 = k & 1, k >>= 1;
    o.strip_waves = waves[k % 5], k /= 5;
    return o;
}
constexpr int kCombos = 3 * 16 * 5;

static void pinned()
{
    // configs/sgbm.yml at 1280x960, window (9, 7): the BT plan keeps its bit planes, the census plan has none
    const KernelOptions def;
    for (int mode = 0; mode < 2; mode++)
        for (int n : {1, 8}) {
            SgbmEff bt;
            eff(1280, 1, 128, 13, 0, 0, 0, 0, mode, 1, &bt);
            SgbmEff e = bt;
            e.cw = 9, e.ch = 7;
            const SgbmPlan a = sgbm_make_plan(def, 256, bt, n, 1280, 960), b = sgbm_make_plan(def, 256, e, n, 1280, 960);
            CHECK((a.bits() & kPlanBitslice) && a.cost2, "sgbm.yml BT mode %d x%d: bits %d", mode, n, a.bits());
            CHECK(!(b.bits() & (kPlanBitslice | kPlanResidual)) && !b.cost2 && b.family == kFamPacked16 && b.acc == kAccNib,
                  "sgbm.yml census mode %d x%d: bits %d", mode, n, b.bits());
            CHECK(b.nw, "sgbm.yml census mode %d x%d: 2 * 5 + 169 * 62 fits int16", mode, n);
        }
}

static void grid()
{
    static const int sizes[][2] = {{40, 9}, {135, 33}, {321, 97}, {640, 480}, {643, 481}, {1280, 960}};
    long i = 0;
    for (int n : {1, 2, 3, 8})
        for (const auto& wh : sizes)
            for (int D : {16, 32, 48, 64, 128, 256, 512})
                for (int bs = 1; bs <= 21; bs += 2)
                    for (int P2 : {5, 15, 40, 2592})
                        for (int mode = 0; mode < 3; mode++)  // 2: MODE_HH4
                            for (int uniq : {0, 10}) {
                                SgbmEff e;
                                const int P1 = P2 == 5 ? 2 : P2 == 15 ? 4 : P2 / 4;
                                if (!eff(wh[0], (int)(i % 3) - 1, D, bs, P1, P2, (i & 4) ? 63 : 0, uniq, mode == 1, 1, &e)) continue;
                                e.hh4 = mode == 2;
                                // eight of the option combinations per point, all of them over the grid
                                for (int k = 0; k < 8; k++, i++)
                                    check_census_plan(option_combo((int)((i * 37) % kCombos)),
                                                      (i % 3) == 0 ? 64 : (i % 3) == 1 ? 256 : 304, e, (int)(i % 8), n, wh[0],
                                                      wh[1]);
                            }
}

int main()
{
    pinned();
    grid();
    std::printf("%ld census plans (%ld beyond the int16 bound skipped), %ld violations\n", g_plans, g_skipped, g_fail);
    return g_fail || g_plans < 100000 ? 1 : 0;
}
