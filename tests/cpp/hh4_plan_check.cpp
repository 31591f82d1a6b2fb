// hh4_plan_check.cpp — host-only check of the SGBM launch plan for MODE_HH4
// (mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp): no MODE_HH4 launch runs a strip
// chain, a bit-sliced kernel or touches a spin-wait buffer, its planes are three
// side by side (+ the R->L plane of the split WTA form) and one per direction; and
// the plans of MODE_SGBM and MODE_HH at the same shapes are, field by field, what
// the header gave before the mode existed (kBefore, hh4_plan_before.inc: printed by
// this file built with -DHH4_PLAN_PRINT_BEFORE against the header of the commit
// before MODE_HH4).
// Plain g++, no library, no GPU.
#include <cstdio>
#include <cstring>

#include "../../mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp"
#include "sgbm_eff.hpp"  // eff(): resolve_sgbm's rules (memsets the struct: hh4 = 0)

using namespace mvsv;

struct Shape {
    const char* name;
    int W, H, n, minD, D, bs, P1, P2;
};
static const Shape kShapes[] = {
    // configs/sgbm.yml's values (P1 = P2 = 0 -> 2 / 5)
    {"sgbm.yml 640x480 x1", 640, 480, 1, 1, 128, 13, 0, 0},
    {"sgbm.yml 1280x960 x1", 1280, 960, 1, 1, 128, 13, 0, 0},
    {"sgbm.yml 1280x960 x8", 1280, 960, 8, 1, 128, 13, 0, 0},
    // liveDisparity: create(0, 64, 9, 648, 2592)
    {"live 1280x960 x1", 1280, 960, 1, 0, 64, 9, 648, 2592},
    {"live 1280x960 x8", 1280, 960, 8, 0, 64, 9, 648, 2592},
    // captureDisparity: create(0, 16, 5, 200, 800); D 16 on nibble planes; a D no packed kernel takes
    {"capture 640x480 x1", 640, 480, 1, 0, 16, 5, 200, 800},
    {"D16 nibble 640x480 x8", 640, 480, 8, 0, 16, 3, 0, 0},
    {"D48 640x480 x1", 640, 480, 1, 0, 48, 5, 8, 32},
    {"D48 1280x960 x8", 1280, 960, 8, 0, 48, 9, 648, 2592},
};
constexpr int kNShapes = sizeof kShapes / sizeof kShapes[0];
constexpr int kCus = 256;

// every field of a plan, in declaration order
constexpr int kFields = 31;
static void fields(const SgbmPlan& p, long long (&f)[kFields])
{
    const long long v[kFields] = {p.empty,      p.family,          p.sched,          p.cost2,      p.cost_ty,
                                  p.residual,   p.no_wrap,         p.nw,             p.acc,        p.nplanes,
                                  p.split,      p.passes,          p.lpc,            p.waves,      p.bs_groups,
                                  (long long)p.bs_aplane, (long long)p.bs_dplane, p.strip_cols, p.nstrips, p.blocks,
                                  p.lines_aux,  (long long)p.pre,  (long long)p.cost, (long long)p.cres, (long long)p.cres_min,
                                  (long long)p.agg, (long long)p.raw, (long long)p.keys, (long long)p.dummy,
                                  (long long)(p.tri_bnd + p.bs_bnd), (long long)p.status};
    std::memcpy(f, v, sizeof v);
}

#ifndef HH4_PLAN_PRINT_BEFORE
static long g_fail = 0, g_plans = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (g_fail++ < 40) {                                            \
                std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                                   \
                std::printf("\n");                                          \
            }                                                               \
        }                                                                   \
    } while (0)

// [shape][mode 0 / 1][path_sched 0 / 1 / 2]
static const long long kBefore[kNShapes][2][3][kFields] = {
#include "hh4_plan_before.inc"
};

static SgbmPlan plan_of(const Shape& s, int mode, int hh4, int path_sched, SgbmEff* e)
{
    KernelOptions o;
    o.path_sched = path_sched;
    eff(s.W, s.minD, s.D, s.bs, s.P1, s.P2, 0, 0, mode, 1, e);
    if (hh4) e->hh4 = 1;
    return sgbm_make_plan(o, kCus, *e, s.n, s.W, s.H);
}

#else
// -DHH4_PLAN_PRINT_BEFORE: nothing of MODE_HH4 is compiled, so the file builds against
// the header of the commit before it and prints hh4_plan_before.inc
int main()
{
    for (const Shape& s : kShapes) {
        std::printf("    {  // %s\n", s.name);
        for (int mode = 0; mode < 2; mode++) {
            std::printf("        {\n");
            for (int ps = 0; ps < 3; ps++) {
                KernelOptions o;
                o.path_sched = ps;
                SgbmEff e;
                eff(s.W, s.minD, s.D, s.bs, s.P1, s.P2, 0, 0, mode, 1, &e);
                long long f[kFields];
                fields(sgbm_make_plan(o, kCus, e, s.n, s.W, s.H), f);
                std::printf("            {");
                for (int i = 0; i < kFields; i++) std::printf("%lld%s", f[i], i + 1 < kFields ? ", " : "");
                std::printf("},\n");
            }
            std::printf("        },\n");
        }
        std::printf("    },\n");
    }
    return 0;
}
#endif

#ifndef HH4_PLAN_PRINT_BEFORE  // (to the end of the file)
static void old_modes_unchanged()
{
    for (int k = 0; k < kNShapes; k++)
        for (int mode = 0; mode < 2; mode++)
            for (int ps = 0; ps < 3; ps++) {
                SgbmEff e;
                long long f[kFields];
                fields(plan_of(kShapes[k], mode, 0, ps, &e), f);
                g_plans++;
                CHECK(e.hh4 == 0, "%s", kShapes[k].name);
                for (int i = 0; i < kFields; i++)
                    CHECK(f[i] == kBefore[k][mode][ps][i], "%s mode %d path_sched %d field %d: %lld, was %lld", kShapes[k].name,
                          mode, ps, i, f[i], kBefore[k][mode][ps][i]);
            }
}

// what every MODE_HH4 plan must satisfy
static void check_hh4(const KernelOptions& o, const SgbmEff& e, int n, int W, int H, const char* t)
{
    const SgbmPlan p = sgbm_make_plan(o, kCus, e, n, W, H);
    g_plans++;
    if (p.empty) return;
    CHECK(p.sched != 1, "%s: strips", t);
    CHECK(p.family != kFamBitslice, "%s: bit-sliced", t);
    CHECK(!(p.bits() & (kPlanBitslice | kPlanStrips)), "%s bits %d", t, p.bits());
    CHECK(p.status == 0 && p.tri_bnd == 0 && p.bs_bnd == 0, "%s: spin-wait buffers", t);
    CHECK(p.passes == 0 && p.blocks == 0 && p.nstrips == 0 && p.lines_aux == 0, "%s", t);
    CHECK(p.sched == 0 || p.sched == 2, "%s sched %d", t, p.sched);
    CHECK(p.graphable() == (p.sched == 2), "%s", t);
    const bool split = p.sched == 2 && o.final_split && e.P2 > 15 && e.D <= 32;
    CHECK(p.split == split, "%s", t);
    CHECK(p.nplanes == (p.sched == 2 ? 3 + (split ? 1 : 0) : 1), "%s planes %d", t, p.nplanes);
    const bool packed_d = e.D == 32 || e.D == 64 || e.D == 128 || e.D == 256;
    if (!(packed_d || e.D == 16) || !o.path16) CHECK(p.family == kFamGeneric && p.sched == 0, "%s family %d", t, p.family);
    if (p.family == kFamGeneric) CHECK(p.sched == 0 && p.acc != kAccNib, "%s", t);
    if (p.family == kFamPacked8) CHECK(e.D == 16 && p.sched == 2, "%s", t);
    if (p.acc == kAccNib) CHECK(p.sched == 2 && e.P2 <= 15, "%s", t);
    if (p.acc == kAccU8) CHECK(4 * e.P2 <= 255, "%s", t);  // four directions
    if (p.acc == kAccU16) CHECK(4 * e.P2 > 255 && (p.sched == 0 || e.P2 > 15), "%s", t);
    if (p.sched == 0) CHECK(p.acc == kAccU8 || p.acc == kAccU16, "%s", t);
    if (p.residual) CHECK(p.sched == 2 && p.cost2 && p.no_wrap && 3 * e.P2 <= 15 && e.D <= 128 && e.cn == 1, "%s", t);
    // path_sched: 2 = side by side wherever a packed kernel runs, 1 = one launch per direction
    if (o.path16 && packed_d && o.path_sched == 2) CHECK(p.sched == 2, "%s", t);
    if (o.path_sched == 1) CHECK(p.sched == 0, "%s", t);
    if (o.path_sched == 0 && o.path16 && packed_d && e.P2 <= 15) CHECK(p.sched == 2 && p.acc == kAccNib, "%s", t);
    const size_t vol = (size_t)n * H * e.W1 * e.D;
    CHECK(p.agg >= (size_t)p.nplanes * vol * p.acc / 8, "%s", t);
    CHECK(p.total_bytes() == p.pre + p.cost + p.cres + p.agg + p.raw + p.keys + p.dummy, "%s", t);
}

static void hh4_shapes()
{
    SgbmEff e;
    // sgbm.yml's regime: the packed nibble planes on the residual input, never the bit planes
    for (int k = 0; k < 3; k++) {
        const SgbmPlan p = plan_of(kShapes[k], 0, 1, 0, &e);
        CHECK(p.bits() == (kPlanSide | kPlanResidual) && p.family == kFamPacked16 && p.acc == kAccNib && p.nplanes == 3,
              "%s: bits %d acc %d planes %d", kShapes[k].name, p.bits(), p.acc, p.nplanes);
    }
    // liveDisparity: three u16 planes side by side within the plane-byte bound (one frame:
    // 0.45 GB, eight: 3.59 GB <= kHh4SidePlaneBytes), one launch per direction into one
    // plane beyond it (sixteen frames: 7.2 GB)
    SgbmPlan p = plan_of(kShapes[3], 0, 1, 0, &e);
    CHECK(p.bits() == kPlanSide && p.acc == kAccU16 && p.nplanes == 3 && !p.split, "live x1: bits %d", p.bits());
    p = plan_of(kShapes[4], 0, 1, 0, &e);
    CHECK(p.bits() == kPlanSide && p.acc == kAccU16 && p.nplanes == 3, "live x8: bits %d", p.bits());
    Shape live16 = kShapes[4];
    live16.n = 16;
    p = plan_of(live16, 0, 1, 0, &e);
    CHECK(p.bits() == 0 && p.sched == 0 && p.family == kFamPacked16 && p.acc == kAccU16 && p.nplanes == 1, "live x16: bits %d",
          p.bits());
    p = plan_of(live16, 0, 1, 2, &e);
    CHECK(p.bits() == kPlanSide && p.nplanes == 3, "live x16 forced side by side");
    p = plan_of(kShapes[3], 0, 1, 1, &e);
    CHECK(p.sched == 0 && p.nplanes == 1, "live x1 forced per direction");
    // D 16: eight lanes per line, side by side; P2 > 15 splits the WTA (R->L as a fourth plane)
    p = plan_of(kShapes[5], 0, 1, 0, &e);
    CHECK(p.bits() == kPlanSide && p.family == kFamPacked8 && p.acc == kAccU16 && p.split && p.nplanes == 4, "capture: planes %d",
          p.nplanes);
    p = plan_of(kShapes[6], 0, 1, 0, &e);
    CHECK(p.bits() == kPlanSide && p.family == kFamPacked8 && p.acc == kAccNib && !p.split && p.nplanes == 3, "D16 nibble");
    // D 48: the generic family, one launch per direction
    for (int k = 7; k < 9; k++)
        for (int ps = 0; ps < 3; ps++) {
            p = plan_of(kShapes[k], 0, 1, ps, &e);
            CHECK(p.bits() == 0 && p.family == kFamGeneric && p.nplanes == 1, "%s path_sched %d", kShapes[k].name, ps);
        }
    // u8 planes count four directions: 4 * 63 <= 255 < 5 * 63
    eff(640, 0, 64, 5, 8, 63, 0, 0, 0, 1, &e);
    CHECK(!acc_is_u8(e), "MODE_SGBM P2 63");
    e.hh4 = 1;
    CHECK(acc_is_u8(e) && sgbm_ndir(e) == 4, "MODE_HH4 P2 63");
    CHECK(sgbm_pass_dir(e, 0) == 0 && sgbm_pass_dir(e, 1) == 2 && sgbm_pass_dir(e, 2) == 5, "MODE_HH4 directions");
    e.hh4 = 0;
    CHECK(sgbm_ndir(e) == 5 && sgbm_pass_dir(e, 3) == 3, "MODE_SGBM directions");
    e.fullDP = 1;
    CHECK(sgbm_ndir(e) == 8 && sgbm_pass_dir(e, 6) == 6, "MODE_HH directions");
}

static void hh4_grid()
{
    static const int sizes[][2] = {{40, 9}, {135, 33}, {321, 97}, {640, 480}, {1280, 960}};
    char t[200];
    for (int n : {1, 2, 8})
        for (const auto& wh : sizes)
            for (int D : {16, 32, 48, 64, 128, 256, 512})
                for (int bs : {1, 5, 9, 13, 17})
                    for (int P2 : {5, 15, 40, 63, 64, 2592})
                        for (int uniq : {0, 10})
                            for (int cn : {1, 3})
                                for (int k = 0; k < 3 * 16; k++) {
                                    KernelOptions o;
                                    int q = k;
                                    o.path_sched = q % 3, q /= 3;
                                    o.bitslice = q & 1, q >>= 1;
                                    o.cost_res = q & 1, q >>= 1;
                                    o.tri = q & 1, q >>= 1;
                                    o.path16 = q & 1;
                                    SgbmEff e;
                                    if (!eff(wh[0], 1, D, bs, P2 == 5 ? 2 : P2 / 4, P2, 0, uniq, 0, cn, &e)) continue;
                                    e.hh4 = 1;
                                    std::snprintf(t, sizeof t, "n=%d %dx%d D=%d bs=%d P2=%d uniq=%d cn=%d opt %d", n, wh[0], wh[1], D,
                                                  bs, P2, uniq, cn, k);
                                    check_hh4(o, e, n, wh[0], wh[1], t);
                                }
}

int main()
{
    old_modes_unchanged();
    hh4_shapes();
    hh4_grid();
    std::printf("%ld plans, %ld violations\n", g_plans, g_fail);
    return g_fail ? 1 : 0;
}
#endif
