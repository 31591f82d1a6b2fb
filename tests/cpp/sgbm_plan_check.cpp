// sgbm_plan_check.cpp — host-only check of the SGBM launch plan
// (mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp): the shapes this repository's
// comments and tests name, pinned; and invariants of every plan over a grid of
// launch shapes, parameters, options and CU counts.  Plain g++, no library, no GPU.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../mvstereovision3_amd/csrc/mvsv_sgbm_plan.hpp"
#include "sgbm_eff.hpp"  // eff(): resolve_sgbm's rules

using namespace mvsv;

static long g_fail = 0, g_plans = 0;
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
    static char b[200];
    std::snprintf(b, sizeof b, "n=%d %dx%d D=%d bs=%d P1=%d P2=%d mode=%d uniq=%d cn=%d minD=%d", n, W, H, e.D,
                  2 * e.SW2 + 1, e.P1, e.P2, e.fullDP, e.uniq, e.cn, e.minD);
    return b;
}

static size_t padq(size_t w) { return (w + 3) & ~(size_t)3; }

// the invariants of one plan
static void check_plan(const KernelOptions& o, int cus, const SgbmEff& e, int n, int W, int H)
{
    const SgbmPlan p = sgbm_make_plan(o, cus, e, n, W, H);
    const char* t = tag(e, n, W, H);
    g_plans++;
    const bool nonempty = e.minX1 < e.maxX1;
    CHECK(p.graphable() == (nonempty && e.D <= 512 && p.sched == 2 && !p.empty), "%s", t);
    CHECK(p.empty == !(nonempty && e.D <= 512), "%s", t);
    CHECK(p.total_bytes() == p.pre + p.cost + p.cres + p.agg + p.raw + p.keys + p.dummy + p.tri_bnd + p.bs_bnd + p.status,
          "%s", t);
    if (p.empty) {
        CHECK(p.bits() == 0 && p.total_bytes() == 0, "%s", t);
        return;
    }
    const bool bits = p.family == kFamBitslice;
    const size_t frame = (size_t)W * H, pix = (size_t)n * H * e.W1, vol = pix * e.D, pixq = (size_t)n * H * padq(e.W1);
    CHECK(!(bits || p.residual) || (e.cn == 1 && p.cost2), "%s: planes without the register-ring kernel", t);
    CHECK(!(bits && p.residual), "%s", t);
    CHECK(!p.cost2 || (e.cn == 1 && e.SH2 <= 7 && o.cost2), "%s", t);
    CHECK(((p.bits() & kPlanBitslice) != 0) == bits && ((p.bits() & kPlanResidual) != 0) == p.residual &&
              ((p.bits() & kPlanSide) != 0) == (p.sched == 2) && ((p.bits() & kPlanStrips) != 0) == (p.sched == 1),
          "%s bits %d", t, p.bits());
    if (p.acc == kAccNib) {
        // a delta <= P2 per plane side by side; sums of three directions <= 3 * P2 on strips
        CHECK(p.sched == 2 ? e.P2 <= 15 : (p.sched == 1 && 3 * e.P2 <= 15), "%s sched %d", t, p.sched);
    }
    if (p.acc == kAccU8) CHECK((e.fullDP ? 8 : 5) * e.P2 <= 255, "%s", t);
    if (p.sched == 1) CHECK((unsigned long long)H * e.W1 * e.D < (1ull << 31), "%s: int32 offsets", t);
    const long bsz = 2L * e.SW2 + 1;
    const bool no_wrap = 2L * e.P2 + bsz * bsz * e.cn * (2L * e.ftzero + 63) <= 32767;
    CHECK(p.no_wrap == no_wrap, "%s", t);
    CHECK(!p.nw || no_wrap, "%s", t);
    CHECK(!p.residual || (p.nw && 3 * e.P2 <= 15 && e.D <= 128), "%s", t);
    CHECK(!bits || (e.D == 128 && e.P1 == 2 && e.P2 == 5 && e.uniq == 0 && no_wrap && p.sched != 0), "%s", t);
    switch (p.family) {
    case kFamPacked8: CHECK(e.D == 16 && p.sched == 2, "%s", t); break;
    case kFamPacked16: CHECK(e.D == 32 || e.D == 64 || e.D == 128 || e.D == 256, "%s", t); break;
    case kFamGeneric: CHECK(p.sched == 0 && p.nplanes == 1 && p.acc != kAccNib, "%s", t); break;
    default: break;
    }
    // tile height: forced, 16 for short images, else one the cost kernel is checked for
    bool ty_ok = p.cost_ty == (o.cost_ty > 0 ? o.cost_ty : 16);
    if (o.cost_ty <= 0 && H >= 256)
        for (int ty : kCostTileHeights) ty_ok = ty_ok || p.cost_ty == ty;
    CHECK(ty_ok, "%s TY %d", t, p.cost_ty);
    // buffers
    CHECK(p.pre >= (size_t)n * 2 * e.cn * frame * 8, "%s", t);
    CHECK(p.cost >= pixq * e.D * 2, "%s", t);
    CHECK(p.raw >= (size_t)n * frame * 2, "%s", t);
    CHECK(p.family == kFamGeneric || p.keys >= (size_t)n * frame * 4, "%s", t);
    CHECK(p.sched != 1 || p.status >= 16, "%s", t);
    CHECK(p.lines_aux >= 0 && p.lines_aux <= 2, "%s", t);
    const int npass = e.fullDP ? 2 : 1;
    if (bits) {
        CHECK(p.cres_min % 256 == 0 && p.cres_min >= pixq * 64 && p.cres >= p.cres_min + pix * 2, "%s", t);
        CHECK(p.bs_dplane >= pixq * 12, "%s", t);
        if (p.sched == 2) {
            CHECK(p.nplanes == 3 * npass + 2 && p.agg >= ((size_t)p.nplanes * p.bs_dplane + 256) * 4, "%s", t);
        } else {
            CHECK(p.passes == npass && p.bs_groups >= 1 && p.bs_groups <= 5, "%s", t);
            CHECK(p.strip_cols == 32 * p.bs_groups && (long long)p.nstrips * p.strip_cols >= e.W1 + H - 1 &&
                      (long long)(p.nstrips - 1) * p.strip_cols < e.W1 + H - 1,
                  "%s", t);
            CHECK(p.blocks == (long long)npass * n * p.nstrips, "%s", t);
            CHECK(p.bs_aplane >= pix * 16 && p.agg >= ((size_t)npass * p.bs_aplane + 2 * p.bs_dplane + 512) * 4, "%s", t);
            CHECK(p.bs_bnd >= (size_t)p.blocks * H * 36 * 8, "%s", t);
        }
        return;
    }
    if (p.residual) CHECK(p.cres_min % 256 == 0 && p.cres_min >= vol / 2 && p.cres >= p.cres_min + pix * 2, "%s", t);
    else CHECK(p.cres == 0, "%s", t);
    const bool split = p.sched == 2 && o.final_split && e.P2 > 15 && e.D <= 32;
    CHECK(p.split == split, "%s", t);
    const int planes = p.sched == 2 ? (e.fullDP ? 7 : 4) + (split ? 1 : 0) : p.sched == 1 ? npass + 1 : 1;
    CHECK(p.nplanes == planes, "%s planes %d", t, p.nplanes);
    CHECK(p.agg >= (size_t)planes * vol * p.acc / 8, "%s", t);
    if (p.family == kFamGeneric) return;
    const int np = p.family == kFamPacked8 ? 1 : e.D / 32;
    CHECK(p.dummy >= (size_t)512 * 16 * 2 * np, "%s", t);
    if (p.sched != 1) return;
    CHECK(p.passes == npass && (p.lpc == 16 || (p.lpc == 32 && e.D == 256 && p.waves == 8)), "%s", t);
    if (p.lpc == 16) CHECK(e.D == 256 ? (p.waves == 7 || p.waves == 4) : (p.waves == 15 || p.waves == 8), "%s", t);
    CHECK(p.strip_cols == 64 / p.lpc * p.waves && (long long)p.nstrips * p.strip_cols >= e.W1 + H - 1 &&
              (long long)(p.nstrips - 1) * p.strip_cols < e.W1 + H - 1,
          "%s", t);
    CHECK(p.blocks == (long long)npass * n * p.nstrips, "%s", t);
    // granules: [strip step][3 items, 4 rows][lpc lanes][(2 * pairs + 1 min) / 3 u64]
    const int pairs = e.D / (2 * p.lpc);
    CHECK(p.tri_bnd >= (size_t)p.blocks * H * 4 * p.lpc * ((2 * pairs + 3) / 3) * 8, "%s", t);
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

struct Pin {
    SgbmEff e;
    int W, H;
};
static Pin pin(int W, int H, int minD, int D, int bs, int P1, int P2, int mode, int cn = 1)
{
    Pin p;
    p.W = W, p.H = H;
    eff(W, minD, D, bs, P1, P2, 0, 0, mode, cn, &p.e);
    return p;
}

static void pinned()
{
    const KernelOptions def;
    KernelOptions o;
    // configs/sgbm.yml (P1 = P2 = 0 -> 2 / 5), MODE_HH and MODE_SGBM
    const Pin hh = pin(1280, 960, 1, 128, 13, 0, 0, 1), hs = pin(640, 480, 1, 128, 13, 0, 0, 1),
              sg = pin(640, 480, 1, 128, 13, 0, 0, 0);
    SgbmPlan p = sgbm_make_plan(def, 256, hh.e, 8, 1280, 960);
    CHECK(p.bits() == (kPlanBitslice | kPlanStrips) && p.bs_groups == 3 && p.blocks == 352 && p.cost2, "hh x8: bits %d groups %d blocks %lld",
          p.bits(), p.bs_groups, p.blocks);
    o = def, o.bitslice = 0;
    p = sgbm_make_plan(o, 256, hh.e, 8, 1280, 960);
    CHECK(p.bits() == (kPlanStrips | kPlanResidual) && p.acc == kAccNib && p.nplanes == 3, "hh x8 packed: bits %d", p.bits());
    CHECK(sgbm_make_plan(def, 256, hs.e, 1, 640, 480).bits() == (kPlanBitslice | kPlanSide), "hh 640x480 x1");
    CHECK(sgbm_make_plan(def, 256, sg.e, 8, 640, 480).bits() == (kPlanBitslice | kPlanSide), "mode 0 640x480 x8");
    // config 5: create(0, 256, 9, 648, 2592)
    const Pin c5 = pin(1280, 960, 0, 256, 9, 648, 2592, 0);
    p = sgbm_make_plan(def, 256, c5.e, 1, 1280, 960);
    // (DESIGN.md and the lines_aux comment say 125 blocks; ceil((1024 + 959) / 16) is 124, and two frames have 248)
    CHECK(p.sched == 1 && p.family == kFamPacked16 && p.lpc == 32 && p.waves == 8 && p.blocks == 124 && p.lines_aux == 1,
          "c5 x1: sched %d lpc %d waves %d blocks %lld aux %d", p.sched, p.lpc, p.waves, p.blocks, p.lines_aux);
    p = sgbm_make_plan(def, 256, c5.e, 2, 1280, 960);
    CHECK(p.sched == 1 && p.lpc == 32 && p.blocks == 248 && p.lines_aux != 1, "c5 x2: blocks %lld aux %d", p.blocks, p.lines_aux);
    p = sgbm_make_plan(def, 256, c5.e, 8, 1280, 960);
    CHECK(p.sched == 1 && p.family == kFamPacked16 && p.acc == kAccU16 && p.nplanes == 2 && p.lpc == 16 && p.waves == 7 && p.nw,
          "c5 x8: sched %d acc %d planes %d", p.sched, p.acc, p.nplanes);
    // D = 128 MODE_HH on the packed strips, one 1280x960 frame (strips forced: by
    // launch size one frame runs side by side)
    o = def, o.bitslice = 0, o.path_sched = 1;
    p = sgbm_make_plan(o, 256, hh.e, 1, 1280, 960);
    CHECK(p.sched == 1 && p.lpc == 16 && p.waves == 8 && p.blocks == 132 && p.lines_aux == 1, "hh x1 packed: waves %d blocks %lld",
          p.waves, p.blocks);
    // one 640x480 frame, wide strips forced
    o.strip_waves = 15;
    p = sgbm_make_plan(o, 256, hs.e, 1, 640, 480);
    CHECK(p.sched == 1 && p.waves == 15 && p.blocks == 34, "hh 640x480 wide: waves %d blocks %lld", p.waves, p.blocks);
    // captureDisparity: create(0, 16, 5, 200, 800)
    const Pin cap = pin(640, 480, 0, 16, 5, 200, 800, 0);
    for (int n : {1, 8}) {
        p = sgbm_make_plan(def, 256, cap.e, n, 640, 480);
        CHECK(p.bits() == kPlanSide && p.family == kFamPacked8 && p.acc == kAccU16 && p.nplanes == 5 && p.split, "capture x%d", n);
    }
    // liveDisparity: create(0, 64, 9, 648, 2592); the 1.4 GB rule
    const Pin live = pin(1280, 960, 0, 64, 9, 648, 2592, 0);
    CHECK(sgbm_make_plan(def, 256, live.e, 1, 1280, 960).bits() == kPlanSide, "live x1");
    CHECK(sgbm_make_plan(def, 256, live.e, 4, 1280, 960).bits() == kPlanStrips, "live x4");
    // a colour launch of the sgbm.yml regime
    const Pin col = pin(1280, 960, 1, 128, 13, 0, 0, 1, 3);
    p = sgbm_make_plan(def, 256, col.e, 8, 1280, 960);
    CHECK(!p.residual && p.family == kFamPacked16 && !p.cost2 && p.sched == 1, "colour x8: bits %d", p.bits());
    // every option combination on the pinned shapes
    for (const Pin* q : {&hh, &hs, &sg, &c5, &cap, &live, &col})
        for (int k = 0; k < kCombos; k++)
            for (int cus : {64, 256, 304})
                for (int n : {1, 2, 8}) check_plan(option_combo(k), cus, q->e, n, q->W, q->H);
}

static void layouts()
{
    // the register-ring cost kernel's layout and fit do not depend on the tile height
    for (int D = 16; D <= 512; D += 16)
        for (int bs = 1; bs <= 21; bs += 2)
            for (int fixed = 0; fixed < 2; fixed++) {
                SgbmEff e;
                eff(4096, 0, D, bs, 0, 0, 0, 0, 0, 1, &e);
                const Cost2Launch a = cost2_launch(e, fixed, kCostTileHeights[0]);
                for (int ty : kCostTileHeights) {
                    const Cost2Launch b = cost2_launch(e, fixed, ty);
                    CHECK(a.fits == b.fits && a.stg == b.stg && a.ppc == b.ppc && a.lds == b.lds, "D %d bs %d TY %d", D, bs, ty);
                    if (!a.fits) continue;
                    Cost2Layout x = cost2_layout(D, e.SW2, kCostTileHeights[0]), y = cost2_layout(D, e.SW2, ty);
                    CHECK(y.TY == ty, "D %d bs %d TY %d", D, bs, ty);
                    x.TY = y.TY = 0;
                    CHECK(x.PP == y.PP && x.CL == y.CL && x.TX == y.TX && x.NX == y.NX && x.PS == y.PS && x.nQmax == y.nQmax &&
                              x.qhalf == y.qhalf && x.off_l4 == y.off_l4 && x.off_l2 == y.off_l2 && x.off_q4 == y.off_q4 &&
                              x.off_q2 == y.off_q2 && x.off_pix == y.off_pix && x.bytes == y.bytes &&
                              x.lstride4 == y.lstride4 && x.lstride2 == y.lstride2 && x.qstride4 == y.qstride4 &&
                              x.qstride2 == y.qstride2 && x.pstride == y.pstride,
                          "D %d bs %d TY %d", D, bs, ty);
                }
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
                        for (int mode = 0; mode < 2; mode++)
                            for (int uniq : {0, 10})
                                for (int cn : {1, 3}) {
                                    SgbmEff e;
                                    const int P1 = P2 == 5 ? 2 : P2 == 15 ? 4 : P2 / 4;
                                    if (!eff(wh[0], (int)(i % 3) - 1, D, bs, P1, P2, (i & 4) ? 63 : 0, uniq, mode, cn, &e)) continue;
                                    // eight of the option combinations per point, all of them over the grid
                                    for (int k = 0; k < 8; k++, i++)
                                        check_plan(option_combo((int)((i * 37) % kCombos)), (i % 3) == 0 ? 64 : (i % 3) == 1 ? 256 : 304,
                                                   e, n, wh[0], wh[1]);
                                }
}

int main()
{
    pinned();
    layouts();
    grid();
    std::printf("%ld plans, %ld violations\n", g_plans, g_fail);
    return g_fail ? 1 : 0;
}
