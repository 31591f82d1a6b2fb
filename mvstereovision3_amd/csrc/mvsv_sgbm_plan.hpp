// mvsv_sgbm_plan.hpp — the launch plan of one sgbm_device call: which kernels
// run, how their launches are cut and how large every cached buffer is.
// sgbm_make_plan is a pure function of the kernel options, the CU count, the
// effective parameters and the launch shape; sgbm_device, mvsv_sgbm_plan and
// mvsv_sgbm_workspace_bytes all read its result, and no launcher decides again.
// Host-pure (no HIP): tests/cpp/sgbm_plan_check.cpp compiles it with plain g++.
// The launch-shape constants the kernels' templates need (strip waves, columns
// per strip, granules per item) are constexpr functions here, and the templates
// call them.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "mvsv_bitslice.hpp"
#include "mvsv_cost_layout.hpp"

namespace mvsv {

// the MVSV_PLAN_* bits of include/mvsv.h (mvsv_internal.hpp asserts the equality)
constexpr int kPlanBitslice = 1, kPlanSide = 2, kPlanStrips = 4, kPlanResidual = 8;

// Effective StereoSGBM parameters after OpenCV's defaulting rules
// ([OpenCV] computeDisparitySGBM prologue).
struct SgbmEff {
    int minD, maxD, D;
    int SW2, SH2;
    int ftzero;
    int uniq, disp12;
    int P1, P2;
    int minX1, maxX1, W1;
    int invalid;  // (minD - 1) * 16
    int fullDP;   // MODE_HH
    int variant;
    int speckle_window, speckle_diff;  // speckle_diff = 16 * speckleRange
    // colour channels of the pair: 1 (grey; resolve_sgbm) or 3 (interleaved BGR,
    // set by the colour entry points).  A pixel cost is <= cn * (2*ftzero + 63).
    int cn;
    // MODE_HH4: the four axis directions L->R, R->L, down, up on the clean cost
    // volume (no 3.4 cost-row quirk).  0 for MODE_SGBM / MODE_HH; fullDP stays 0
    // (the WTA is fused with the R->L pass, so MODE_SGBM's tie rule applies).
    int hh4;
    // census matching cost (mvsv_sgbm_census): the cw x ch window of the census
    // transform, both odd, 3 <= cw * ch <= 65.  0, 0: the Birchfield-Tomasi cost.
    // A pixel cost is then the Hamming distance of two (cw * ch - 1)-bit descriptors.
    int cw, ch;
};

// the pair is matched on the census cost
MVSV_HD inline bool sgbm_census(const SgbmEff& e) { return e.cw != 0 || e.ch != 0; }
// a grey pair on the Birchfield-Tomasi cost: what the register-ring cost kernel,
// the residual plane and the bit-sliced pipeline are written for
MVSV_HD inline bool sgbm_bt_grey(const SgbmEff& e) { return e.cn == 1 && !sgbm_census(e); }
// the largest pixel cost: every descriptor bit differs, or every channel's BT
// cost is at its ceiling
MVSV_HD inline int sgbm_max_pixel_cost(const SgbmEff& e)
{
    return sgbm_census(e) ? e.cw * e.ch - 1 : e.cn * (2 * e.ftzero + 63);
}

// The path directions of a mode, counted with R->L (which the final kernels
// run): 5 (MODE_SGBM), 8 (MODE_HH), 4 (MODE_HH4).  The direction passes run
// the other sgbm_ndir - 1; sgbm_pass_dir names the k-th of them as a row of
// kPathDirs (mvsv_sgbm_lines.hpp): {(1,0) (1,1) (0,1) (-1,1) (1,-1) (0,-1) (-1,-1)
// (-1,0)} -- the first four are MODE_SGBM's, the first seven MODE_HH's, and
// MODE_HH4 takes L->R, down and up.
MVSV_HD inline int sgbm_ndir(const SgbmEff& e) { return e.hh4 ? 4 : e.fullDP ? 8 : 5; }
MVSV_HD inline int sgbm_pass_dir(const SgbmEff& e, int k) { return !e.hh4 ? k : k == 0 ? 0 : k == 1 ? 2 : 5; }
constexpr int kPathDirRL = 7;  // R->L as a chain set of its own (the split WTA form)

// Default number of polls a strip-boundary wait of the sheared-strip kernel
// makes before it gives up (each poll = one s_sleep + one L2 load of the
// producer's granule, ~1 us): ~1 s, far beyond any producer delay of a
// healthy launch; the wait only exists to turn a lost hand-off into an error
// instead of a hang.  mvsv_set_option(MVSV_OPT_STRIP_SPIN_LIMIT) overrides it.
constexpr unsigned kStripSpinLimitDefault = 1u << 20;

// The launch-shape options of a context (MVSV_* environment at creation,
// mvsv_set_option): which kernels run and how their launches are cut.  A frame
// stream's own lane contexts take the caller context's as a whole.
struct KernelOptions {
    // strip blocks draw their strip as a ticket (status[2]) unless strip_tickets
    // is 0 (blockIdx order, MVSV_STRIP_ORDER=blockidx)
    int strip_tickets = 1;
    unsigned spin_limit = kStripSpinLimitDefault;
    int path16 = 1;  // 16-lanes-per-scanline path kernels where D allows
    int cost2 = 1;   // register-ring cost kernel where blockSize <= 15
    int cost_fixed_pp = 1;  // fixed-pair-count cost kernels for D = 128 / 256 (MVSV_KERNELS=cost-generic: off)
    int cost_ty = 0;  // cost-volume tile height (0 = by image height); MVSV_COST_TY for A/B runs
    int tri = 1;     // sheared-strip kernels: three directions per sweep
    int path_sched = 0;   // 16-lane path schedule: 0 = by launch size, 1 = strips, 2 = directions side by side
    int tri32 = 1;        // D = 256 narrow strips on 32 lanes per column (MVSV_TRI32)
    int final_split = 1;  // side by side on byte / u16 planes: R->L as a chain set + per-pixel WTA (MVSV_FINAL_SPLIT)
    int strip_waves = 0;  // compute waves per strip (0 = by launch size; 4 or the wide count forces)
    int cost_res = 1;     // direction passes read the cost residual plane where exact (MVSV_OPT_COST_RESIDUAL)
    int lines_aux = -1;  // L->R line kernel beside the strip kernel: -1 = small launches only, 0 / 1 / 2 force
    int bitslice = 1;    // bit-sliced MODE_HH paths where they apply (MVSV_OPT_BITSLICE, env MVSV_BITSLICE)
    int bs_groups = 0;   // column groups (3 direction waves each) per bit-sliced strip: 1-5 (MVSV_BS_GROUPS), 0 = by mode
    int cost_xcd = 1;    // cost kernel: whole row bands per XCD (MVSV_COST_XCD=0: blockIdx order, A/B)
    int bs_fuse = 1;     // bit-sliced batches: R->L lines fused with the WTA (MVSV_BS_FUSE=0: separate, A/B)
    int bs_serial = 0;   // 1: bit-sliced line kernel after the strips on the context stream (MVSV_BS_SERIAL, A/B)
    int bm2 = 1;     // StereoBM: disparities-on-lanes match kernel where blockSize <= 21, D <= 128
    int bm_ty = 0;   // its tile height (0 = chosen per launch); MVSV_BM_TY for A/B runs
    // diagnostics of the strip launches (read once, at context creation)
    int tri_stats = 0;      // MVSV_TRI_STATS: per-strip summary of the packed strips on stderr
    std::string tri_trace;  // MVSV_TRI_TRACE=path: also every step's publish / consume time, to that file
    int bs_stats = 0;       // MVSV_BS_STATS: per-strip spans and hand-off spin time of the bit-sliced strips
    long bs_ldspad = -1;    // MVSV_BS_LDSPAD: LDS bytes of a bit-sliced strip block (< 0: kBsStripLds; A/B)
};

// ---------------------------------------------------------------------------
// Launch-shape constants shared by the kernels' templates and the plan
// ---------------------------------------------------------------------------
// Packed strips (sgbm_tri_kernel): compute waves per strip for np disparity
// pairs per lane at lpc lanes per U-column (D = 2 * np * lpc).  Wide strips
// (15 waves, 7 for D = 256 on 16 lanes) are the throughput shape, narrow ones
// (8 / 4) the latency shape for one or two frames.
constexpr int tri_wide_waves(int np, int lpc) { return lpc == 8 ? 7 : (np >= 8 ? 7 : 15); }
constexpr int tri_narrow_waves(int np, int lpc) { return lpc == 8 ? 4 : lpc == 32 ? 8 : (np >= 8 ? 4 : 8); }
// U-columns per strip: 64 / lpc columns per compute wave
constexpr int tri_strip_cols(int waves, int lpc) { return (64 / lpc) * waves; }
// u64 boundary granules per item: 2 * np int16 costs + the column minimum,
// three int16 per granule
constexpr int tri_granules(int np) { return (2 * np + 3) / 3; }
// Bit-sliced strips (bsgm_strip_kernel): 32 U-columns per column group, and
// the boundary words per strip step ((dir b, column 0), (dir c, column 0),
// (dir c, column 1), each 2 lanes x 6 words; one u64 granule = tag | word)
constexpr int bs_strip_cols(int groups) { return 32 * groups; }
constexpr int kBsGran = 36;

constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------
// Predicates: one definition each
// ---------------------------------------------------------------------------
// Every cost C = P2 + (box sum of blockSize^2 pixel costs, each <= sgbm_max_pixel_cost),
// every L <= C and delta = minLp + P2: when that bound stays <= 32767 nothing
// wraps in int16 and the path kernels may use the NW recurrence (sgm_pair).
inline bool sgbm_no_wrap(const SgbmEff& e)
{
    const long bs = 2L * e.SW2 + 1;
    return (long)e.P2 + bs * bs * sgbm_max_pixel_cost(e) + e.P2 <= 32767;
}

// The same bound for the kernels (device code): a cost may pass 32767.  OpenCV
// keeps such a cost as a wrapped -- negative -- int16: its path costs are
// negative with it, S saturates at -32768 on that side too, and the disparity
// wins the WTA.  The final kernels then read C as signed and carry a signed S
// (DESIGN.md 4b-wrap); where this is false the unsigned and the signed reading
// of a cost are the same number and the kernels keep their unsigned forms.
MVSV_HD inline bool sgbm_signed_costs(const SgbmEff& e)
{
    const long bs = 2L * e.SW2 + 1;
    return (long)e.P2 + bs * bs * sgbm_max_pixel_cost(e) + e.P2 > 32767;
}

// u8 accumulator when the summed path deltas (each <= P2) fit a byte
MVSV_HD inline bool acc_is_u8(const SgbmEff& e) { return sgbm_ndir(e) * e.P2 <= 255; }
// 4-bit accumulator planes: the sheared-strip schedule writes one plane per
// group of at most three directions (3 strip directions, or the L->R line),
// so each plane holds sums <= 3 * P2; with P2 <= 5 (OpenCV's default P2 = 5,
// which configs/sgbm.yml gets because it leaves P1/P2 at 0) they fit a nibble.
MVSV_HD inline bool acc_is_nib(const SgbmEff& e) { return 3 * e.P2 <= 15; }

// The register-ring cost kernel's launch for (D, window): whether its tile
// fits (blockSize <= 15, square window, <= 2 staged items per thread, LDS
// image <= 160 KiB), staged items per thread, the compile-time pair count
// (numDisparities 128 / 256: unrolled pixel-cost loop, immediate LDS offsets)
// and the LDS bytes.  None of it depends on the tile height.
struct Cost2Launch {
    bool fits;
    int stg, ppc;
    size_t lds;
    Cost2Layout l;
};
inline Cost2Launch cost2_launch(const SgbmEff& e, int fixed_pp, int TY)
{
    Cost2Launch c{};
    if (e.SH2 > 7 || e.SW2 != e.SH2 || e.D < 2 || e.D / 2 > kCost2Threads) return c;
    c.l = cost2_layout(e.D, e.SW2, TY);
    const int items = 2 * c.l.NX + e.D - 1;
    c.stg = items > kCost2Threads ? 2 : 1;
    c.ppc = !fixed_pp ? 0 : c.l.PP == 64 ? 64 : (c.l.PP == 128 ? 128 : 0);
    c.lds = cost2_total_bytes(c.l, 2 * e.SH2 + 1, c.stg, c.ppc);
    c.fits = c.l.CL >= 1 && items <= kCost2Threads * 2 && c.lds <= 160 * 1024;
    return c;
}
// the register-ring cost kernel runs (grey pairs on the BT cost: colour pairs
// always take the LDS-ring kernel, which sums the channels, and so do census
// launches, whose pixel phase only that kernel has); it alone writes the
// residual plane and the bit-sliced C' planes
inline bool cost2_runs(const KernelOptions& o, const SgbmEff& e)
{
    return sgbm_bt_grey(e) && o.cost2 && cost2_launch(e, o.cost_fixed_pp, kCostTileHeights[0]).fits;
}

// Bit-sliced path aggregation (mvsv_bsgm.hip): the parameters admit it
// (configs/sgbm.yml's effective penalties, numDisparities 128, no uniqueness
// test, no int16 wrap) and int32 word offsets cover the C' planes
inline bool bsgm_eligible(const KernelOptions& o, const SgbmEff& e, int n, int H)
{
    return sgbm_bt_grey(e) && !e.hh4 && o.bitslice && e.D == 128 && e.P1 == 2 && e.P2 == 5 && e.uniq == 0 && sgbm_no_wrap(e) &&
           e.W1 > 0 && (size_t)n * H * bs::padq(e.W1) * 16 < ((size_t)1 << 31);
}

// The split side-by-side form (sgbm_wta_planes_kernel): byte / u16 planes,
// D <= 32.  Measured (MI355X r06 sp2, split vs fused R->L + WTA): D 16 640x480
// x 1 / 2 / 8 frames 0.278 -> 0.196, 0.297 -> 0.220, 0.515 -> 0.477 ms; D 32
// 1280x960 0.522 -> 0.491; D 64 x 1 / 2 0.746 -> 0.802, 1.125 -> 1.282 and D 128
// 1.083 -> 1.370 (the fifth chain set lengthens the direction pass more than
// the chain-free WTA saves); MODE_HH D 64 1.01 either way
inline bool wta_split(const KernelOptions& o, const SgbmEff& e) { return o.final_split && e.P2 > 15 && e.D <= 32; }

// The direction passes read the residual plane (CostIn, mvsv_sgbm_common.hpp) when it is
// exact and smaller: no-wrap regime, residuals <= 3 * P2 in a nibble, a
// 16-lane path schedule (1 = strips + lines, 2 = side by side) and D <= 128
// (one cost kernel wave segment holds a pixel's D costs).  Written by the
// register-ring cost kernel only.
inline bool use_residual(const KernelOptions& o, const SgbmEff& e, int sched)
{
    return sgbm_bt_grey(e) && o.cost_res && (sched == 1 || sched == 2) && sgbm_no_wrap(e) && 3 * e.P2 <= 15 &&
           (e.D == 32 || e.D == 64 || e.D == 128);
}

// sheared-strip schedule: enabled, and int32 element offsets cover a frame
inline bool use_strips(const KernelOptions& o, const SgbmEff& e, int H)
{
    return o.tri && (size_t)H * e.W1 * e.D < ((size_t)1 << 31);
}

// Path schedule of the 16-lane kernels (D = 32 / 64 / 128 / 256):
// 2 = all line directions side by side (sgbm_pathdirs16_kernel, one 4-bit plane
// per direction, P2 <= 15) -- the latency shape for launches too small to fill
// the chip with strips (one camera frame); 1 = sheared strips (batches).
// path_sched: 0 = by launch size, 1 / 2 force (tests, A/B).
//
// MODE_HH4 has no diagonal direction, so every launch is a set of independent
// chains and schedule 1 (strips) never runs: side by side (2) on nibble planes
// (P2 <= 15), on byte / u16 planes while the three planes stay within
// kHh4SidePlaneBytes, else one launch per direction into one plane (0).
// path_sched 1 forces that last shape (there are no strips to force).
//
// The plane-byte bound: MODE_SGBM / MODE_HH leave side by side at 1.4 GB of
// planes because the strip chain overtakes it there.  MODE_HH4's alternative is
// one launch per direction, which reads and writes its single plane three times
// and never overtook the three planes: measured (MI355X, tools/hh4_bench.py,
// create(0, 64, 9, 648, 2592) at 1280x960, forced schedule 1 against 2, ms):
// x 1 0.76 / 0.55, x 2 0.97 / 0.83, x 3 1.23 / 1.20, x 4 1.82 / 1.64, x 8 (3.59 GB
// of planes) 3.33 / 3.16.  No crossover up to the largest launch measured, so the
// bound sits there: beyond it nothing is measured and the per-direction schedule
// keeps the planes at a third of the bytes.
constexpr double kHh4SidePlaneBytes = 3.6e9;
inline int path_schedule_hh4(const KernelOptions& o, const SgbmEff& e, int H, int n)
{
    if (e.D == 16 && o.path16 && o.path_sched != 1) return 2;
    if (!o.path16 || !(e.D == 32 || e.D == 64 || e.D == 128 || e.D == 256)) return 0;
    if (o.path_sched == 2) return 2;
    if (o.path_sched == 1) return 0;
    if (e.P2 <= 15) return 2;
    const double bytes = (double)n * e.W1 * H * e.D * (sgbm_ndir(e) - 1) * (acc_is_u8(e) ? 1 : 2);
    return bytes <= kHh4SidePlaneBytes ? 2 : 0;
}

inline int path_schedule(const KernelOptions& o, int cus, const SgbmEff& e, int H, int n)
{
    if (e.hh4) return path_schedule_hh4(o, e, H, n);
    // D = 16 (captureDisparity's create(0, 16, 5, 200, 800)): the directions
    // side by side at 8 lanes per line in every launch shape -- the per-pixel
    // work is small enough that the planes' traffic never outweighs the
    // single-frame latency of a strip chain
    if (e.D == 16 && o.path16 && o.path_sched != 1) return 2;
    if (!o.path16 || !(e.D == 32 || e.D == 64 || e.D == 128 || e.D == 256)) return 0;
    const bool dirs_ok = e.P2 <= 15 || o.path_sched == 2;  // nibble planes; wider planes when forced
    if (o.path_sched == 2) return 2;
    if (o.path_sched == 0 && bsgm_eligible(o, e, n, H) && e.SH2 <= 7 && e.SW2 == e.SH2) {
        // bit-sliced regime (round 6): the side-by-side chains' work grows with
        // the direction-pixels, the strips' time with the chain length; measured
        // (8 frames, MI355X r06e): 640x480 5 paths 0.90 side vs 1.11 ms strips,
        // 8 paths 1.10 vs 1.06; 1280x960 5 paths 3.49 vs 3.07, 8 paths 4.53 vs
        // 3.20; one 1280x960 frame, 8 paths 0.73 vs 1.03 (round 5)
        const long long dirpix = (long long)n * e.W1 * H * (e.fullDP ? 8 : 5);
        if (dirpix <= 12000000LL) return 2;
        return use_strips(o, e, H) ? 1 : 0;
    }
    if (o.path_sched == 0 && dirs_ok) {
        const int wide = e.D > 128 ? 7 : 15;
        const long long blocks = (long long)(e.fullDP ? 2 : 1) * n * ((e.W1 + H - 1 + 4 * wide - 1) / (4 * wide));
        // measured: one 640x480 or 1280x960 frame and two 640x480 frames gain
        // (0.76 -> 0.43, 1.62 -> 1.11, 0.83 -> 0.60 ms); two 1280x960 frames
        // lose (1.87 -> 1.95 ms: seven planes into the final kernel)
        if (2 * blocks <= cus) return 2;
    }
    if (o.path_sched == 0 && e.P2 > 15) {
        // byte / u16 planes (liveDisparity's create(0, 64, 9, 648, 2592)): side by
        // side while the planes stay small -- their bytes against the strip
        // chain's latency.  Measured (1280x960, MI355X r06 s2a / d16a): MODE_SGBM
        // D 32 x 1-3 frames 0.91 -> 0.53, 1.20 -> 1.07 ms; D 64 x 1, 2 frames
        // 1.16 -> 0.71, 1.34 -> 1.12 ms, x 4 1.98 -> 2.14 (strips kept); D 128 x 1
        // 1.50 -> 1.08, x 2 1.86 -> 1.90; D 256 x 1 2.08 -> 2.16; MODE_HH D 64 x 1
        // 1.18 -> 0.90, x 2 1.52 -> 1.59
        const double bytes = (double)n * e.W1 * H * e.D * (e.fullDP ? 7 : 4) * (acc_is_u8(e) ? 1 : 2);
        if (bytes <= 1.4e9) return 2;
    }
    return use_strips(o, e, H) ? 1 : 0;
}

// Cost-volume tile height: one block per TX x TY tile.  Taller tiles re-read
// fewer halo rows (2*SH2 per tile); shorter ones give small batches enough
// blocks (>= 2 per CU) to fill the chip.
inline int cost_tile_height(const KernelOptions& o, int cus, const SgbmEff& e, int n, int H)
{
    if (o.cost_ty > 0) return o.cost_ty;
    if (H < 256) return 16;
    const int TX = cost2_layout(e.D, e.SW2, 120).TX;
    const long tiles_x = (e.W1 + TX - 1) / TX;
    auto tiles = [&](int ty) { return tiles_x * ((H + ty - 1) / ty) * n; };
    int TY = 120;
    if (tiles(120) < 1024) {
        // small launches: least per-CU work, tiles per CU x rows per tile
        // incl. the 2*SH2 halo, a lone tile on a CU counted 1.5x (8 waves
        // hide less latency than 16); measured against forced heights: one
        // 640x480 frame 0.097 -> 0.073 ms, two 0.124 -> 0.110 ms, one
        // 1280x960 frame 0.227 -> 0.187 ms
        long best = -1;
        for (int ty : kCostTileHeights) {
            const long per_cu = (tiles(ty) + cus - 1) / cus;
            const long c = per_cu * (ty + 2 * e.SH2) * (per_cu == 1 ? 3 : 2);
            if (best < 0 || c < best) {
                best = c;
                TY = ty;
            }
        }
    }
    return TY;
}

// ---------------------------------------------------------------------------
// The plan
// ---------------------------------------------------------------------------
enum SgbmFamily {
    kFamGeneric = 0,  // sgbm_path_kernel: one wave per scanline, any D <= 512
    kFamPacked16,     // 16 lanes per scanline / U-column (D = 32 / 64 / 128 / 256)
    kFamPacked8,      // 8 lanes per line, D = 16, side by side only
    kFamBitslice      // bit planes (mvsv_bsgm.hip)
};
enum SgbmAcc { kAccNib = 4, kAccU8 = 8, kAccU16 = 16, kAccWords = 32 };  // accumulator element bits

struct SgbmPlan {
    bool empty = true;      // empty column range (or D > 512, which sgbm_device rejects): no pipeline
    int family = kFamGeneric;
    int sched = 0;          // 0 = one launch per direction, 1 = sheared strips + lines, 2 = side by side
    bool cost2 = false;     // the register-ring cost kernel runs (else the LDS-ring kernel)
    int cost_ty = 16;       // cost tile height
    bool residual = false;  // the cost kernel writes the residual plane and the direction passes read it
    bool no_wrap = false;   // sgbm_no_wrap
    bool nw = false;        // the packed path kernels run the no-wrap recurrence
    int acc = kAccU16;      // accumulator plane element
    int nplanes = 1;        // accumulator planes (bit-sliced: delta planes)
    bool split = false;     // side by side: R->L as one more plane, per-pixel WTA kernel
    // strips (sched 1)
    int passes = 0;         // strip passes: down, and up for MODE_HH
    int lpc = 0;            // lanes per U-column: 16 / 32 (packed)
    int waves = 0;          // compute waves per strip block
    int bs_groups = 0;      // bit-sliced: column groups per strip
    size_t bs_aplane = 0, bs_dplane = 0;  // bit-sliced: words per strip-pass plane / per line or delta plane
    int strip_cols = 0;     // U-columns per strip
    int nstrips = 0;        // strips per frame and pass
    long long blocks = 0;   // strip blocks of the launch: passes * n * nstrips
    int lines_aux = 0;      // L->R lines: 0 = after the strips on the context stream, 1 = on the second
                            // stream before them (beside), 2 = on the second stream after them
    // bytes of every cached buffer the call touches (0: not touched)
    size_t pre = 0, cost = 0, cres = 0, cres_min = 0 /* offset of the per-pixel minimum in cres */, agg = 0,
           raw = 0, keys = 0, dummy = 0, tri_bnd = 0, bs_bnd = 0, status = 0;

    size_t total_bytes() const
    {
        return pre + cost + cres + agg + raw + keys + dummy + tri_bnd + bs_bnd + status;
    }
    // the MVSV_PLAN_* word of mvsv_sgbm_plan
    int bits() const
    {
        if (empty) return 0;
        return (family == kFamBitslice ? kPlanBitslice : 0) | (sched == 2 ? kPlanSide : 0) |
               (sched == 1 ? kPlanStrips : 0) | (residual ? kPlanResidual : 0);
    }
    // the launch runs no strip chain (whose launches carry per-launch epochs):
    // its kernels and arguments are the same on every call with the same
    // arguments, so it may be replayed as a graph
    bool graphable() const { return !empty && sched == 2; }
};

inline SgbmPlan sgbm_make_plan(const KernelOptions& o, int cus, const SgbmEff& e, int n, int W, int H)
{
    SgbmPlan p;
    if (e.minX1 >= e.maxX1 || e.D > 512) return p;
    p.empty = false;
    const size_t frame = (size_t)W * H, pix = (size_t)n * e.W1 * H, vol = (size_t)e.W1 * H * e.D;
    p.sched = path_schedule(o, cus, e, H, n);
    p.cost2 = cost2_runs(o, e);
    p.cost_ty = cost_tile_height(o, cus, e, n, H);
    p.no_wrap = sgbm_no_wrap(e);
    p.passes = p.sched == 1 ? (e.fullDP ? 2 : 1) : 0;
    // frame batches: the bit-sliced strips; launches too small to fill the GPU
    // with strips (one camera frame, schedule 2): the bit-sliced directions
    // side by side, each on its own chains.  The cost kernel writes the C' bit
    // planes instead of the residual nibbles (D = 128 register-ring kernel).
    const bool bits = bsgm_eligible(o, e, n, H) && p.sched != 0 && o.path16 && o.tri && o.cost_fixed_pp && p.cost2;
    const bool wide = o.path16 && (e.D == 32 || e.D == 64 || e.D == 128 || e.D == 256);
    p.family = bits ? kFamBitslice : (e.D == 16 && p.sched == 2) ? kFamPacked8 : wide ? kFamPacked16 : kFamGeneric;
    p.residual = !bits && p.cost2 && use_residual(o, e, p.sched);

    p.pre = (size_t)n * 2 * e.cn * frame * 8;  // BT interval planes (census descriptors) of both views
    // (rows padded to a multiple of 4 pixels: the bit-sliced pipeline's layout)
    p.cost = (size_t)n * H * bs::padq(e.W1) * e.D * 2;
    p.raw = (size_t)n * frame * 2;
    if (p.family != kFamGeneric) p.keys = (size_t)n * frame * 4;  // right-view keys of the final kernels
    if (p.sched == 1) p.status = 16;  // [0] give-up epoch, [2] strip tickets drawn

    if (bits) {
        p.acc = kAccWords;
        const size_t dplane = p.bs_dplane = (size_t)n * H * bs::padq(e.W1) * 12;  // (grouped, padded rows)
        p.cres_min = align256((size_t)n * H * bs::padq(e.W1) * 64);  // C' planes
        p.cres = p.cres_min + pix * 2;
        if (p.sched == 2) {
            // all eight (five) directions as independent chains, one delta plane
            // each; + 256 words: dummy store slots of cells outside the image
            p.nplanes = 3 * (e.fullDP ? 2 : 1) + 2;
            p.agg = (p.nplanes * dplane + 256) * 4;
            return p;
        }
        // 3 column groups (96 U-columns, 10 waves) for MODE_HH batches: 352
        // strip blocks per 8-frame batch instead of 528 overlap better with
        // the other batch in flight (bench 3114-3120 -> 3164-3169 Mpix/s,
        // same box, r06n; one batch alone: strips 1.14 -> 1.15 ms); 4 groups
        // leave no room for the line waves beside them (lines 0.55 -> 2.0 ms)
        const int ng = o.bs_groups ? o.bs_groups : (e.fullDP ? 3 : 2);
        p.bs_groups = (ng == 1 || ng == 3 || ng == 4 || ng == 5) ? ng : 2;
        p.waves = 3 * p.bs_groups;
        p.strip_cols = bs_strip_cols(p.bs_groups);
        p.nstrips = ceil_div(e.W1 + H - 1, p.strip_cols);
        p.blocks = (long long)p.passes * n * p.nstrips;
        // the row directions beside the strips on the second stream (the strip
        // chain leaves CUs idle while it fills and drains, the line waves are
        // few and memory-bound): bench 2970 vs 2850 Mpix/s with the lines after
        // the strips on the context stream (bs_serial, same box, with
        // one-block-per-CU 2-group strips and the grouped planes)
        p.lines_aux = o.bs_serial ? 0 : 1;
        p.nplanes = p.passes + 2;  // strip-pass planes of 16 words per pixel, two line planes
        // + 512 words: the strip kernel's dummy store slots (cells outside the image)
        p.bs_aplane = pix * 16;
        p.agg = (p.passes * p.bs_aplane + 2 * dplane + 512) * 4;
        p.bs_bnd = (size_t)p.blocks * H * kBsGran * 8;
        return p;
    }

    if (p.residual) {
        // 0.5 byte per cost instead of 2, + the per-pixel cost minimum (u16) behind it
        p.cres_min = align256(n * vol / 2);
        p.cres = p.cres_min + pix * 2;
    }
    // accumulator planes: one per concurrently written direction group.  4-bit
    // planes: one per direction (side by side, P2 <= 15: a delta <= P2 each) or
    // per strip pass + lines (sums <= 3 * P2); bytes when all directions' sum
    // fits, else u16
    p.split = p.sched == 2 && wta_split(o, e);
    p.nplanes = p.sched == 2 ? sgbm_ndir(e) - 1 + (p.split ? 1 : 0) : p.sched == 1 ? p.passes + 1 : 1;
    p.acc = ((p.sched == 2 && e.P2 <= 15) || (p.sched == 1 && acc_is_nib(e))) ? kAccNib
            : acc_is_u8(e)                                                   ? kAccU8
                                                                             : kAccU16;
    p.agg = p.acc == kAccNib ? (size_t)p.nplanes * n * vol / 2 : (size_t)p.nplanes * n * vol * (p.acc / 8);
    if (p.family == kFamGeneric) return p;
    const int np = p.family == kFamPacked8 ? 1 : e.D / 32;  // disparity pairs per lane at 16 (8) lanes
    p.dummy = (size_t)512 * 16 * 2 * np;  // store slots of lanes outside the image
    // u8 / u16 planes at D = 256 (liveDisparity, config 5) on strips: the
    // no-wrap recurrence wherever no int16 can wrap -- its adds / subtracts
    // run at the full 32-bit rate, so it is the cheaper form here too (one
    // frame 2.04 -> 1.99 ms, profiles/r04/c5ab04); other D keep the general
    // form (compile time)
    p.nw = p.no_wrap && (p.acc == kAccNib || (p.sched == 1 && np == 8));
    if (p.sched != 1) return p;

    // Strip width: wide strips while the launch has at least one block per CU
    // (frame batches: the kernel is VALU-bound and wide strips share the step
    // barrier and the exchange wave among 15 compute waves); narrow strips when it
    // would not (one 640x480 frame: 34 wide blocks on 256 CUs, each strip step the
    // serial VALU work of 15 waves on one CU) -- the chain of strips then spreads
    // over more CUs at about half the per-step work (640x480, one frame: strips
    // 0.62 -> 0.41 ms; 4 waves per strip: 0.42 ms, its longer chain of strips
    // eats the shorter steps).  strip_waves forces either shape.
    // D = 256 launches that would run narrow strips (one or two frames): 32
    // lanes per column (tri32 = 0: the 16-lane narrow strips).
    const int wide_wv = tri_wide_waves(np, 16), narrow_wv = tri_narrow_waves(np, 16);
    const bool few = (long long)p.passes * n * ceil_div(e.W1 + H - 1, tri_strip_cols(wide_wv, 16)) < cus;
    p.lpc = 16;
    if (np == 8 && o.tri32 && o.strip_waves == 0 && few) {
        p.lpc = 32;
        p.waves = tri_narrow_waves(np / 2, 32);
    } else if (o.strip_waves == wide_wv || o.strip_waves == narrow_wv) {
        p.waves = o.strip_waves;
    } else {
        p.waves = few ? narrow_wv : wide_wv;
    }
    p.strip_cols = tri_strip_cols(p.waves, p.lpc);
    p.nstrips = ceil_div(e.W1 + H - 1, p.strip_cols);
    p.blocks = (long long)p.passes * n * p.nstrips;
    p.tri_bnd = (size_t)p.blocks * H * 4 * p.lpc * tri_granules(np * 16 / p.lpc) * 8;
    // L->R lines (lines_aux < 0, default): beside the strips when the launch is
    // small (the strips then occupy a fraction of the CUs -- one frame: ~60 of
    // 256 -- and the L->R lines fill idle ones); after them for batches,
    // where both kernels saturate the GPU and running them together was
    // measured slower.
    // Round 4: with the residual input the line kernel needs 53 VGPRs and
    // the wide strip kernel 103, so a line wave fits beside a strip block
    // on every SIMD -- launched after the strips on the second stream, the
    // lines fill the strips' step-barrier and hand-off waits (one batch of
    // 8 frames: 4.49 -> 4.37-4.40 ms, MI355X r04d A/B).
    // Round 6: "small" counts the strip blocks the launch really has: beside
    // the strips only while those occupy at most 60 % of the CUs (one 1280x960
    // frame: 124 narrow D = 256 blocks, 132 narrow D = 128 MODE_HH blocks).
    // Two config-5 frames (D 256, 248 narrow blocks) had the lines beside them
    // at 2.68 ms instead of 0.66 for one frame (r04g c5_frame.jsonl): every CU
    // held a strip.  Byte / u16 planes at D <= 64 run the lines on the second
    // stream in batches too (liveDisparity default, 1280x960 x 4 / x 8:
    // 1.97 -> 1.87, 3.13 -> 2.88 ms); D = 256 keeps them after the strips
    // (x 4: 4.90 -> 5.7 ms beside, x 8: 8.60 -> 8.50; profiles/r06/aux/lines_aux_ab.txt)
    p.lines_aux = o.lines_aux >= 0           ? o.lines_aux
                  : 5 * p.blocks <= 3LL * cus ? 1
                  : (p.residual || np <= 2)   ? 2
                                              : 0;
    return p;
}

// The speckle filter's buffers for n W x H maps (speckle_device, mvsv_post.hip):
// parent, size and tile words, u16 local roots, the compact root list + its count
struct SpeckleBytes {
    size_t parent, size, tile, lroot, list;
    size_t total() const { return parent + size + tile + lroot + list; }
};
inline SpeckleBytes speckle_bytes(int n, int W, int H)
{
    const size_t npix = (size_t)n * W * H;
    return {npix * 4, npix * 4, npix * 4, npix * 2, (npix + 1) * 4};
}

}  // namespace mvsv
