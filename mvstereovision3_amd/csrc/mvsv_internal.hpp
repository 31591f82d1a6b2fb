// mvsv_internal.hpp — shared declarations of libmvsv (host + HIP kernels).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mvsv.h"
#include "mvsv_sgbm_plan.hpp"

namespace mvsv {

constexpr int kMaxCost = 32767;    // OpenCV StereoSGBM MAX_COST (SHRT_MAX)
constexpr int kDispShift = 4;      // StereoMatcher::DISP_SHIFT
constexpr int kDispScale = 16;

struct BmEff {
    int ndisp, mindisp, wsz2, cap, tex, uniq;
    int lofs, rofs, width1, ncol;
    int xmin, xmax, ymin, ymax;  // validDisparityRect (half-open)
    int filtered;                // (minD - 1) << 4
    int disp12;                  // < 0: off
    int speckle_window, speckle_range;
    int prefilter_type, prefilter_size;
    int cw, ch;                  // census window (mvsv_bm_census); 0, 0: the SAD cost
};
inline bool bm_census(const BmEff& e) { return e.cw != 0; }

// Resolve + validate (OpenCV's asserts). Return MVSV_OK or MVSV_E_INVALID_ARG
// and an explanation in *why.
int resolve_sgbm(const mvsv_sgbm_params* p, int W, int H, SgbmEff* e, std::string* why);
int resolve_bm(const mvsv_bm_params* p, int W, int H, BmEff* e, std::string* why);
// resolve_bm plus the window rule of a census call (include/mvsv.h mvsv_bm_census_validate);
// e->cw, e->ch are set
int resolve_bm_census(const mvsv_bm_params* p, int W, int H, int cw, int ch, BmEff* e, std::string* why);

// Grow-only cached device buffer.
struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
};

// Entry points switch to the context's device and give the caller's current
// device back on return (a compute on cuda:1 must not change the thread's
// device under the torch code that runs next).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) {
            (void)hipGetLastError();
            prev = -1;
        }
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

static_assert(kPlanBitslice == MVSV_PLAN_BITSLICE && kPlanSide == MVSV_PLAN_SIDE && kPlanStrips == MVSV_PLAN_STRIPS &&
                  kPlanResidual == MVSV_PLAN_RESIDUAL,
              "SgbmPlan::bits() speaks include/mvsv.h's MVSV_PLAN_* word");

}  // namespace mvsv

struct mvsv_ctx {
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    // SGBM
    mvsv::DevBuf pre, cost, cres, agg, raw, uf_parent, uf_size, uf_tile, uf_lroot, uf_list, dummy, keys, tri_bnd, bs_bnd, status;
    bool uf_list_dirty = false;  // a speckle run launched its first stage but not its last
    // launch number of the last sheared-strip launch: its low 16 bits tag the
    // boundary granules (tri_bnd is re-zeroed whenever they wrap), all 32 bits
    // go into status[0] when that launch gives up a wait (no per-call reset)
    unsigned tri_epoch = 0;
    // the first ticket of the next strip launch (opt.strip_tickets; the counter is
    // zeroed with the status word)
    unsigned tri_tickets = 0;
    mvsv::KernelOptions opt;
    // given-up strip waits are reported into host-mapped ints: `report` is the
    // context's sticky word (device calls; read and cleared by the next call,
    // mvsv_synchronize and the host-pointer calls), report_target is where the
    // next launches report (a frame stream points it at its run's own word)
    int* report = nullptr;      // host view
    int* report_dev = nullptr;  // device view of report
    int* report_target = nullptr;
    // context-owned "last use" event: recorded on ctx->stream at the end of every
    // enqueueing entry point; a stream switch makes the new stream wait on it
    // (never records on the previous stream handle, which the caller may have
    // destroyed since)
    hipEvent_t ev_last = nullptr;
    bool last_valid = false;
    hipStream_t aux = nullptr;  // second stream for concurrent direction passes
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int cus = 256;   // compute units of the device (launch-shape choices)
    // HIP graphs (round 6): a small SGBM launch (no strip chain, whose launches
    // carry per-launch epochs) repeated with the same arguments is captured once
    // on the capture stream and then replayed as one graph launch; every cached
    // buffer (re)allocation or free bumps alloc_epoch and retires the graphs
    // measured slower than eager launches on ROCm 7.2 / MI355X (config 3 one
    // frame 0.259 vs 0.250 ms, config 2 0.041 vs 0.033 ms; profiles/r06/graphs),
    // so opt-in: MVSV_GRAPHS=1
    int graphs = 0;
    unsigned alloc_epoch = 0;
    struct GraphEntry {
        std::vector<unsigned char> key;
        hipGraphExec_t exec = nullptr;
        unsigned epoch = 0;
        unsigned long long used = 0;
    };
    std::vector<GraphEntry> graph_cache;
    std::vector<unsigned char> graph_seen;  // arguments of the last eager launch
    unsigned long long graph_clock = 0;
    hipStream_t cap = nullptr;  // capture stream
    // BM
    mvsv::DevBuf bm_lf, bm_rf, bm_cost, bm_sad;
    // the host-pointer calls' staging arena (mvsv_stage.hpp)
    mvsv::DevBuf stage;
    // display maps: one (min, max) pair per block of minmax_kernel, [n][blocks][2] ints
    mvsv::DevBuf mm_part;
    // point clouds: (min, max) per frame, then (first record, min | max) per row, int pairs
    mvsv::DevBuf cl_rows;
    // focus measure: one 64-bit partial sum per block of sharpness_kernel, [n][blocks]
    mvsv::DevBuf sh_part;
    // mvsv_undistort_pair: both cameras' fixed-point maps ([2][H][W] int16 pairs, then
    // [2][H][W] u16) for the calibration in ud_key (K, dist, size of both sides)
    mvsv::DevBuf ud_maps;
    std::vector<double> ud_key;
    // stage profiling (HIP events on the context stream)
    int prof = 0;
    struct Mark {
        int stage;
        hipEvent_t a, b;
    };
    std::vector<Mark> marks;
    std::vector<hipEvent_t> event_pool;
};

namespace mvsv {

int set_error(mvsv_ctx* ctx, int code, const std::string& msg);
int ensure(mvsv_ctx* ctx, DevBuf& b, size_t bytes, const char* what);
int check_hip(mvsv_ctx* ctx, hipError_t e, const char* what);
// Reads and clears the context's sticky report word: MVSV_E_TIMEOUT if a
// strip-boundary wait of an earlier launch gave up.  No synchronisation.
int check_report(mvsv_ctx* ctx);
// Host-mapped int (host and device views), zeroed.
int alloc_report(mvsv_ctx* ctx, int count, int** host, int** dev);
// Records the context's last-use event on ctx->stream after an entry point
// enqueued work (keeps rc: an error code passes through unchanged).
int mark_last_use(mvsv_ctx* ctx, int rc);

enum Stage {
    kStagePre = 0,
    kStageCost,
    kStageFixup,
    kStagePath,
    kStageFinal,
    kStagePost,
    kStageBm,
    kStageStrips,
    kStageLines
};
// RAII: records a start / stop event pair around the launches in its scope
// when profiling is enabled (no-op otherwise).
struct StageTimer {
    mvsv_ctx* ctx;
    int stage;
    hipStream_t st;  // stream the events are recorded on (default: the context stream)
    hipEvent_t a = nullptr, b = nullptr;
    StageTimer(mvsv_ctx* c, int s, hipStream_t on = nullptr);
    ~StageTimer();
};

// Device pipelines (defined in the .hip translation units). All enqueue on
// ctx->stream. Strides are in elements (sgbm_device with e.cn == 3: W in pixels,
// input strides in bytes, rows of 3 W interleaved bytes).
int sgbm_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                size_t rs, size_t rfs, int W, int H, const SgbmEff& e, int16_t* out, size_t os,
                size_t ofs);
// The plan of an SGBM call on this context (mvsv_sgbm_plan.hpp)
inline SgbmPlan sgbm_make_plan(const mvsv_ctx* ctx, const SgbmEff& e, int n, int W, int H)
{
    return sgbm_make_plan(ctx->opt, ctx->cus, e, n, W, H);
}
int bm_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
              size_t rs, size_t rfs, int W, int H, const BmEff& e, int16_t* out, size_t os,
              size_t ofs);
// A census call's descriptors and match kernel (mvsv_bm_census.hip), between bm_device's
// fill and its finishing passes; cost: the minimum-cost map validateDisparity reads, or null
int bm_census_match(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R, size_t rs,
                    size_t rfs, int W, int H, const BmEff& e, int16_t* out, size_t os, size_t ofs, int* cost);
// SGBM stages 1-3 (mvsv_cost.hip): BT interval planes, the cost volume (the kernel
// and tile height the plan names; the register-ring kernel also writes the residual
// plane Rv or the bit-sliced C' planes Bv where the plan says so), and OpenCV 3.4's
// cost-row quirks on the int16 volume.
int launch_prefilter(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R, size_t rs,
                     size_t rfs, int W, int H, int ftzero, int cn, uint64_t* pre);
int launch_cost(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int W, int H, const SgbmEff& e, const uint64_t* pre,
                int16_t* Cv, uint8_t* Rv, uint16_t* Mv, uint32_t* Bv);
int launch_cost_fixup(mvsv_ctx* ctx, int n, int H, const SgbmEff& e, int16_t* Cv, uint8_t* Rv, uint16_t* Mv);
// The census transform (mvsv_census.hip): the window rule as a message (nullptr: the
// window is valid), and one launch over nimg views (1: L alone, 2: L and R) of n
// frames.  Input strides in bytes; descriptor (f, img, y, x) goes to
// out[f * ofs + img * ois + y * ors + x] (strides in u64 elements).
const char* census_window_check(int cw, int ch);
int census_device(mvsv_ctx* ctx, int n, int nimg, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                  size_t rs, size_t rfs, int W, int H, int cw, int ch, uint64_t* out, size_t ors, size_t ois,
                  size_t ofs);
// resolve_sgbm plus the rules of a census call (include/mvsv.h mvsv_sgbm_census_validate);
// e->cw, e->ch are set
int resolve_sgbm_census(const mvsv_sgbm_params* p, int W, int H, int cw, int ch, SgbmEff* e, std::string* why);
// Bit-sliced path aggregation + WTA, MODE_HH and MODE_SGBM (mvsv_bsgm.hip): where the
// plan's family is kFamBitslice the cost kernel writes the C' planes Bv and bsgm_paths
// computes raw disparities from them, on the plan's schedule, strip width and planes.
int bsgm_paths(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, int W, const SgbmEff& e, const int16_t* Cv,
               const uint32_t* Bv, const uint16_t* Mv, int16_t* raw);
// The packed-int16 path kernels + WTA at 16 lanes per line, D = 32 NP (NP = 1, 2, 4, 8):
// launches the template instance for the plan's schedule, plane element, recurrence and
// cost input (Rv: the residual plane).  Each NP is instantiated in an object of its own
// (mvsv_sgbm_packed.hip, compiled with -DMVSV_SGBM_NP=NP).
template <int NP>
int launch_packed16(mvsv_ctx* ctx, const SgbmPlan& plan, int n, int H, int W, const SgbmEff& e, int16_t* Cv,
                    const uint8_t* Rv, const uint16_t* Mv, void* Av, int16_t* raw);
// The second stream and its fork / join events (the L->R lines beside the strips)
int ensure_aux(mvsv_ctx* ctx);
// The preamble of a strip launch, packed or bit-sliced (one launch counter for both).
// *epoch: the next launch number whose low 16 bits are not 0 -- tag 0 means "never
// written".  16-bit tags (tag_bits 16) repeat when they wrap, so every granule of bnd
// is zeroed again then and a slot carrying this launch's tag was written by it; 32-bit
// tags only skip 0.  *ticket0: the launch's first strip ticket, -1 for blockIdx order
// (strip tickets, round 4: a launch of at most one block per CU is not resident all at
// once when other work shares the GPU, so blockIdx order would rest on in-order
// dispatch; tickets never do).  The caller adds its block count to ctx->tri_tickets.
int strip_begin(mvsv_ctx* ctx, DevBuf& bnd, int tag_bits, unsigned* epoch, long long* ticket0);
// Strip statistics (diagnostics only): a zeroed device buffer, cleared on the context
// stream -- nullptr on any failure, which switches the statistics off; and its words
// after the stream has drained (frees the buffer; false: nothing to print).
unsigned long long* strip_stats_alloc(mvsv_ctx* ctx, size_t bytes);
bool strip_stats_read(mvsv_ctx* ctx, unsigned long long* stats, size_t words, std::vector<unsigned long long>* h);
// MODE_SGBM's never-recomputed rows and column 0 on the bit-sliced layouts (C'
// planes, pixel-quad C, m); no-op for MODE_HH, whose cost kernel pins them
int bsgm_cost_fixup(mvsv_ctx* ctx, int n, int H, const SgbmEff& e, int16_t* Cv, uint32_t* Bv, uint16_t* Mv);
// Post filters shared by both matchers.
// poison != nullptr: when *poison == epoch (the launch `epoch` gave up a strip
// wait) every output pixel is `invalid` instead of the median -- no map computed
// from stale hand-off data leaves the pipeline.
int median3x3_device(mvsv_ctx* ctx, int n, const int16_t* src, size_t ss, size_t sfs,
                     int16_t* dst, size_t ds, size_t dfs, int W, int H,
                     const int* poison = nullptr, unsigned epoch = 0, int invalid = 0);
int speckle_device(mvsv_ctx* ctx, int n, int16_t* img, size_t st, size_t fs, int W, int H,
                   int new_val, int max_size, int max_diff);

int remap_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t ss, size_t sfs, int sw, int sh,
                 const float* mx, const float* my, size_t ms, uint8_t* dst, size_t ds, size_t dfs,
                 int dw, int dh);
// The raw frame stream's rectification (mvsv_post.hip): raw = [n][2][sh][sw], maps
// in mvsv_convert_maps' form as [2][dh][ms] entries (ms a multiple of 4, >= dw,
// padding entries zero); frame f goes to dL / dR + f * dfs, rows ds bytes apart.
int rectify_pair_device(mvsv_ctx* ctx, int n, const uint8_t* raw, int sw, int sh, const int16_t* xy,
                        const uint16_t* frac, size_t ms, int dw, int dh, uint8_t* dL, uint8_t* dR, size_t ds,
                        size_t dfs);
// cv::resize INTER_LINEAR (CV_8UC1) output size / launch (mvsv_post.hip)
int resize_size(int sw, int sh, double fx, double fy, int* dw, int* dh);
int resize_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t ss, size_t sfs, int sw, int sh, double fx,
                  double fy, uint8_t* dst, size_t ds, size_t dfs);
// Grey pair preparation (mvsv_prepare.hip): interleaved BGR -> grey, halved 2 x 2
// first with halve = 1 (include/mvsv.h); strides in bytes
int prepare_size(int sw, int sh, int halve, int* dw, int* dh);
int prepare_gray_device(mvsv_ctx* ctx, int n, const uint8_t* bgr, size_t ss, size_t sfs, int sw, int sh, int halve,
                        int variant, uint8_t* dst, size_t ds, size_t dfs);
// The INTER_AREA half of prepare_gray_device alone, per channel: interleaved BGR in,
// interleaved BGR of mvsv_prepare_size(sw, sh, 1) out (the colour-matched stream frames)
int halve_bgr_device(mvsv_ctx* ctx, int n, const uint8_t* bgr, size_t ss, size_t sfs, int sw, int sh, uint8_t* dst,
                     size_t ds, size_t dfs);
// The frame stream's device push (mvsv_prepare.hip): rows of row_bytes bytes of both
// sides of n frames (strides in bytes) into dL / dR, which share ds / dfs; one launch
// on `stream`.  The pointers must be readable / writable by the device.
int stream_copy_device(mvsv_ctx* ctx, hipStream_t stream, int n, const uint8_t* L, size_t ls, size_t lfs,
                       const uint8_t* R, size_t rs, size_t rfs, uint8_t* dL, uint8_t* dR, size_t ds, size_t dfs,
                       int row_bytes, int rows);
// Disparity::tm (mvsv_tm.hip): the accepted kernel sizes, and n frames on ctx->stream;
// elem_bytes 1 stores the shift's low byte, 2 the shift as uint16 (strides in bytes)
int tm_validate(int k, int W, int H, std::string* why);
int tm_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R, size_t rs, size_t rfs,
              int W, int H, int k, void* dst, size_t ds, size_t dfs, int elem_bytes);
int reproject_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                     const float* Q, float* out, size_t os, size_t ofs);
int mean_grid_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W,
                     int H, float* means);
// SamplepointDetection's lattice (mvsv_post.hip).  sample_layout: steps and point
// counts of a W x H map (nx * ny == 0: no point); the launches return MVSV_OK
// without a launch for such a map.  values: nx * ny floats per frame, point
// (c, r) at c * ny + r; hits: max_hits records per frame, counts: one int each.
int sample_layout(int W, int H, int* step_x, int* step_y, int* nx, int* ny);
int sample_grid_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H, int radius,
                       float* values);
int sample_detect_device(mvsv_ctx* ctx, int n, const float* values, int W, int H, const float* Q, float first,
                         float second, int max_hits, int* counts, mvsv_sample_hit* hits);
// Display maps (mvsv_post.hip).  minmax: [n][2] int16 (min, max) of every frame,
// positive_only: over the values > 0 only, (32767, -32768) for none.
// normalize_minmax_device: cv::normalize(NORM_MINMAX, CV_8U) of every frame with
// its own min / max, which also go to minmax where it is not null.
int minmax_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H, bool positive_only,
                  int16_t* minmax);
int normalize_minmax_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                            double alpha, double beta, uint8_t* out, size_t os, size_t ofs, int16_t* minmax);
// What the display kernels share with the detection view (mvsv_post.hip).
// display_split: the head | packed groups | tail walk of a row (head = W: narrow
// loads only).  minmax_partials: *nblk (min, max) pairs per frame into ctx->mm_part.
void display_split(const int16_t* dmap, size_t st, size_t fs, int n, int W, int* head, int* nvec);
int minmax_partials(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H, bool positive_only,
                    int* nblk);
// Detection view (mvsv_view.hip): the BGR frame of every map with the layers of
// spec drawn in (include/mvsv.h); spec's means / values are device pointers,
// [n][81] and [n][nx * ny].  view_check: the argument rules, without a device.
const char* view_check(const mvsv_view_spec* spec, int W, int H);
int view_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                const mvsv_view_spec& spec, uint8_t* out, size_t os, size_t ofs, int16_t* minmax);
// the layers of spec painted over a host BGR image, one after the other (host pointers)
void view_draw_host(uint8_t* img, size_t stride, int W, int H, const mvsv_view_spec& spec);
// Focus measure (mvsv_post.hip): S4 (include/mvsv.h) of roi q of every u8 frame
// into sums[f * ss]; q non-empty and inside the W x H image, strides in bytes.
int sharpness_device(mvsv_ctx* ctx, int n, const uint8_t* img, size_t st, size_t fs, int W, int H, const mvsv_rect& q,
                     int64_t* sums, size_t ss);
// cv::remap with fixed-point maps (mvsv_post.hip): xs in int16 pairs, fs in elements
int remap_fixed_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t ss, size_t sfs, int sw, int sh,
                       const int16_t* xy, size_t xs, const uint16_t* frac, size_t fs, uint8_t* dst, size_t ds,
                       size_t dfs, int dw, int dh);
// Point clouds (mvsv_post.hip): the records of the pixels with v > 0 of every frame
// in raster order, frame f into records[f * capacity ..]; counts[f * cs] = the
// number of such pixels, minmax[f * ms], [f * ms + 1] = their (min, max) where
// minmax is not null.
int point_cloud_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H, const float* Q,
                       mvsv_cloud_point* records, int capacity, int* counts, size_t cs, int* minmax, size_t ms);

}  // namespace mvsv
