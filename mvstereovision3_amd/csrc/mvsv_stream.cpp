// mvsv_stream.cpp — double-buffered frame stream for a camera loop.
//
// Replaces the reference's worker-thread pattern (trgt/mean_test.cpp:61-70: one
// thread waits on a condition variable, runs Disparity::sgbm on the shared
// Stereopair, flags newDisparityMap; the main loop then runs
// MeanDisparityDetection::build on an ROI of the map, :258-318).  Here every
// pushed frame owns a slot (pinned host staging + device buffers + events); the
// upload of frame i+1 (copy stream), the compute of frame i (context stream:
// SGBM + the 9x9 mean grid of the ROI) and the download of frame i-1 (second
// copy stream) overlap, and frames come back in push order.
// With mvsv_stream_enable_samplepoints, SamplepointDetection's lattice values and
// hits of every frame (trgt/demo.cpp:206-209,271-276 runs both detectors) are
// computed next to the mean grid and come back with the frame (front_samples).
// With mvsv_stream_enable_display, the 8-bit display map of every frame
// (cv::normalize NORM_MINMAX, the last step of trgt/liveDisparity.cpp's loop) is
// computed after them and comes back with the frame too (front_display).
// With mvsv_stream_enable_cloud, the point cloud of every frame (the dmap2pcl call
// that ends the detector loops' key handler, trgt/demo.cpp:394) is compacted after
// them into a device ring; only its (count, min, max) come back with the frame and
// front_cloud copies the records that exist on demand.
// With mvsv_stream_enable_sharpness, the focus measure of the pushed pair
// (Utility::checkSharpness, what trgt/liveView.cpp prints; on a raw stream the raw
// camera pair) is summed on the same device stream and its two int64 sums come back
// with the frame (front_sharpness).
// With mvsv_stream_set_batch(b), pushed frames are computed b at a time: the
// slots' device buffers are one contiguous [depth][frame] array, so a group of
// consecutive slots is one frame-batch launch (sustained rate of the batch
// kernels instead of the single-frame ones, at b frames of extra latency);
// pop and set_params launch a partial group when they need to.
// With mvsv_stream_set_inflight(n), consecutive launches go round-robin to n
// compute lanes: the caller's context and n-1 contexts the stream owns (each
// its own HIP stream and scratch buffers), so up to n frame-batch launches run
// concurrently and one fills the chip's gaps left by another's
// latency-bound kernels.
// A stream runs one matcher at a time, SGBM or StereoBM (mvsv_stream_create_bm,
// mvsv_stream_set_bm_params: trgt/disparityTest.cpp:267-268 runs both on every
// pair); everything behind the matcher is a function of the int16 map.
// With mvsv_stream_enable_bgr, a stream of rectified pairs also takes interleaved
// BGR pairs (mvsv_stream_push_bgr): uploaded once as BGR, halved and converted to
// grey into the slot's dL / dR ahead of the matcher (disparityTest.cpp:201-211).
// With mvsv_stream_push_device (and its raw / BGR forms), frames come from device
// memory: one copy kernel per contiguous piece of the ring puts them into the
// slots, ordered against the producer's stream by events; set_host_outputs drops
// the per-frame downloads nobody reads, pop_device and front_*_device hand the
// results out on the device, and fence orders the stream behind a zero-copy
// reader.
// The host copies of a frame (caller rows -> pinned slot on push, pinned map ->
// caller rows on pop) are split over a small pool of copy threads that the
// stream owns (MVSV_STREAM_COPY_THREADS, default 4 including the caller), so a
// host whose single-core memcpy is slow still feeds the GPU at its rate.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "mvsv_internal.hpp"
#include "mvsv_ring.hpp"

using namespace mvsv;

static constexpr int kStreamMaxInflight = 4;
static constexpr size_t kPoolMinBytes = (size_t)1 << 20;  // smaller copies stay on the caller's thread

// Persistent row-copy pool: run(fn) calls fn(p, parts) once for every part
// p < parts = size(), the calling thread taking parts too, and returns when
// every worker has checked out of the run (so none touches fn or the part
// counter after run returns).
class CopyPool {
  public:
    // A worker that cannot be created (std::system_error, bad_alloc) leaves the
    // pool with the workers made so far: nothing escapes into the C ABI.
    explicit CopyPool(int threads)
    {
        try {
            workers_.reserve((size_t)std::max(threads - 1, 0));
            for (int i = 1; i < threads; i++) workers_.emplace_back([this] { loop(); });
        } catch (...) {
        }
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    int size() const { return (int)workers_.size() + 1; }
    void run(const std::function<void(int, int)>& fn)
    {
        const int parts = size();
        if (parts == 1) {
            fn(0, 1);
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            fn_ = &fn;
            next_.store(0, std::memory_order_relaxed);
            active_ = parts - 1;
            gen_++;
        }
        cv_.notify_all();
        for (int p; (p = next_.fetch_add(1, std::memory_order_relaxed)) < parts;) fn(p, parts);
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [&] { return active_ == 0; });
        fn_ = nullptr;
    }

  private:
    void loop()
    {
        long seen = 0;
        for (;;) {
            const std::function<void(int, int)>* fn;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                fn = fn_;
            }
            const int parts = size();
            for (int p; (p = next_.fetch_add(1, std::memory_order_relaxed)) < parts;) (*fn)(p, parts);
            std::lock_guard<std::mutex> g(m_);
            if (--active_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int, int)>* fn_ = nullptr;
    std::atomic<int> next_{0};
    int active_ = 0;
    long gen_ = 0;
    bool stop_ = false;
};

// rows [0, H) of W-byte rows: src (stride ss) -> dst (stride ds), split by part
static void copy_rows(uint8_t* dst, size_t ds, const uint8_t* src, size_t ss, size_t W, int H, int part,
                      int parts)
{
    const int y0 = (int)((long)H * part / parts), y1 = (int)((long)H * (part + 1) / parts);
    if (ds == W && ss == W) {
        std::memcpy(dst + (size_t)y0 * W, src + (size_t)y0 * W, (size_t)(y1 - y0) * W);
        return;
    }
    for (int y = y0; y < y1; y++) std::memcpy(dst + (size_t)y * ds, src + (size_t)y * ss, W);
}

struct mvsv_stream {
    mvsv_ctx* ctx = nullptr;
    std::vector<mvsv_ctx*> lanes;  // [0] = ctx; the rest are owned by the stream
    long runs = 0;                 // launches enqueued (lane = runs % lanes)
    int W = 0, H = 0;
    int matcher = MVSV_MATCHER_SGBM;  // of the frames pushed from now on
    mvsv_sgbm_params params{};
    SgbmEff eff{};
    mvsv_bm_params bm_params{};
    BmEff bm_eff{};
    bool grid = false;
    mvsv_rect roi{};
    hipStream_t up = nullptr, down = nullptr;
    struct Slot {
        uint8_t *hL = nullptr, *hR = nullptr;  // pinned
        uint8_t *hRectL = nullptr, *hRectR = nullptr;  // pinned, keep_rectified streams
        uint8_t* dRaw = nullptr;                       // [2][rawH][rawW], raw streams
        uint8_t *hBgr = nullptr, *dBgr = nullptr;      // [2][bgrH][bgrRow], pinned / device, with enable_bgr
        bool is_bgr = false;                           // the pending frame was pushed as BGR
        int16_t* hOut = nullptr;
        float* hMeans = nullptr;
        uint8_t *dL = nullptr, *dR = nullptr;
        int16_t* dOut = nullptr;
        float* dMeans = nullptr;
        hipEvent_t uploaded = nullptr, computed = nullptr, done = nullptr;
        hipEvent_t released = nullptr;  // pop_device's copy of dOut on the consumer's stream
        bool release_pending = false;   // the slot's next launch waits for `released`
        int status = MVSV_OK;
        int run_len = 0;     // > 0: this slot starts a frame-batch launch of run_len slots
        bool gave_up = false;  // the launch of this frame gave up a strip wait
    };
    std::vector<Slot> slots;
    uint8_t *dL_all = nullptr, *dR_all = nullptr;  // [depth][H][W]
    int16_t* dOut_all = nullptr;
    float* dMeans_all = nullptr;  // [depth][81]
    // per-slot report words (host-mapped): a launch starting at slot i reports
    // a given-up strip wait into rep[i], read when slot i is popped
    int* rep = nullptr;
    int* rep_dev = nullptr;
    long head = 0, tail = 0;      // pushed / popped frame counters
    long launched = 0;            // frames whose compute is enqueued
    int batch = 1;
    int host_mask = MVSV_HOST_ALL;     // the per-frame D2H copies that are enqueued (set_host_outputs)
    hipEvent_t producer_ev = nullptr;  // push_device: what the producer had queued
    hipEvent_t fence_ev = nullptr;     // mvsv_stream_fence
    bool fenced = false;
    CopyPool* pool = nullptr;     // host copies of push / pop (nullptr: caller's thread only)
    // raw stream (mvsv_stream_create_raw): pushed frames are raw camera pairs,
    // rectified (cropped, resized) into the slots' dL / dR ahead of their SGBM
    bool raw = false;
    int rawW = 0, rawH = 0;       // the camera frame; a slot's hL / hR hold one each
    int cropW = 0, cropH = 0;     // the display ROI's size
    double factor = 0;            // 0: the crop is the frame; else cv::resize of the crop
    bool keep = false;            // the rectified pair comes back to the host too
    uint8_t* dRaw_all = nullptr;  // [depth][2][rawH][rawW]
    int16_t* dMapXY = nullptr;    // [2][cropH][mapStride] (sx, sy), ROI only
    uint16_t* dMapFrac = nullptr; // [2][cropH][mapStride] ay * 32 + ax
    size_t mapStride = 0;         // entries per map row: cropW rounded up to 4, padding zero
    uint8_t *dCropL = nullptr, *dCropR = nullptr;  // [depth][cropH][cropW] each, with a factor
    // SamplepointDetection's lattice over sp_roi of every frame
    // (mvsv_stream_enable_samplepoints): values, hit count and hit records per
    // slot, on the device and in one pinned host block
    bool sp = false;
    mvsv_rect sp_roi{};
    int sp_radius = 0, sp_max = 0, sp_npts = 0;
    float sp_Q[16] = {}, sp_first = 0, sp_second = 0;
    float* dSpVal = nullptr;            // [depth][sp_npts]
    int* dSpCnt = nullptr;              // [depth]
    mvsv_sample_hit* dSpHits = nullptr; // [depth][sp_max]
    uint8_t* hSp = nullptr;             // pinned: [depth] x (values, count, hits), sp_slot_bytes each
    size_t sp_slot_bytes = 0;
    float* sp_values(long i) const { return (float*)(hSp + (size_t)i * sp_slot_bytes); }
    int* sp_count(long i) const { return (int*)(sp_values(i) + sp_npts); }
    mvsv_sample_hit* sp_hits(long i) const { return (mvsv_sample_hit*)(sp_count(i) + 1); }
    // the display map of disp_roi of every frame (mvsv_stream_enable_display): a
    // dense u8 map and (smin, smax) per slot, on the device and in one pinned host block
    bool disp = false;
    mvsv_rect disp_roi{};
    double disp_alpha = 0, disp_beta = 255;
    uint8_t* dDisp = nullptr;    // [depth][rh][rw]
    int16_t* dDispMM = nullptr;  // [depth][2]
    uint8_t* hDisp = nullptr;    // pinned: [depth] x (map, min, max), disp_slot_bytes each
    size_t disp_px = 0, disp_slot_bytes = 0;
    uint8_t* disp_map(long i) const { return hDisp + (size_t)i * disp_slot_bytes; }
    int16_t* disp_minmax(long i) const { return (int16_t*)(disp_map(i) + ((disp_px + 1) & ~(size_t)1)); }
    // the detection view of view_roi of every frame (mvsv_stream_enable_view): a
    // dense BGR image and (smin, smax) per slot, on the device and in one pinned
    // host block; view_spec's pointers are set per launch
    bool view = false;
    mvsv_rect view_roi{};
    mvsv_view_spec view_spec{};
    uint8_t* dView = nullptr;    // [depth][rh][rw][3]
    int16_t* dViewMM = nullptr;  // [depth][2]
    uint8_t* hView = nullptr;    // pinned: [depth] x (image, min, max), view_slot_bytes each
    size_t view_bytes = 0, view_slot_bytes = 0;
    uint8_t* view_img(long i) const { return hView + (size_t)i * view_slot_bytes; }
    int16_t* view_minmax(long i) const { return (int16_t*)(view_img(i) + ((view_bytes + 1) & ~(size_t)1)); }
    // the point cloud of cloud_roi of every frame (mvsv_stream_enable_cloud): the
    // records stay in a device ring, (count, min, max) per slot come to the host
    bool cloud = false;
    mvsv_rect cloud_roi{};
    float cloud_Q[16] = {};
    int cloud_max = 0;
    mvsv_cloud_point* dCloud = nullptr;  // [depth][cloud_max]
    int* dCloudHdr = nullptr;            // [depth][3] (count, min, max)
    int* hCloudHdr = nullptr;            // pinned, [depth][3]
    hipStream_t cloud_copy = nullptr;    // front_cloud's copies: not behind the later frames' downloads
    // the focus measure of every pushed pair (mvsv_stream_enable_sharpness): S4 of
    // sharp_roi[0] of the left and sharp_roi[1] of the right pushed image per slot
    bool sharp = false;
    mvsv_rect sharp_roi[2] = {};
    int64_t* dSharp = nullptr;  // [depth][2]
    int64_t* hSharp = nullptr;  // pinned, [depth][2]
    // colour frames (mvsv_stream_enable_bgr): a pushed BGR pair is staged per slot and
    // prepared into the slot's dL / dR on the lane's stream
    bool bgr = false;
    int bgrW = 0, bgrH = 0, bgr_halve = 0, bgr_variant = 0;
    size_t bgrRow = 0;            // bytes per staged row: 3 * bgrW rounded up to 4 (packed loads)
    uint8_t* dBgr_all = nullptr;  // [depth][2][bgrH][bgrRow]
};

static void bgr_free(mvsv_stream* st)
{
    for (auto& s : st->slots) {
        if (s.hBgr) (void)hipHostFree(s.hBgr);
        s.hBgr = s.dBgr = nullptr;
        s.is_bgr = false;
    }
    if (st->dBgr_all) (void)hipFree(st->dBgr_all);
    st->dBgr_all = nullptr;
    st->bgr = false;
}

static void sharpness_free(mvsv_stream* st)
{
    if (st->dSharp) (void)hipFree(st->dSharp);
    if (st->hSharp) (void)hipHostFree(st->hSharp);
    st->dSharp = nullptr;
    st->hSharp = nullptr;
    st->sharp = false;
}

static void cloud_free(mvsv_stream* st)
{
    if (st->dCloud) (void)hipFree(st->dCloud);
    if (st->dCloudHdr) (void)hipFree(st->dCloudHdr);
    if (st->hCloudHdr) (void)hipHostFree(st->hCloudHdr);
    if (st->cloud_copy) (void)hipStreamDestroy(st->cloud_copy);
    st->cloud_copy = nullptr;
    st->dCloud = nullptr;
    st->dCloudHdr = nullptr;
    st->hCloudHdr = nullptr;
    st->cloud = false;
}

static void display_free(mvsv_stream* st)
{
    if (st->dDisp) (void)hipFree(st->dDisp);
    if (st->dDispMM) (void)hipFree(st->dDispMM);
    if (st->hDisp) (void)hipHostFree(st->hDisp);
    st->dDisp = nullptr;
    st->dDispMM = nullptr;
    st->hDisp = nullptr;
    st->disp = false;
}

static void view_free(mvsv_stream* st)
{
    if (st->dView) (void)hipFree(st->dView);
    if (st->dViewMM) (void)hipFree(st->dViewMM);
    if (st->hView) (void)hipHostFree(st->hView);
    st->dView = nullptr;
    st->dViewMM = nullptr;
    st->hView = nullptr;
    st->view = false;
}

static void samplepoints_free(mvsv_stream* st)
{
    if (st->dSpVal) (void)hipFree(st->dSpVal);
    if (st->dSpCnt) (void)hipFree(st->dSpCnt);
    if (st->dSpHits) (void)hipFree(st->dSpHits);
    if (st->hSp) (void)hipHostFree(st->hSp);
    st->dSpVal = nullptr;
    st->dSpCnt = nullptr;
    st->dSpHits = nullptr;
    st->hSp = nullptr;
    st->sp = false;
}

// what mvsv_stream_create_raw adds to a stream's creation
struct RawSetup {
    const mvsv_rectification* rect;
    int cropW, cropH;
    bool resized;
};

static void stream_free(mvsv_stream* st)
{
    for (size_t i = 1; i < st->lanes.size(); i++) mvsv_destroy(st->lanes[i]);
    for (auto& s : st->slots) {
        if (s.hL) (void)hipHostFree(s.hL);
        if (s.hR) (void)hipHostFree(s.hR);
        if (s.hOut) (void)hipHostFree(s.hOut);
        if (s.hMeans) (void)hipHostFree(s.hMeans);
        if (s.hRectL) (void)hipHostFree(s.hRectL);
        if (s.hRectR) (void)hipHostFree(s.hRectR);
        for (hipEvent_t e : {s.uploaded, s.computed, s.done, s.released})
            if (e) (void)hipEventDestroy(e);
    }
    for (hipEvent_t e : {st->producer_ev, st->fence_ev})
        if (e) (void)hipEventDestroy(e);
    if (st->dL_all) (void)hipFree(st->dL_all);
    if (st->dR_all) (void)hipFree(st->dR_all);
    if (st->dOut_all) (void)hipFree(st->dOut_all);
    if (st->dMeans_all) (void)hipFree(st->dMeans_all);
    if (st->dRaw_all) (void)hipFree(st->dRaw_all);
    if (st->dMapXY) (void)hipFree(st->dMapXY);
    if (st->dMapFrac) (void)hipFree(st->dMapFrac);
    if (st->dCropL) (void)hipFree(st->dCropL);
    if (st->dCropR) (void)hipFree(st->dCropR);
    samplepoints_free(st);
    display_free(st);
    view_free(st);
    cloud_free(st);
    sharpness_free(st);
    bgr_free(st);
    if (st->rep) (void)hipHostFree(st->rep);
    if (st->up) (void)hipStreamDestroy(st->up);
    if (st->down) (void)hipStreamDestroy(st->down);
    delete st->pool;
    delete st;
}

// The display ROI of both map pairs in cv::convertMaps' form, on the device.
static bool upload_maps(mvsv_stream* st, const mvsv_rectification* r)
{
    const int cw = st->cropW, ch = st->cropH;
    const size_t ms = ((size_t)cw + 3) & ~(size_t)3, side = ms * ch;
    st->mapStride = ms;
    std::vector<int16_t> xy;
    std::vector<uint16_t> frac;
    try {
        xy.assign(side * 4, 0);
        frac.assign(side * 2, 0);
    } catch (...) {
        return false;
    }
    for (int k = 0; k < 2; k++) {
        const size_t o = (size_t)r->roi.y0 * r->map_stride + r->roi.x0;
        if (mvsv_convert_maps(r->maps[2 * k] + o, r->maps[2 * k + 1] + o, r->map_stride, cw, ch,
                              xy.data() + k * side * 2, ms, frac.data() + k * side, ms) != MVSV_OK)
            return false;
    }
    return hipMalloc((void**)&st->dMapXY, xy.size() * sizeof(int16_t)) == hipSuccess &&
           hipMalloc((void**)&st->dMapFrac, frac.size() * sizeof(uint16_t)) == hipSuccess &&
           hipMemcpy(st->dMapXY, xy.data(), xy.size() * sizeof(int16_t), hipMemcpyHostToDevice) == hipSuccess &&
           hipMemcpy(st->dMapFrac, frac.data(), frac.size() * sizeof(uint16_t), hipMemcpyHostToDevice) ==
               hipSuccess;
}

// The copy pool, once a frame's host copies are large enough to be worth splitting.
static void stream_pool(mvsv_stream* st, size_t frame_bytes)
{
    if (st->pool || frame_bytes < kPoolMinBytes) return;
    int threads = 4;
    if (const char* v = std::getenv("MVSV_STREAM_COPY_THREADS")) threads = std::max(1, std::min(16, std::atoi(v)));
    if (threads > 1) {
        try {
            st->pool = new CopyPool(threads);
        } catch (...) {
            st->pool = nullptr;  // copies on the caller's thread
        }
    }
}

// p: an SGBM stream; bp (p null): a StereoBM stream
static int stream_create(mvsv_ctx* ctx, int W, int H, const mvsv_sgbm_params* p, const mvsv_bm_params* bp, int depth,
                         const mvsv_rect* grid_roi, const RawSetup* raw, mvsv_stream** out)
{
    if (depth < 1 || depth > 64) return set_error(ctx, MVSV_E_INVALID_ARG, "stream depth must be 1..64");
    SgbmEff e{};
    BmEff be{};
    std::string why;
    int rc = p ? resolve_sgbm(p, W, H, &e, &why) : resolve_bm(bp, W, H, &be, &why);
    if (rc) return set_error(ctx, rc, why);
    if (grid_roi && (grid_roi->x0 < 0 || grid_roi->y0 < 0 || grid_roi->x1 > W || grid_roi->y1 > H ||
                     grid_roi->x1 - grid_roi->x0 < 9 || grid_roi->y1 - grid_roi->y0 < 9))
        return set_error(ctx, MVSV_E_INVALID_ARG, "grid ROI outside the image or smaller than 9x9");
    DeviceGuard dev_guard(ctx->device);
    mvsv_stream* st = new (std::nothrow) mvsv_stream();
    if (!st) return MVSV_E_OOM;
    st->ctx = ctx;
    st->lanes.push_back(ctx);
    st->W = W;
    st->H = H;
    if (p) {
        st->params = *p;
        st->eff = e;
    } else {
        st->matcher = MVSV_MATCHER_BM;
        st->bm_params = *bp;
        st->bm_eff = be;
    }
    st->grid = grid_roi != nullptr;
    if (grid_roi) st->roi = *grid_roi;
    const size_t px = (size_t)W * H;
    size_t in_px = px;  // a slot's pinned input images
    if (raw) {
        st->raw = true;
        st->rawW = raw->rect->raw_width;
        st->rawH = raw->rect->raw_height;
        st->cropW = raw->cropW;
        st->cropH = raw->cropH;
        st->factor = raw->resized ? raw->rect->factor : 0;
        st->keep = raw->rect->keep_rectified != 0;
        in_px = (size_t)st->rawW * st->rawH;
    }
    const size_t crop_px = (size_t)st->cropW * st->cropH;
    bool ok = hipStreamCreateWithFlags(&st->up, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&st->down, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&st->producer_ev, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&st->fence_ev, hipEventDisableTiming) == hipSuccess;
    st->slots.resize(depth);
    if (raw) {
        ok = ok && hipMalloc((void**)&st->dRaw_all, 2 * in_px * depth) == hipSuccess && upload_maps(st, raw->rect);
        if (raw->resized)
            ok = ok && hipMalloc((void**)&st->dCropL, crop_px * depth) == hipSuccess &&
                 hipMalloc((void**)&st->dCropR, crop_px * depth) == hipSuccess;
    }
    ok = ok && hipMalloc((void**)&st->dL_all, px * depth) == hipSuccess &&
         hipMalloc((void**)&st->dR_all, px * depth) == hipSuccess &&
         hipMalloc((void**)&st->dOut_all, px * 2 * depth) == hipSuccess &&
         hipMalloc((void**)&st->dMeans_all, 81 * sizeof(float) * depth) == hipSuccess;
    for (size_t i = 0; i < st->slots.size(); i++) {
        auto& s = st->slots[i];
        if (!ok) break;
        s.dL = st->dL_all + i * px;
        s.dR = st->dR_all + i * px;
        s.dOut = st->dOut_all + i * px;
        s.dMeans = st->dMeans_all + i * 81;
        if (raw) s.dRaw = st->dRaw_all + i * 2 * in_px;
        if (st->keep)
            ok = hipHostMalloc((void**)&s.hRectL, px, hipHostMallocDefault) == hipSuccess &&
                 hipHostMalloc((void**)&s.hRectR, px, hipHostMallocDefault) == hipSuccess;
        ok = ok && hipHostMalloc((void**)&s.hL, in_px, hipHostMallocDefault) == hipSuccess &&
             hipHostMalloc((void**)&s.hR, in_px, hipHostMallocDefault) == hipSuccess &&
             hipHostMalloc((void**)&s.hOut, px * 2, hipHostMallocDefault) == hipSuccess &&
             hipHostMalloc((void**)&s.hMeans, 81 * sizeof(float), hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&s.computed, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&s.released, hipEventDisableTiming) == hipSuccess;
    }
    ok = ok && alloc_report(ctx, depth, &st->rep, &st->rep_dev) == MVSV_OK;
    if (ok) stream_pool(st, std::max(px, in_px) * 2);
    if (!ok) {
        (void)hipGetLastError();
        stream_free(st);
        return set_error(ctx, MVSV_E_OOM, "stream slot allocation failed");
    }
    *out = st;
    return MVSV_OK;
}

int mvsv_stream_create(mvsv_ctx* ctx, int W, int H, const mvsv_sgbm_params* p, int depth,
                       const mvsv_rect* grid_roi, mvsv_stream** out)
{
    if (!ctx || !out) return MVSV_E_INVALID_ARG;
    *out = nullptr;
    return stream_create(ctx, W, H, p, nullptr, depth, grid_roi, nullptr, out);
}

int mvsv_stream_create_bm(mvsv_ctx* ctx, int W, int H, const mvsv_bm_params* p, int depth, const mvsv_rect* grid_roi,
                          mvsv_stream** out)
{
    if (!ctx || !out) return MVSV_E_INVALID_ARG;
    *out = nullptr;
    if (!p) return set_error(ctx, MVSV_E_INVALID_ARG, "null StereoBM parameters");
    return stream_create(ctx, W, H, nullptr, p, depth, grid_roi, nullptr, out);
}

static int stream_create_raw(mvsv_ctx* ctx, const mvsv_rectification* r, const mvsv_sgbm_params* p,
                             const mvsv_bm_params* bp, int depth, const mvsv_rect* grid_roi, mvsv_stream** out)
{
    if (!r) return set_error(ctx, MVSV_E_INVALID_ARG, "null rectification");
    // the kernel's tap coordinates are shorts (cv::remap's own limit)
    if (r->raw_width < 1 || r->raw_height < 1 || r->raw_width > 32767 || r->raw_height > 32767)
        return set_error(ctx, MVSV_E_INVALID_ARG, "raw frame size must be 1..32767 each way");
    for (int i = 0; i < 4; i++)
        if (!r->maps[i]) return set_error(ctx, MVSV_E_INVALID_ARG, "null map");
    if (r->map_stride < (size_t)r->raw_width)
        return set_error(ctx, MVSV_E_INVALID_ARG, "map stride smaller than the raw width");
    const mvsv_rect& q = r->roi;
    if (q.x0 < 0 || q.y0 < 0 || q.x1 > r->raw_width || q.y1 > r->raw_height || q.x1 <= q.x0 || q.y1 <= q.y0)
        return set_error(ctx, MVSV_E_INVALID_ARG, "display ROI empty or outside the raw frame");
    RawSetup raw{r, q.x1 - q.x0, q.y1 - q.y0, false};
    int W = raw.cropW, H = raw.cropH;
    if (r->factor != 0 && r->factor != 1) {
        if (resize_size(raw.cropW, raw.cropH, r->factor, r->factor, &W, &H))
            return set_error(ctx, MVSV_E_INVALID_ARG, "bad resize factor");
        raw.resized = true;
    }
    return stream_create(ctx, W, H, p, bp, depth, grid_roi, &raw, out);
}

int mvsv_stream_create_raw(mvsv_ctx* ctx, const mvsv_rectification* r, const mvsv_sgbm_params* p, int depth,
                           const mvsv_rect* grid_roi, mvsv_stream** out)
{
    if (!ctx || !out) return MVSV_E_INVALID_ARG;
    *out = nullptr;
    return stream_create_raw(ctx, r, p, nullptr, depth, grid_roi, out);
}

int mvsv_stream_create_raw_bm(mvsv_ctx* ctx, const mvsv_rectification* r, const mvsv_bm_params* p, int depth,
                              const mvsv_rect* grid_roi, mvsv_stream** out)
{
    if (!ctx || !out) return MVSV_E_INVALID_ARG;
    *out = nullptr;
    if (!p) return set_error(ctx, MVSV_E_INVALID_ARG, "null StereoBM parameters");
    return stream_create_raw(ctx, r, nullptr, p, depth, grid_roi, out);
}

int mvsv_stream_matcher(const mvsv_stream* st) { return st ? st->matcher : -1; }

int mvsv_stream_size(const mvsv_stream* st, int* width, int* height)
{
    if (!st || !width || !height) return MVSV_E_INVALID_ARG;
    *width = st->W;
    *height = st->H;
    return MVSV_OK;
}

// A raw stream's run of n slots from slot i0: the raw pairs rectified into the
// slots' dL / dR on the lane's stream -- through the crop buffer and cv::resize
// with a factor.
static int stream_rectify(mvsv_stream* st, mvsv_ctx* ctx, long i0, int n)
{
    const size_t px = (size_t)st->W * st->H, crop_px = (size_t)st->cropW * st->cropH;
    auto& first = st->slots[i0];
    if (!st->dCropL)
        return rectify_pair_device(ctx, n, first.dRaw, st->rawW, st->rawH, st->dMapXY, st->dMapFrac, st->mapStride,
                                   st->cropW, st->cropH, first.dL, first.dR, st->W, px);
    uint8_t *cL = st->dCropL + i0 * crop_px, *cR = st->dCropR + i0 * crop_px;
    int rc;
    if ((rc = rectify_pair_device(ctx, n, first.dRaw, st->rawW, st->rawH, st->dMapXY, st->dMapFrac, st->mapStride,
                                  st->cropW, st->cropH, cL, cR, st->cropW, crop_px)) ||
        (rc = resize_device(ctx, n, cL, st->cropW, crop_px, st->cropW, st->cropH, st->factor, st->factor, first.dL,
                            st->W, px)))
        return rc;
    return resize_device(ctx, n, cR, st->cropW, crop_px, st->cropW, st->cropH, st->factor, st->factor, first.dR,
                         st->W, px);
}

// The frames of a run that were pushed as BGR: their grey pairs into the slots'
// dL / dR on the lane's stream, one launch per side and stretch of such slots.
static int stream_prepare(mvsv_stream* st, mvsv_ctx* ctx, long i0, int n)
{
    const size_t px = (size_t)st->W * st->H, side = (size_t)st->bgrH * st->bgrRow;
    for (int k = 0; k < n;) {
        if (!st->slots[i0 + k].is_bgr) {
            k++;
            continue;
        }
        int m = 1;
        while (k + m < n && st->slots[i0 + k + m].is_bgr) m++;
        auto& s = st->slots[i0 + k];
        int rc;
        if ((rc = prepare_gray_device(ctx, m, s.dBgr, st->bgrRow, 2 * side, st->bgrW, st->bgrH, st->bgr_halve,
                                      st->bgr_variant, s.dL, st->W, px)) ||
            (rc = prepare_gray_device(ctx, m, s.dBgr + side, st->bgrRow, 2 * side, st->bgrW, st->bgrH, st->bgr_halve,
                                      st->bgr_variant, s.dR, st->W, px)))
            return rc;
        k += m;
    }
    return MVSV_OK;
}

// Enqueue compute + download for the pushed frames [launched, head): one
// frame-batch launch per run of consecutive slots (a run ends at the ring's end).
static int stream_launch(mvsv_stream* st)
{
    const int W = st->W, H = st->H;
    const size_t px = (size_t)W * H;
    const long depth = (long)st->slots.size();
    int rc;
    RingRun run;
    while (ring_next_run(st->launched, st->head, depth, &run)) {
        const long i0 = run.i0;
        const int n = run.n;
        auto& first = st->slots[i0];
        auto& last = st->slots[i0 + n - 1];
        mvsv_ctx* ctx = st->lanes[st->runs % (long)st->lanes.size()];
        // the upload stream is in order: the last slot's upload covers the run
        if ((rc = check_hip(ctx, hipStreamWaitEvent(ctx->stream, last.uploaded, 0), "stream wait")))
            return rc;
        // a slot whose map pop_device is still copying on the consumer's stream
        for (int k = 0; k < n; k++) {
            auto& s = st->slots[i0 + k];
            if (!s.release_pending) continue;
            if ((rc = check_hip(ctx, hipStreamWaitEvent(ctx->stream, s.released, 0), "stream wait"))) return rc;
            s.release_pending = false;
        }
        // slot i0 was popped (or never used): nothing reads rep[i0] any more
        __atomic_store_n(&st->rep[i0], 0, __ATOMIC_RELEASE);
        first.run_len = n;
        int* prev_target = ctx->report_target;
        ctx->report_target = st->rep_dev + i0;
        int status = st->raw ? stream_rectify(st, ctx, i0, n) : st->bgr ? stream_prepare(st, ctx, i0, n) : MVSV_OK;
        if (status == MVSV_OK)
            status = st->matcher == MVSV_MATCHER_BM
                         ? bm_device(ctx, n, first.dL, W, px, first.dR, W, px, W, H, st->bm_eff, first.dOut, W, px)
                         : sgbm_device(ctx, n, first.dL, W, px, first.dR, W, px, W, H, st->eff, first.dOut, W, px);
        ctx->report_target = prev_target;
        if (status == MVSV_OK && st->grid) {
            const mvsv_rect& q = st->roi;
            status = mean_grid_device(ctx, n, first.dOut + (size_t)q.y0 * W + q.x0, W, px, q.x1 - q.x0,
                                      q.y1 - q.y0, first.dMeans);
        }
        if (status == MVSV_OK && st->sp && st->sp_npts > 0) {
            const mvsv_rect& q = st->sp_roi;
            const int rw = q.x1 - q.x0, rh = q.y1 - q.y0;
            float* vals = st->dSpVal + (size_t)i0 * st->sp_npts;
            status = sample_grid_device(ctx, n, first.dOut + (size_t)q.y0 * W + q.x0, W, px, rw, rh, st->sp_radius,
                                        vals);
            if (status == MVSV_OK)
                status = sample_detect_device(ctx, n, vals, rw, rh, st->sp_Q, st->sp_first, st->sp_second,
                                              st->sp_max, st->dSpCnt + i0, st->dSpHits + (size_t)i0 * st->sp_max);
        }
        if (status == MVSV_OK && st->disp) {
            const mvsv_rect& q = st->disp_roi;
            const int rw = q.x1 - q.x0, rh = q.y1 - q.y0;
            status = normalize_minmax_device(ctx, n, first.dOut + (size_t)q.y0 * W + q.x0, W, px, rw, rh,
                                             st->disp_alpha, st->disp_beta, st->dDisp + (size_t)i0 * st->disp_px, rw,
                                             st->disp_px, st->dDispMM + 2 * i0);
        }
        if (status == MVSV_OK && st->view) {  // after the mean grid and the lattice: it reads both
            const mvsv_rect& q = st->view_roi;
            const int rw = q.x1 - q.x0, rh = q.y1 - q.y0;
            mvsv_view_spec spec = st->view_spec;
            spec.means = first.dMeans;
            spec.values = st->dSpVal ? st->dSpVal + (size_t)i0 * st->sp_npts : nullptr;
            spec.point_first = st->sp_first;
            spec.point_second = st->sp_second;
            status = view_device(ctx, n, first.dOut + (size_t)q.y0 * W + q.x0, W, px, rw, rh, spec,
                                 st->dView + (size_t)i0 * st->view_bytes, 3 * (size_t)rw, st->view_bytes,
                                 st->dViewMM + 2 * i0);
        }
        if (status == MVSV_OK && st->cloud) {
            const mvsv_rect& q = st->cloud_roi;
            status = point_cloud_device(ctx, n, first.dOut + (size_t)q.y0 * W + q.x0, W, px, q.x1 - q.x0, q.y1 - q.y0,
                                        st->cloud_Q, st->dCloud + (size_t)i0 * st->cloud_max, st->cloud_max,
                                        st->dCloudHdr + 3 * i0, 3, st->dCloudHdr + 3 * i0 + 1, 3);
        }
        if (status == MVSV_OK && st->sharp) {
            // the pushed pair: a raw slot holds it as [2][rawH][rawW]
            const int iw = st->raw ? st->rawW : W, ih = st->raw ? st->rawH : H;
            const size_t ipx = (size_t)iw * ih;
            const uint8_t* pl = st->raw ? first.dRaw : first.dL;
            const uint8_t* pr = st->raw ? first.dRaw + ipx : first.dR;
            const size_t ifs = st->raw ? 2 * ipx : ipx;
            status = sharpness_device(ctx, n, pl, iw, ifs, iw, ih, st->sharp_roi[0], st->dSharp + 2 * i0, 2);
            if (status == MVSV_OK)
                status = sharpness_device(ctx, n, pr, iw, ifs, iw, ih, st->sharp_roi[1], st->dSharp + 2 * i0 + 1, 2);
        }
        if (status != MVSV_OK && ctx != st->ctx) st->ctx->err = ctx->err;  // reported by pop
        st->runs++;
        if ((rc = mark_last_use(ctx, MVSV_OK)) ||
            (rc = check_hip(ctx, hipEventRecord(last.computed, ctx->stream), "stream event")) ||
            (rc = check_hip(ctx, hipStreamWaitEvent(st->down, last.computed, 0), "stream wait"))) {
            if (ctx != st->ctx) st->ctx->err = ctx->err;
            return rc;
        }
        for (int k = 0; k < n; k++) {
            auto& s = st->slots[i0 + k];
            s.status = status;
            mvsv_ctx* c = st->ctx;
            if ((st->host_mask & MVSV_HOST_MAP) &&
                (rc = check_hip(c, hipMemcpyAsync(s.hOut, s.dOut, px * 2, hipMemcpyDeviceToHost, st->down),
                                "stream D2H")))
                return rc;
            if (st->grid &&
                (rc = check_hip(c, hipMemcpyAsync(s.hMeans, s.dMeans, 81 * sizeof(float),
                                                  hipMemcpyDeviceToHost, st->down), "stream D2H")))
                return rc;
            if (st->keep && (st->host_mask & MVSV_HOST_RECTIFIED) &&
                ((rc = check_hip(c, hipMemcpyAsync(s.hRectL, s.dL, px, hipMemcpyDeviceToHost, st->down),
                                 "stream D2H")) ||
                 (rc = check_hip(c, hipMemcpyAsync(s.hRectR, s.dR, px, hipMemcpyDeviceToHost, st->down),
                                 "stream D2H"))))
                return rc;
            if (st->sp && st->sp_npts > 0) {
                // values, count and hit records are adjacent in the pinned slot
                const long i = i0 + k;
                if ((rc = check_hip(c, hipMemcpyAsync(st->sp_values(i), st->dSpVal + (size_t)i * st->sp_npts,
                                                      (size_t)st->sp_npts * sizeof(float), hipMemcpyDeviceToHost,
                                                      st->down), "stream D2H")) ||
                    (rc = check_hip(c, hipMemcpyAsync(st->sp_count(i), st->dSpCnt + i, sizeof(int),
                                                      hipMemcpyDeviceToHost, st->down), "stream D2H")) ||
                    (rc = check_hip(c, hipMemcpyAsync(st->sp_hits(i), st->dSpHits + (size_t)i * st->sp_max,
                                                      (size_t)st->sp_max * sizeof(mvsv_sample_hit),
                                                      hipMemcpyDeviceToHost, st->down), "stream D2H")))
                    return rc;
            }
            if (st->disp) {
                const long i = i0 + k;
                if (((st->host_mask & MVSV_HOST_DISPLAY) &&
                     (rc = check_hip(c, hipMemcpyAsync(st->disp_map(i), st->dDisp + (size_t)i * st->disp_px, st->disp_px,
                                                       hipMemcpyDeviceToHost, st->down), "stream D2H"))) ||
                    (rc = check_hip(c, hipMemcpyAsync(st->disp_minmax(i), st->dDispMM + 2 * i, 2 * sizeof(int16_t),
                                                      hipMemcpyDeviceToHost, st->down), "stream D2H")))
                    return rc;
            }
            if (st->view) {
                const long i = i0 + k;
                if (((st->host_mask & MVSV_HOST_VIEW) &&
                     (rc = check_hip(c, hipMemcpyAsync(st->view_img(i), st->dView + (size_t)i * st->view_bytes,
                                                       st->view_bytes, hipMemcpyDeviceToHost, st->down), "stream D2H"))) ||
                    (rc = check_hip(c, hipMemcpyAsync(st->view_minmax(i), st->dViewMM + 2 * i, 2 * sizeof(int16_t),
                                                      hipMemcpyDeviceToHost, st->down), "stream D2H")))
                    return rc;
            }
            if (st->cloud &&  // the header only: the records wait on the device for front_cloud
                (rc = check_hip(c, hipMemcpyAsync(st->hCloudHdr + 3 * (i0 + k), st->dCloudHdr + 3 * (i0 + k),
                                                  3 * sizeof(int), hipMemcpyDeviceToHost, st->down), "stream D2H")))
                return rc;
            if (st->sharp &&
                (rc = check_hip(c, hipMemcpyAsync(st->hSharp + 2 * (i0 + k), st->dSharp + 2 * (i0 + k),
                                                  2 * sizeof(int64_t), hipMemcpyDeviceToHost, st->down), "stream D2H")))
                return rc;
            if ((rc = check_hip(c, hipEventRecord(s.done, st->down), "stream event"))) return rc;
        }
        st->launched += n;
    }
    return MVSV_OK;
}

int mvsv_stream_set_batch(mvsv_stream* st, int batch)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (batch < 1 || batch > (int)st->slots.size())
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "stream batch must be 1..depth");
    DeviceGuard dev_guard(st->ctx->device);
    int rc = stream_launch(st);  // frames already pushed keep the old grouping
    if (rc) return rc;
    st->batch = batch;
    return MVSV_OK;
}

// The stream's own lanes follow the caller context's kernel options.
static void copy_options(mvsv_ctx* d, const mvsv_ctx* s)
{
    d->spin_limit = s->spin_limit;
    d->path16 = s->path16;
    d->cost2 = s->cost2;
    d->cost_fixed_pp = s->cost_fixed_pp;
    d->cost_ty = s->cost_ty;
    d->tri = s->tri;
    d->path_sched = s->path_sched;
    d->strip_waves = s->strip_waves;
    d->cost_res = s->cost_res;
    d->lines_aux = s->lines_aux;
    d->strip_tickets = s->strip_tickets;
    d->bm2 = s->bm2;
    d->bm_ty = s->bm_ty;
    d->bitslice = s->bitslice;
    d->bs_groups = s->bs_groups;
    d->bs_serial = s->bs_serial;
    d->cost_xcd = s->cost_xcd;
    d->bs_fuse = s->bs_fuse;
}

int mvsv_stream_set_inflight(mvsv_stream* st, int n)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (n < 1 || n > kStreamMaxInflight)
        return set_error(ctx, MVSV_E_INVALID_ARG, "stream launches in flight must be 1..4");
    DeviceGuard dev_guard(ctx->device);
    int rc = stream_launch(st);  // frames already pushed keep the old lanes
    if (rc) return rc;
    while ((int)st->lanes.size() < n) {
        mvsv_ctx* c = nullptr;
        if ((rc = mvsv_create(&c, ctx->device))) return set_error(ctx, rc, "stream lane context creation failed");
        copy_options(c, ctx);
        st->lanes.push_back(c);
        if (st->fenced && (rc = check_hip(ctx, hipStreamWaitEvent(c->stream, st->fence_ev, 0), "stream wait")))
            return rc;
    }
    while ((int)st->lanes.size() > n) {  // mvsv_destroy waits for the lane's work
        mvsv_destroy(st->lanes.back());
        st->lanes.pop_back();
    }
    st->runs = 0;
    return MVSV_OK;
}

int mvsv_stream_set_params(mvsv_stream* st, const mvsv_sgbm_params* p)
{
    if (!st) return MVSV_E_INVALID_ARG;
    SgbmEff e;
    std::string why;
    int rc = resolve_sgbm(p, st->W, st->H, &e, &why);
    if (rc) return set_error(st->ctx, rc, why);
    DeviceGuard dev_guard(st->ctx->device);
    if ((rc = stream_launch(st))) return rc;  // pending frames keep the old parameters
    st->params = *p;  // applies to frames pushed from now on (trgt/mean_test.cpp:348 setters)
    st->eff = e;
    st->matcher = MVSV_MATCHER_SGBM;
    return MVSV_OK;
}

int mvsv_stream_set_bm_params(mvsv_stream* st, const mvsv_bm_params* p)
{
    if (!st) return MVSV_E_INVALID_ARG;
    BmEff e;
    std::string why;
    int rc = resolve_bm(p, st->W, st->H, &e, &why);
    if (rc) return set_error(st->ctx, rc, why);
    DeviceGuard dev_guard(st->ctx->device);
    if ((rc = stream_launch(st))) return rc;  // pending frames keep their matcher and parameters
    st->bm_params = *p;
    st->bm_eff = e;
    st->matcher = MVSV_MATCHER_BM;
    return MVSV_OK;
}

int mvsv_stream_pending(const mvsv_stream* st) { return st ? (int)(st->head - st->tail) : 0; }

int mvsv_stream_push(mvsv_stream* st, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (st->raw) return set_error(ctx, MVSV_E_INVALID_ARG, "raw stream: push raw pairs with mvsv_stream_push_raw");
    if (!L || !R || ls < (size_t)st->W || rs < (size_t)st->W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "null frame or stride smaller than width");
    if (ring_full(st->head, st->tail, (long)st->slots.size()))
        return set_error(ctx, MVSV_E_INVALID_ARG, "stream full: pop a frame first");
    DeviceGuard dev_guard(ctx->device);
    auto& s = st->slots[st->head % st->slots.size()];
    s.is_bgr = false;
    const int W = st->W, H = st->H;
    // the slot's previous frame was popped, so its copies are complete
    auto copy_in = [&](int part, int parts) {
        copy_rows(s.hL, W, L, ls, W, H, part, parts);
        copy_rows(s.hR, W, R, rs, W, H, part, parts);
    };
    if (st->pool)
        st->pool->run(copy_in);
    else
        copy_in(0, 1);
    const size_t px = (size_t)W * H;
    int rc;
    if ((rc = check_hip(ctx, hipMemcpyAsync(s.dL, s.hL, px, hipMemcpyHostToDevice, st->up), "stream H2D")) ||
        (rc = check_hip(ctx, hipMemcpyAsync(s.dR, s.hR, px, hipMemcpyHostToDevice, st->up), "stream H2D")) ||
        (rc = check_hip(ctx, hipEventRecord(s.uploaded, st->up), "stream event")))
        return rc;
    st->head++;
    // a full group, or a group that would otherwise wrap past the ring's end
    if (ring_launch_after_push(st->head, st->launched, st->batch, (long)st->slots.size()))
        return stream_launch(st);
    return MVSV_OK;
}

int mvsv_stream_disable_bgr(mvsv_stream* st)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (st->head != st->tail)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "colour input changes only while no frame is pending");
    DeviceGuard dev_guard(st->ctx->device);
    bgr_free(st);  // every frame was popped: nothing in flight uses the buffers
    return MVSV_OK;
}

int mvsv_stream_enable_bgr(mvsv_stream* st, int sw, int sh, int halve, int variant)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (st->raw) return set_error(ctx, MVSV_E_INVALID_ARG, "colour input is for streams of rectified pairs");
    if (st->head != st->tail)
        return set_error(ctx, MVSV_E_INVALID_ARG, "colour input changes only while no frame is pending");
    int dw, dh;
    if (prepare_size(sw, sh, halve, &dw, &dh) || dw != st->W || dh != st->H)
        return set_error(ctx, MVSV_E_INVALID_ARG, "mvsv_prepare_size of the colour frame is not the stream's size");
    if (variant != MVSV_GRAY_Q14 && variant != MVSV_GRAY_Q15)
        return set_error(ctx, MVSV_E_INVALID_ARG, "unknown grey variant");
    DeviceGuard dev_guard(ctx->device);
    bgr_free(st);
    st->bgrW = sw;
    st->bgrH = sh;
    st->bgr_halve = halve;
    st->bgr_variant = variant;
    st->bgrRow = (3 * (size_t)sw + 3) & ~(size_t)3;
    const size_t pair = 2 * (size_t)sh * st->bgrRow;
    bool ok = hipMalloc((void**)&st->dBgr_all, pair * st->slots.size()) == hipSuccess;
    for (size_t i = 0; ok && i < st->slots.size(); i++) {
        st->slots[i].dBgr = st->dBgr_all + i * pair;
        ok = hipHostMalloc((void**)&st->slots[i].hBgr, pair, hipHostMallocDefault) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        bgr_free(st);
        return set_error(ctx, MVSV_E_OOM, "colour staging allocation failed");
    }
    stream_pool(st, pair);
    st->bgr = true;
    return MVSV_OK;
}

int mvsv_stream_push_bgr(mvsv_stream* st, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (st->raw) return set_error(ctx, MVSV_E_INVALID_ARG, "raw stream: push raw pairs with mvsv_stream_push_raw");
    if (!st->bgr) return set_error(ctx, MVSV_E_INVALID_ARG, "colour input is not enabled on this stream");
    const size_t row = 3 * (size_t)st->bgrW;
    if (!L || !R || ls < row || rs < row)
        return set_error(ctx, MVSV_E_INVALID_ARG, "null frame or stride smaller than three times the width");
    if (ring_full(st->head, st->tail, (long)st->slots.size()))
        return set_error(ctx, MVSV_E_INVALID_ARG, "stream full: pop a frame first");
    DeviceGuard dev_guard(ctx->device);
    auto& s = st->slots[st->head % st->slots.size()];
    const int H = st->bgrH;
    const size_t side = (size_t)H * st->bgrRow;
    // the slot's previous frame was popped, so its copies and its preparation are complete
    auto copy_in = [&](int part, int parts) {
        copy_rows(s.hBgr, st->bgrRow, L, ls, row, H, part, parts);
        copy_rows(s.hBgr + side, st->bgrRow, R, rs, row, H, part, parts);
    };
    if (st->pool)
        st->pool->run(copy_in);
    else
        copy_in(0, 1);
    int rc;
    if ((rc = check_hip(ctx, hipMemcpyAsync(s.dBgr, s.hBgr, 2 * side, hipMemcpyHostToDevice, st->up), "stream H2D")) ||
        (rc = check_hip(ctx, hipEventRecord(s.uploaded, st->up), "stream event")))
        return rc;
    s.is_bgr = true;
    st->head++;
    if (ring_launch_after_push(st->head, st->launched, st->batch, (long)st->slots.size()))
        return stream_launch(st);
    return MVSV_OK;
}

int mvsv_stream_push_raw(mvsv_stream* st, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!st->raw)
        return set_error(ctx, MVSV_E_INVALID_ARG, "stream of rectified pairs: push them with mvsv_stream_push");
    const int W = st->rawW, H = st->rawH;
    if (!L || !R || ls < (size_t)W || rs < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "null frame or stride smaller than the raw width");
    if (ring_full(st->head, st->tail, (long)st->slots.size()))
        return set_error(ctx, MVSV_E_INVALID_ARG, "stream full: pop a frame first");
    DeviceGuard dev_guard(ctx->device);
    auto& s = st->slots[st->head % st->slots.size()];
    // the slot's previous frame was popped, so its copies and its rectification are complete
    auto copy_in = [&](int part, int parts) {
        copy_rows(s.hL, W, L, ls, W, H, part, parts);
        copy_rows(s.hR, W, R, rs, W, H, part, parts);
    };
    if (st->pool)
        st->pool->run(copy_in);
    else
        copy_in(0, 1);
    const size_t px = (size_t)W * H;
    int rc;
    if ((rc = check_hip(ctx, hipMemcpyAsync(s.dRaw, s.hL, px, hipMemcpyHostToDevice, st->up), "stream H2D")) ||
        (rc = check_hip(ctx, hipMemcpyAsync(s.dRaw + px, s.hR, px, hipMemcpyHostToDevice, st->up), "stream H2D")) ||
        (rc = check_hip(ctx, hipEventRecord(s.uploaded, st->up), "stream event")))
        return rc;
    st->head++;
    if (ring_launch_after_push(st->head, st->launched, st->batch, (long)st->slots.size()))
        return stream_launch(st);
    return MVSV_OK;
}

// Wait for the oldest pending frame and release its slot: its status, and the
// slot whose pinned map / means hold the result (valid until the slot's reuse).
static int stream_pop_slot(mvsv_stream* st, mvsv_stream::Slot** slot)
{
    mvsv_ctx* ctx = st->ctx;
    if (st->head == st->tail) return set_error(ctx, MVSV_E_INVALID_ARG, "stream empty");
    auto& s = st->slots[st->tail % st->slots.size()];
    *slot = &s;
    int rc = MVSV_OK;
    if (st->tail >= st->launched && (rc = stream_launch(st))) return rc;  // partial group
    rc = check_hip(ctx, hipEventSynchronize(s.done), "stream sync");
    const long idx = st->tail % (long)st->slots.size();
    st->tail++;
    if (rc) return rc;
    if (s.run_len > 0) {  // first frame of its launch: that launch has completed
        const bool gave_up = __atomic_exchange_n(&st->rep[idx], 0, __ATOMIC_ACQ_REL) != 0;
        for (int k = 0; k < s.run_len; k++) st->slots[idx + k].gave_up = gave_up;
        s.run_len = 0;
    }
    if (s.status) return s.status;
    if (s.gave_up) {
        s.gave_up = false;
        return set_error(ctx, MVSV_E_TIMEOUT,
                         "stream frame: a strip-boundary wait of its SGBM launch gave up");
    }
    return MVSV_OK;
}

static void stream_means(const mvsv_stream* st, const mvsv_stream::Slot& s, float* means)
{
    if (!means) return;
    if (st->grid)
        std::memcpy(means, s.hMeans, 81 * sizeof(float));
    else
        std::memset(means, 0, 81 * sizeof(float));
}

int mvsv_stream_pop_pair(mvsv_stream* st, int16_t* out, size_t os, float* means, uint8_t* rl, size_t rls,
                         uint8_t* rr, size_t rrs)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (out && os < (size_t)st->W) return set_error(st->ctx, MVSV_E_INVALID_ARG, "stride smaller than width");
    if ((rl || rr) && !st->keep)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the stream was not created with keep_rectified");
    if ((rl && rls < (size_t)st->W) || (rr && rrs < (size_t)st->W))
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "stride smaller than width");
    if (out && !(st->host_mask & MVSV_HOST_MAP))
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the host map is switched off (mvsv_stream_set_host_outputs)");
    if ((rl || rr) && !(st->host_mask & MVSV_HOST_RECTIFIED))
        return set_error(st->ctx, MVSV_E_INVALID_ARG,
                         "the host rectified pair is switched off (mvsv_stream_set_host_outputs)");
    DeviceGuard dev_guard(st->ctx->device);
    mvsv_stream::Slot* sp = nullptr;
    int rc = stream_pop_slot(st, &sp);
    if (rc) return rc;
    const auto& s = *sp;
    if (out || rl || rr) {
        auto copy_out = [&](int part, int parts) {
            if (out)
                copy_rows((uint8_t*)out, os * 2, (const uint8_t*)s.hOut, (size_t)st->W * 2, (size_t)st->W * 2,
                          st->H, part, parts);
            if (rl) copy_rows(rl, rls, s.hRectL, (size_t)st->W, (size_t)st->W, st->H, part, parts);
            if (rr) copy_rows(rr, rrs, s.hRectR, (size_t)st->W, (size_t)st->W, st->H, part, parts);
        };
        if (st->pool)
            st->pool->run(copy_out);
        else
            copy_out(0, 1);
    }
    stream_means(st, s, means);
    return MVSV_OK;
}

int mvsv_stream_pop(mvsv_stream* st, int16_t* out, size_t os, float* means)
{
    return mvsv_stream_pop_pair(st, out, os, means, nullptr, 0, nullptr, 0);
}

int mvsv_stream_pop_view(mvsv_stream* st, const int16_t** map, float* means)
{
    if (!st || !map) return MVSV_E_INVALID_ARG;
    *map = nullptr;
    if (!(st->host_mask & MVSV_HOST_MAP))
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the host map is switched off (mvsv_stream_set_host_outputs)");
    DeviceGuard dev_guard(st->ctx->device);
    mvsv_stream::Slot* sp = nullptr;
    int rc = stream_pop_slot(st, &sp);
    if (rc) return rc;
    *map = sp->hOut;
    stream_means(st, *sp, means);
    return MVSV_OK;
}

static bool view_uses_samplepoints(const mvsv_stream* st)
{
    return st->view && (st->view_spec.layers & MVSV_VIEW_FOUND_POINTS);
}

int mvsv_stream_disable_samplepoints(mvsv_stream* st)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (st->head != st->tail)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "sample points change only while no frame is pending");
    if (view_uses_samplepoints(st))
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the view draws the found points: disable the view first");
    DeviceGuard dev_guard(st->ctx->device);
    samplepoints_free(st);  // every frame was popped: nothing in flight uses the buffers
    return MVSV_OK;
}

int mvsv_stream_enable_samplepoints(mvsv_stream* st, const mvsv_rect* roi, int radius, const float* Q, float first,
                                    float second, int max_hits)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!Q) return set_error(ctx, MVSV_E_INVALID_ARG, "null Q");
    if (st->head != st->tail)
        return set_error(ctx, MVSV_E_INVALID_ARG, "sample points change only while no frame is pending");
    const mvsv_rect q = roi ? *roi : mvsv_rect{0, 0, st->W, st->H};
    if (q.x0 < 0 || q.y0 < 0 || q.x1 > st->W || q.y1 > st->H || q.x1 <= q.x0 || q.y1 <= q.y0)
        return set_error(ctx, MVSV_E_INVALID_ARG, "sample point ROI empty or outside the image");
    if (view_uses_samplepoints(st) && !(q.x0 == st->view_roi.x0 && q.y0 == st->view_roi.y0 && q.x1 == st->view_roi.x1 &&
                                        q.y1 == st->view_roi.y1))
        return set_error(ctx, MVSV_E_INVALID_ARG, "the view draws the found points of its own ROI: disable the view first");
    int sx, sy, nx, ny;
    sample_layout(q.x1 - q.x0, q.y1 - q.y0, &sx, &sy, &nx, &ny);
    const int npts = nx * ny;
    if (npts > 0 && (radius < 0 || radius >= std::min(sx, sy)))
        return set_error(ctx, MVSV_E_INVALID_ARG, "sample point radius must be 0 .. min(step_x, step_y) - 1");
    DeviceGuard dev_guard(ctx->device);
    samplepoints_free(st);
    st->sp_roi = q;
    st->sp_radius = radius;
    st->sp_npts = npts;
    st->sp_max = max_hits <= 0 ? npts : std::min(max_hits, npts);
    std::memcpy(st->sp_Q, Q, sizeof(st->sp_Q));
    st->sp_first = first;
    st->sp_second = second;
    const size_t depth = st->slots.size();
    st->sp_slot_bytes = ((size_t)npts * sizeof(float) + sizeof(int) + (size_t)st->sp_max * sizeof(mvsv_sample_hit) + 15) &
                        ~(size_t)15;
    if (npts > 0) {
        const bool ok = hipMalloc((void**)&st->dSpVal, depth * npts * sizeof(float)) == hipSuccess &&
                        hipMalloc((void**)&st->dSpCnt, depth * sizeof(int)) == hipSuccess &&
                        hipMalloc((void**)&st->dSpHits, depth * st->sp_max * sizeof(mvsv_sample_hit)) == hipSuccess &&
                        hipHostMalloc((void**)&st->hSp, depth * st->sp_slot_bytes, hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            samplepoints_free(st);
            return set_error(ctx, MVSV_E_OOM, "sample point buffer allocation failed");
        }
    }
    st->sp = true;
    return MVSV_OK;
}

int mvsv_stream_front_samples(mvsv_stream* st, float* values, int* count, mvsv_sample_hit* hits, int capacity)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!st->sp) return set_error(ctx, MVSV_E_INVALID_ARG, "sample points are not enabled on this stream");
    if (st->head == st->tail) return set_error(ctx, MVSV_E_INVALID_ARG, "stream empty");
    if (hits && capacity < 0) return set_error(ctx, MVSV_E_INVALID_ARG, "negative capacity");
    DeviceGuard dev_guard(ctx->device);
    const long idx = st->tail % (long)st->slots.size();
    auto& s = st->slots[idx];
    int rc;
    if (st->tail >= st->launched && (rc = stream_launch(st))) return rc;  // partial group
    if ((rc = check_hip(ctx, hipEventSynchronize(s.done), "stream sync"))) return rc;
    if (s.status) return s.status;
    // the report word is left for pop to read and clear
    if (s.gave_up || (s.run_len > 0 && __atomic_load_n(&st->rep[idx], __ATOMIC_ACQUIRE) != 0))
        return set_error(ctx, MVSV_E_TIMEOUT, "stream frame: a strip-boundary wait of its SGBM launch gave up");
    if (st->sp_npts == 0) {
        if (count) *count = 0;
        return MVSV_OK;
    }
    const int total = *st->sp_count(idx);
    if (values) std::memcpy(values, st->sp_values(idx), (size_t)st->sp_npts * sizeof(float));
    if (count) *count = total;
    if (hits)
        std::memcpy(hits, st->sp_hits(idx),
                    (size_t)std::min(std::min(total, st->sp_max), capacity) * sizeof(mvsv_sample_hit));
    return MVSV_OK;
}

int mvsv_stream_disable_display(mvsv_stream* st)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (st->head != st->tail)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the display changes only while no frame is pending");
    DeviceGuard dev_guard(st->ctx->device);
    display_free(st);  // every frame was popped: nothing in flight uses the buffers
    return MVSV_OK;
}

int mvsv_stream_enable_display(mvsv_stream* st, const mvsv_rect* roi, double alpha, double beta)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!std::isfinite(alpha) || !std::isfinite(beta))
        return set_error(ctx, MVSV_E_INVALID_ARG, "display alpha / beta must be finite");
    if (st->head != st->tail)
        return set_error(ctx, MVSV_E_INVALID_ARG, "the display changes only while no frame is pending");
    const mvsv_rect q = roi ? *roi : mvsv_rect{0, 0, st->W, st->H};
    if (q.x0 < 0 || q.y0 < 0 || q.x1 > st->W || q.y1 > st->H || q.x1 <= q.x0 || q.y1 <= q.y0)
        return set_error(ctx, MVSV_E_INVALID_ARG, "display ROI empty or outside the image");
    DeviceGuard dev_guard(ctx->device);
    display_free(st);
    st->disp_roi = q;
    st->disp_alpha = alpha;
    st->disp_beta = beta;
    st->disp_px = (size_t)(q.x1 - q.x0) * (q.y1 - q.y0);
    st->disp_slot_bytes = (((st->disp_px + 1) & ~(size_t)1) + 2 * sizeof(int16_t) + 15) & ~(size_t)15;
    const size_t depth = st->slots.size();
    const bool ok = hipMalloc((void**)&st->dDisp, depth * st->disp_px) == hipSuccess &&
                    hipMalloc((void**)&st->dDispMM, depth * 2 * sizeof(int16_t)) == hipSuccess &&
                    hipHostMalloc((void**)&st->hDisp, depth * st->disp_slot_bytes, hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        display_free(st);
        return set_error(ctx, MVSV_E_OOM, "display buffer allocation failed");
    }
    st->disp = true;
    return MVSV_OK;
}

// the oldest pending frame, complete: its slot index in *idx
static int front_slot(mvsv_stream* st, bool enabled, const char* not_enabled, long* idx)
{
    mvsv_ctx* ctx = st->ctx;
    if (!enabled) return set_error(ctx, MVSV_E_INVALID_ARG, not_enabled);
    if (st->head == st->tail) return set_error(ctx, MVSV_E_INVALID_ARG, "stream empty");
    *idx = st->tail % (long)st->slots.size();
    auto& s = st->slots[*idx];
    int rc;
    if (st->tail >= st->launched && (rc = stream_launch(st))) return rc;  // partial group
    if ((rc = check_hip(ctx, hipEventSynchronize(s.done), "stream sync"))) return rc;
    if (s.status) return s.status;
    // the report word is left for pop to read and clear
    if (s.gave_up || (s.run_len > 0 && __atomic_load_n(&st->rep[*idx], __ATOMIC_ACQUIRE) != 0))
        return set_error(ctx, MVSV_E_TIMEOUT, "stream frame: a strip-boundary wait of its SGBM launch gave up");
    return MVSV_OK;
}

static int display_front(mvsv_stream* st, long* idx, bool host = true)
{
    if (host && st->disp && !(st->host_mask & MVSV_HOST_DISPLAY))
        return set_error(st->ctx, MVSV_E_INVALID_ARG,
                         "the host display map is switched off (mvsv_stream_set_host_outputs)");
    return front_slot(st, st->disp, "the display is not enabled on this stream", idx);
}

int mvsv_stream_front_display(mvsv_stream* st, uint8_t* out, size_t out_stride, int16_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    const int rw = st->disp_roi.x1 - st->disp_roi.x0, rh = st->disp_roi.y1 - st->disp_roi.y0;
    if (st->disp && out && out_stride < (size_t)rw)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "display stride smaller than the ROI's width");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = display_front(st, &idx))) return rc;
    if (out) copy_rows(out, out_stride, st->disp_map(idx), (size_t)rw, (size_t)rw, rh, 0, 1);
    if (minmax) std::memcpy(minmax, st->disp_minmax(idx), 2 * sizeof(int16_t));
    return MVSV_OK;
}

int mvsv_stream_front_display_view(mvsv_stream* st, const uint8_t** map, int16_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (!map) return set_error(st->ctx, MVSV_E_INVALID_ARG, "null map pointer");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = display_front(st, &idx))) return rc;
    *map = st->disp_map(idx);
    if (minmax) std::memcpy(minmax, st->disp_minmax(idx), 2 * sizeof(int16_t));
    return MVSV_OK;
}

int mvsv_stream_disable_sharpness(mvsv_stream* st)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (st->head != st->tail)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the sharpness changes only while no frame is pending");
    DeviceGuard dev_guard(st->ctx->device);
    sharpness_free(st);  // every frame was popped: nothing in flight uses the buffers
    return MVSV_OK;
}

int mvsv_stream_enable_sharpness(mvsv_stream* st, const mvsv_rect* roi_left, const mvsv_rect* roi_right)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (st->head != st->tail)
        return set_error(ctx, MVSV_E_INVALID_ARG, "the sharpness changes only while no frame is pending");
    // the pushed images' size
    const int iw = st->raw ? st->rawW : st->W, ih = st->raw ? st->rawH : st->H;
    const mvsv_rect* rois[2] = {roi_left, roi_right};
    mvsv_rect q[2];
    for (int i = 0; i < 2; i++) {
        q[i] = rois[i] ? *rois[i] : mvsv_rect{0, 0, iw, ih};
        if (q[i].x0 < 0 || q[i].y0 < 0 || q[i].x1 > iw || q[i].y1 > ih || q[i].x1 <= q[i].x0 || q[i].y1 <= q[i].y0)
            return set_error(ctx, MVSV_E_INVALID_ARG, "sharpness ROI empty or outside the pushed image");
    }
    DeviceGuard dev_guard(ctx->device);
    sharpness_free(st);
    st->sharp_roi[0] = q[0];
    st->sharp_roi[1] = q[1];
    const size_t bytes = st->slots.size() * 2 * sizeof(int64_t);
    const bool ok = hipMalloc((void**)&st->dSharp, bytes) == hipSuccess &&
                    hipHostMalloc((void**)&st->hSharp, bytes, hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        sharpness_free(st);
        return set_error(ctx, MVSV_E_OOM, "sharpness buffer allocation failed");
    }
    st->sharp = true;
    return MVSV_OK;
}

int mvsv_stream_front_sharpness(mvsv_stream* st, double value[2], int64_t sum4[2])
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!st->sharp) return set_error(ctx, MVSV_E_INVALID_ARG, "the sharpness is not enabled on this stream");
    if (st->head == st->tail) return set_error(ctx, MVSV_E_INVALID_ARG, "stream empty");
    DeviceGuard dev_guard(ctx->device);
    const long idx = st->tail % (long)st->slots.size();
    auto& s = st->slots[idx];
    int rc;
    if (st->tail >= st->launched && (rc = stream_launch(st))) return rc;  // partial group
    if ((rc = check_hip(ctx, hipEventSynchronize(s.done), "stream sync"))) return rc;
    if (s.status) return s.status;
    // the report word is left for pop to read and clear
    if (s.gave_up || (s.run_len > 0 && __atomic_load_n(&st->rep[idx], __ATOMIC_ACQUIRE) != 0))
        return set_error(ctx, MVSV_E_TIMEOUT, "stream frame: a strip-boundary wait of its SGBM launch gave up");
    for (int i = 0; i < 2; i++) {
        const mvsv_rect& q = st->sharp_roi[i];
        const int64_t s4 = st->hSharp[2 * idx + i];
        if (sum4) sum4[i] = s4;
        // cv::mean: sum * (1.0 / N), a reciprocal and a product, each rounded
        if (value) value[i] = ((double)s4 / 4.0) * (1.0 / ((double)(q.x1 - q.x0) * (double)(q.y1 - q.y0)));
    }
    return MVSV_OK;
}

int mvsv_stream_disable_cloud(mvsv_stream* st)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (st->head != st->tail)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the point cloud changes only while no frame is pending");
    DeviceGuard dev_guard(st->ctx->device);
    cloud_free(st);  // every frame was popped: nothing in flight uses the buffers
    return MVSV_OK;
}

int mvsv_stream_enable_cloud(mvsv_stream* st, const mvsv_rect* roi, const float* Q, int max_points)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!Q) return set_error(ctx, MVSV_E_INVALID_ARG, "null Q matrix");
    if (st->head != st->tail)
        return set_error(ctx, MVSV_E_INVALID_ARG, "the point cloud changes only while no frame is pending");
    const mvsv_rect q = roi ? *roi : mvsv_rect{0, 0, st->W, st->H};
    if (q.x0 < 0 || q.y0 < 0 || q.x1 > st->W || q.y1 > st->H || q.x1 <= q.x0 || q.y1 <= q.y0)
        return set_error(ctx, MVSV_E_INVALID_ARG, "point cloud ROI empty or outside the image");
    const size_t roi_px = (size_t)(q.x1 - q.x0) * (q.y1 - q.y0);
    if (roi_px > (size_t)INT32_MAX) return set_error(ctx, MVSV_E_INVALID_ARG, "point cloud ROI too large");
    DeviceGuard dev_guard(ctx->device);
    cloud_free(st);
    st->cloud_roi = q;
    std::memcpy(st->cloud_Q, Q, sizeof(st->cloud_Q));
    st->cloud_max = (int)(max_points <= 0 ? roi_px : std::min((size_t)max_points, roi_px));
    const size_t depth = st->slots.size();
    const bool ok =
        hipMalloc((void**)&st->dCloud, depth * (size_t)st->cloud_max * sizeof(mvsv_cloud_point)) == hipSuccess &&
        hipMalloc((void**)&st->dCloudHdr, depth * 3 * sizeof(int)) == hipSuccess &&
        hipHostMalloc((void**)&st->hCloudHdr, depth * 3 * sizeof(int), hipHostMallocDefault) == hipSuccess &&
        hipStreamCreateWithFlags(&st->cloud_copy, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        cloud_free(st);
        return set_error(ctx, MVSV_E_OOM, "point cloud buffer allocation failed");
    }
    st->cloud = true;
    return MVSV_OK;
}

// the oldest pending frame, complete: its slot index in *idx
static int cloud_front(mvsv_stream* st, long* idx, int* count, int32_t* minmax)
{
    mvsv_ctx* ctx = st->ctx;
    if (!st->cloud) return set_error(ctx, MVSV_E_INVALID_ARG, "the point cloud is not enabled on this stream");
    if (st->head == st->tail) return set_error(ctx, MVSV_E_INVALID_ARG, "stream empty");
    *idx = st->tail % (long)st->slots.size();
    auto& s = st->slots[*idx];
    int rc;
    if (st->tail >= st->launched && (rc = stream_launch(st))) return rc;  // partial group
    if ((rc = check_hip(ctx, hipEventSynchronize(s.done), "stream sync"))) return rc;
    if (s.status) return s.status;
    // the report word is left for pop to read and clear
    if (s.gave_up || (s.run_len > 0 && __atomic_load_n(&st->rep[*idx], __ATOMIC_ACQUIRE) != 0))
        return set_error(ctx, MVSV_E_TIMEOUT, "stream frame: a strip-boundary wait of its SGBM launch gave up");
    const int* h = st->hCloudHdr + 3 * *idx;
    if (count) *count = h[0];
    if (minmax) {
        minmax[0] = h[1];
        minmax[1] = h[2];
    }
    return MVSV_OK;
}

int mvsv_stream_front_cloud(mvsv_stream* st, mvsv_cloud_point* records, int capacity, int* count, int32_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (records && capacity < 0) return set_error(st->ctx, MVSV_E_INVALID_ARG, "negative point cloud capacity");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = cloud_front(st, &idx, count, minmax))) return rc;
    const size_t k = records ? (size_t)std::min(std::min(st->hCloudHdr[3 * idx], st->cloud_max), capacity) : 0;
    if (k == 0) return MVSV_OK;
    // the frame is complete; a stream of its own, so the copy does not queue behind the later frames' downloads
    if ((rc = check_hip(st->ctx, hipMemcpyAsync(records, st->dCloud + (size_t)idx * st->cloud_max,
                                                k * sizeof(mvsv_cloud_point), hipMemcpyDeviceToHost, st->cloud_copy),
                        "stream D2H")))
        return rc;
    return check_hip(st->ctx, hipStreamSynchronize(st->cloud_copy), "stream sync");
}

int mvsv_stream_front_cloud_device(mvsv_stream* st, const mvsv_cloud_point** records_dev, int* count, int32_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (!records_dev) return set_error(st->ctx, MVSV_E_INVALID_ARG, "null records pointer");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = cloud_front(st, &idx, count, minmax))) return rc;
    *records_dev = st->dCloud + (size_t)idx * st->cloud_max;
    return MVSV_OK;
}

static bool same_rect(const mvsv_rect& a, const mvsv_rect& b)
{
    return a.x0 == b.x0 && a.y0 == b.y0 && a.x1 == b.x1 && a.y1 == b.y1;
}

int mvsv_stream_disable_view(mvsv_stream* st)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (st->head != st->tail)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the view changes only while no frame is pending");
    DeviceGuard dev_guard(st->ctx->device);
    view_free(st);  // every frame was popped: nothing in flight uses the buffers
    return MVSV_OK;
}

int mvsv_stream_enable_view(mvsv_stream* st, const mvsv_rect* roi, const mvsv_view_spec* spec)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    const mvsv_rect q = roi ? *roi : mvsv_rect{0, 0, st->W, st->H};
    if (q.x0 < 0 || q.y0 < 0 || q.x1 > st->W || q.y1 > st->H || q.x1 <= q.x0 || q.y1 <= q.y0)
        return set_error(ctx, MVSV_E_INVALID_ARG, "view ROI empty or outside the image");
    if (const char* why = view_check(spec, q.x1 - q.x0, q.y1 - q.y0)) return set_error(ctx, MVSV_E_INVALID_ARG, why);
    if (st->head != st->tail)
        return set_error(ctx, MVSV_E_INVALID_ARG, "the view changes only while no frame is pending");
    if ((spec->layers & MVSV_VIEW_FOUND_TILES) && !(st->grid && same_rect(st->roi, q)))
        return set_error(ctx, MVSV_E_INVALID_ARG, "FOUND_TILES needs a stream created with a grid_roi equal to the view's ROI");
    if ((spec->layers & MVSV_VIEW_FOUND_POINTS) && !(st->sp && same_rect(st->sp_roi, q)))
        return set_error(ctx, MVSV_E_INVALID_ARG, "FOUND_POINTS needs sample points enabled with the view's ROI");
    DeviceGuard dev_guard(ctx->device);
    view_free(st);
    st->view_roi = q;
    st->view_spec = *spec;
    st->view_bytes = 3 * (size_t)(q.x1 - q.x0) * (q.y1 - q.y0);
    st->view_slot_bytes = (((st->view_bytes + 1) & ~(size_t)1) + 2 * sizeof(int16_t) + 15) & ~(size_t)15;
    const size_t depth = st->slots.size();
    const bool ok = hipMalloc((void**)&st->dView, depth * st->view_bytes) == hipSuccess &&
                    hipMalloc((void**)&st->dViewMM, depth * 2 * sizeof(int16_t)) == hipSuccess &&
                    hipHostMalloc((void**)&st->hView, depth * st->view_slot_bytes, hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        view_free(st);
        return set_error(ctx, MVSV_E_OOM, "view buffer allocation failed");
    }
    st->view = true;
    return MVSV_OK;
}

static int view_front(mvsv_stream* st, long* idx, bool host = true)
{
    if (host && st->view && !(st->host_mask & MVSV_HOST_VIEW))
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the host view is switched off (mvsv_stream_set_host_outputs)");
    return front_slot(st, st->view, "the view is not enabled on this stream", idx);
}

int mvsv_stream_front_view(mvsv_stream* st, uint8_t* out, size_t out_stride, int16_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    const size_t rb = 3 * (size_t)(st->view_roi.x1 - st->view_roi.x0);
    if (st->view && out && out_stride < rb)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "view stride smaller than three times the ROI's width");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = view_front(st, &idx))) return rc;
    if (out) copy_rows(out, out_stride, st->view_img(idx), rb, rb, st->view_roi.y1 - st->view_roi.y0, 0, 1);
    if (minmax) std::memcpy(minmax, st->view_minmax(idx), 2 * sizeof(int16_t));
    return MVSV_OK;
}

int mvsv_stream_front_view_view(mvsv_stream* st, const uint8_t** view, int16_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (!view) return set_error(st->ctx, MVSV_E_INVALID_ARG, "null view pointer");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = view_front(st, &idx))) return rc;
    *view = st->view_img(idx);
    if (minmax) std::memcpy(minmax, st->view_minmax(idx), 2 * sizeof(int16_t));
    return MVSV_OK;
}

// ---- device ends of the stream ----

// Both ends of a source span may be read by the stream's device.
static bool source_ok(const mvsv_stream* st, const uint8_t* p, size_t span)
{
    for (const uint8_t* q : {p, p + span - 1}) {
        hipPointerAttribute_t a{};
        const bool ok = hipPointerGetAttributes(&a, q) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        PtrKind kind = kPtrOther;
        switch (a.type) {
        case hipMemoryTypeUnregistered: kind = kPtrUnregistered; break;
        case hipMemoryTypeHost: kind = kPtrHost; break;
        case hipMemoryTypeDevice: kind = kPtrDevice; break;
        case hipMemoryTypeManaged: kind = kPtrManaged; break;
        default: break;
        }
        if (!ring_source_ok(ok, kind, a.device, st->ctx->device, a.devicePointer != nullptr)) return false;
    }
    return true;
}

enum PushKind { kPushRectified, kPushRaw, kPushBgr };

// n frames from device-readable memory into the next n slots: one copy launch per
// contiguous ring segment on the upload stream, ordered against the producer's
// stream by events in both directions; then the bookkeeping of n single pushes.
static int stream_push_device(mvsv_stream* st, PushKind kind, int n, const uint8_t* L, size_t ls, size_t lfs,
                              const uint8_t* R, size_t rs, size_t rfs, void* producer)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (kind == kPushRaw && !st->raw)
        return set_error(ctx, MVSV_E_INVALID_ARG, "stream of rectified pairs: push them with mvsv_stream_push_device");
    if (kind != kPushRaw && st->raw)
        return set_error(ctx, MVSV_E_INVALID_ARG, "raw stream: push raw pairs with mvsv_stream_push_raw_device");
    if (kind == kPushBgr && !st->bgr)
        return set_error(ctx, MVSV_E_INVALID_ARG, "colour input is not enabled on this stream");
    const int rows = kind == kPushRaw ? st->rawH : kind == kPushBgr ? st->bgrH : st->H;
    const size_t row = kind == kPushRaw ? (size_t)st->rawW : kind == kPushBgr ? 3 * (size_t)st->bgrW : (size_t)st->W;
    if (!L || !R || ls < row || rs < row)
        return set_error(ctx, MVSV_E_INVALID_ARG, "null frame or stride smaller than the row");
    const long depth = (long)st->slots.size();
    if (n < 1 || n > depth - (st->head - st->tail))
        return set_error(ctx, MVSV_E_INVALID_ARG, "device push: 1 .. depth - pending frames expected");
    if (n > 1 && (lfs < (size_t)(rows - 1) * ls + row || rfs < (size_t)(rows - 1) * rs + row))
        return set_error(ctx, MVSV_E_INVALID_ARG, "frame stride smaller than a frame");
    DeviceGuard dev_guard(ctx->device);
    if (!source_ok(st, L, (size_t)(n - 1) * lfs + (size_t)(rows - 1) * ls + row) ||
        !source_ok(st, R, (size_t)(n - 1) * rfs + (size_t)(rows - 1) * rs + row))
        return set_error(ctx, MVSV_E_INVALID_ARG,
                         "device push: memory of the stream's device or device-accessible host memory expected");
    hipStream_t prod = (hipStream_t)producer;
    int rc;
    if ((rc = check_hip(ctx, hipEventRecord(st->producer_ev, prod), "stream event")) ||
        (rc = check_hip(ctx, hipStreamWaitEvent(st->up, st->producer_ev, 0), "stream wait")))
        return rc;
    RingRun seg[2];
    const int nseg = ring_push_segments(st->head, n, depth, seg);
    // the slots' previous frames were popped, so everything that read or wrote them is complete
    int done = 0;
    for (int g = 0; g < nseg; g++) {
        auto& first = st->slots[seg[g].i0];
        uint8_t *dl, *dr;
        size_t ds, dfs;
        if (kind == kPushRaw) {
            dl = first.dRaw, dr = first.dRaw + row * rows, ds = row, dfs = 2 * row * rows;
        } else if (kind == kPushBgr) {
            dl = first.dBgr, dr = first.dBgr + st->bgrRow * rows, ds = st->bgrRow, dfs = 2 * st->bgrRow * rows;
        } else {
            dl = first.dL, dr = first.dR, ds = row, dfs = row * rows;
        }
        if ((rc = stream_copy_device(ctx, st->up, seg[g].n, L + done * lfs, ls, lfs, R + done * rfs, rs, rfs, dl, dr,
                                     ds, dfs, (int)row, rows)))
            return rc;
        done += seg[g].n;
    }
    // n single pushes: a launch waits for the `uploaded` event of its last slot, which is
    // the frame that completes a group, the ring's last slot or the call's last frame
    hipEvent_t last = nullptr;
    for (int k = 0; k < n; k++) {
        auto& s = st->slots[st->head % depth];
        if (kind != kPushRaw) s.is_bgr = kind == kPushBgr;
        st->head++;
        const bool launch = ring_launch_after_push(st->head, st->launched, st->batch, depth);
        if (launch || k == n - 1) {
            if ((rc = check_hip(ctx, hipEventRecord(s.uploaded, st->up), "stream event"))) return rc;
            last = s.uploaded;
        }
        if (launch && (rc = stream_launch(st))) return rc;
    }
    // what the producer enqueues from now on may overwrite or free the source
    return check_hip(ctx, hipStreamWaitEvent(prod, last, 0), "stream wait");
}

int mvsv_stream_push_device(mvsv_stream* st, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                            size_t rs, size_t rfs, void* producer_stream)
{
    return stream_push_device(st, kPushRectified, n, L, ls, lfs, R, rs, rfs, producer_stream);
}

int mvsv_stream_push_raw_device(mvsv_stream* st, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                                size_t rs, size_t rfs, void* producer_stream)
{
    return stream_push_device(st, kPushRaw, n, L, ls, lfs, R, rs, rfs, producer_stream);
}

int mvsv_stream_push_bgr_device(mvsv_stream* st, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                                size_t rs, size_t rfs, void* producer_stream)
{
    return stream_push_device(st, kPushBgr, n, L, ls, lfs, R, rs, rfs, producer_stream);
}

int mvsv_stream_set_host_outputs(mvsv_stream* st, int mask)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (mask & ~MVSV_HOST_ALL) return set_error(st->ctx, MVSV_E_INVALID_ARG, "unknown host output bit");
    if (st->head != st->tail)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the host outputs change only while no frame is pending");
    st->host_mask = mask;
    return MVSV_OK;
}

int mvsv_stream_pop_device(mvsv_stream* st, int16_t* out, size_t os, float* means, void* consumer_stream)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!out || os < (size_t)st->W) return set_error(ctx, MVSV_E_INVALID_ARG, "null map or stride smaller than width");
    DeviceGuard dev_guard(ctx->device);
    mvsv_stream::Slot* sp = nullptr;
    int rc = stream_pop_slot(st, &sp);
    if (rc) return rc;
    // the frame is complete: the consumer's stream needs no wait.  The slot's next
    // launch waits for this copy before it overwrites the map.
    hipStream_t cons = (hipStream_t)consumer_stream;
    if ((rc = check_hip(ctx, hipMemcpy2DAsync(out, os * 2, sp->dOut, (size_t)st->W * 2, (size_t)st->W * 2, st->H,
                                              hipMemcpyDeviceToDevice, cons), "stream D2D")) ||
        (rc = check_hip(ctx, hipEventRecord(sp->released, cons), "stream event")))
        return rc;
    sp->release_pending = true;
    stream_means(st, *sp, means);
    return MVSV_OK;
}

int mvsv_stream_front_map_device(mvsv_stream* st, const int16_t** map_dev, float* means)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (!map_dev) return set_error(st->ctx, MVSV_E_INVALID_ARG, "null map pointer");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = front_slot(st, true, "", &idx))) return rc;
    *map_dev = st->slots[idx].dOut;
    stream_means(st, st->slots[idx], means);
    return MVSV_OK;
}

int mvsv_stream_front_rectified_device(mvsv_stream* st, const uint8_t** left_dev, const uint8_t** right_dev)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (!left_dev || !right_dev) return set_error(st->ctx, MVSV_E_INVALID_ARG, "null pair pointer");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = front_slot(st, st->keep, "the stream was not created with keep_rectified", &idx))) return rc;
    *left_dev = st->slots[idx].dL;
    *right_dev = st->slots[idx].dR;
    return MVSV_OK;
}

int mvsv_stream_front_display_device(mvsv_stream* st, const uint8_t** map_dev, int16_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (!map_dev) return set_error(st->ctx, MVSV_E_INVALID_ARG, "null map pointer");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = display_front(st, &idx, false))) return rc;
    *map_dev = st->dDisp + (size_t)idx * st->disp_px;
    if (minmax) std::memcpy(minmax, st->disp_minmax(idx), 2 * sizeof(int16_t));
    return MVSV_OK;
}

int mvsv_stream_front_view_device(mvsv_stream* st, const uint8_t** bgr_dev, int16_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (!bgr_dev) return set_error(st->ctx, MVSV_E_INVALID_ARG, "null view pointer");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    int rc;
    if ((rc = view_front(st, &idx, false))) return rc;
    *bgr_dev = st->dView + (size_t)idx * st->view_bytes;
    if (minmax) std::memcpy(minmax, st->view_minmax(idx), 2 * sizeof(int16_t));
    return MVSV_OK;
}

int mvsv_stream_fence(mvsv_stream* st, void* hip_stream)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    DeviceGuard dev_guard(ctx->device);
    int rc;
    if ((rc = check_hip(ctx, hipEventRecord(st->fence_ev, (hipStream_t)hip_stream), "stream event")) ||
        (rc = check_hip(ctx, hipStreamWaitEvent(st->up, st->fence_ev, 0), "stream wait")))
        return rc;
    // frames that are pushed but not launched yet run on the lanes
    for (mvsv_ctx* c : st->lanes)
        if ((rc = check_hip(ctx, hipStreamWaitEvent(c->stream, st->fence_ev, 0), "stream wait"))) return rc;
    st->fenced = true;
    return MVSV_OK;
}

void mvsv_stream_destroy(mvsv_stream* st)
{
    if (!st) return;
    DeviceGuard dev_guard(st->ctx->device);
    (void)hipStreamSynchronize(st->up);
    for (mvsv_ctx* c : st->lanes) (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(st->down);
    stream_free(st);
}

int mvsv_mean_disparity_grid(mvsv_ctx* ctx, const int16_t* dmap, size_t st, int W, int H,
                             float* means)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (!dmap || !means || W <= 0 || H <= 0 || st < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad mean-grid arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, [&]() -> int {  // every exit after an enqueue
    const size_t px = (size_t)W * H;
    int rc;
    if ((rc = ensure(ctx, ctx->h_out, px * 2 + 4 + 81 * sizeof(float), "grid staging"))) return rc;
    int16_t* d = (int16_t*)ctx->h_out.ptr;
    float* m = (float*)(d + px + (px & 1));
    hipStream_t s = ctx->stream;
    if ((rc = check_hip(ctx, hipMemcpy2DAsync(d, (size_t)W * 2, dmap, st * 2, (size_t)W * 2, H,
                                              hipMemcpyHostToDevice, s), "H2D map")) ||
        (rc = mean_grid_device(ctx, 1, d, W, px, W, H, m)) ||
        (rc = check_hip(ctx, hipMemcpyAsync(means, m, 81 * sizeof(float), hipMemcpyDeviceToHost, s),
                        "D2H means")))
        return rc;
    return check_hip(ctx, hipStreamSynchronize(s), "hipStreamSynchronize");
    }());
}
