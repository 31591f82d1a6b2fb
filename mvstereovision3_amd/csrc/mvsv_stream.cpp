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
// With mvsv_stream_set_bgr_match the map of such a frame comes from SGBM on the
// halved BGR pair itself (cv::StereoSGBM matches CV_8UC3 pairs in colour), in
// launches that hold no grey-matched frame.
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
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "mvsv_internal.hpp"
#include "mvsv_ring.hpp"
#include "mvsv_stream_mem.hpp"

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

// The optional stages of a stream: plain structs that own their buffers, so
// `stage = {}` switches one off and frees it.  stream_launch walks them in a fixed
// order: mean grid, sample points, display, view (reads the two before it), cloud,
// sharpness.

// SamplepointDetection's lattice over roi of every frame
// (mvsv_stream_enable_samplepoints): values, hit count and hit records per slot, on
// the device and in one pinned host block
struct Samplepoints {
    bool on = false;
    mvsv_rect roi{};
    int radius = 0, max_hits = 0, npts = 0;
    float Q[16] = {}, first = 0, second = 0;
    DevArray<float> dVal;             // [depth][npts]
    DevArray<int> dCnt;               // [depth]
    DevArray<mvsv_sample_hit> dHits;  // [depth][max_hits]
    PinnedArray<uint8_t> host;        // [depth] x (values, count, hits), lay.bytes each
    SlotBlock lay;
    float* values(long i) const { return (float*)(host + (size_t)i * lay.bytes); }
    int* count(long i) const { return (int*)(host + (size_t)i * lay.bytes + lay.mid); }
    mvsv_sample_hit* hits(long i) const { return (mvsv_sample_hit*)(host + (size_t)i * lay.bytes + lay.tail); }
    float* dev_values(long i) const { return dVal ? dVal + (size_t)i * npts : nullptr; }
    mvsv_sample_hit* dev_hits(long i) const { return dHits + (size_t)i * max_hits; }
};

// A dense image of roi of every frame and the (smin, smax) it was scaled by, per
// slot, on the device and in one pinned host block: the 8-bit display map
// (mvsv_stream_enable_display) and the BGR detection view (mvsv_stream_enable_view)
struct ImageStage {
    bool on = false;
    mvsv_rect roi{};
    size_t bytes = 0, row_bytes = 0;  // of a frame's image, of one of its rows
    DevArray<uint8_t> dImg;           // [depth][bytes]
    DevArray<int16_t> dMM;            // [depth][2]
    PinnedArray<uint8_t> host;        // [depth] x (image, min, max), lay.bytes each
    SlotBlock lay;
    int width() const { return roi.x1 - roi.x0; }
    int height() const { return roi.y1 - roi.y0; }
    uint8_t* image(long i) const { return host + (size_t)i * lay.bytes; }
    int16_t* minmax(long i) const { return (int16_t*)(image(i) + lay.mid); }
    uint8_t* dev_image(long i) const { return dImg + (size_t)i * bytes; }
    int16_t* dev_minmax(long i) const { return dMM + 2 * i; }
};

// What tells the display from the view at the entry points: the bit of
// mvsv_stream_set_host_outputs that keeps its image on the device, and its messages.
struct ImageTexts {
    int host_bit;
    const char *not_enabled, *host_off, *stride, *null_out;
};
static const ImageTexts kDisplayTexts = {
    MVSV_HOST_DISPLAY, "the display is not enabled on this stream",
    "the host display map is switched off (mvsv_stream_set_host_outputs)",
    "display stride smaller than the ROI's width", "null map pointer"};
static const ImageTexts kViewTexts = {
    MVSV_HOST_VIEW, "the view is not enabled on this stream",
    "the host view is switched off (mvsv_stream_set_host_outputs)",
    "view stride smaller than three times the ROI's width", "null view pointer"};

// the point cloud of roi of every frame (mvsv_stream_enable_cloud): the records
// stay in a device ring, (count, min, max) per slot come to the host
struct Cloud {
    bool on = false;
    mvsv_rect roi{};
    float Q[16] = {};
    int max_points = 0;
    DevArray<mvsv_cloud_point> dRec;  // [depth][max_points]
    DevArray<int> dHdr;               // [depth][3] (count, min, max)
    PinnedArray<int> hHdr;            // [depth][3]
    Stream copy;                      // front_cloud's copies: not behind the later frames' downloads
    mvsv_cloud_point* dev_records(long i) const { return dRec + (size_t)i * max_points; }
};

// the focus measure of every pushed pair (mvsv_stream_enable_sharpness): S4 of
// roi[0] of the left and roi[1] of the right pushed image per slot
struct Sharpness {
    bool on = false;
    mvsv_rect roi[2] = {};
    DevArray<int64_t> dSum;     // [depth][2]
    PinnedArray<int64_t> hSum;  // [depth][2]
};

// colour frames (mvsv_stream_enable_bgr): a pushed BGR pair is staged per slot and
// prepared into the slot's dL / dR on the lane's stream
struct Bgr {
    bool on = false;
    int W = 0, H = 0, halve = 0, variant = 0;
    DevArray<uint8_t> dev;      // [depth] pairs in kPushBgr's geometry
    PinnedArray<uint8_t> host;  // the same, staged
    // colour matching (mvsv_stream_set_bgr_match): a BGR frame's map comes from the
    // colour matcher on the pair at the stream's size -- the halved pair in `half`
    // ([depth][2][H][3 W]), or the staged pair itself without halving
    bool match = false;
    DevArray<uint8_t> half;
};

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
    Stream up, down;
    struct Slot {
        PinnedArray<uint8_t> hL, hR;          // the pushed pair
        PinnedArray<uint8_t> hRectL, hRectR;  // keep_rectified streams
        PinnedArray<int16_t> hOut;
        PinnedArray<float> hMeans;
        // the slot's part of the stream's device arrays
        uint8_t* dRaw = nullptr;  // [2][rawH][rawW], raw streams
        uint8_t *dL = nullptr, *dR = nullptr;
        int16_t* dOut = nullptr;
        float* dMeans = nullptr;
        bool is_bgr = false;  // the pending frame was pushed as BGR (written by every push)
        bool colour = false;  // ... and is matched in colour (bgr.match at its push)
        Event uploaded, computed, done;
        Event released;                // pop_device's copy of dOut on the consumer's stream
        bool release_pending = false;  // the slot's next launch waits for `released`
        int status = MVSV_OK;
        int run_len = 0;       // > 0: this slot starts a frame-batch launch of run_len slots
        bool gave_up = false;  // the launch of this frame gave up a strip wait
    };
    std::vector<Slot> slots;
    DevArray<uint8_t> dL_all, dR_all;  // [depth][H][W]
    DevArray<int16_t> dOut_all;
    DevArray<float> dMeans_all;  // [depth][81]
    // per-slot report words (host-mapped): a launch starting at slot i reports
    // a given-up strip wait into rep[i], read when slot i is popped
    PinnedArray<int> rep;
    int* rep_dev = nullptr;
    long head = 0, tail = 0;  // pushed / popped frame counters
    long launched = 0;        // frames whose compute is enqueued
    int batch = 1;
    int host_mask = MVSV_HOST_ALL;  // the per-frame D2H copies that are enqueued (set_host_outputs)
    Event producer_ev;              // push_device: what the producer had queued
    Event fence_ev;                 // mvsv_stream_fence
    bool fenced = false;
    std::unique_ptr<CopyPool> pool;  // host copies of push / pop (null: caller's thread only)
    // raw stream (mvsv_stream_create_raw): pushed frames are raw camera pairs,
    // rectified (cropped, resized) into the slots' dL / dR ahead of their SGBM
    bool raw = false;
    int rawW = 0, rawH = 0;        // the camera frame; a slot's hL / hR hold one each
    int cropW = 0, cropH = 0;      // the display ROI's size
    double factor = 0;             // 0: the crop is the frame; else cv::resize of the crop
    bool keep = false;             // the rectified pair comes back to the host too
    DevArray<uint8_t> dRaw_all;    // [depth][2][rawH][rawW]
    DevArray<int16_t> dMapXY;      // [2][cropH][mapStride] (sx, sy), ROI only
    DevArray<uint16_t> dMapFrac;   // [2][cropH][mapStride] ay * 32 + ax
    size_t mapStride = 0;          // entries per map row: cropW rounded up to 4, padding zero
    DevArray<uint8_t> dCropL, dCropR;  // [depth][cropH][cropW] each, with a factor
    Samplepoints sp;
    ImageStage disp;
    double disp_alpha = 0, disp_beta = 255;
    ImageStage view;
    mvsv_view_spec view_spec{};  // its means / values pointers are set per launch
    Cloud cloud;
    Sharpness sharp;
    Bgr bgr;

    ~mvsv_stream()
    {
        for (size_t i = 1; i < lanes.size(); i++) mvsv_destroy(lanes[i]);
    }
    PushGeom push_geom(PushKind kind) const { return ring_push_geom(kind, W, H, rawW, rawH, bgr.W, bgr.H); }
};

// what mvsv_stream_create_raw adds to a stream's creation
struct RawSetup {
    const mvsv_rectification* rect;
    int cropW, cropH;
    bool resized;
};

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
    return st->dMapXY.alloc(xy.size()) && st->dMapFrac.alloc(frac.size()) &&
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
            st->pool.reset(new CopyPool(threads));
        } catch (...) {  // copies on the caller's thread
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
    std::unique_ptr<mvsv_stream> st(new (std::nothrow) mvsv_stream());
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
    bool ok = st->up.create() && st->down.create() && st->producer_ev.create() && st->fence_ev.create();
    st->slots.resize(depth);
    if (raw) {
        ok = ok && st->dRaw_all.alloc(2 * in_px * depth) && upload_maps(st.get(), raw->rect);
        if (raw->resized) ok = ok && st->dCropL.alloc(crop_px * depth) && st->dCropR.alloc(crop_px * depth);
    }
    ok = ok && st->dL_all.alloc(px * depth) && st->dR_all.alloc(px * depth) && st->dOut_all.alloc(px * depth) &&
         st->dMeans_all.alloc((size_t)81 * depth);
    for (size_t i = 0; i < st->slots.size(); i++) {
        auto& s = st->slots[i];
        if (!ok) break;
        s.dL = st->dL_all + i * px;
        s.dR = st->dR_all + i * px;
        s.dOut = st->dOut_all + i * px;
        s.dMeans = st->dMeans_all + i * 81;
        if (raw) s.dRaw = st->dRaw_all + i * 2 * in_px;
        if (st->keep) ok = s.hRectL.alloc(px) && s.hRectR.alloc(px);
        ok = ok && s.hL.alloc(in_px) && s.hR.alloc(in_px) && s.hOut.alloc(px) && s.hMeans.alloc(81) &&
             s.uploaded.create() && s.computed.create() && s.done.create() && s.released.create();
    }
    int* rep = nullptr;
    ok = ok && alloc_report(ctx, depth, &rep, &st->rep_dev) == MVSV_OK;
    st->rep = PinnedArray<int>(rep);
    if (ok) stream_pool(st.get(), std::max(px, in_px) * 2);
    if (!ok) {
        (void)hipGetLastError();
        st.reset();
        return set_error(ctx, MVSV_E_OOM, "stream slot allocation failed");
    }
    *out = st.release();
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
    const size_t px = (size_t)st->W * st->H;
    const PushGeom g = st->push_geom(kPushBgr);
    const Bgr& b = st->bgr;
    for (int k = 0; k < n;) {
        if (!st->slots[i0 + k].is_bgr) {
            k++;
            continue;
        }
        int m = 1;
        while (k + m < n && st->slots[i0 + k + m].is_bgr) m++;
        auto& s = st->slots[i0 + k];
        const uint8_t* pair = b.dev + (size_t)(i0 + k) * g.frame;
        int rc;
        if ((rc = prepare_gray_device(ctx, m, pair, g.stride, g.frame, b.W, b.H, b.halve, b.variant, s.dL, st->W,
                                      px)) ||
            (rc = prepare_gray_device(ctx, m, pair + g.right, g.stride, g.frame, b.W, b.H, b.halve, b.variant, s.dR,
                                      st->W, px)))
            return rc;
        k += m;
    }
    return MVSV_OK;
}

// The map of the colour-matched frames of a run (all of it: pushes keep the two kinds
// of frames in launches of their own): mvsv_sgbm_bgr_device's pipeline on the BGR
// pair at the stream's size.
static int stream_match_colour(mvsv_stream* st, mvsv_ctx* ctx, long i0, int n)
{
    const int W = st->W, H = st->H;
    const size_t px = (size_t)W * H;
    const PushGeom g = st->push_geom(kPushBgr);
    const Bgr& b = st->bgr;
    auto& first = st->slots[i0];
    SgbmEff e = st->eff;
    e.cn = 3;
    const uint8_t* pair = b.dev + (size_t)i0 * g.frame;
    if (!b.halve)
        return sgbm_device(ctx, n, pair, g.stride, g.frame, pair + g.right, g.stride, g.frame, W, H, e, first.dOut,
                           W, px);
    const size_t row = 3 * (size_t)W, side = row * H;
    uint8_t* half = b.half + (size_t)i0 * 2 * side;
    int rc;
    if ((rc = halve_bgr_device(ctx, n, pair, g.stride, g.frame, b.W, b.H, half, row, 2 * side)) ||
        (rc = halve_bgr_device(ctx, n, pair + g.right, g.stride, g.frame, b.W, b.H, half + side, row, 2 * side)))
        return rc;
    return sgbm_device(ctx, n, half, row, 2 * side, half + side, row, 2 * side, W, H, e, first.dOut, W, px);
}

// A frame-batch launch holds frames of one kind of matching: a frame that is matched
// in colour where the pending ones are not, or the reverse, sends those off first,
// as a change of matcher or parameters does.
static int stream_launch(mvsv_stream* st);
static int stream_kind_boundary(mvsv_stream* st, bool colour)
{
    if (st->launched == st->head) return MVSV_OK;
    const auto& prev = st->slots[(st->head - 1) % (long)st->slots.size()];
    return prev.colour == colour ? MVSV_OK : stream_launch(st);
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
        int status = st->raw ? stream_rectify(st, ctx, i0, n) : st->bgr.on ? stream_prepare(st, ctx, i0, n) : MVSV_OK;
        if (status == MVSV_OK)
            status = st->matcher == MVSV_MATCHER_BM
                         ? bm_device(ctx, n, first.dL, W, px, first.dR, W, px, W, H, st->bm_eff, first.dOut, W, px)
                     : first.colour
                         ? stream_match_colour(st, ctx, i0, n)
                         : sgbm_device(ctx, n, first.dL, W, px, first.dR, W, px, W, H, st->eff, first.dOut, W, px);
        ctx->report_target = prev_target;
        // the run's maps at a stage's ROI
        auto at = [&](const mvsv_rect& q) { return first.dOut + (size_t)q.y0 * W + q.x0; };
        if (status == MVSV_OK && st->grid) {
            const mvsv_rect& q = st->roi;
            status = mean_grid_device(ctx, n, at(q), W, px, q.x1 - q.x0, q.y1 - q.y0, first.dMeans);
        }
        const Samplepoints& sp = st->sp;
        if (status == MVSV_OK && sp.on && sp.npts > 0) {
            const mvsv_rect& q = sp.roi;
            const int rw = q.x1 - q.x0, rh = q.y1 - q.y0;
            status = sample_grid_device(ctx, n, at(q), W, px, rw, rh, sp.radius, sp.dev_values(i0));
            if (status == MVSV_OK)
                status = sample_detect_device(ctx, n, sp.dev_values(i0), rw, rh, sp.Q, sp.first, sp.second, sp.max_hits,
                                              sp.dCnt + i0, sp.dev_hits(i0));
        }
        if (status == MVSV_OK && st->disp.on) {
            const ImageStage& g = st->disp;
            status = normalize_minmax_device(ctx, n, at(g.roi), W, px, g.width(), g.height(), st->disp_alpha,
                                             st->disp_beta, g.dev_image(i0), g.row_bytes, g.bytes, g.dev_minmax(i0));
        }
        if (status == MVSV_OK && st->view.on) {  // after the mean grid and the lattice: it reads both
            const ImageStage& g = st->view;
            mvsv_view_spec spec = st->view_spec;
            spec.means = first.dMeans;
            spec.values = sp.dev_values(i0);
            spec.point_first = sp.first;
            spec.point_second = sp.second;
            status = view_device(ctx, n, at(g.roi), W, px, g.width(), g.height(), spec, g.dev_image(i0), g.row_bytes,
                                 g.bytes, g.dev_minmax(i0));
        }
        if (status == MVSV_OK && st->cloud.on) {
            const Cloud& c = st->cloud;
            const mvsv_rect& q = c.roi;
            status = point_cloud_device(ctx, n, at(q), W, px, q.x1 - q.x0, q.y1 - q.y0, c.Q, c.dev_records(i0),
                                        c.max_points, c.dHdr + 3 * i0, 3, c.dHdr + 3 * i0 + 1, 3);
        }
        if (status == MVSV_OK && st->sharp.on) {
            // the pushed pair: a raw slot holds it as [2][rawH][rawW]
            const int iw = st->raw ? st->rawW : W, ih = st->raw ? st->rawH : H;
            const size_t ipx = (size_t)iw * ih;
            const uint8_t* pl = st->raw ? first.dRaw : first.dL;
            const uint8_t* pr = st->raw ? first.dRaw + ipx : first.dR;
            const size_t ifs = st->raw ? 2 * ipx : ipx;
            int64_t* sums = st->sharp.dSum + 2 * i0;
            status = sharpness_device(ctx, n, pl, iw, ifs, iw, ih, st->sharp.roi[0], sums, 2);
            if (status == MVSV_OK)
                status = sharpness_device(ctx, n, pr, iw, ifs, iw, ih, st->sharp.roi[1], sums + 1, 2);
        }
        if (status != MVSV_OK && ctx != st->ctx) st->ctx->err = ctx->err;  // reported by pop
        st->runs++;
        if ((rc = mark_last_use(ctx, MVSV_OK)) ||
            (rc = check_hip(ctx, hipEventRecord(last.computed, ctx->stream), "stream event")) ||
            (rc = check_hip(ctx, hipStreamWaitEvent(st->down, last.computed, 0), "stream wait"))) {
            if (ctx != st->ctx) st->ctx->err = ctx->err;
            return rc;
        }
        // what the host reads of every frame, in this order on the download stream
        auto d2h = [&](void* dst, const void* src, size_t bytes) {
            return check_hip(st->ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st->down), "stream D2H");
        };
        // an image stage: the image unless set_host_outputs keeps it on the device, and its (min, max)
        auto d2h_image = [&](const ImageStage& g, int host_bit, long i) {
            int e = MVSV_OK;
            if (!g.on) return e;
            if ((st->host_mask & host_bit) && (e = d2h(g.image(i), g.dev_image(i), g.bytes))) return e;
            return d2h(g.minmax(i), g.dev_minmax(i), 2 * sizeof(int16_t));
        };
        for (long i = i0; i < i0 + n; i++) {
            auto& s = st->slots[i];
            s.status = status;
            if ((st->host_mask & MVSV_HOST_MAP) && (rc = d2h(s.hOut, s.dOut, px * 2))) return rc;
            if (st->grid && (rc = d2h(s.hMeans, s.dMeans, 81 * sizeof(float)))) return rc;
            if (st->keep && (st->host_mask & MVSV_HOST_RECTIFIED) &&
                ((rc = d2h(s.hRectL, s.dL, px)) || (rc = d2h(s.hRectR, s.dR, px))))
                return rc;
            if (sp.on && sp.npts > 0 &&  // values, count and hit records are adjacent in the pinned slot
                ((rc = d2h(sp.values(i), sp.dev_values(i), (size_t)sp.npts * sizeof(float))) ||
                 (rc = d2h(sp.count(i), sp.dCnt + i, sizeof(int))) ||
                 (rc = d2h(sp.hits(i), sp.dev_hits(i), (size_t)sp.max_hits * sizeof(mvsv_sample_hit)))))
                return rc;
            if ((rc = d2h_image(st->disp, MVSV_HOST_DISPLAY, i)) || (rc = d2h_image(st->view, MVSV_HOST_VIEW, i)))
                return rc;
            // the cloud's header only: the records wait on the device for front_cloud
            if (st->cloud.on && (rc = d2h(st->cloud.hHdr + 3 * i, st->cloud.dHdr + 3 * i, 3 * sizeof(int)))) return rc;
            if (st->sharp.on && (rc = d2h(st->sharp.hSum + 2 * i, st->sharp.dSum + 2 * i, 2 * sizeof(int64_t))))
                return rc;
            if ((rc = check_hip(st->ctx, hipEventRecord(s.done, st->down), "stream event"))) return rc;
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
        c->opt = ctx->opt;  // the stream's own lanes follow the caller context's kernel options
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
    // (a census window set with mvsv_stream_set_census stays: the new parameters must satisfy its rules)
    int rc = sgbm_census(st->eff) ? resolve_sgbm_census(p, st->W, st->H, st->eff.cw, st->eff.ch, &e, &why)
                                  : resolve_sgbm(p, st->W, st->H, &e, &why);
    if (rc) return set_error(st->ctx, rc, why);
    if (st->matcher == MVSV_MATCHER_BM && bm_census(st->bm_eff))
        return set_error(st->ctx, MVSV_E_INVALID_ARG,
                         "the StereoBM census cost is on (mvsv_stream_set_bm_census): switch it off before a switch to SGBM");
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
    // (a window set with mvsv_stream_set_bm_census stays: the new parameters must satisfy its rules)
    const bool census = st->matcher == MVSV_MATCHER_BM && bm_census(st->bm_eff);
    int rc = census ? resolve_bm_census(p, st->W, st->H, st->bm_eff.cw, st->bm_eff.ch, &e, &why)
                    : resolve_bm(p, st->W, st->H, &e, &why);
    if (rc) return set_error(st->ctx, rc, why);
    if (st->bgr.match)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "colour matching is on: StereoBM takes grey pairs only");
    if (st->matcher == MVSV_MATCHER_SGBM && sgbm_census(st->eff))
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the census cost is on: it is for the SGBM matcher only");
    DeviceGuard dev_guard(st->ctx->device);
    if ((rc = stream_launch(st))) return rc;  // pending frames keep their matcher and parameters
    st->bm_params = *p;
    st->bm_eff = e;
    st->matcher = MVSV_MATCHER_BM;
    return MVSV_OK;
}

int mvsv_stream_pending(const mvsv_stream* st) { return st ? (int)(st->head - st->tail) : 0; }

// ---- steps the entry points share ----

// Stages and outputs change only while the ring is empty: nothing in flight uses
// the buffers then.  subject: "the display changes", "sample points change", ...
static int idle_check(mvsv_stream* st, const char* subject)
{
    if (st->head == st->tail) return MVSV_OK;
    return set_error(st->ctx, MVSV_E_INVALID_ARG, std::string(subject) + " only while no frame is pending");
}

// *q = roi, or the whole iw x ih image without one; false unless it is inside the image and not empty
static bool roi_or_whole(const mvsv_rect* roi, int iw, int ih, mvsv_rect* q)
{
    *q = roi ? *roi : mvsv_rect{0, 0, iw, ih};
    return q->x0 >= 0 && q->y0 >= 0 && q->x1 <= iw && q->y1 <= ih && q->x1 > q->x0 && q->y1 > q->y0;
}

static bool same_rect(const mvsv_rect& a, const mvsv_rect& b)
{
    return a.x0 == b.x0 && a.y0 == b.y0 && a.x1 == b.x1 && a.y1 == b.y1;
}

template <class Stage>
static int stage_disable(mvsv_stream* st, Stage mvsv_stream::*stage, const char* subject)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (int rc = idle_check(st, subject)) return rc;
    DeviceGuard dev_guard(st->ctx->device);
    st->*stage = Stage{};
    return MVSV_OK;
}

// a stage's allocation failed: the stage is off again
template <class Stage>
static int stage_oom(mvsv_stream* st, Stage* stage, const char* msg)
{
    (void)hipGetLastError();
    *stage = Stage{};
    return set_error(st->ctx, MVSV_E_OOM, msg);
}

// fn(part, parts) over the copy pool, or on the caller's thread without one
template <class Fn>
static void run_copy(mvsv_stream* st, const Fn& fn)
{
    if (st->pool)
        st->pool->run(fn);
    else
        fn(0, 1);
}

// ---- pushes ----

// The stream takes frames of this kind: from the host (mvsv_stream_push, _raw, _bgr)
// or, with device, from device memory (the same names + _device).
static int push_kind_check(mvsv_stream* st, PushKind kind, bool device)
{
    const char* suffix = device ? "_device" : "";
    if (kind == kPushRaw && !st->raw)
        return set_error(st->ctx, MVSV_E_INVALID_ARG,
                         std::string("stream of rectified pairs: push them with mvsv_stream_push") + suffix);
    if (kind != kPushRaw && st->raw)
        return set_error(st->ctx, MVSV_E_INVALID_ARG,
                         std::string("raw stream: push raw pairs with mvsv_stream_push_raw") + suffix);
    if (kind == kPushBgr && !st->bgr.on)
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "colour input is not enabled on this stream");
    return MVSV_OK;
}

// Where a frame of this kind lands in slot i: pinned staging (host pushes) and device.
struct PushEnds {
    uint8_t *hl, *hr, *dl, *dr;
};
static PushEnds push_ends(mvsv_stream* st, PushKind kind, const PushGeom& g, long i)
{
    auto& s = st->slots[i];
    if (kind == kPushRectified) return {s.hL, s.hR, s.dL, s.dR};
    if (kind == kPushRaw) return {s.hL, s.hR, s.dRaw, s.dRaw + g.right};
    uint8_t *h = st->bgr.host + (size_t)i * g.frame, *d = st->bgr.dev + (size_t)i * g.frame;
    return {h, h + g.right, d, d + g.right};
}

// One frame from host memory: rows through the copy pool into the slot's pinned
// staging, H2D on the upload stream, then the push's bookkeeping.
static int stream_push_host(mvsv_stream* st, PushKind kind, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs)
{
    static const char* const bad_frame[] = {"null frame or stride smaller than width",
                                            "null frame or stride smaller than the raw width",
                                            "null frame or stride smaller than three times the width"};
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    int rc;
    if ((rc = push_kind_check(st, kind, false))) return rc;
    const PushGeom g = st->push_geom(kind);
    if (!L || !R || ls < g.row || rs < g.row) return set_error(ctx, MVSV_E_INVALID_ARG, bad_frame[kind]);
    const long depth = (long)st->slots.size();
    if (ring_full(st->head, st->tail, depth))
        return set_error(ctx, MVSV_E_INVALID_ARG, "stream full: pop a frame first");
    DeviceGuard dev_guard(ctx->device);
    const bool colour = kind == kPushBgr && st->bgr.match;
    if ((rc = stream_kind_boundary(st, colour))) return rc;
    auto& s = st->slots[st->head % depth];
    const PushEnds e = push_ends(st, kind, g, st->head % depth);
    // the slot's previous frame was popped, so its copies and what read its device buffers are complete
    run_copy(st, [&](int part, int parts) {
        copy_rows(e.hl, g.stride, L, ls, g.row, g.rows, part, parts);
        copy_rows(e.hr, g.stride, R, rs, g.row, g.rows, part, parts);
    });
    const size_t side = g.stride * g.rows;
    const bool one = e.hr == e.hl + side && e.dr == e.dl + side;  // the pair is one block at both ends
    auto h2d = [&](void* dst, const void* src, size_t bytes) {
        return check_hip(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st->up), "stream H2D");
    };
    if ((rc = h2d(e.dl, e.hl, one ? 2 * side : side)) || (!one && (rc = h2d(e.dr, e.hr, side))) ||
        (rc = check_hip(ctx, hipEventRecord(s.uploaded, st->up), "stream event")))
        return rc;
    if (kind != kPushRaw) s.is_bgr = kind == kPushBgr;
    s.colour = colour;
    st->head++;
    // a full group, or a group that would otherwise wrap past the ring's end
    if (ring_launch_after_push(st->head, st->launched, st->batch, depth)) return stream_launch(st);
    return MVSV_OK;
}

int mvsv_stream_push(mvsv_stream* st, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs)
{
    return stream_push_host(st, kPushRectified, L, ls, R, rs);
}

int mvsv_stream_push_raw(mvsv_stream* st, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs)
{
    return stream_push_host(st, kPushRaw, L, ls, R, rs);
}

int mvsv_stream_push_bgr(mvsv_stream* st, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs)
{
    return stream_push_host(st, kPushBgr, L, ls, R, rs);
}

int mvsv_stream_disable_bgr(mvsv_stream* st) { return stage_disable(st, &mvsv_stream::bgr, "colour input changes"); }

int mvsv_stream_enable_bgr(mvsv_stream* st, int sw, int sh, int halve, int variant)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (st->raw) return set_error(ctx, MVSV_E_INVALID_ARG, "colour input is for streams of rectified pairs");
    if (int rc = idle_check(st, "colour input changes")) return rc;
    int dw, dh;
    if (prepare_size(sw, sh, halve, &dw, &dh) || dw != st->W || dh != st->H)
        return set_error(ctx, MVSV_E_INVALID_ARG, "mvsv_prepare_size of the colour frame is not the stream's size");
    if (variant != MVSV_GRAY_Q14 && variant != MVSV_GRAY_Q15)
        return set_error(ctx, MVSV_E_INVALID_ARG, "unknown grey variant");
    DeviceGuard dev_guard(ctx->device);
    Bgr& b = st->bgr;
    b = {};
    b.W = sw;
    b.H = sh;
    b.halve = halve;
    b.variant = variant;
    const size_t pair = st->push_geom(kPushBgr).frame;
    if (!b.dev.alloc(pair * st->slots.size()) || !b.host.alloc(pair * st->slots.size()))
        return stage_oom(st, &b, "colour staging allocation failed");
    stream_pool(st, pair);
    b.on = true;
    return MVSV_OK;
}

int mvsv_stream_set_bgr_match(mvsv_stream* st, int on)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!st->bgr.on) return set_error(ctx, MVSV_E_INVALID_ARG, "colour input is not enabled on this stream");
    if (int rc = idle_check(st, "colour matching changes")) return rc;
    if (on && st->matcher != MVSV_MATCHER_SGBM)
        return set_error(ctx, MVSV_E_INVALID_ARG, "colour matching is for the SGBM matcher: StereoBM takes grey pairs only");
    if (on && sgbm_census(st->eff))
        return set_error(ctx, MVSV_E_INVALID_ARG, "the census cost is on: it takes grey pairs only");
    DeviceGuard dev_guard(ctx->device);
    Bgr& b = st->bgr;
    if (on && b.halve && !b.half &&
        !b.half.alloc((size_t)st->W * st->H * 6 * st->slots.size())) {
        (void)hipGetLastError();
        return set_error(ctx, MVSV_E_OOM, "colour pair allocation failed");
    }
    b.match = on != 0;
    return MVSV_OK;
}

int mvsv_stream_set_census(mvsv_stream* st, int cw, int ch)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (int rc = idle_check(st, "the census cost changes")) return rc;
    if (st->matcher != MVSV_MATCHER_SGBM)
        return set_error(ctx, MVSV_E_INVALID_ARG, "the census cost is for the SGBM matcher only");
    SgbmEff e;
    std::string why;
    if (cw == 0 && ch == 0) {  // back to the Birchfield-Tomasi cost
        if (int rc = resolve_sgbm(&st->params, st->W, st->H, &e, &why)) return set_error(ctx, rc, why);
        st->eff = e;
        return MVSV_OK;
    }
    if (st->bgr.match)
        return set_error(ctx, MVSV_E_INVALID_ARG, "colour matching is on: the census cost takes grey pairs only");
    if (int rc = resolve_sgbm_census(&st->params, st->W, st->H, cw, ch, &e, &why)) return set_error(ctx, rc, why);
    st->eff = e;
    return MVSV_OK;
}

int mvsv_stream_set_bm_census(mvsv_stream* st, int cw, int ch)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (int rc = idle_check(st, "the census cost changes")) return rc;
    if (st->matcher != MVSV_MATCHER_BM)
        return set_error(ctx, MVSV_E_INVALID_ARG,
                         "the StereoBM census cost is for the StereoBM matcher only (mvsv_stream_set_census is SGBM's)");
    BmEff e;
    std::string why;
    if (int rc = (cw == 0 && ch == 0) ? resolve_bm(&st->bm_params, st->W, st->H, &e, &why)  // back to the SAD cost
                                      : resolve_bm_census(&st->bm_params, st->W, st->H, cw, ch, &e, &why))
        return set_error(ctx, rc, why);
    st->bm_eff = e;
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
    if (out || rl || rr)
        run_copy(st, [&](int part, int parts) {
            if (out)
                copy_rows((uint8_t*)out, os * 2, (const uint8_t*)s.hOut.get(), (size_t)st->W * 2, (size_t)st->W * 2,
                          st->H, part, parts);
            if (rl) copy_rows(rl, rls, s.hRectL, (size_t)st->W, (size_t)st->W, st->H, part, parts);
            if (rr) copy_rows(rr, rrs, s.hRectR, (size_t)st->W, (size_t)st->W, st->H, part, parts);
        });
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

// ---- the oldest pending frame (front_*) ----

// what is asked for is switched on, and a frame is pending
static int front_check(mvsv_stream* st, bool enabled, const char* not_enabled)
{
    if (!enabled) return set_error(st->ctx, MVSV_E_INVALID_ARG, not_enabled);
    if (st->head == st->tail) return set_error(st->ctx, MVSV_E_INVALID_ARG, "stream empty");
    return MVSV_OK;
}

// Wait for the oldest pending frame and report its status; its slot index in *idx.
// The frame stays pending.
static int front_wait(mvsv_stream* st, long* idx)
{
    mvsv_ctx* ctx = st->ctx;
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

static int front_slot(mvsv_stream* st, bool enabled, const char* not_enabled, long* idx)
{
    if (int rc = front_check(st, enabled, not_enabled)) return rc;
    return front_wait(st, idx);
}

// ---- sample points ----

static bool view_uses_samplepoints(const mvsv_stream* st)
{
    return st->view.on && (st->view_spec.layers & MVSV_VIEW_FOUND_POINTS);
}

int mvsv_stream_disable_samplepoints(mvsv_stream* st)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (int rc = idle_check(st, "sample points change")) return rc;
    if (view_uses_samplepoints(st))
        return set_error(st->ctx, MVSV_E_INVALID_ARG, "the view draws the found points: disable the view first");
    DeviceGuard dev_guard(st->ctx->device);
    st->sp = {};
    return MVSV_OK;
}

int mvsv_stream_enable_samplepoints(mvsv_stream* st, const mvsv_rect* roi, int radius, const float* Q, float first,
                                    float second, int max_hits)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!Q) return set_error(ctx, MVSV_E_INVALID_ARG, "null Q");
    if (int rc = idle_check(st, "sample points change")) return rc;
    mvsv_rect q;
    if (!roi_or_whole(roi, st->W, st->H, &q))
        return set_error(ctx, MVSV_E_INVALID_ARG, "sample point ROI empty or outside the image");
    if (view_uses_samplepoints(st) && !same_rect(q, st->view.roi))
        return set_error(ctx, MVSV_E_INVALID_ARG, "the view draws the found points of its own ROI: disable the view first");
    int sx, sy, nx, ny;
    sample_layout(q.x1 - q.x0, q.y1 - q.y0, &sx, &sy, &nx, &ny);
    const int npts = nx * ny;
    if (npts > 0 && (radius < 0 || radius >= std::min(sx, sy)))
        return set_error(ctx, MVSV_E_INVALID_ARG, "sample point radius must be 0 .. min(step_x, step_y) - 1");
    DeviceGuard dev_guard(ctx->device);
    Samplepoints& sp = st->sp;
    sp = {};
    sp.roi = q;
    sp.radius = radius;
    sp.npts = npts;
    sp.max_hits = max_hits <= 0 ? npts : std::min(max_hits, npts);
    std::memcpy(sp.Q, Q, sizeof(sp.Q));
    sp.first = first;
    sp.second = second;
    const size_t depth = st->slots.size();
    sp.lay = ring_slot_block((size_t)npts * sizeof(float), alignof(int), sizeof(int),
                             (size_t)sp.max_hits * sizeof(mvsv_sample_hit));
    if (npts > 0 && !(sp.dVal.alloc(depth * npts) && sp.dCnt.alloc(depth) && sp.dHits.alloc(depth * sp.max_hits) &&
                      sp.host.alloc(depth * sp.lay.bytes)))
        return stage_oom(st, &sp, "sample point buffer allocation failed");
    sp.on = true;
    return MVSV_OK;
}

int mvsv_stream_front_samples(mvsv_stream* st, float* values, int* count, mvsv_sample_hit* hits, int capacity)
{
    if (!st) return MVSV_E_INVALID_ARG;
    const Samplepoints& sp = st->sp;
    int rc;
    if ((rc = front_check(st, sp.on, "sample points are not enabled on this stream"))) return rc;
    if (hits && capacity < 0) return set_error(st->ctx, MVSV_E_INVALID_ARG, "negative capacity");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    if ((rc = front_wait(st, &idx))) return rc;
    if (sp.npts == 0) {
        if (count) *count = 0;
        return MVSV_OK;
    }
    const int total = *sp.count(idx);
    if (values) std::memcpy(values, sp.values(idx), (size_t)sp.npts * sizeof(float));
    if (count) *count = total;
    if (hits)
        std::memcpy(hits, sp.hits(idx),
                    (size_t)std::min(std::min(total, sp.max_hits), capacity) * sizeof(mvsv_sample_hit));
    return MVSV_OK;
}

// ---- display and view ----

// The rings of an image stage over q, bytes_per_px bytes a pixel; the stage is off before and on failure.
static int image_alloc(mvsv_stream* st, ImageStage* g, const mvsv_rect& q, int bytes_per_px, const char* oom)
{
    *g = {};
    g->roi = q;
    g->row_bytes = (size_t)bytes_per_px * g->width();
    g->bytes = g->row_bytes * g->height();
    g->lay = ring_slot_block(g->bytes, alignof(int16_t), 2 * sizeof(int16_t), 0);
    const size_t depth = st->slots.size();
    if (!(g->dImg.alloc(depth * g->bytes) && g->dMM.alloc(depth * 2) && g->host.alloc(depth * g->lay.bytes)))
        return stage_oom(st, g, oom);
    g->on = true;
    return MVSV_OK;
}

// The oldest pending frame of an image stage; host: what is read is the pinned image.
static int image_front(mvsv_stream* st, const ImageStage& g, const ImageTexts& t, bool host, long* idx)
{
    if (host && g.on && !(st->host_mask & t.host_bit)) return set_error(st->ctx, MVSV_E_INVALID_ARG, t.host_off);
    return front_slot(st, g.on, t.not_enabled, idx);
}

// front_display / front_view: the image copied into the caller's rows
static int image_front_copy(mvsv_stream* st, ImageStage mvsv_stream::*stage, const ImageTexts& t, uint8_t* out,
                            size_t out_stride, int16_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    const ImageStage& g = st->*stage;
    if (g.on && out && out_stride < g.row_bytes) return set_error(st->ctx, MVSV_E_INVALID_ARG, t.stride);
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    if (int rc = image_front(st, g, t, true, &idx)) return rc;
    if (out) copy_rows(out, out_stride, g.image(idx), g.row_bytes, g.row_bytes, g.height(), 0, 1);
    if (minmax) std::memcpy(minmax, g.minmax(idx), 2 * sizeof(int16_t));
    return MVSV_OK;
}

// front_*_view (host) / front_*_device: the image where it is, valid until the slot's reuse
static int image_front_ptr(mvsv_stream* st, ImageStage mvsv_stream::*stage, const ImageTexts& t, bool host,
                           const uint8_t** image, int16_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (!image) return set_error(st->ctx, MVSV_E_INVALID_ARG, t.null_out);
    const ImageStage& g = st->*stage;
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    if (int rc = image_front(st, g, t, host, &idx)) return rc;
    *image = host ? g.image(idx) : g.dev_image(idx);
    if (minmax) std::memcpy(minmax, g.minmax(idx), 2 * sizeof(int16_t));
    return MVSV_OK;
}

int mvsv_stream_disable_display(mvsv_stream* st)
{
    return stage_disable(st, &mvsv_stream::disp, "the display changes");
}

int mvsv_stream_enable_display(mvsv_stream* st, const mvsv_rect* roi, double alpha, double beta)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!std::isfinite(alpha) || !std::isfinite(beta))
        return set_error(ctx, MVSV_E_INVALID_ARG, "display alpha / beta must be finite");
    if (int rc = idle_check(st, "the display changes")) return rc;
    mvsv_rect q;
    if (!roi_or_whole(roi, st->W, st->H, &q))
        return set_error(ctx, MVSV_E_INVALID_ARG, "display ROI empty or outside the image");
    DeviceGuard dev_guard(ctx->device);
    st->disp_alpha = alpha;
    st->disp_beta = beta;
    return image_alloc(st, &st->disp, q, 1, "display buffer allocation failed");
}

int mvsv_stream_front_display(mvsv_stream* st, uint8_t* out, size_t out_stride, int16_t* minmax)
{
    return image_front_copy(st, &mvsv_stream::disp, kDisplayTexts, out, out_stride, minmax);
}

int mvsv_stream_front_display_view(mvsv_stream* st, const uint8_t** map, int16_t* minmax)
{
    return image_front_ptr(st, &mvsv_stream::disp, kDisplayTexts, true, map, minmax);
}

int mvsv_stream_disable_view(mvsv_stream* st) { return stage_disable(st, &mvsv_stream::view, "the view changes"); }

int mvsv_stream_enable_view(mvsv_stream* st, const mvsv_rect* roi, const mvsv_view_spec* spec)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    mvsv_rect q;
    if (!roi_or_whole(roi, st->W, st->H, &q))
        return set_error(ctx, MVSV_E_INVALID_ARG, "view ROI empty or outside the image");
    if (const char* why = view_check(spec, q.x1 - q.x0, q.y1 - q.y0)) return set_error(ctx, MVSV_E_INVALID_ARG, why);
    if (int rc = idle_check(st, "the view changes")) return rc;
    if ((spec->layers & MVSV_VIEW_FOUND_TILES) && !(st->grid && same_rect(st->roi, q)))
        return set_error(ctx, MVSV_E_INVALID_ARG, "FOUND_TILES needs a stream created with a grid_roi equal to the view's ROI");
    if ((spec->layers & MVSV_VIEW_FOUND_POINTS) && !(st->sp.on && same_rect(st->sp.roi, q)))
        return set_error(ctx, MVSV_E_INVALID_ARG, "FOUND_POINTS needs sample points enabled with the view's ROI");
    DeviceGuard dev_guard(ctx->device);
    st->view_spec = *spec;
    return image_alloc(st, &st->view, q, 3, "view buffer allocation failed");
}

int mvsv_stream_front_view(mvsv_stream* st, uint8_t* out, size_t out_stride, int16_t* minmax)
{
    return image_front_copy(st, &mvsv_stream::view, kViewTexts, out, out_stride, minmax);
}

int mvsv_stream_front_view_view(mvsv_stream* st, const uint8_t** view, int16_t* minmax)
{
    return image_front_ptr(st, &mvsv_stream::view, kViewTexts, true, view, minmax);
}

// ---- sharpness ----

int mvsv_stream_disable_sharpness(mvsv_stream* st)
{
    return stage_disable(st, &mvsv_stream::sharp, "the sharpness changes");
}

int mvsv_stream_enable_sharpness(mvsv_stream* st, const mvsv_rect* roi_left, const mvsv_rect* roi_right)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (int rc = idle_check(st, "the sharpness changes")) return rc;
    // the pushed images' size
    const int iw = st->raw ? st->rawW : st->W, ih = st->raw ? st->rawH : st->H;
    mvsv_rect q[2];
    if (!roi_or_whole(roi_left, iw, ih, &q[0]) || !roi_or_whole(roi_right, iw, ih, &q[1]))
        return set_error(ctx, MVSV_E_INVALID_ARG, "sharpness ROI empty or outside the pushed image");
    DeviceGuard dev_guard(ctx->device);
    Sharpness& sh = st->sharp;
    sh = {};
    sh.roi[0] = q[0];
    sh.roi[1] = q[1];
    if (!(sh.dSum.alloc(2 * st->slots.size()) && sh.hSum.alloc(2 * st->slots.size())))
        return stage_oom(st, &sh, "sharpness buffer allocation failed");
    sh.on = true;
    return MVSV_OK;
}

int mvsv_stream_front_sharpness(mvsv_stream* st, double value[2], int64_t sum4[2])
{
    if (!st) return MVSV_E_INVALID_ARG;
    const Sharpness& sh = st->sharp;
    int rc;
    if ((rc = front_check(st, sh.on, "the sharpness is not enabled on this stream"))) return rc;
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    if ((rc = front_wait(st, &idx))) return rc;
    for (int i = 0; i < 2; i++) {
        const mvsv_rect& q = sh.roi[i];
        const int64_t s4 = sh.hSum[2 * idx + i];
        if (sum4) sum4[i] = s4;
        // cv::mean: sum * (1.0 / N), a reciprocal and a product, each rounded
        if (value) value[i] = ((double)s4 / 4.0) * (1.0 / ((double)(q.x1 - q.x0) * (double)(q.y1 - q.y0)));
    }
    return MVSV_OK;
}

// ---- point cloud ----

int mvsv_stream_disable_cloud(mvsv_stream* st)
{
    return stage_disable(st, &mvsv_stream::cloud, "the point cloud changes");
}

int mvsv_stream_enable_cloud(mvsv_stream* st, const mvsv_rect* roi, const float* Q, int max_points)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    if (!Q) return set_error(ctx, MVSV_E_INVALID_ARG, "null Q matrix");
    if (int rc = idle_check(st, "the point cloud changes")) return rc;
    mvsv_rect q;
    if (!roi_or_whole(roi, st->W, st->H, &q))
        return set_error(ctx, MVSV_E_INVALID_ARG, "point cloud ROI empty or outside the image");
    const size_t roi_px = (size_t)(q.x1 - q.x0) * (q.y1 - q.y0);
    if (roi_px > (size_t)INT32_MAX) return set_error(ctx, MVSV_E_INVALID_ARG, "point cloud ROI too large");
    DeviceGuard dev_guard(ctx->device);
    Cloud& c = st->cloud;
    c = {};
    c.roi = q;
    std::memcpy(c.Q, Q, sizeof(c.Q));
    c.max_points = (int)(max_points <= 0 ? roi_px : std::min((size_t)max_points, roi_px));
    const size_t depth = st->slots.size();
    if (!(c.dRec.alloc(depth * (size_t)c.max_points) && c.dHdr.alloc(depth * 3) && c.hHdr.alloc(depth * 3) &&
          c.copy.create()))
        return stage_oom(st, &c, "point cloud buffer allocation failed");
    c.on = true;
    return MVSV_OK;
}

// the oldest pending frame's cloud header; its slot index in *idx
static int cloud_front(mvsv_stream* st, long* idx, int* count, int32_t* minmax)
{
    if (int rc = front_slot(st, st->cloud.on, "the point cloud is not enabled on this stream", idx)) return rc;
    const int* h = st->cloud.hHdr + 3 * *idx;
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
    const Cloud& c = st->cloud;
    long idx;
    int rc;
    if ((rc = cloud_front(st, &idx, count, minmax))) return rc;
    const size_t k = records ? (size_t)std::min(std::min(c.hHdr[3 * idx], c.max_points), capacity) : 0;
    if (k == 0) return MVSV_OK;
    // the frame is complete; a stream of its own, so the copy does not queue behind the later frames' downloads
    if ((rc = check_hip(st->ctx, hipMemcpyAsync(records, c.dev_records(idx), k * sizeof(mvsv_cloud_point),
                                                hipMemcpyDeviceToHost, c.copy), "stream D2H")))
        return rc;
    return check_hip(st->ctx, hipStreamSynchronize(c.copy), "stream sync");
}

int mvsv_stream_front_cloud_device(mvsv_stream* st, const mvsv_cloud_point** records_dev, int* count, int32_t* minmax)
{
    if (!st) return MVSV_E_INVALID_ARG;
    if (!records_dev) return set_error(st->ctx, MVSV_E_INVALID_ARG, "null records pointer");
    DeviceGuard dev_guard(st->ctx->device);
    long idx;
    if (int rc = cloud_front(st, &idx, count, minmax)) return rc;
    *records_dev = st->cloud.dev_records(idx);
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

// n frames from device-readable memory into the next n slots: one copy launch per
// contiguous ring segment on the upload stream, ordered against the producer's
// stream by events in both directions; then the bookkeeping of n single pushes.
static int stream_push_device(mvsv_stream* st, PushKind kind, int n, const uint8_t* L, size_t ls, size_t lfs,
                              const uint8_t* R, size_t rs, size_t rfs, void* producer)
{
    if (!st) return MVSV_E_INVALID_ARG;
    mvsv_ctx* ctx = st->ctx;
    int rc;
    if ((rc = push_kind_check(st, kind, true))) return rc;
    const PushGeom g = st->push_geom(kind);
    const int rows = g.rows;
    const size_t row = g.row;  // of the source; the slots' rows are g.stride apart
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
    const bool colour = kind == kPushBgr && st->bgr.match;
    if ((rc = stream_kind_boundary(st, colour))) return rc;
    hipStream_t prod = (hipStream_t)producer;
    if ((rc = check_hip(ctx, hipEventRecord(st->producer_ev, prod), "stream event")) ||
        (rc = check_hip(ctx, hipStreamWaitEvent(st->up, st->producer_ev, 0), "stream wait")))
        return rc;
    RingRun seg[2];
    const int nseg = ring_push_segments(st->head, n, depth, seg);
    // the slots' previous frames were popped, so everything that read or wrote them is complete
    int done = 0;
    for (int s = 0; s < nseg; s++) {
        const PushEnds e = push_ends(st, kind, g, seg[s].i0);
        if ((rc = stream_copy_device(ctx, st->up, seg[s].n, L + done * lfs, ls, lfs, R + done * rfs, rs, rfs, e.dl,
                                     e.dr, g.stride, g.frame, (int)row, rows)))
            return rc;
        done += seg[s].n;
    }
    // n single pushes: a launch waits for the `uploaded` event of its last slot, which is
    // the frame that completes a group, the ring's last slot or the call's last frame
    hipEvent_t last = nullptr;
    for (int k = 0; k < n; k++) {
        auto& s = st->slots[st->head % depth];
        if (kind != kPushRaw) s.is_bgr = kind == kPushBgr;
        s.colour = colour;
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
    if (int rc = idle_check(st, "the host outputs change")) return rc;
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
    return image_front_ptr(st, &mvsv_stream::disp, kDisplayTexts, false, map_dev, minmax);
}

int mvsv_stream_front_view_device(mvsv_stream* st, const uint8_t** bgr_dev, int16_t* minmax)
{
    return image_front_ptr(st, &mvsv_stream::view, kViewTexts, false, bgr_dev, minmax);
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
    delete st;
}
