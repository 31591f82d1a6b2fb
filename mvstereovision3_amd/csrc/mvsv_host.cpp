// mvsv_host.cpp — host side of libmvsv: parameter resolution (OpenCV's
// defaulting + assert rules), context / stream / buffer management, and the
// one-shot entry points: each _device call next to its host-pointer twin, which
// stages one frame through the context's arena (mvsv_stage.hpp): check the
// arguments, reserve, upload, the _device call, download, finish.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>

#include "mvsv_internal.hpp"
#include "mvsv_stage.hpp"

namespace mvsv {

int set_error(mvsv_ctx* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

int check_hip(mvsv_ctx* ctx, hipError_t e, const char* what)
{
    if (e == hipSuccess) return MVSV_OK;
    return set_error(ctx, e == hipErrorOutOfMemory ? MVSV_E_OOM : MVSV_E_HIP,
                     std::string(what) + ": " + hipGetErrorString(e));
}

int ensure(mvsv_ctx* ctx, DevBuf& b, size_t bytes, const char* what)
{
    if (bytes <= b.bytes && b.ptr) return MVSV_OK;
    ++ctx->alloc_epoch;  // captured graphs hold the old addresses
    if (b.ptr) {
        // the stream may still use the old buffer
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(b.ptr);
        b.ptr = nullptr;
        b.bytes = 0;
    }
    if (bytes == 0) return MVSV_OK;
    hipError_t e = hipMalloc(&b.ptr, bytes);
    if (e != hipSuccess) {
        b.ptr = nullptr;
        (void)hipGetLastError();
        return set_error(ctx, MVSV_E_OOM,
                         std::string("device allocation of ") + std::to_string(bytes) +
                             " bytes for " + what + " failed");
    }
    b.bytes = bytes;
    return MVSV_OK;
}

int check_report(mvsv_ctx* ctx)
{
    if (!ctx->report) return MVSV_OK;
    // one read-and-clear: a give-up stored by a launch still in flight between a
    // separate load and store would be erased unreported
    const int v = __atomic_exchange_n(ctx->report, 0, __ATOMIC_ACQ_REL);
    if (v == 0) return MVSV_OK;
    return set_error(ctx, MVSV_E_TIMEOUT,
                     "sgbm path kernel: a strip-boundary wait gave up (that launch's maps are all "
                     "INVALID)");
}

int mark_last_use(mvsv_ctx* ctx, int rc)
{
    if (hipEventRecord(ctx->ev_last, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        return rc ? rc : set_error(ctx, MVSV_E_HIP, "last-use event record failed");
    }
    ctx->last_valid = true;
    return rc;
}

int alloc_report(mvsv_ctx* ctx, int count, int** host, int** dev)
{
    *host = nullptr;
    *dev = nullptr;
    void* h = nullptr;
    // fine-grained, coherent: kernels store into it with system scope and the
    // host reads it without a copy
    hipError_t e = hipHostMalloc(&h, sizeof(int) * (size_t)count,
                                 hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return check_hip(ctx, e, "report word allocation");
    std::memset(h, 0, sizeof(int) * (size_t)count);
    void* d = nullptr;
    e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(h);
        return check_hip(ctx, e, "report word mapping");
    }
    *host = (int*)h;
    *dev = (int*)d;
    return MVSV_OK;
}

static hipEvent_t pool_get(mvsv_ctx* ctx)
{
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return e;
}

StageTimer::StageTimer(mvsv_ctx* c, int s, hipStream_t on) : ctx(c), stage(s), st(on ? on : c->stream)
{
    if (!ctx->prof) return;
    a = pool_get(ctx);
    b = pool_get(ctx);
    if (a) (void)hipEventRecord(a, st);
}

StageTimer::~StageTimer()
{
    if (!ctx->prof || !a || !b) return;
    (void)hipEventRecord(b, st);
    ctx->marks.push_back({stage, a, b});
}

// [OpenCV] StereoSGBMImpl::compute asserts + computeDisparitySGBM prologue.
int resolve_sgbm(const mvsv_sgbm_params* p, int W, int H, SgbmEff* e, std::string* why)
{
    if (!p) { *why = "null parameters"; return MVSV_E_INVALID_ARG; }
    if (W <= 0 || H <= 0) { *why = "empty image"; return MVSV_E_INVALID_ARG; }
    if (p->num_disparities <= 0 || p->num_disparities % 16 != 0) {
        *why = "numDisparities must be positive and divisible by 16";
        return MVSV_E_INVALID_ARG;
    }
    if (p->mode == MVSV_MODE_SGBM_3WAY) {
        *why = "MODE_SGBM_3WAY (2) is not supported: mode must be MODE_SGBM (0), MODE_HH (1) or MODE_HH4 (3)";
        return MVSV_E_INVALID_ARG;
    }
    if (p->mode != MVSV_MODE_SGBM && p->mode != MVSV_MODE_HH && p->mode != MVSV_MODE_HH4) {
        *why = "mode must be MODE_SGBM (0), MODE_HH (1) or MODE_HH4 (3)";
        return MVSV_E_INVALID_ARG;
    }
    int bs = p->block_size > 0 ? p->block_size : 5;
    e->minD = p->min_disparity;
    e->D = p->num_disparities;
    e->maxD = e->minD + e->D;
    e->SW2 = bs / 2;
    e->SH2 = bs / 2;
    e->ftzero = std::max(p->pre_filter_cap, 15) | 1;
    e->uniq = p->uniqueness_ratio >= 0 ? p->uniqueness_ratio : 10;
    e->disp12 = p->disp12_max_diff > 0 ? p->disp12_max_diff : 1;
    e->P1 = p->p1 > 0 ? p->p1 : 2;
    e->P2 = std::max(p->p2 > 0 ? p->p2 : 5, e->P1 + 1);
    e->minX1 = std::max(e->maxD, 0);
    e->maxX1 = W + std::min(e->minD, 0);
    e->W1 = e->maxX1 - e->minX1;
    e->invalid = (e->minD - 1) * kDispScale;
    e->fullDP = p->mode == MVSV_MODE_HH;
    e->hh4 = p->mode == MVSV_MODE_HH4;
    e->variant = p->variant;
    e->speckle_window = p->speckle_window_size;
    e->speckle_diff = kDispScale * p->speckle_range;
    e->cn = 1;
    e->cw = e->ch = 0;
    if (e->W1 > 0 && e->W1 <= e->SW2) {
        *why = "image narrower than the SGBM block half-width (OpenCV reads uninitialised memory)";
        return MVSV_E_INVALID_ARG;
    }
    return MVSV_OK;
}

// A census call: mvsv_sgbm_validate's rules, the window rule, and no cost beyond int16.
int resolve_sgbm_census(const mvsv_sgbm_params* p, int W, int H, int cw, int ch, SgbmEff* e, std::string* why)
{
    if (int rc = resolve_sgbm(p, W, H, e, why)) return rc;
    if (const char* bad = census_window_check(cw, ch)) {
        *why = bad;
        return MVSV_E_INVALID_ARG;
    }
    e->cw = cw;
    e->ch = ch;
    const long bs = 2L * e->SW2 + 1;
    if ((long)e->P2 + bs * bs * sgbm_max_pixel_cost(*e) > 32767) {
        *why = "census cost: P2 + blockSize^2 * (width * height - 1) must be <= 32767 (no cost may leave int16)";
        return MVSV_E_INVALID_ARG;
    }
    return MVSV_OK;
}

// [OpenCV] StereoBMImpl::compute checks + findStereoCorrespondenceBM setup.
int resolve_bm(const mvsv_bm_params* p, int W, int H, BmEff* e, std::string* why)
{
    if (!p) { *why = "null parameters"; return MVSV_E_INVALID_ARG; }
    if (W <= 0 || H <= 0) { *why = "empty image"; return MVSV_E_INVALID_ARG; }
    if (p->pre_filter_type != MVSV_PREFILTER_NORMALIZED_RESPONSE &&
        p->pre_filter_type != MVSV_PREFILTER_XSOBEL) {
        *why = "preFilterType must be = CV_STEREO_BM_NORMALIZED_RESPONSE";
        return MVSV_E_INVALID_ARG;
    }
    if (p->pre_filter_size < 5 || p->pre_filter_size > 255 || p->pre_filter_size % 2 == 0) {
        *why = "preFilterSize must be odd and be within 5..255";
        return MVSV_E_INVALID_ARG;
    }
    if (p->pre_filter_cap < 1 || p->pre_filter_cap > 63) {
        *why = "preFilterCap must be within 1..63";
        return MVSV_E_INVALID_ARG;
    }
    if (p->block_size < 5 || p->block_size > 255 || p->block_size % 2 == 0 ||
        p->block_size >= std::min(W, H)) {
        *why = "SADWindowSize must be odd, be within 5..255 and be not larger than image width or height";
        return MVSV_E_INVALID_ARG;
    }
    if (p->num_disparities <= 0 || p->num_disparities % 16 != 0) {
        *why = "numDisparities must be positive and divisible by 16";
        return MVSV_E_INVALID_ARG;
    }
    if (p->texture_threshold < 0) { *why = "texture threshold must be non-negative"; return MVSV_E_INVALID_ARG; }
    if (p->uniqueness_ratio < 0) { *why = "uniqueness ratio must be non-negative"; return MVSV_E_INVALID_ARG; }
    e->ndisp = p->num_disparities;
    e->mindisp = p->min_disparity;
    e->wsz2 = p->block_size / 2;
    e->cap = p->pre_filter_cap;
    e->tex = p->texture_threshold;
    e->uniq = p->uniqueness_ratio;
    e->lofs = std::max(e->ndisp - 1 + e->mindisp, 0);
    e->rofs = -std::min(e->ndisp - 1 + e->mindisp, 0);
    e->width1 = W - e->rofs - e->ndisp + 1;
    e->ncol = std::min(e->width1, W - e->lofs);
    e->filtered = (e->mindisp - 1) * kDispScale;
    int maxDm1 = e->mindisp + e->ndisp - 1;
    e->xmin = std::max(0, maxDm1) + e->wsz2;
    e->xmax = W - e->wsz2;
    e->ymin = e->wsz2;
    e->ymax = H - e->wsz2;
    e->disp12 = p->disp12_max_diff;
    e->speckle_window = p->speckle_window_size;
    e->speckle_range = p->speckle_range;
    e->prefilter_type = p->pre_filter_type;
    e->prefilter_size = p->pre_filter_size;
    e->cw = e->ch = 0;
    return MVSV_OK;
}

// A census call: mvsv_bm_validate's rules and the window rule.  blockSize^2 * bits is
// at most 255^2 * 64 < 2^24: no sum leaves 32 bits or the (cost << 8 | index) keys.
int resolve_bm_census(const mvsv_bm_params* p, int W, int H, int cw, int ch, BmEff* e, std::string* why)
{
    if (int rc = resolve_bm(p, W, H, e, why)) return rc;
    if (const char* bad = census_window_check(cw, ch)) {
        *why = bad;
        return MVSV_E_INVALID_ARG;
    }
    e->cw = cw;
    e->ch = ch;
    return MVSV_OK;
}

}  // namespace mvsv

using namespace mvsv;

static void drop_graphs(mvsv_ctx* ctx)
{
    for (auto& g : ctx->graph_cache)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    ctx->graph_cache.clear();
    ctx->graph_seen.clear();
}

// Replay of repeated small launches as HIP graphs.  `key` holds every argument
// of the call; the first call with a key runs eagerly, an immediate repeat is
// captured (on the context's capture stream, so a caller on the legacy null
// stream is served too) and every later one launches the instantiated graph on
// the context stream.  Any failure of the capture path turns graphs off for the
// context and runs the call eagerly.
constexpr size_t kGraphCache = 4;
static int graph_run(mvsv_ctx* ctx, const std::vector<unsigned char>& key, const std::function<int()>& body)
{
    for (auto& g : ctx->graph_cache) {
        if (g.key != key) continue;
        if (g.epoch == ctx->alloc_epoch) {
            g.used = ++ctx->graph_clock;
            return check_hip(ctx, hipGraphLaunch(g.exec, ctx->stream), "graph launch");
        }
        (void)hipGraphExecDestroy(g.exec);  // its buffers were reallocated
        g.exec = nullptr;
        g.key.clear();
    }
    if (ctx->graph_seen != key) {
        ctx->graph_seen = key;
        return body();
    }
    static const bool dbg = std::getenv("MVSV_GRAPH_DEBUG") != nullptr;
    auto fail = [&]() {
        const hipError_t le = hipGetLastError();
        if (dbg) std::fprintf(stderr, "[mvsv graph] capture failed (%s); graphs off for this context\n",
                              hipGetErrorString(le));
        ctx->graphs = 0;
        ctx->graph_seen.clear();
        return body();
    };
    if (!ctx->cap && hipStreamCreateWithFlags(&ctx->cap, hipStreamNonBlocking) != hipSuccess) return fail();
    const unsigned ep = ctx->alloc_epoch;
    if (hipStreamBeginCapture(ctx->cap, hipStreamCaptureModeRelaxed) != hipSuccess) return fail();
    hipStream_t keep = ctx->stream;
    ctx->stream = ctx->cap;
    const int rc = body();
    ctx->stream = keep;
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(ctx->cap, &graph);
    hipGraphExec_t exec = nullptr;
    const bool ok = rc == MVSV_OK && ce == hipSuccess && graph && ctx->alloc_epoch == ep &&
                    hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) return fail();
    // keep the kGraphCache most recently used graphs
    auto slot = ctx->graph_cache.end();
    for (auto it = ctx->graph_cache.begin(); it != ctx->graph_cache.end(); ++it)
        if (!it->exec) slot = it;
    if (slot == ctx->graph_cache.end() && ctx->graph_cache.size() >= kGraphCache) {
        slot = std::min_element(ctx->graph_cache.begin(), ctx->graph_cache.end(),
                                [](const mvsv_ctx::GraphEntry& a, const mvsv_ctx::GraphEntry& b) {
                                    return a.used < b.used;
                                });
        (void)hipGraphExecDestroy(slot->exec);
    }
    if (slot == ctx->graph_cache.end()) {
        ctx->graph_cache.emplace_back();
        slot = ctx->graph_cache.end() - 1;
    }
    slot->key = key;
    slot->exec = exec;
    slot->epoch = ep;
    slot->used = ++ctx->graph_clock;
    ctx->graph_seen.clear();
    if (dbg)
        std::fprintf(stderr, "[mvsv graph] captured a %zu-byte key, %zu cached\n", key.size(),
                     ctx->graph_cache.size());
    return check_hip(ctx, hipGraphLaunch(exec, ctx->stream), "graph launch");
}

template <typename T>
static void key_put(std::vector<unsigned char>& k, const T& v)
{
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
    k.insert(k.end(), p, p + sizeof(T));
}

extern "C" {

int mvsv_sgbm_validate(const mvsv_sgbm_params* p, int W, int H)
{
    SgbmEff e;
    std::string why;
    return resolve_sgbm(p, W, H, &e, &why);
}

int mvsv_sgbm_census_validate(const mvsv_sgbm_params* p, int W, int H, int cw, int ch)
{
    SgbmEff e;
    std::string why;
    return resolve_sgbm_census(p, W, H, cw, ch, &e, &why);
}

int mvsv_bm_validate(const mvsv_bm_params* p, int W, int H)
{
    BmEff e;
    std::string why;
    return resolve_bm(p, W, H, &e, &why);
}

int mvsv_bm_census_validate(const mvsv_bm_params* p, int W, int H, int cw, int ch)
{
    BmEff e;
    std::string why;
    return resolve_bm_census(p, W, H, cw, ch, &e, &why);
}

int mvsv_create(mvsv_ctx** out, int hip_device)
{
    if (!out) return MVSV_E_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return MVSV_E_NODEV;
    }
    if (hip_device < 0 || hip_device >= count) return MVSV_E_INVALID_ARG;
    mvsv_ctx* c = new (std::nothrow) mvsv_ctx();
    if (!c) return MVSV_E_OOM;
    c->device = hip_device;
    DeviceGuard dev_guard(hip_device);
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_last, hipEventDisableTiming) != hipSuccess ||
        alloc_report(c, 1, &c->report, &c->report_dev) != MVSV_OK) {
        (void)hipGetLastError();
        if (c->ev_last) (void)hipEventDestroy(c->ev_last);
        if (c->own) (void)hipStreamDestroy(c->own);
        delete c;
        return MVSV_E_HIP;
    }
    c->report_target = c->report_dev;
    c->stream = c->own;
    if (const char* v = std::getenv("MVSV_STRIP_SPIN_LIMIT"))
        c->opt.spin_limit = (unsigned)std::strtoul(v, nullptr, 0);
    // kernel-variant switches for A/B measurement and for testing the
    // general-shape kernels on shapes the specialised ones also cover
    if (const char* v = std::getenv("MVSV_KERNELS")) {
        if (std::strstr(v, "cost-lds")) c->opt.cost2 = 0;
        if (std::strstr(v, "path-wave")) c->opt.path16 = 0;
        if (std::strstr(v, "path-lines")) c->opt.tri = 0;
        if (std::strstr(v, "bm-tile")) c->opt.bm2 = 0;
        if (std::strstr(v, "cost-generic")) c->opt.cost_fixed_pp = 0;
    }
    if (const char* v = std::getenv("MVSV_COST_TY")) c->opt.cost_ty = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("MVSV_PATH_SCHEDULE")) c->opt.path_sched = std::max(0, std::min(2, std::atoi(v)));
    if (const char* v = std::getenv("MVSV_STRIP_WAVES")) c->opt.strip_waves = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("MVSV_TRI32")) c->opt.tri32 = std::atoi(v) != 0;
    if (const char* v = std::getenv("MVSV_FINAL_SPLIT")) c->opt.final_split = std::atoi(v) != 0;
    if (const char* v = std::getenv("MVSV_COST_RESIDUAL")) c->opt.cost_res = std::atoi(v) != 0;
    if (const char* v = std::getenv("MVSV_BM_TY")) c->opt.bm_ty = std::max(0, std::min(128, std::atoi(v)));
    if (hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, hip_device) != hipSuccess) {
        (void)hipGetLastError();
        c->cus = 256;
    }
    if (const char* v = std::getenv("MVSV_STRIP_ORDER")) c->opt.strip_tickets = std::strcmp(v, "blockidx") != 0;
    if (const char* v = std::getenv("MVSV_LINES_AUX")) c->opt.lines_aux = std::max(-1, std::min(2, std::atoi(v)));
    if (const char* v = std::getenv("MVSV_BITSLICE")) c->opt.bitslice = std::atoi(v) != 0;
    if (const char* v = std::getenv("MVSV_GRAPHS")) c->graphs = std::atoi(v) != 0;
    if (const char* v = std::getenv("MVSV_BS_SERIAL")) c->opt.bs_serial = std::atoi(v) != 0;
    if (const char* v = std::getenv("MVSV_COST_XCD")) c->opt.cost_xcd = std::atoi(v) != 0;
    if (const char* v = std::getenv("MVSV_BS_FUSE")) c->opt.bs_fuse = std::atoi(v) != 0;
    c->opt.tri_stats = std::getenv("MVSV_TRI_STATS") != nullptr;
    if (const char* v = std::getenv("MVSV_TRI_TRACE")) c->opt.tri_trace = v;
    c->opt.bs_stats = std::getenv("MVSV_BS_STATS") != nullptr;
    if (const char* v = std::getenv("MVSV_BS_LDSPAD")) c->opt.bs_ldspad = std::max(0L, std::atol(v));
    if (const char* v = std::getenv("MVSV_BS_GROUPS")) {
        const int g = std::atoi(v);
        c->opt.bs_groups = (g >= 1 && g <= 5) ? g : 0;
    }
    *out = c;
    return MVSV_OK;
}

static void free_buf(DevBuf& b)
{
    if (b.ptr) (void)hipFree(b.ptr);  // (the caller bumps alloc_epoch)
    b.ptr = nullptr;
    b.bytes = 0;
}

int mvsv_trim(mvsv_ctx* ctx)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    ++ctx->alloc_epoch;
    DeviceGuard dev_guard(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    DevBuf* all[] = {&ctx->pre, &ctx->cost, &ctx->cres, &ctx->agg, &ctx->raw, &ctx->uf_parent, &ctx->uf_size, &ctx->uf_lroot, &ctx->uf_list,
                     &ctx->uf_tile, &ctx->tri_bnd, &ctx->bs_bnd, &ctx->status,
                     &ctx->dummy, &ctx->keys,
                     &ctx->bm_lf, &ctx->bm_rf, &ctx->bm_cost, &ctx->bm_sad, &ctx->stage,
                     &ctx->mm_part, &ctx->cl_rows, &ctx->sh_part, &ctx->ud_maps};
    for (DevBuf* b : all) free_buf(*b);
    ctx->ud_key.clear();
    return MVSV_OK;
}

static const char* kStageNames[MVSV_NUM_STAGES] = {
    "prefilter", "cost_volume", "cost_fixup", "path_aggregation", "final_wta_lr", "post_filters",
    "bm_match", "path_strips", "path_lines"};

const char* mvsv_profile_stage_name(int s)
{
    return (s >= 0 && s < MVSV_NUM_STAGES) ? kStageNames[s] : "";
}

int mvsv_profile_enable(mvsv_ctx* ctx, int on)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    ctx->prof = on ? 1 : 0;
    return MVSV_OK;
}

int mvsv_profile_reset(mvsv_ctx* ctx)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& m : ctx->marks) {
        ctx->event_pool.push_back(m.a);
        ctx->event_pool.push_back(m.b);
    }
    ctx->marks.clear();
    return MVSV_OK;
}

int mvsv_profile_read(mvsv_ctx* ctx, double* ms, int* launches, int n)
{
    if (!ctx || n < 0) return MVSV_E_INVALID_ARG;
    DeviceGuard dev_guard(ctx->device);
    int rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        if (ms) ms[i] = 0.0;
        if (launches) launches[i] = 0;
    }
    for (auto& m : ctx->marks) {
        if (m.stage >= n) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, m.a, m.b) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        if (ms) ms[m.stage] += t;
        if (launches) launches[m.stage] += 1;
    }
    return MVSV_OK;
}

void mvsv_destroy(mvsv_ctx* ctx)
{
    if (!ctx) return;
    drop_graphs(ctx);
    mvsv_trim(ctx);
    if (ctx->cap) (void)hipStreamDestroy(ctx->cap);
    mvsv_profile_reset(ctx);
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_last) (void)hipEventDestroy(ctx->ev_last);
    if (ctx->report) (void)hipHostFree(ctx->report);
    if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
    if (ctx->own) (void)hipStreamDestroy(ctx->own);
    delete ctx;
}

const char* mvsv_last_error(const mvsv_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// Every launch of a context shares its cached buffers, so work enqueued on a
// new stream must not start before the context's work already enqueued: the
// new stream waits on the context's last-use event (recorded by the entry
// points themselves, so neither the previous stream handle -- possibly
// destroyed by its owner since -- nor unrelated work queued on it is touched).
static int switch_stream(mvsv_ctx* ctx, hipStream_t s)
{
    if (s == ctx->stream) return MVSV_OK;
    DeviceGuard dev_guard(ctx->device);
    if (ctx->last_valid) {
        int rc = check_hip(ctx, hipStreamWaitEvent(s, ctx->ev_last, 0), "stream switch wait");
        if (rc) return rc;
    }
    ctx->stream = s;
    return MVSV_OK;
}

int mvsv_set_stream(mvsv_ctx* ctx, void* s)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    return switch_stream(ctx, (hipStream_t)s);  // NULL = the HIP null stream
}

int mvsv_use_own_stream(mvsv_ctx* ctx)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    return switch_stream(ctx, ctx->own);
}

int mvsv_set_option(mvsv_ctx* ctx, int option, long long value)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    switch (option) {
    case MVSV_OPT_STRIP_SPIN_LIMIT:
        if (value < 0 || value > 0xffffffffLL)
            return set_error(ctx, MVSV_E_INVALID_ARG, "spin limit must be 0..2^32-1");
        ctx->opt.spin_limit = (unsigned)value;
        return MVSV_OK;
    case MVSV_OPT_BM_TILE_ROWS:
        if (value < 0 || value > 128) return set_error(ctx, MVSV_E_INVALID_ARG, "BM tile rows must be 0..128");
        ctx->opt.bm_ty = (int)value;
        return MVSV_OK;
    case MVSV_OPT_PATH_SCHEDULE:
        if (value < 0 || value > 2) return set_error(ctx, MVSV_E_INVALID_ARG, "path schedule must be 0..2");
        ctx->opt.path_sched = (int)value;
        return MVSV_OK;
    case MVSV_OPT_STRIP_WAVES:
        if (value < 0 || value > 64) return set_error(ctx, MVSV_E_INVALID_ARG, "strip waves must be 0..64");
        ctx->opt.strip_waves = (int)value;
        return MVSV_OK;
    case MVSV_OPT_STRIP_TICKETS:
        if (value < 0 || value > 1) return set_error(ctx, MVSV_E_INVALID_ARG, "strip tickets must be 0 or 1");
        ctx->opt.strip_tickets = (int)value;
        return MVSV_OK;
    case MVSV_OPT_COST_RESIDUAL:
        if (value < 0 || value > 1) return set_error(ctx, MVSV_E_INVALID_ARG, "cost residual must be 0 or 1");
        ctx->opt.cost_res = (int)value;
        return MVSV_OK;
    case MVSV_OPT_BITSLICE:
        if (value < 0 || value > 1) return set_error(ctx, MVSV_E_INVALID_ARG, "bitslice must be 0 or 1");
        ctx->opt.bitslice = (int)value;
        return MVSV_OK;
    default:
        return set_error(ctx, MVSV_E_INVALID_ARG, "unknown option");
    }
}

void* mvsv_get_stream(mvsv_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int mvsv_synchronize(mvsv_ctx* ctx)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    DeviceGuard dev_guard(ctx->device);
    int rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return rc ? rc : check_report(ctx);
}

// the bytes of the call whose effective parameters are e
static size_t workspace_bytes(const SgbmEff& e, int n, int W, int H)
{
    // what a context with default kernel options on a 256-CU device allocates:
    // the plan's buffers, and the speckle filter's
    const SgbmPlan plan = sgbm_make_plan(KernelOptions(), 256, e, n, W, H);
    if (plan.empty) return 0;  // an empty column range only fills the map
    return plan.total_bytes() + (e.speckle_window > 0 ? speckle_bytes(n, W, H).total() : 0);
}

size_t mvsv_sgbm_workspace_bytes_census(int n, int W, int H, const mvsv_sgbm_params* p, int cw, int ch)
{
    SgbmEff e;
    std::string why;
    if (n <= 0 || resolve_sgbm_census(p, W, H, cw, ch, &e, &why) != MVSV_OK) return 0;
    return workspace_bytes(e, n, W, H);
}

int mvsv_sgbm_plan_census(mvsv_ctx* ctx, int n, int W, int H, const mvsv_sgbm_params* p, int cw, int ch, int* plan)
{
    if (!ctx || !plan || n <= 0) return MVSV_E_INVALID_ARG;
    SgbmEff e;
    std::string why;
    const int rc = resolve_sgbm_census(p, W, H, cw, ch, &e, &why);
    if (rc) return set_error(ctx, rc, why);
    *plan = sgbm_make_plan(ctx, e, n, W, H).bits();
    return MVSV_OK;
}

size_t mvsv_sgbm_workspace_bytes_cn(int n, int W, int H, const mvsv_sgbm_params* p, int cn)
{
    SgbmEff e;
    std::string why;
    if (n <= 0 || (cn != 1 && cn != 3) || resolve_sgbm(p, W, H, &e, &why) != MVSV_OK) return 0;
    e.cn = cn;
    return workspace_bytes(e, n, W, H);
}

size_t mvsv_sgbm_workspace_bytes(int n, int W, int H, const mvsv_sgbm_params* p)
{
    return mvsv_sgbm_workspace_bytes_cn(n, W, H, p, 1);
}

int mvsv_sgbm_plan_cn(mvsv_ctx* ctx, int n, int W, int H, const mvsv_sgbm_params* p, int cn, int* plan)
{
    if (!ctx || !plan || n <= 0) return MVSV_E_INVALID_ARG;
    if (cn != 1 && cn != 3) return set_error(ctx, MVSV_E_INVALID_ARG, "channels must be 1 or 3");
    SgbmEff e;
    std::string why;
    const int rc = resolve_sgbm(p, W, H, &e, &why);
    if (rc) return set_error(ctx, rc, why);
    e.cn = cn;
    *plan = sgbm_make_plan(ctx, e, n, W, H).bits();
    return MVSV_OK;
}

int mvsv_sgbm_plan(mvsv_ctx* ctx, int n, int W, int H, const mvsv_sgbm_params* p, int* plan)
{
    return mvsv_sgbm_plan_cn(ctx, n, W, H, p, 1, plan);
}

}  // extern "C"

// mvsv_sgbm_device (cn 1) / mvsv_sgbm_bgr_device (cn 3: W in pixels, rows of 3 W bytes) /
// mvsv_sgbm_census_device (cn 1, census: the cw x ch window)
static int sgbm_device_call(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                            size_t rs, size_t rfs, int W, int H, const mvsv_sgbm_params* p, int16_t* out,
                            size_t os, size_t ofs, int cn, bool census = false, int cw = 0, int ch = 0)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !L || !R || !out) return set_error(ctx, MVSV_E_INVALID_ARG, "null buffer or n <= 0");
    if (ls < (size_t)W * cn || rs < (size_t)W * cn || os < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "stride smaller than width");
    SgbmEff e;
    std::string why;
    int rc = census ? resolve_sgbm_census(p, W, H, cw, ch, &e, &why) : resolve_sgbm(p, W, H, &e, &why);
    if (rc) return set_error(ctx, rc, why);
    e.cn = cn;
    // an earlier launch that has finished by now gave up a strip wait: its
    // maps are INVALID; say so before anything else runs on this context
    if ((rc = check_report(ctx))) return rc;
    DeviceGuard dev_guard(ctx->device);
    auto body = [&]() { return sgbm_device(ctx, n, L, ls, lfs, R, rs, rfs, W, H, e, out, os, ofs); };
    // small launches (one camera frame): one graph launch instead of ~8 kernel
    // launches (config 3, one 640x480 frame: ~5 us of launch gap per kernel)
    if (ctx->graphs && !ctx->prof && sgbm_make_plan(ctx, e, n, W, H).graphable()) {
        std::vector<unsigned char> key;
        key_put(key, 'S');
        key_put(key, n);
        key_put(key, L);
        key_put(key, ls);
        key_put(key, lfs);
        key_put(key, R);
        key_put(key, rs);
        key_put(key, rfs);
        key_put(key, W);
        key_put(key, H);
        key_put(key, e);
        key_put(key, out);
        key_put(key, os);
        key_put(key, ofs);
        return mark_last_use(ctx, graph_run(ctx, key, body));
    }
    return mark_last_use(ctx, body());
}

extern "C" {

int mvsv_sgbm_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs,
                     const uint8_t* R, size_t rs, size_t rfs, int W, int H,
                     const mvsv_sgbm_params* p, int16_t* out, size_t os, size_t ofs)
{
    return sgbm_device_call(ctx, n, L, ls, lfs, R, rs, rfs, W, H, p, out, os, ofs, 1);
}

int mvsv_sgbm_bgr_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs,
                         const uint8_t* R, size_t rs, size_t rfs, int W, int H,
                         const mvsv_sgbm_params* p, int16_t* out, size_t os, size_t ofs)
{
    return sgbm_device_call(ctx, n, L, ls, lfs, R, rs, rfs, W, H, p, out, os, ofs, 3);
}

int mvsv_sgbm_census_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs,
                            const uint8_t* R, size_t rs, size_t rfs, int W, int H,
                            const mvsv_sgbm_params* p, int16_t* out, size_t os, size_t ofs, int cw, int ch)
{
    return sgbm_device_call(ctx, n, L, ls, lfs, R, rs, rfs, W, H, p, out, os, ofs, 1, true, cw, ch);
}

int mvsv_census_device(mvsv_ctx* ctx, int n, const uint8_t* img, size_t st, size_t fs, int W, int H, int cw, int ch,
                       uint64_t* out, size_t os, size_t ofs)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !img || !out || W <= 0 || H <= 0) return set_error(ctx, MVSV_E_INVALID_ARG, "null buffer, empty image or n <= 0");
    if (st < (size_t)W || os < (size_t)W) return set_error(ctx, MVSV_E_INVALID_ARG, "stride smaller than width");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, census_device(ctx, n, 1, img, st, fs, img, st, fs, W, H, cw, ch, out, os, 0, ofs));
}

// mvsv_bm_device / mvsv_bm_census_device (census: the cw x ch window)
static int bm_device_call(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                          size_t rs, size_t rfs, int W, int H, const mvsv_bm_params* p, int16_t* out, size_t os,
                          size_t ofs, bool census, int cw, int ch)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !L || !R || !out) return set_error(ctx, MVSV_E_INVALID_ARG, "null buffer or n <= 0");
    if (ls < (size_t)W || rs < (size_t)W || os < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "stride smaller than width");
    BmEff e;
    std::string why;
    int rc = census ? resolve_bm_census(p, W, H, cw, ch, &e, &why) : resolve_bm(p, W, H, &e, &why);
    if (rc) return set_error(ctx, rc, why);
    DeviceGuard dev_guard(ctx->device);
    auto body = [&]() { return bm_device(ctx, n, L, ls, lfs, R, rs, rfs, W, H, e, out, os, ofs); };
    // StereoBM launches carry no per-launch state: repeats replay as a graph
    // (config 2, one 640x480 frame: 0.045 ms per call, ~6 kernel launches)
    if (ctx->graphs && !ctx->prof) {
        std::vector<unsigned char> key;
        key_put(key, 'B');
        key_put(key, n);
        key_put(key, L);
        key_put(key, ls);
        key_put(key, lfs);
        key_put(key, R);
        key_put(key, rs);
        key_put(key, rfs);
        key_put(key, W);
        key_put(key, H);
        key_put(key, e);
        key_put(key, out);
        key_put(key, os);
        key_put(key, ofs);
        return mark_last_use(ctx, graph_run(ctx, key, body));
    }
    return mark_last_use(ctx, body());
}

int mvsv_bm_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs,
                   const uint8_t* R, size_t rs, size_t rfs, int W, int H,
                   const mvsv_bm_params* p, int16_t* out, size_t os, size_t ofs)
{
    return bm_device_call(ctx, n, L, ls, lfs, R, rs, rfs, W, H, p, out, os, ofs, false, 0, 0);
}

int mvsv_bm_census_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
                          size_t rs, size_t rfs, int W, int H, const mvsv_bm_params* p, int16_t* out, size_t os,
                          size_t ofs, int cw, int ch)
{
    return bm_device_call(ctx, n, L, ls, lfs, R, rs, rfs, W, H, p, out, os, ofs, true, cw, ch);
}

int mvsv_mean_disparity_grid_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st,
                                    size_t fs, int W, int H, float* means)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !dmap || !means || W <= 0 || H <= 0 || st < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad mean-grid arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, mean_grid_device(ctx, n, dmap, st, fs, W, H, means));
}

int mvsv_mean_disparity_grid(mvsv_ctx* ctx, const int16_t* dmap, size_t st, int W, int H, float* means)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (!dmap || !means || W <= 0 || H <= 0 || st < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad mean-grid arguments");
    DeviceGuard dev_guard(ctx->device);
    const MapFloatsStage s(W, H, 81);
    return staged_call(ctx, s, "grid staging", [&](Staging& sg) -> int {
        int rc;
        int16_t* d = sg.at<int16_t>(s.map);
        float* m = sg.at<float>(s.floats);
        if ((rc = sg.up(d, s.map.pitch, dmap, st * 2, (size_t)W * 2, H, "H2D map")) ||
            (rc = mean_grid_device(ctx, 1, d, W, s.map.bytes / 2, W, H, m)) ||
            (rc = sg.down(means, m, s.floats.bytes, "D2H means")))
            return rc;
        return sg.finish();
    });
}

int mvsv_median_blur3_device(mvsv_ctx* ctx, int n, const int16_t* src, size_t ss, size_t sfs, int16_t* dst,
                             size_t ds, size_t dfs, int W, int H)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !src || !dst || W <= 0 || H <= 0 || ss < (size_t)W || ds < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad median arguments");
    // one element past the last one the n frames of a view reach
    auto extent = [&](size_t st, size_t fs) { return (size_t)(n - 1) * fs + (size_t)(H - 1) * st + (size_t)W; };
    const uintptr_t s0 = (uintptr_t)src, s1 = (uintptr_t)(src + extent(ss, sfs));
    const uintptr_t d0 = (uintptr_t)dst, d1 = (uintptr_t)(dst + extent(ds, dfs));
    if (s0 < d1 && d0 < s1) return set_error(ctx, MVSV_E_INVALID_ARG, "median: src and dst overlap");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, median3x3_device(ctx, n, src, ss, sfs, dst, ds, dfs, W, H, nullptr, 0u, 0));
}

int mvsv_filter_speckles_device(mvsv_ctx* ctx, int n, int16_t* img, size_t st, size_t fs, int W, int H, int new_val,
                                int max_speckle_size, int max_diff)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !img || W <= 0 || H <= 0 || st < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad speckle filter arguments");
    if (new_val < -32768 || new_val > 32767)
        return set_error(ctx, MVSV_E_INVALID_ARG, "speckle filter: new_val is not an int16 value");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, speckle_device(ctx, n, img, st, fs, W, H, new_val, max_speckle_size, max_diff));
}

int mvsv_samplepoint_layout(int W, int H, int* step_x, int* step_y, int* nx, int* ny)
{
    if (!step_x || !step_y || !nx || !ny) return MVSV_E_INVALID_ARG;
    return sample_layout(W, H, step_x, step_y, nx, ny);
}

// What both sample point calls ask of their arguments; *npts: the lattice's points, and
// a map without one (narrower or lower than 16) asks for nothing: the call has nothing to do
static bool sample_args_ok(const int16_t* dmap, size_t st, int W, int H, const float* values, int* min_step, size_t* npts)
{
    if (!dmap || W <= 0 || H <= 0 || st < (size_t)W) return false;
    int sx, sy, nx, ny;
    sample_layout(W, H, &sx, &sy, &nx, &ny);
    *min_step = std::min(sx, sy);
    *npts = (size_t)nx * ny;
    return *npts == 0 || values;
}

int mvsv_samplepoint_values_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                                   int radius, float* values)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    int min_step;
    size_t npts;
    if (n <= 0 || !sample_args_ok(dmap, st, W, H, values, &min_step, &npts))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad sample point arguments");
    if (npts == 0) return MVSV_OK;
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, sample_grid_device(ctx, n, dmap, st, fs, W, H, radius, values));
}

int mvsv_samplepoint_values(mvsv_ctx* ctx, const int16_t* dmap, size_t st, int W, int H, int radius, float* values)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    int min_step;
    size_t npts;
    if (!sample_args_ok(dmap, st, W, H, values, &min_step, &npts))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad sample point arguments");
    if (npts == 0) return MVSV_OK;
    if (radius < 0 || radius >= min_step)
        return set_error(ctx, MVSV_E_INVALID_ARG, "sample point radius must be 0 .. min(step_x, step_y) - 1");
    DeviceGuard dev_guard(ctx->device);
    const MapFloatsStage s(W, H, npts);
    return staged_call(ctx, s, "sample point staging", [&](Staging& sg) -> int {
        int rc;
        int16_t* d = sg.at<int16_t>(s.map);
        float* v = sg.at<float>(s.floats);
        if ((rc = sg.up(d, s.map.pitch, dmap, st * 2, (size_t)W * 2, H, "H2D map")) ||
            (rc = sample_grid_device(ctx, 1, d, W, s.map.bytes / 2, W, H, radius, v)) ||
            (rc = sg.down(values, v, s.floats.bytes, "D2H sample point values")))
            return rc;
        return sg.finish();
    });
}

int mvsv_samplepoint_detect_device(mvsv_ctx* ctx, int n, const float* values, int W, int H, const float* Q,
                                   float first, float second, int max_hits, int* counts, mvsv_sample_hit* hits)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || W <= 0 || H <= 0 || !Q || max_hits < 0 || (max_hits > 0 && !hits))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad sample point detection arguments");
    int sx, sy, nx, ny;
    sample_layout(W, H, &sx, &sy, &nx, &ny);
    if (nx == 0 || ny == 0) return MVSV_OK;
    if (!values || !counts) return set_error(ctx, MVSV_E_INVALID_ARG, "bad sample point detection arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, sample_detect_device(ctx, n, values, W, H, Q, first, second, max_hits, counts, hits));
}

int mvsv_minmax_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                       int positive_only, int16_t* minmax)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !dmap || !minmax || W <= 0 || H <= 0 || st < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad min / max arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, minmax_device(ctx, n, dmap, st, fs, W, H, positive_only != 0, minmax));
}

static bool normalize_args_ok(const int16_t* dmap, size_t st, int W, int H, double alpha, double beta, const uint8_t* out,
                              size_t os)
{
    return dmap && out && W > 0 && H > 0 && st >= (size_t)W && os >= (size_t)W && std::isfinite(alpha) &&
           std::isfinite(beta);
}

int mvsv_normalize_minmax_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                                 double alpha, double beta, uint8_t* out, size_t os, size_t ofs, int16_t* minmax)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !normalize_args_ok(dmap, st, W, H, alpha, beta, out, os))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad normalize arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, normalize_minmax_device(ctx, n, dmap, st, fs, W, H, alpha, beta, out, os, ofs, minmax));
}

int mvsv_normalize_minmax(mvsv_ctx* ctx, const int16_t* dmap, size_t st, int W, int H, double alpha, double beta,
                          uint8_t* out, size_t os, int16_t* minmax)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (!normalize_args_ok(dmap, st, W, H, alpha, beta, out, os))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad normalize arguments");
    DeviceGuard dev_guard(ctx->device);
    const NormalizeStage s(W, H);
    return staged_call(ctx, s, "normalize staging", [&](Staging& sg) -> int {
        int rc;
        int16_t* d = sg.at<int16_t>(s.map);
        uint8_t* o = sg.at<uint8_t>(s.out);
        int16_t* mm = sg.at<int16_t>(s.minmax);
        if ((rc = sg.up(d, s.map.pitch, dmap, st * 2, (size_t)W * 2, H, "H2D map")) ||
            (rc = normalize_minmax_device(ctx, 1, d, s.map.pitch / 2, s.map.bytes / 2, W, H, alpha, beta, o, s.out.pitch,
                                          s.out.bytes, mm)) ||
            (rc = sg.down(out, os, o, s.out.pitch, (size_t)W, H, "D2H display map")) ||
            (minmax && (rc = sg.down(minmax, mm, 4, "D2H min / max"))))
            return rc;
        return sg.finish();
    });
}

// the rules of a one-shot view call that need no device; a message, or nullptr
static const char* view_call_check(const int16_t* dmap, size_t st, int W, int H, const mvsv_view_spec* spec,
                                   const uint8_t* out, size_t os)
{
    if (const char* why = view_check(spec, W, H)) return why;
    if (!dmap || !out || st < (size_t)W || os < 3 * (size_t)W) return "null view map / image or stride too small";
    if ((spec->layers & MVSV_VIEW_FOUND_TILES) && !spec->means) return "FOUND_TILES needs means";
    if ((spec->layers & MVSV_VIEW_FOUND_POINTS) && !spec->values) return "FOUND_POINTS needs values";
    return nullptr;
}

int mvsv_view_draw(uint8_t* img, size_t stride, int W, int H, const mvsv_view_spec* spec)
{
    if (view_call_check((const int16_t*)img, (size_t)std::max(W, 0), W, H, spec, img, stride)) return MVSV_E_INVALID_ARG;
    view_draw_host(img, stride, W, H, *spec);
    return MVSV_OK;
}

int mvsv_view_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                     const mvsv_view_spec* spec, uint8_t* out, size_t os, size_t ofs, int16_t* minmax)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0) return set_error(ctx, MVSV_E_INVALID_ARG, "bad view arguments");
    if (const char* why = view_call_check(dmap, st, W, H, spec, out, os)) return set_error(ctx, MVSV_E_INVALID_ARG, why);
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, view_device(ctx, n, dmap, st, fs, W, H, *spec, out, os, ofs, minmax));
}

int mvsv_view(mvsv_ctx* ctx, const int16_t* dmap, size_t st, int W, int H, const mvsv_view_spec* spec, uint8_t* out,
              size_t os, int16_t* minmax)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (const char* why = view_call_check(dmap, st, W, H, spec, out, os)) return set_error(ctx, MVSV_E_INVALID_ARG, why);
    DeviceGuard dev_guard(ctx->device);
    int sx, sy, nx, ny;
    sample_layout(W, H, &sx, &sy, &nx, &ny);
    const ViewStage s(W, H, (spec->layers & MVSV_VIEW_FOUND_POINTS) ? (size_t)nx * ny : 0);
    return staged_call(ctx, s, "view staging", [&](Staging& sg) -> int {
        int rc;
        int16_t* d = sg.at<int16_t>(s.map);
        uint8_t* o = sg.at<uint8_t>(s.out);
        int16_t* mm = sg.at<int16_t>(s.minmax);
        mvsv_view_spec dspec = *spec;
        dspec.means = sg.at<float>(s.means);
        dspec.values = sg.at<float>(s.values);
        if ((rc = sg.up(d, s.map.pitch, dmap, st * 2, (size_t)W * 2, H, "H2D map")) ||
            ((spec->layers & MVSV_VIEW_FOUND_TILES) &&
             (rc = sg.up(sg.at<float>(s.means), spec->means, s.means.bytes, "H2D means"))) ||
            (s.values.bytes && (rc = sg.up(sg.at<float>(s.values), spec->values, s.values.bytes, "H2D sample values"))) ||
            (rc = view_device(ctx, 1, d, s.map.pitch / 2, s.map.bytes / 2, W, H, dspec, o, s.out.pitch, s.out.bytes, mm)) ||
            (rc = sg.down(out, os, o, s.out.pitch, 3 * (size_t)W, H, "D2H view")) ||
            (minmax && (rc = sg.down(minmax, mm, 4, "D2H min / max"))))
            return rc;
        return sg.finish();
    });
}

// One host pair through either matcher; cn: bytes per input pixel (3: mvsv_sgbm_bgr);
// census: mvsv_sgbm_census / mvsv_bm_census with the cw x ch window
static int host_call(mvsv_ctx* ctx, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs,
                     int W, int H, int16_t* out, size_t os, bool sgbm, const void* params, int cn = 1,
                     bool census = false, int cw = 0, int ch = 0)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (!L || !R || !out || W <= 0 || H <= 0)
        return set_error(ctx, MVSV_E_INVALID_ARG, "null buffer or empty image");
    if (ls < (size_t)W * cn || rs < (size_t)W * cn || os < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "stride smaller than width");
    int rc;
    SgbmEff se;
    BmEff be;
    std::string why;
    rc = sgbm ? (census ? resolve_sgbm_census((const mvsv_sgbm_params*)params, W, H, cw, ch, &se, &why)
                        : resolve_sgbm((const mvsv_sgbm_params*)params, W, H, &se, &why))
              : (census ? resolve_bm_census((const mvsv_bm_params*)params, W, H, cw, ch, &be, &why)
                        : resolve_bm((const mvsv_bm_params*)params, W, H, &be, &why));
    if (rc) return set_error(ctx, rc, why);
    if (sgbm) se.cn = cn;
    if (sgbm && (rc = check_report(ctx))) return rc;  // an earlier device call's give-up
    DeviceGuard dev_guard(ctx->device);
    const PairStage s(W, H, cn, 2);
    return staged_call(ctx, s, "matcher staging", [&](Staging& sg) -> int {
        int rc;
        uint8_t* dl = sg.at<uint8_t>(s.left);
        uint8_t* dr = sg.at<uint8_t>(s.right);
        int16_t* dout = sg.at<int16_t>(s.out);
        const size_t rb = s.left.pitch, ib = s.left.bytes, fb = (size_t)W * H;  // input row / frame bytes
        if ((rc = sg.up(dl, rb, L, ls, rb, H, "H2D left")) || (rc = sg.up(dr, rb, R, rs, rb, H, "H2D right")) ||
            (rc = sgbm ? sgbm_device(ctx, 1, dl, rb, ib, dr, rb, ib, W, H, se, dout, W, fb)
                       : bm_device(ctx, 1, dl, rb, ib, dr, rb, ib, W, H, be, dout, W, fb)) ||
            (rc = sg.down(out, os * 2, dout, s.out.pitch, (size_t)W * 2, H, "D2H out")) || (rc = sg.finish()))
            return rc;
        // only an SGBM call reads the sticky give-up word: a BM call's valid map is
        // returned and the word waits for the next SGBM call or mvsv_synchronize
        return sgbm ? check_report(ctx) : MVSV_OK;
    });
}

int mvsv_sgbm(mvsv_ctx* ctx, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs, int W,
              int H, const mvsv_sgbm_params* p, int16_t* out, size_t os)
{
    return host_call(ctx, L, ls, R, rs, W, H, out, os, true, p);
}

int mvsv_sgbm_bgr(mvsv_ctx* ctx, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs, int W,
                  int H, const mvsv_sgbm_params* p, int16_t* out, size_t os)
{
    return host_call(ctx, L, ls, R, rs, W, H, out, os, true, p, 3);
}

int mvsv_sgbm_census(mvsv_ctx* ctx, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs, int W,
                     int H, const mvsv_sgbm_params* p, int16_t* out, size_t os, int cw, int ch)
{
    return host_call(ctx, L, ls, R, rs, W, H, out, os, true, p, 1, true, cw, ch);
}

int mvsv_census(mvsv_ctx* ctx, const uint8_t* img, size_t st, int W, int H, int cw, int ch, uint64_t* out, size_t os)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (!img || !out || W <= 0 || H <= 0) return set_error(ctx, MVSV_E_INVALID_ARG, "null buffer or empty image");
    if (st < (size_t)W || os < (size_t)W) return set_error(ctx, MVSV_E_INVALID_ARG, "stride smaller than width");
    if (const char* why = census_window_check(cw, ch)) return set_error(ctx, MVSV_E_INVALID_ARG, why);
    DeviceGuard dev_guard(ctx->device);
    const ImageStage s(H, W, kRowTight, (size_t)W * 8, H);
    return staged_call(ctx, s, "census staging", [&](Staging& sg) -> int {
        int rc;
        uint8_t* in = sg.at<uint8_t>(s.in);
        uint64_t* o = sg.at<uint64_t>(s.out);
        if ((rc = sg.up(in, s.in.pitch, img, st, (size_t)W, H, "H2D image")) ||
            (rc = census_device(ctx, 1, 1, in, s.in.pitch, s.in.bytes, in, s.in.pitch, s.in.bytes, W, H, cw, ch, o,
                                (size_t)W, 0, (size_t)W * H)) ||
            (rc = sg.down(out, os * 8, o, s.out.pitch, (size_t)W * 8, H, "D2H descriptors")))
            return rc;
        return sg.finish();
    });
}

int mvsv_bm(mvsv_ctx* ctx, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs, int W,
            int H, const mvsv_bm_params* p, int16_t* out, size_t os)
{
    return host_call(ctx, L, ls, R, rs, W, H, out, os, false, p);
}

int mvsv_bm_census(mvsv_ctx* ctx, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs, int W, int H,
                   const mvsv_bm_params* p, int16_t* out, size_t os, int cw, int ch)
{
    return host_call(ctx, L, ls, R, rs, W, H, out, os, false, p, 1, true, cw, ch);
}

}  // extern "C"

// ---- reprojection and PLY output -------------------------

int mvsv_reproject_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W,
                          int H, const float* Q, float* xyzw, size_t xs, size_t xfs)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !dmap || !Q || !xyzw || W <= 0 || H <= 0 || st < (size_t)W || xs < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad reprojection arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, reproject_device(ctx, n, dmap, st, fs, W, H, Q, xyzw, xs, xfs));
}

// what every point cloud call asks of its map
static bool cloud_args_ok(const int16_t* dmap, size_t st, int W, int H, const float* Q)
{
    return dmap && Q && W > 0 && H > 0 && st >= (size_t)W && (size_t)W * H <= (size_t)INT32_MAX;
}

int mvsv_point_cloud_device(mvsv_ctx* ctx, int n, const int16_t* dmap, size_t st, size_t fs, int W, int H,
                            const float* Q, mvsv_cloud_point* records, int capacity, int* counts, int32_t* minmax)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !cloud_args_ok(dmap, st, W, H, Q) || !records || !counts || capacity < 1 ||
        ((uintptr_t)records & 15) != 0)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad point cloud arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, point_cloud_device(ctx, n, dmap, st, fs, W, H, Q, records, capacity, counts, 1, minmax, 2));
}

// One host map through the device, up to the header (count, min, max) on the host:
// it comes back first, so that a caller copies only the records that exist, from
// *dev_records.
static int host_cloud(Staging& sg, const CloudStage& s, const int16_t* dmap, size_t st, int W, int H, const float* Q,
                      int hdr[3], const mvsv_cloud_point** dev_records)
{
    int16_t* d = sg.at<int16_t>(s.map);
    int* dh = sg.at<int>(s.header);
    mvsv_cloud_point* rec = sg.at<mvsv_cloud_point>(s.records);
    *dev_records = rec;
    int rc;
    if ((rc = sg.up(d, s.map.pitch, dmap, st * 2, (size_t)W * 2, H, "H2D dmap")) ||
        (rc = point_cloud_device(sg.ctx, 1, d, s.map.pitch / 2, s.map.bytes / 2, W, H, Q, rec,
                                 (int)(s.records.bytes / sizeof *rec), dh, 3, dh + 1, 3)) ||
        (rc = sg.down(hdr, dh, s.header.bytes, "D2H cloud header")))
        return rc;
    return sg.finish();
}

int mvsv_point_cloud(mvsv_ctx* ctx, const int16_t* dmap, size_t st, int W, int H, const float* Q,
                     mvsv_cloud_point* records, int capacity, int* count, int32_t* minmax)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (!cloud_args_ok(dmap, st, W, H, Q) || !records || !count || capacity < 1)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad point cloud arguments");
    DeviceGuard dev_guard(ctx->device);
    const CloudStage s(W, H, capacity);
    return staged_call(ctx, s, "point cloud staging", [&](Staging& sg) -> int {
        int rc, hdr[3];
        const mvsv_cloud_point* dev = nullptr;
        if ((rc = host_cloud(sg, s, dmap, st, W, H, Q, hdr, &dev))) return rc;
        *count = hdr[0];
        if (minmax) {
            minmax[0] = hdr[1];
            minmax[1] = hdr[2];
        }
        const size_t k = (size_t)std::min(hdr[0], capacity);
        if (k == 0) return MVSV_OK;
        if ((rc = sg.down(records, dev, k * sizeof(mvsv_cloud_point), "D2H points"))) return rc;
        return sg.finish();
    });
}

// [Utility::dmap2pcl] src/utility.cpp:242-262
int mvsv_dmap2pcl(mvsv_ctx* ctx, const char* path, const int16_t* dmap, size_t st, int W, int H,
                  const float* Q)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (!path || !cloud_args_ok(dmap, st, W, H, Q)) return set_error(ctx, MVSV_E_INVALID_ARG, "bad dmap2pcl arguments");
    DeviceGuard dev_guard(ctx->device);
    const CloudStage s(W, H, INT32_MAX);
    return staged_call(ctx, s, "point cloud staging", [&](Staging& sg) -> int {
        int rc, hdr[3];
        const mvsv_cloud_point* dev = nullptr;
        if ((rc = host_cloud(sg, s, dmap, st, W, H, Q, hdr, &dev))) return rc;
        // the records are (x, y, z, grey): vertices 4 floats apart; the writer prints its own grey
        const size_t k = (size_t)hdr[0];
        std::vector<float> pts(k * 4);
        if (k && ((rc = sg.down(pts.data(), dev, k * sizeof(mvsv_cloud_point), "D2H points")) || (rc = sg.finish())))
            return rc;
        rc = mvsv_write_ply(path, "Hagen Hiller", "disparity pointcloud", pts.data(), k, 4,
                            MVSV_PLY_WITH_COLOR, dmap, st, W, H);
        if (rc == MVSV_E_IO) return set_error(ctx, rc, std::string("cannot write ") + path);
        if (rc) return set_error(ctx, rc, "dmap2pcl: map has no positive disparity");
        return MVSV_OK;
    });
}

// ---- rectification ------------------------------------------

int mvsv_remap_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t ss, size_t sfs, int sw,
                      int sh, const float* mx, const float* my, size_t ms, uint8_t* dst, size_t ds,
                      size_t dfs, int dw, int dh)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !src || !mx || !my || !dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 ||
        ss < (size_t)sw || ds < (size_t)dw || ms < (size_t)dw)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad remap arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, remap_device(ctx, n, src, ss, sfs, sw, sh, mx, my, ms, dst, ds, dfs, dw, dh));
}

int mvsv_resize_size(int sw, int sh, double fx, double fy, int* dw, int* dh)
{
    if (!dw || !dh) return MVSV_E_INVALID_ARG;
    return resize_size(sw, sh, fx, fy, dw, dh);
}

static bool resize_args_ok(const uint8_t* src, size_t ss, int sw, int sh, double fx, double fy, const uint8_t* dst,
                           int* dw, int* dh)
{
    return src && dst && ss >= (size_t)std::max(sw, 0) && !resize_size(sw, sh, fx, fy, dw, dh);
}

// [cv::resize in Stereosystem::getRectifiedImagepair(Stereopair&, float)] src/Stereosystem.cpp:279-315
int mvsv_resize_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t ss, size_t sfs, int sw, int sh,
                       double fx, double fy, uint8_t* dst, size_t ds, size_t dfs)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    int dw, dh;
    if (n <= 0 || !resize_args_ok(src, ss, sw, sh, fx, fy, dst, &dw, &dh))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad resize arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, resize_device(ctx, n, src, ss, sfs, sw, sh, fx, fy, dst, ds, dfs));
}

int mvsv_resize(mvsv_ctx* ctx, const uint8_t* src, size_t ss, int sw, int sh, double fx, double fy,
                uint8_t* dst, size_t ds)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    int dw, dh;
    if (!resize_args_ok(src, ss, sw, sh, fx, fy, dst, &dw, &dh) || ds < (size_t)dw)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad resize arguments");
    DeviceGuard dev_guard(ctx->device);
    const ImageStage s(sh, sw, kRowTight, dw, dh);
    return staged_call(ctx, s, "resize staging", [&](Staging& sg) -> int {
        int rc;
        uint8_t* in = sg.at<uint8_t>(s.in);
        uint8_t* out = sg.at<uint8_t>(s.out);
        if ((rc = sg.up(in, s.in.pitch, src, ss, sw, sh, "H2D image")) ||
            (rc = resize_device(ctx, 1, in, s.in.pitch, s.in.bytes, sw, sh, fx, fy, out, s.out.pitch, s.out.bytes)) ||
            (rc = sg.down(dst, ds, out, s.out.pitch, dw, dh, "D2H image")))
            return rc;
        return sg.finish();
    });
}

int mvsv_prepare_size(int sw, int sh, int halve, int* dw, int* dh)
{
    if (!dw || !dh) return MVSV_E_INVALID_ARG;
    return prepare_size(sw, sh, halve, dw, dh);
}

static bool prepare_args_ok(const uint8_t* bgr, size_t ss, int sw, int sh, int halve, int variant, const uint8_t* dst,
                            size_t ds, int* dw, int* dh)
{
    return bgr && dst && !prepare_size(sw, sh, halve, dw, dh) && ss >= 3 * (size_t)sw && ds >= (size_t)*dw &&
           (variant == MVSV_GRAY_Q14 || variant == MVSV_GRAY_Q15);
}

// [cv::resize INTER_AREA 0.5 + cv::cvtColor BGR2GRAY] trgt/disparityTest.cpp:201-211
int mvsv_prepare_gray_device(mvsv_ctx* ctx, int n, const uint8_t* bgr, size_t ss, size_t sfs, int sw, int sh,
                             int halve, int variant, uint8_t* dst, size_t ds, size_t dfs)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    int dw, dh;
    if (n <= 0 || !prepare_args_ok(bgr, ss, sw, sh, halve, variant, dst, ds, &dw, &dh))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad prepare arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, prepare_gray_device(ctx, n, bgr, ss, sfs, sw, sh, halve, variant, dst, ds, dfs));
}

int mvsv_prepare_gray(mvsv_ctx* ctx, const uint8_t* bgr, size_t ss, int sw, int sh, int halve, int variant,
                      uint8_t* dst, size_t ds)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    int dw, dh;
    if (!prepare_args_ok(bgr, ss, sw, sh, halve, variant, dst, ds, &dw, &dh))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad prepare arguments");
    DeviceGuard dev_guard(ctx->device);
    const ImageStage s(sh, 3 * (size_t)sw, kRow4, dw, dh);
    return staged_call(ctx, s, "prepare staging", [&](Staging& sg) -> int {
        int rc;
        uint8_t* in = sg.at<uint8_t>(s.in);
        uint8_t* out = sg.at<uint8_t>(s.out);
        if ((rc = sg.up(in, s.in.pitch, bgr, ss, s.in.row_bytes, sh, "H2D image")) ||
            (rc = prepare_gray_device(ctx, 1, in, s.in.pitch, s.in.bytes, sw, sh, halve, variant, out, s.out.pitch,
                                      s.out.bytes)) ||
            (rc = sg.down(dst, ds, out, s.out.pitch, dw, dh, "D2H image")))
            return rc;
        return sg.finish();
    });
}

// [Stereosystem::getRectifiedImagepair] src/Stereosystem.cpp:243-262
int mvsv_rectify_pair(mvsv_ctx* ctx, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs,
                      int W, int H, const float* const* maps, const mvsv_rect* roi, uint8_t* oL,
                      size_t ols, uint8_t* oR, size_t ors)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (!L || !R || !maps || !roi || !oL || !oR || W <= 0 || H <= 0 || ls < (size_t)W ||
        rs < (size_t)W || roi->x0 < 0 || roi->y0 < 0 || roi->x1 > W || roi->y1 > H ||
        roi->x1 <= roi->x0 || roi->y1 <= roi->y0 || ols < (size_t)(roi->x1 - roi->x0) ||
        ors < (size_t)(roi->x1 - roi->x0))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad rectification arguments");
    for (int i = 0; i < 4; i++)
        if (!maps[i]) return set_error(ctx, MVSV_E_INVALID_ARG, "null map");
    DeviceGuard dev_guard(ctx->device);
    const size_t px = (size_t)W * H;
    const RemapStage s(W, H, 4 * px);
    return staged_call(ctx, s, "rectify staging", [&](Staging& sg) -> int {
        int rc;
        uint8_t* dsrc = sg.at<uint8_t>(s.src);  // [2][H][W] inputs
        uint8_t* ddst = sg.at<uint8_t>(s.dst);  // [2][H][W] outputs
        float* dmap = sg.at<float>(s.maps);     // [4][H][W]
        if ((rc = sg.up(dsrc, W, L, ls, W, H, "H2D image")) || (rc = sg.up(dsrc + px, W, R, rs, W, H, "H2D image")))
            return rc;
        for (int i = 0; i < 4; i++)
            if ((rc = sg.up(dmap + i * px, maps[i], px * sizeof(float), "H2D map"))) return rc;
        for (int i = 0; i < 2; i++)
            if ((rc = remap_device(ctx, 1, dsrc + i * px, W, px, W, H, dmap + (2 * i) * px, dmap + (2 * i + 1) * px, W,
                                   ddst + i * px, W, px, W, H)))
                return rc;
        const int cw = roi->x1 - roi->x0, ch = roi->y1 - roi->y0;
        const uint8_t* crop = ddst + (size_t)roi->y0 * W + roi->x0;
        if ((rc = sg.down(oL, ols, crop, W, cw, ch, "D2H image")) ||
            (rc = sg.down(oR, ors, crop + px, W, cw, ch, "D2H image")))
            return rc;
        return sg.finish();
    });
}

// ---- camera set-up: focus measure and undistorted pairs ---------------------------

static bool rect_inside(const mvsv_rect& q, int W, int H)
{
    return q.x0 >= 0 && q.y0 >= 0 && q.x1 <= W && q.y1 <= H && q.x1 > q.x0 && q.y1 > q.y0;
}

static bool sharpness_args_ok(const uint8_t* img, size_t st, int W, int H, const mvsv_rect& q)
{
    return img && W > 0 && H > 0 && st >= (size_t)W && rect_inside(q, W, H) && (size_t)W * H <= (size_t)INT32_MAX;
}

// [Utility::checkSharpness] src/utility.cpp:163-174: the integer sum S4
int mvsv_sharpness_device(mvsv_ctx* ctx, int n, const uint8_t* img, size_t st, size_t fs, int W, int H,
                          const mvsv_rect* roi, int64_t* sums)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    const mvsv_rect q = roi ? *roi : mvsv_rect{0, 0, W, H};
    if (n <= 0 || !sums || !sharpness_args_ok(img, st, W, H, q))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad sharpness arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, sharpness_device(ctx, n, img, st, fs, W, H, q, sums, 1));
}

int mvsv_sharpness(mvsv_ctx* ctx, const uint8_t* img, size_t st, int W, int H, const mvsv_rect* roi, double* value,
                   int64_t* sum4)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    const mvsv_rect q = roi ? *roi : mvsv_rect{0, 0, W, H};
    if (!sharpness_args_ok(img, st, W, H, q)) return set_error(ctx, MVSV_E_INVALID_ARG, "bad sharpness arguments");
    DeviceGuard dev_guard(ctx->device);
    int64_t s4 = 0;
    const SharpnessStage s(W, H);
    const int rc = staged_call(ctx, s, "sharpness staging", [&](Staging& sg) -> int {
        int rc;
        uint8_t* d = sg.at<uint8_t>(s.img);
        int64_t* ds = sg.at<int64_t>(s.sum);
        if ((rc = sg.up(d, s.img.pitch, img, st, (size_t)W, H, "H2D image")) ||
            (rc = sharpness_device(ctx, 1, d, s.img.pitch, s.img.bytes, W, H, q, ds, 1)) ||
            (rc = sg.down(&s4, ds, sizeof s4, "D2H sharpness")))
            return rc;
        return sg.finish();
    });
    if (rc) return rc;
    if (sum4) *sum4 = s4;
    // cv::mean: sum * (1.0 / N), a reciprocal and a product, each rounded
    if (value) *value = ((double)s4 / 4.0) * (1.0 / ((double)(q.x1 - q.x0) * (double)(q.y1 - q.y0)));
    return MVSV_OK;
}

// [cv::remap, CV_16SC2 + CV_16UC1 maps]
int mvsv_remap_fixed_device(mvsv_ctx* ctx, int n, const uint8_t* src, size_t ss, size_t sfs, int sw, int sh,
                            const int16_t* xy, size_t xs, const uint16_t* frac, size_t fs, uint8_t* dst, size_t ds,
                            size_t dfs, int dw, int dh)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (n <= 0 || !src || !xy || !frac || !dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || ss < (size_t)sw ||
        xs < (size_t)dw || fs < (size_t)dw || ds < (size_t)dw || ((uintptr_t)xy & 1) || ((uintptr_t)frac & 1))
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad fixed-point remap arguments");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, remap_fixed_device(ctx, n, src, ss, sfs, sw, sh, xy, xs, frac, fs, dst, ds, dfs, dw, dh));
}

// [Stereosystem::getUndistortedImagepair] src/Stereosystem.cpp:179-191: two cv::undistort
int mvsv_undistort_pair(mvsv_ctx* ctx, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs, int W, int H,
                        const double* KL, const double* DL, int nL, const double* KR, const double* DR, int nR,
                        uint8_t* oL, size_t ols, uint8_t* oR, size_t ors)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    auto dist_ok = [](const double* d, int nd) { return (nd == 0 || nd == 4 || nd == 5 || nd == 8) && (nd == 0 || d); };
    if (!L || !R || !oL || !oR || !KL || !KR || W <= 0 || H <= 0 || ls < (size_t)W || rs < (size_t)W ||
        ols < (size_t)W || ors < (size_t)W || !dist_ok(DL, nL) || !dist_ok(DR, nR) ||
        (size_t)W * H > (size_t)INT32_MAX)
        return set_error(ctx, MVSV_E_INVALID_ARG, "bad undistortion arguments");
    DeviceGuard dev_guard(ctx->device);
    const size_t px = (size_t)W * H;
    const RemapStage s(W, H, 0);
    return staged_call(ctx, s, "undistort staging", [&](Staging& sg) -> int {
        int rc;
        // the maps of a calibration are built and uploaded once: the key is all they depend on
        std::vector<double> key = {(double)W, (double)H, (double)nL, (double)nR};
        key.insert(key.end(), KL, KL + 9);
        key.insert(key.end(), KR, KR + 9);
        key.insert(key.end(), DL, DL + nL);
        key.insert(key.end(), DR, DR + nR);
        const bool cached = ctx->ud_maps.ptr && key.size() == ctx->ud_key.size() &&
                            std::memcmp(key.data(), ctx->ud_key.data(), key.size() * sizeof(double)) == 0;
        if (!cached) {
            ctx->ud_key.clear();
            if ((rc = ensure(ctx, ctx->ud_maps, 2 * px * 6, "undistort maps"))) return rc;
            std::vector<int16_t> xy(2 * px * 2);
            std::vector<uint16_t> fr(2 * px);
            if (mvsv_undistort_maps(KL, DL, nL, nullptr, W, H, xy.data(), W, fr.data(), W) ||
                mvsv_undistort_maps(KR, DR, nR, nullptr, W, H, xy.data() + 2 * px, W, fr.data() + px, W))
                return set_error(ctx, MVSV_E_INVALID_ARG, "singular camera matrix");
            // synchronous copies: the host vectors end with this scope
            if ((rc = sg.finish()) ||
                (rc = check_hip(ctx, hipMemcpy(ctx->ud_maps.ptr, xy.data(), 4 * px * sizeof(int16_t),
                                               hipMemcpyHostToDevice), "H2D map")) ||
                (rc = check_hip(ctx, hipMemcpy((uint8_t*)ctx->ud_maps.ptr + 8 * px, fr.data(),
                                               2 * px * sizeof(uint16_t), hipMemcpyHostToDevice), "H2D map")))
                return rc;
            ctx->ud_key = key;
        }
        const int16_t* dxy = (const int16_t*)ctx->ud_maps.ptr;
        const uint16_t* dfr = (const uint16_t*)((const uint8_t*)ctx->ud_maps.ptr + 8 * px);
        uint8_t* dsrc = sg.at<uint8_t>(s.src);  // [2][H][W] inputs
        uint8_t* ddst = sg.at<uint8_t>(s.dst);  // [2][H][W] outputs: in-place calls are safe
        if ((rc = sg.up(dsrc, W, L, ls, W, H, "H2D image")) || (rc = sg.up(dsrc + px, W, R, rs, W, H, "H2D image")))
            return rc;
        for (int i = 0; i < 2; i++)
            if ((rc = remap_fixed_device(ctx, 1, dsrc + i * px, W, px, W, H, dxy + i * 2 * px, W, dfr + i * px, W,
                                         ddst + i * px, W, px, W, H)))
                return rc;
        if ((rc = sg.down(oL, ols, ddst, W, W, H, "D2H image")) || (rc = sg.down(oR, ors, ddst + px, W, W, H, "D2H image")))
            return rc;
        return sg.finish();
    });
}
